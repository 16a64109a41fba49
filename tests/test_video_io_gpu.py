"""The two kernels of include/lkgd_hip_video.h on the GPU, bit for bit: ``lkgd_video_postprocess`` against torch's own statements on the
same device (``(x / 2 + 0.5).clamp(0, 1)`` on the half tensor, ``.float()``, ``(. * 255).round().to(uint8)``, the permutes) over every
non-NaN fp16 bit pattern on the narrow and on the wide path, ``lkgd_image_preprocess`` against the host chain of
``VaeImageProcessor`` over all 256 byte values in every channel position, both at the shapes where the indexing can go wrong and on
windowed operands (tests/footprint.py).  Equality is exact everywhere: there is no tolerance in this file."""
import pytest
import torch

from cogvideox_support import DEV
from footprint import run_case

pytestmark = pytest.mark.gpu

#: every name in lkgd_amd._lib.VIDEO_SYMBOLS -> its footprint tests in this module
FOOTPRINT = {
    "lkgd_video_postprocess": ["test_footprint_postprocess"],
    "lkgd_image_preprocess": ["test_footprint_preprocess"],
}

MODES = ["u8", "f32", "f16"]


def _mode(name):
    from lkgd_amd import ops
    return {"u8": ops.VIDEO_U8, "f32": ops.VIDEO_F32, "f16": ops.VIDEO_F16}[name]


def torch_postprocess(x, mode):
    """the statements the kernel replaces, on x's device: denormalize on the half tensor, then per output type the permute of
    ``postprocess_video`` / ``pt_to_numpy``, ``.float()`` and ``numpy_to_pil``'s rounding"""
    d = (x / 2 + 0.5).clamp(0, 1)
    if mode == "f16":
        return d.permute(0, 2, 1, 3, 4).contiguous()
    f = d.permute(0, 2, 3, 4, 1).float().contiguous()
    return f if mode == "f32" else (f * 255).round().to(torch.uint8)


def host_preprocess(u):
    """pil_to_numpy -> numpy_to_pt -> normalize -> .to(fp16) of lkgd_amd/image_processor.py on the uint8 images [N, H, W, C]"""
    from lkgd_amd.image_processor import VaeImageProcessor as P
    return P.normalize(P.numpy_to_pt(P.pil_to_numpy([im for im in u.cpu().numpy()]))).to(torch.float16)


def _same(got, want, what):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, got.shape, want.shape)
    g, w = got.detach().cpu().reshape(-1).contiguous(), want.detach().cpu().reshape(-1).contiguous()
    if not torch.equal(g.view(torch.uint8), w.view(torch.uint8)):
        bad = (g.view(torch.uint8) != w.view(torch.uint8)).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} bytes differ, first at {bad[0].tolist()}")


# ---------------------------------------------------------------------------------------------------------- exhaustive values
@pytest.fixture(scope="module")
def all_halves():
    """every non-NaN fp16 bit pattern, in three differently permuted planes [3, 63490]"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    vals = bits[~torch.isnan(bits)]
    assert vals.numel() == 63490
    g = torch.Generator().manual_seed(7)
    return torch.stack([vals, vals[torch.randperm(63490, generator=g)], vals.flip(0)[torch.randperm(63490, generator=g)]])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L,T,H,W", [(63490, 1, 1, 63490), (63496, 1, 8, 7937)], ids=["narrow", "wide"])
def test_postprocess_every_half_value(all_halves, mode, L, T, H, W):
    from lkgd_amd import ops
    planes = all_halves
    if L > planes.shape[1]:                   # padded to a multiple of 8 with the planes' own first values
        planes = torch.cat([planes, planes[:, :L - planes.shape[1]]], dim=1)
    assert planes.shape[1] == L == T * H * W and (L % 8 == 0) == (W != L)
    x = planes.reshape(1, 3, T, H, W).to(DEV).contiguous()
    _same(ops.video_postprocess(x, _mode(mode)), torch_postprocess(x, mode), f"{mode} L={L}")


def test_preprocess_every_byte_value_in_every_channel_position():
    from lkgd_amd import ops
    v = torch.arange(256, dtype=torch.int32)
    for C_ in (1, 2, 3, 4):
        for H, W in ((16, 16), (1, 256), (4, 64)):          # 256 pixels: H*W % 8 == 0, the wide path
            u = torch.stack([(v * (2 * c + 1) + 37 * c) % 256 for c in range(C_)], dim=1).to(torch.uint8).reshape(1, H, W, C_)
            assert all(sorted(u[..., c].flatten().tolist()) == list(range(256)) for c in range(C_))
            _same(ops.image_preprocess(u.to(DEV)), host_preprocess(u), f"C={C_} {H}x{W}")
        u = torch.cat([u.reshape(1, 1, 256, C_), u.reshape(1, 1, 256, C_)[:, :, :5]], dim=2)      # 261 pixels: the narrow path
        _same(ops.image_preprocess(u.to(DEV)), host_preprocess(u), f"C={C_} narrow")


# ------------------------------------------------------------------------------------------------------------------- shapes
#: (B, C, T, H, W): smallest; L = 105 odd, every plane after the first misaligned, two batch entries; L % 8 == 0; C = 4 with a long
#: run and L % 8 == 1; C = 1
SHAPES = [(1, 3, 1, 1, 1), (2, 3, 3, 5, 7), (1, 3, 2, 8, 24), (1, 4, 1, 3, 1003), (1, 1, 2, 4, 6)]


def _clip(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.5 * torch.randn(shape, generator=g)).half()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_postprocess_shapes(shape, mode):
    from lkgd_amd import ops
    x = _clip(shape, 11).to(DEV)
    _same(ops.video_postprocess(x, _mode(mode)), torch_postprocess(x, mode), f"{mode} {shape}")


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_preprocess_shapes(shape, N):
    from lkgd_amd import ops
    _, C_, _, H, W = shape
    u = torch.randint(0, 256, (N, H, W, C_), generator=torch.Generator().manual_seed(13), dtype=torch.uint8)
    _same(ops.image_preprocess(u.to(DEV)), host_preprocess(u), f"{shape} N={N}")


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from lkgd_amd import ops
    from lkgd_amd._lib import LkgdHipError
    x = _clip((1, 3, 2, 4, 6), 3).to(DEV)
    for bad in (x.float(), x.permute(0, 2, 1, 3, 4), x[0], x.cpu()):
        with pytest.raises(LkgdHipError):
            ops.video_postprocess(bad, ops.VIDEO_U8)
    with pytest.raises(LkgdHipError):
        ops.video_postprocess(x, 3)
    with pytest.raises(LkgdHipError, match="LKGD_E_SHAPE"):
        ops.video_postprocess(torch.zeros(1, 5, 1, 2, 2, dtype=torch.float16, device=DEV), ops.VIDEO_U8)
    u = torch.zeros(1, 4, 6, 3, dtype=torch.uint8, device=DEV)
    for bad in (u.float(), u.permute(0, 2, 1, 3), u[0], u.cpu()):
        with pytest.raises(LkgdHipError):
            ops.image_preprocess(bad)


# ---------------------------------------------------------------------------------------------------------------- footprint
def _pad(col0, n):
    """a gap of 8 .. 15 elements that makes the row stride a multiple of 8 elements: the window's base alignment is col0's"""
    return 8 + (-(col0 + n)) % 8


def _flat_in(W, data, col0, name):
    """``data`` (any shape, contiguous) as one row of an input window, NaN around it; col0 moves its base off 16 bytes"""
    return W.inp(data.reshape(1, -1), pad=_pad(col0, data.numel()), col0=col0, guard=4, name=name)[0].view(data.shape)


def _bytes_as_halves(t):
    return t.contiguous().view(-1).view(torch.uint8).view(torch.float16)


#: (shape, col0 of the input window, col0 of the output window): wide; the same shape pushed onto the narrow path by a misaligned
#: input and by a misaligned output; L % 8 != 0
POST_FOOTPRINT = [((2, 3, 2, 4, 8), 8, 8), ((2, 3, 2, 4, 8), 1, 8), ((2, 3, 2, 4, 8), 8, 1), ((2, 3, 3, 5, 6), 8, 8), ((1, 4, 1, 2, 20), 0, 16)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,ci,co", POST_FOOTPRINT)
def test_footprint_postprocess(shape, ci, co, mode):
    from lkgd_amd import ops
    x = _clip(shape, 17)
    B, C_, T, H, Wd = shape
    oshape = (B, T, C_, H, Wd) if mode == "f16" else (B, T, H, Wd, C_)
    n = x.numel()
    want = torch_postprocess(x.to(DEV), mode)

    def case(W):
        xin = _flat_in(W, x, ci, "video")
        if mode == "u8":                  # the harness poisons with NaN: a uint8 window is the bytes of an fp16 one (n is even)
            o16 = W.out(1, n // 2, torch.float16, pad=_pad(co, n // 2), col0=co, guard=4, name="frames")
            out = o16.view(torch.uint8)[0].view(oshape)
        else:
            dt = torch.float32 if mode == "f32" else torch.float16
            out = W.out(1, n, dt, pad=_pad(co, n), col0=co, guard=4, name="frames")[0].view(oshape)
        ops.video_postprocess(xin, _mode(mode), out=out)
        return {"frames": out.to(torch.int32) if mode == "u8" else out}

    def close(got, ref, name):
        _same(got.to(ref.dtype) if mode == "u8" else got, ref, name)

    run_case(case, DEV, refs=lambda: {"frames": want}, close=close, sync=torch.cuda.synchronize, guard=4)


#: (N, H, W, C, col0 in halves of the input window, col0 of the output window): wide, narrow by either pointer, narrow by H*W
PRE_FOOTPRINT = [(2, 4, 8, 3, 8, 8), (2, 4, 8, 3, 1, 8), (2, 4, 8, 3, 8, 1), (2, 5, 6, 3, 8, 8), (1, 2, 20, 4, 4, 16)]


@pytest.mark.parametrize("N,H,Wd,C_,ci,co", PRE_FOOTPRINT)
def test_footprint_preprocess(N, H, Wd, C_, ci, co):
    from lkgd_amd import ops
    u = torch.randint(0, 256, (N, H, Wd, C_), generator=torch.Generator().manual_seed(19), dtype=torch.uint8)
    want = host_preprocess(u)

    def case(W):
        h16 = W.inp(_bytes_as_halves(u).reshape(1, -1), pad=_pad(ci, u.numel() // 2), col0=ci, guard=4, name="images")
        uin = h16.view(torch.uint8)[0].view(u.shape)
        out = W.out(1, u.numel(), torch.float16, pad=_pad(co, u.numel()), col0=co, guard=4, name="planes")[0].view(N, C_, H, Wd)
        ops.image_preprocess(uin, out=out)
        return {"planes": out}

    run_case(case, DEV, refs=lambda: {"planes": want}, close=_same, sync=torch.cuda.synchronize, guard=4)
