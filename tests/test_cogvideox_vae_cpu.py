"""Host side of the CogVideoX 3-D causal VAE decoder without a GPU: chunk boundaries and frame counts, the spatial norm's frame tables
against ``F.interpolate``, the K order of ``pack_cconv3`` against ``F.conv3d``, what the GEMM planner answers for the new A-operand mode
(and that it answers for the existing modes what it answered before the mode existed), state-dict names against the oracle, the
oracle's own cache rule, the refusals."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cogvideox_vae_oracle as oc
from c_interface import ALIGN, MODE, NULL, OK, SHAPE, Host, entry
from cogvideox_support import REPO

A_CCONV3 = 4
P = 1 << 12          # a non-NULL, 16-byte aligned stand-in: lkgd_gemm_plan with cus != 0 dereferences nothing


# --------------------------------------------------------------------------------------------------------------- chunks
@pytest.mark.parametrize("T,bounds,frames", [(1, [(0, 1)], 1), (2, [(0, 2)], 8), (3, [(0, 3)], 9), (5, [(0, 3), (3, 5)], 17),
                                             (13, [(0, 3), (3, 5), (5, 7), (7, 9), (9, 11), (11, 13)], 49)])
def test_chunk_bounds_and_frame_counts(T, bounds, frames):
    from lkgd_amd import cogvideox_vae as pv
    assert pv.chunk_bounds(T) == bounds == oc.chunk_bounds(T)
    n = 0
    for a, b in bounds:
        t = b - a
        for _ in range(2):                       # temporal_compression_ratio 4: two time-doubling upsamplers
            t = len(pv.upsample_frame_map(t, True))
        n += t
    assert n == frames


def test_upsample_frame_map_is_nearest_interpolation():
    from lkgd_amd import cogvideox_vae as pv
    for T in (1, 2, 3, 4, 5, 9):
        x = torch.arange(T, dtype=torch.float32).reshape(1, 1, T, 1, 1).expand(1, 1, T, 2, 2)
        got = oc.Upsample3D(1, True)
        with torch.no_grad():
            got.conv.weight.zero_(); got.conv.bias.zero_()
            got.conv.weight[0, 0, 1, 1] = 1.0
            y = got(x)
        assert y[0, 0, :, 0, 0].long().tolist() == pv.upsample_frame_map(T, True), T
        assert pv.upsample_frame_map(T, False) == list(range(T))


# (Tz, T) pairs the decoder produces: a chunk of 1 / 2 / 3 latent frames at every level
TMAP_PAIRS = [(1, 1), (2, 2), (2, 4), (2, 8), (3, 3), (3, 5), (3, 9)]


@pytest.mark.parametrize("Tz,T", TMAP_PAIRS)
def test_tmap_equals_interpolate_of_an_index_tensor(Tz, T):
    from lkgd_amd import cogvideox_vae as pv
    zq = torch.arange(Tz, dtype=torch.float32).reshape(1, 1, Tz, 1, 1).expand(1, 1, Tz, 3, 5)
    f = torch.zeros(1, 1, T, 6, 10)
    ref = oc.resize_zq(zq, f)[0, 0, :, 0, 0].long().tolist()
    assert pv.spatial_norm_tmap(Tz, T) == ref
    if T > 1 and T % 2 == 1 and T != Tz:
        assert oc.resize_zq(zq, f, no_split=True)[0, 0, :, 0, 0].long().tolist() != ref      # the decoy differs


# -------------------------------------------------------------------------------------------------------------- packing
def test_pack_cconv3_column_order_against_conv3d():
    from lkgd_amd.packing import pack_cconv3
    g = torch.Generator().manual_seed(3)
    B, Cin, T, H, W, N = 1, 64, 3, 4, 5, 8
    x = torch.randn(B, Cin, T, H, W, generator=g).double()
    w = torch.randn(N, Cin, 3, 3, 3, generator=g).half().double()                     # (fp16 values: the packing rounds nothing)
    xp = torch.cat([x[:, :, :1]] * 2 + [x], dim=2)                                    # first-frame prefix
    ref = F.conv3d(xp, w, padding=(0, 1, 1))                                          # [1, N, T, H, W]
    src = xp[0].permute(1, 2, 3, 0).numpy()                                           # [T + 2, H, W, Cin]
    A = np.zeros((T * H * W, 27 * Cin), dtype=np.float64)
    nc = Cin // 64
    for t in range(T):
        for y in range(H):
            for xx in range(W):
                m = (t * H + y) * W + xx
                for kt in range(3):
                    for ky in range(3):
                        for kx in range(3):
                            vy, vx = y + ky - 1, xx + kx - 1
                            if not (0 <= vy < H and 0 <= vx < W):
                                continue
                            for ch in range(nc):
                                k = kt * 9 * Cin + ((ky * nc + ch) * 3 + kx) * 64      # include/lkgd_hip.h: LKGD_A_CCONV3
                                A[m, k:k + 64] = src[t + kt, vy, vx, ch * 64:(ch + 1) * 64]
    wp = pack_cconv3(w)
    assert wp.dtype == torch.float16 and tuple(wp.shape) == (N, 27 * Cin)
    got = torch.from_numpy(A) @ wp.double().t()                                       # [T*H*W, N]
    want = ref[0].permute(1, 2, 3, 0).reshape(T * H * W, N)
    assert (got - want).abs().max().item() < 1e-5


# -------------------------------------------------------------------------------------------------------------- planner
def _plan(cus=256, **kw):
    from lkgd_amd import _lib
    d = _lib.GemmDesc()
    for k, v in dict(a0=P, w=P, out=P, zeros=P, s_acc=1.0, r1=1.0, r2=1.0, **kw).items():
        setattr(d, k, v)
    info = _lib.GemmPlanInfo()
    rc = _lib.lib().lkgd_gemm_plan(C.byref(d), cus, C.byref(info))
    return rc, [info.program, info.k_slices, info.tile_m, info.tile_n, info.colstats_block, info.lds_out]


def _cconv(B, Cin, N, T, H, W, **over):
    kw = dict(mode=A_CCONV3, M=B * T * H * W, N=N, K=27 * Cin, Cin=Cin, csplit=Cin, lda0=Cin, ldc=N, Hout=H, Wout=W, Hin=H, Win=W,
              stride=1, ups=0, F=T + 2, Floc=T, HW=H * W)
    kw.update(over)
    return kw


GPU_TEST_SHAPES = [(1, 64, 64, 1, 5, 7), (2, 64, 192, 3, 5, 7), (1, 128, 64, 2, 9, 16), (1, 64, 4, 2, 6, 10)]
REAL_SHAPES = [(1, 64, 512, 3, 60, 90), (1, 512, 512, 3, 60, 90), (1, 512, 256, 5, 120, 180), (1, 256, 256, 9, 240, 360),
               (1, 256, 128, 8, 480, 720), (1, 128, 128, 8, 480, 720), (1, 128, 4, 9, 480, 720)]


@pytest.mark.parametrize("shape", GPU_TEST_SHAPES + REAL_SHAPES)
def test_planner_sends_the_causal_conv_to_program_4(shape):
    rc, plan = _plan(**_cconv(*shape))
    assert rc == OK and plan[0] == 4 and plan[1] == 1, (rc, plan)
    assert plan[2] in (192, 256) and plan[3] in (256, 320)
    if shape[2] <= 256:                          # up to 256 channels one 256-column tile idles fewer columns than a 320-column one
        assert plan[3] == 256
    assert _plan(**_cconv(1, 64, 640, 2, 6, 10))[1][3] == 320


class _Rows:
    """what ``ops.gemm_plan`` reads of a row matrix that lives off the device - shape, row stride, an aligned address - without its
    memory (the 480 x 720 level's operands are 0.9 GB each)"""
    is_cuda = False

    def __init__(self, rows, cols):
        self.shape = (rows, cols)

    def dim(self):
        return 2

    def stride(self, i):
        return (self.shape[1], 1)[i]

    def data_ptr(self):
        return P


def _launch_form(shape, colstats, cus=256):
    """(tile rows, tile columns, lds_out) of the launch CogVideoXCausalConv3d.run makes for ``shape``, as ops.gemm would plan it"""
    from lkgd_amd import ops
    B, Cin, N, T, H, W = shape
    M = B * T * H * W
    plan = ops.gemm_plan(_Rows(B * (T + 2) * H * W, Cin), _Rows(N, 27 * Cin), _Rows(M, N), cus=cus, M=M, N=N, K=27 * Cin,
                         bias=torch.empty(N), mode=ops.A_CCONV3, Cin=Cin, cconv=(T, H, W), colstats=colstats)
    assert plan.program == ops.GEMM_WIDE and plan.k_slices == 1
    return plan.tile_m, plan.tile_n, plan.lds_out


def test_real_launches_run_a_form_the_width_tests_run():
    """Every causal-conv launch of the real decode (REAL_SHAPES; the module asks for column sums over a chunk's T*H*W rows at every
    convolution but conv_out) runs a form of the 256x320 program - tile rows, tile columns, rows through LDS or not - that a case of
    tests/test_cogvideox_vae_widths_gpu.py holds to F.conv3d.  A planner change that sends a real launch to an untested form fails
    here: add the form to that file's tables."""
    import test_cogvideox_vae_widths_gpu as wt
    tested = wt.case_forms()
    assert tested <= {(m, n, l) for m in (192, 256) for n in (256, 320) for l in (0, 1)}
    for shape in REAL_SHAPES:
        B, Cin, N, T, H, W = shape
        for colstats in (T * H * W, 0):
            form = _launch_form(shape, colstats)
            assert form in tested, f"{shape} with colstats={colstats} runs {form}: no case of the width tests runs that form"
    # and the tables say what their own cases run: the plan of every case at the tile rows it forces
    from lkgd_amd import _lib
    L = _lib.lib()
    try:
        for rows in wt.TILE_ROWS:
            L.lkgd_debug_set_wide_tile_m(rows)
            for s in wt.direct_shapes():
                assert _launch_form(s, 0) == (rows, wt.TILE_N[s[2]], 0), (s, rows)
        for s, rows in wt.COLSTATS_CASES:
            L.lkgd_debug_set_wide_tile_m(rows)
            assert _launch_form(s, s[3] * s[4] * s[5]) == (rows, wt.TILE_N[s[2]], 1), (s, rows)
    finally:
        L.lkgd_debug_set_wide_tile_m(0)


def test_planner_refuses_what_the_causal_conv_cannot_take():
    s = (1, 64, 64, 2, 6, 10)
    assert _plan(**_cconv(*s))[0] == OK
    assert _plan(**_cconv(*s, K=9 * 64))[0] == SHAPE                 # K != 27 Cin
    assert _plan(**_cconv(*s, K=27 * 64 + 64))[0] == SHAPE
    assert _plan(**_cconv(1, 96, 64, 2, 6, 10))[0] == SHAPE          # Cin % 64
    assert _plan(**_cconv(*s, F=2))[0] == SHAPE                      # F != Floc + 2
    assert _plan(**_cconv(*s, F=5))[0] == SHAPE
    assert _plan(**_cconv(*s, stride=2))[0] == SHAPE
    assert _plan(**_cconv(*s, ups=1))[0] == SHAPE
    assert _plan(**_cconv(*s, pad_off=1))[0] == SHAPE
    assert _plan(**_cconv(*s, Hin=7))[0] == SHAPE
    assert _plan(**_cconv(1, 64, 64, 8, 1 << 11, 1 << 10))[0] == SHAPE      # M = 2^24: past the row decomposition of program 4
    assert _plan(**_cconv(*s, mode=5))[0] == MODE


def test_planner_answers_for_existing_modes_are_the_parent_commits():
    """tests/golden/cogvideox_vae_gemm_plan_parent.json was recorded with the library of the commit before LKGD_A_CCONV3 existed"""
    cases = json.load(open(os.path.join(REPO, "tests", "golden", "cogvideox_vae_gemm_plan_parent.json")))
    assert {c["desc"]["mode"] for c in cases} == {0, 1, 2, 3}
    for c in cases:
        kw = {k: v for k, v in c["desc"].items() if k != "name"}
        rc, plan = _plan(**kw)
        assert rc == c["rc"] and plan == c["plan"], (c["desc"]["name"], rc, plan, c["plan"])


# ----------------------------------------------------------------------------------------------------------- state dict
def _module(cfg=oc.TINY):
    from lkgd_amd import cogvideox_vae as pv
    return pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**cfg.__dict__))


def test_state_dict_keys_and_shapes_equal_the_oracles():
    for cfg in (oc.TINY, oc.CogVAEConfig(block_out_channels=(64, 128, 64, 128), layers_per_block=2)):
        o, m = oc.AutoencoderKLCogVideoX(cfg), _module(cfg)
        ko = {k: tuple(v.shape) for k, v in o.state_dict().items()}
        km = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert ko == km
        for name in ("decoder.conv_in.conv.weight", "decoder.mid_block.resnets.0.norm1.norm_layer.weight",
                     "decoder.mid_block.resnets.0.norm1.conv_y.conv.weight", "decoder.mid_block.resnets.0.norm1.conv_b.conv.bias",
                     "decoder.mid_block.resnets.0.conv1.conv.weight", "decoder.up_blocks.0.upsamplers.0.conv.weight",
                     "decoder.norm_out.conv_y.conv.weight", "decoder.conv_out.conv.bias"):
            assert name in km, name
    assert "decoder.up_blocks.1.resnets.0.conv_shortcut.weight" in km            # (64, 128, 64, 128): the width changes at block 1
    assert all(k.startswith("decoder.") for k in km)


def test_checkpoint_keys_encoder_dropped_misspelt_refused():
    o, m = oc.tiny_pair_weights(), _module()
    sd = dict(o.state_dict())
    sd["encoder.conv_in.conv.weight"] = torch.zeros(3)
    sd["quant_conv.weight"] = torch.zeros(3)
    m.load_state_dict(sd)
    assert torch.equal(m.decoder.conv_out.conv.bias, o.decoder.conv_out.conv.bias)
    bad = dict(o.state_dict())
    bad["decoder.conv_in.conv.wieght"] = bad.pop("decoder.conv_in.conv.weight")
    with pytest.raises(RuntimeError, match="decoder.conv_in.conv.w"):
        m.load_state_dict(bad)
    with pytest.raises(RuntimeError, match="post_quant_conv"):
        m.load_state_dict({**o.state_dict(), "post_quant_conv.weight": torch.zeros(3)}, strict=False)


def test_save_and_from_pretrained_round_trip(tmp_path):
    from lkgd_amd import cogvideox_vae as pv
    m = _module()
    m.load_state_dict(oc.tiny_pair_weights().state_dict())
    m.save_pretrained(str(tmp_path / "vae"))
    m2 = pv.AutoencoderKLCogVideoX.from_pretrained(str(tmp_path), subfolder="vae", torch_dtype=torch.float16)
    assert m2.config.block_out_channels == (64, 64, 128, 128) and m2.config.layers_per_block == 1
    assert m2.dtype == torch.float16
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k].float(), v.half().float()), k


# --------------------------------------------------------------------------------------------------------------- oracle
def test_oracle_cached_chunks_equal_the_whole_clip_convolution():
    torch.manual_seed(0)
    conv = oc.CausalConv3d(8, 6, 3, oc.Switches())
    x = torch.randn(2, 8, 7, 5, 6)
    with torch.no_grad():
        whole = conv(x)
        conv.cache = None
        parts = torch.cat([conv(x[:, :, a:b]) for a, b in ((0, 3), (3, 5), (5, 7))], dim=2)
        conv.cache = None
        dropped = []
        for a, b in ((0, 3), (3, 5)):
            dropped.append(conv(x[:, :, a:b]))
            conv.cache = None
    assert (parts - whole).abs().max().item() < 1e-5
    assert (dropped[0] - whole[:, :, :3]).abs().max().item() < 1e-5
    assert (dropped[1] - whole[:, :, 3:5]).abs().max().item() > 1e-2            # without the cache the second chunk is another function
    # and the first frame's context is the frame itself, not zeros
    z = oc.CausalConv3d(8, 6, 3, oc.Switches(zero_time_pad=True))
    z.load_state_dict(conv.state_dict())
    with torch.no_grad():
        assert (z(x)[:, :, 0] - whole[:, :, 0]).abs().max().item() > 1e-2
        z.cache = None
        assert (z(x)[:, :, 2:] - whole[:, :, 2:]).abs().max().item() < 1e-5


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_name_what_they_refuse():
    from lkgd_amd import LkgdHipError
    from lkgd_amd import cogvideox_vae as pv
    m = _module()
    with pytest.raises(LkgdHipError, match="encode"):
        m.encode(torch.zeros(1, 3, 1, 8, 8))
    with pytest.raises(LkgdHipError, match="enable_tiling"):
        m.enable_tiling()
    with pytest.raises(LkgdHipError, match="use_post_quant_conv"):
        pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(block_out_channels=(64, 64), use_post_quant_conv=True))
    with pytest.raises(LkgdHipError, match="block_out_channels.*96"):
        pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(block_out_channels=(64, 96, 128, 128)))
    with pytest.raises(LkgdHipError, match="norm_num_groups"):
        pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(block_out_channels=(64, 64, 128, 128), norm_num_groups=16))
    with pytest.raises(LkgdHipError, match="MI355X"):
        m.decode(torch.zeros(1, 16, 1, 6, 10))                      # no CPU path
    assert callable(pv.decode_latents) and not hasattr(pv.AutoencoderKLCogVideoX, "decode_latents")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_spatial_norm_refuses_before_launching():
    h = Host()
    call = entry("lkgd_spatial_norm3d", f=h.p, ldf=64, stats=h.p, gamma=h.p, beta=h.p, yb=h.p, ldyb=128, tmap=h.p, out=h.p, ldo=64,
                 out_batch_rows=2 * 6 * 10, B=1, T=2, H=6, W=10, C=64, Tz=2, sh=1, act=1)
    for k in ("f", "stats", "gamma", "beta", "yb", "tmap", "out"):
        assert call(**{k: None}) == NULL, k
    for kw in (dict(B=0), dict(T=0), dict(Tz=0), dict(C=32), dict(C=96), dict(sh=4), dict(sh=-1), dict(H=7), dict(W=9), dict(act=2),
               dict(ldf=56), dict(ldo=56), dict(ldyb=120), dict(out_batch_rows=119), dict(B=1 << 20, out_batch_rows=1 << 12)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(f=h.p + 8), dict(yb=h.p + 8), dict(out=h.p + 8), dict(ldf=68), dict(ldo=68), dict(ldyb=132), dict(gamma=h.p + 8),
               dict(stats=h.p + 4), dict(tmap=h.p + 2)):
        assert call(**kw) == ALIGN, kw
