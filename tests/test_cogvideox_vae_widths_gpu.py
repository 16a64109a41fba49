"""The CogVideoX 3-D causal VAE at the widths and grids the shipped model runs: the causal-conv GEMM mode (``LKGD_A_CCONV3``) of the
256x320 program on grids of several rounds per workgroup, on two tile columns, on K = 27 * 512 and in each of its eight tile forms
(tile rows 256 | 192, tile columns 320 | 256, rows direct | through LDS) against ``F.conv3d``; ``lkgd_spatial_norm3d`` at 6, 8 and 16
channels per group and latent grids 4x and 8x coarser; the encoder's conv_in on the program its 480 x 720 launch gets; and the decode and
the encode of the real config, (128, 256, 256, 512) wide with three layers per block, against the fp32 oracles.

Every GEMM case first asserts through ``ops.gemm_plan`` that it runs the tile form it is about; tests/test_cogvideox_vae_cpu.py holds
the forms of the real launches to the tables below without a GPU.

The gate of the real-width decode and encode is the project's 1e-2 (relative L2 from the fp32 oracle: ``GATE`` of the tiny decode, the
encoder file's gate for the moments).  Each case also runs the oracle module itself in torch fp16 on the GPU: where that run is above
1e-2 too, the distance is the arithmetic's (fp16 activations through some thirty convolutions) and no kernel's, and the gate of that
case becomes twice the torch-fp16 distance - the factor of two covers another summation order.  Where HIP alone is above 1e-2 a kernel
is wrong.

Measured distances (relative L2 from the fp32 oracle; weights by ``oc.tiny_pair_weights`` / ``eo.tiny_weights`` with the default
config, inputs by the recipes of ``oc.tiny_latents`` on a 2 x 3 grid and ``eo.tiny_clip`` on a 16 x 24 grid):
    decode T     1            3            5
    HIP          1.03e-03     7.42e-04     6.52e-04
    torch fp16   1.47e-03     9.88e-04     8.20e-04
    encode T     1            5            9
    HIP          1.92e-03     1.59e-03     1.87e-03
    torch fp16   2.59e-03     2.06e-03     2.70e-03   """
import contextlib
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

import cogvideox_vae_encoder_oracle as eo
import cogvideox_vae_oracle as oc
from cogvideox_support import DEV, rel
from test_cogvideox_vae_gpu import GATE, NORM_PAIRS, _close, _conv_data, _conv_ref, _norm_ref, _norm_run, _prefix, _rows_to_ncthw

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------- case tables
# Module constants that import without a GPU: tests/test_cogvideox_vae_cpu.py::test_real_launches_run_a_form_the_width_tests_run asks
# lkgd_gemm_plan for the form of every real launch and looks it up in case_forms().  Shapes are (B, Cin, N, T, H, W).
TILE_ROWS = (256, 192)
#: N -> the tile columns its causal-conv launch runs (up to 256 channels: one 256-column tile; 512 = two of them; else 320)
TILE_N = {64: 256, 128: 256, 256: 256, 512: 256, 384: 320, 640: 320}
ROUNDS_SHAPE = (2, 64, 64, 3, 150, 147)              # M = 132 300: 517 tiles of 256 rows, 690 of 192; 22 050 rows per frame
ROUNDS_TWO_COLUMNS_SHAPE = (1, 64, 512, 3, 150, 147)   # 259 (345) x 2 tiles
COLUMN_SHAPES = [(1, 64, N, 2, 20, 27) for N in (128, 512, 384, 640)]      # M = 1080: last tile of 56 rows (of 120 at 192-row tiles)
DEEP_K_SHAPES = [(1, 256, 128, 2, 9, 16), (1, 512, 64, 2, 9, 16), (1, 512, 512, 1, 9, 16)]
DEEP_K_RANDOM_SHAPE = (1, 512, 512, 1, 9, 16)
LEVEL_SHAPE = (1, 128, 128, 1, 60, 90)
#: (shape, tile rows): column sums, so the rows leave through LDS.  512 rows per sample tile by 256 rows only; 768 = 3 x 256 = 4 x 192
#: brings the 192-row forms and, at N = 640, the 320-column ones
COLSTATS_CASES = [((2, 64, 512, 1, 16, 32), 256), ((2, 64, 256, 1, 16, 32), 256), ((2, 64, 640, 1, 24, 32), 256),
                  ((2, 64, 640, 1, 24, 32), 192), ((2, 64, 256, 1, 24, 32), 192)]


def direct_shapes():
    """every shape whose rows leave by direct stores (no column sums), each run at both tile-row forms"""
    return [ROUNDS_SHAPE, ROUNDS_TWO_COLUMNS_SHAPE] + COLUMN_SHAPES + DEEP_K_SHAPES + [DEEP_K_RANDOM_SHAPE, LEVEL_SHAPE]


def case_forms():
    """the forms (tile rows, tile columns, lds_out) of program 4 that the causal-conv cases of this file run"""
    forms = {(rows, TILE_N[s[2]], 0) for s in direct_shapes() for rows in TILE_ROWS}
    return forms | {(rows, TILE_N[s[2]], 1) for s, rows in COLSTATS_CASES}


# --------------------------------------------------------------------------------------------------- the causal-conv GEMM
@contextlib.contextmanager
def _tile_rows(rows):
    from lkgd_amd import _lib
    L = _lib.lib()
    L.lkgd_debug_set_wide_tile_m(rows)
    try:
        yield
    finally:
        L.lkgd_debug_set_wide_tile_m(0)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tiles(shape, rows):
    B, Cin, N, T, H, W = shape
    return -(-(B * T * H * W) // rows) * -(-N // TILE_N[N])


def _ints(shape, lo, hi, seed=1):
    """integers in lo..hi: clip, weight, bias and residual rows"""
    B, Cin, N, T, H, W = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = torch.randint(lo, hi + 1, (B, Cin, T, H, W), generator=g).half()
    w = torch.randint(lo, hi + 1, (N, Cin, 3, 3, 3), generator=g).half()
    bias = torch.randint(lo, hi + 1, (N,), generator=g).float()
    res = torch.randint(lo, hi + 1, (B * T * H * W, N), generator=g).half()
    return x, w, bias, res


@functools.lru_cache(maxsize=2)
def _int_case(shape, lo, hi, epilogue):
    """(x, w, bias, res, the fp16 rows F.conv3d gives): computed once per shape, shared by the tile-row forms, never written"""
    B, Cin, N, T, H, W = shape
    x, w, bias, res = _ints(shape, lo, hi)
    if not epilogue:
        bias = res = None
    ref = _conv_ref(x, w, bias).permute(0, 2, 3, 4, 1).reshape(-1, N)
    if res is not None:
        ref = ref + res.float()
    peak = ref.abs().max().item()
    print(f"integer case {shape}: reference |max| {peak:.0f}")
    assert peak < 2048                                   # every sum is an integer fp16 holds exactly
    return x, w, bias, res, ref.half()


@functools.lru_cache(maxsize=2)
def _random_case(shape):
    """the random data, bias and residual of test_cconv3_against_conv3d, and the fp32 reference [B, N, T, H, W]"""
    B, Cin, N, T, H, W = shape
    x, w, bias = _conv_data(shape)
    res = torch.randn(B * T * H * W, N, generator=torch.Generator().manual_seed(9)).half()
    return x, w, bias, res, _conv_ref(x, w, bias) + _rows_to_ncthw(res, B, T, H, W)


def _launch(shape, rows, x, w, bias, res, colstats=0):
    """one causal-conv launch into NaN-poisoned rows, after the plan for this very call was held to the form the case is about"""
    from lkgd_amd import ops
    from lkgd_amd.packing import pack_cconv3
    from test_kernels_gpu import _gemm_as
    B, Cin, N, T, H, W = shape
    M = B * T * H * W
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV)
    form = dict(program=ops.GEMM_WIDE, k_slices=1, tile_m=rows, tile_n=TILE_N[N], lds_out=1 if colstats else 0)
    if colstats:
        form["colstats_block"] = rows
    _gemm_as(ops, form, _prefix(x).to(DEV), pack_cconv3(w).to(DEV), out, M=M, N=N, K=27 * Cin, bias=None if bias is None else bias.to(DEV),
             mode=ops.A_CCONV3, Cin=Cin, cconv=(T, H, W), res1=None if res is None else res.to(DEV), colstats=colstats)
    return out


def _bitwise(got, want, what):
    got, want = got.cpu().view(torch.int16), want.view(torch.int16)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} outputs differ, the first at (row, column) "
                             f"{tuple(bad[0].tolist())}, the last at {tuple(bad[-1].tolist())}")


# (the decorator nearest the function varies slowest: the two tile-row forms of a shape run back to back on one cached reference)
@pytest.mark.parametrize("rows", TILE_ROWS)
@pytest.mark.parametrize("shape", [ROUNDS_SHAPE, ROUNDS_TWO_COLUMNS_SHAPE], ids=["one_column", "two_columns"])
def test_cconv3_many_rounds_per_workgroup_exact(rows, shape):
    """every persistent workgroup runs a second tile and at least one a third: rows re-derived per tile, frames and batch entries
    straddled mid-tile, and at N = 512 successive tiles that differ in both tile indices"""
    tiles = _tiles(shape, rows)
    assert tiles >= 2 * _cus() + 1, f"{tiles} tiles on {_cus()} CUs: no workgroup would run a third tile"
    x, w, _, _, want = _int_case(shape, -2, 2, False)
    with _tile_rows(rows):
        got = _launch(shape, rows, x, w, None, None)
    _bitwise(got, want, f"{shape} at {rows}-row tiles")


@pytest.mark.parametrize("rows", TILE_ROWS)
@pytest.mark.parametrize("shape", COLUMN_SHAPES, ids=lambda s: f"N{s[2]}")
def test_cconv3_tile_columns(rows, shape):
    """a half-empty 256-column tile, two 256-column tiles, 320 columns + a ragged 64, two whole 320-column tiles; ragged last row tile"""
    B, Cin, N, T, H, W = shape
    x, w, bias, res, want = _int_case(shape, -2, 2, True)
    with _tile_rows(rows):
        got = _launch(shape, rows, x, w, bias, res)
    _bitwise(got, want, f"{shape} at {rows}-row tiles, integers")
    x, w, bias, res, ref = _random_case(shape)
    with _tile_rows(rows):
        got = _launch(shape, rows, x, w, bias, res)
    _close(_rows_to_ncthw(got, B, T, H, W), ref, what=f"{shape} at {rows}-row tiles")


@pytest.mark.parametrize("rows", TILE_ROWS)
@pytest.mark.parametrize("shape", DEEP_K_SHAPES, ids=lambda s: f"Cin{s[1]}_N{s[2]}")
def test_cconv3_deep_k_exact(rows, shape):
    """Cin = 256 / 512: four / eight 64-channel chunks per tap, up to 216 K-tiles on the odometer"""
    x, w, _, _, want = _int_case(shape, -1, 1, False)
    with _tile_rows(rows):
        got = _launch(shape, rows, x, w, None, None)
    _bitwise(got, want, f"{shape} at {rows}-row tiles")


@pytest.mark.parametrize("rows", TILE_ROWS)
@pytest.mark.parametrize("shape", [DEEP_K_RANDOM_SHAPE, LEVEL_SHAPE], ids=["Cin512_N512", "one_60x90_frame"])
def test_cconv3_real_widths_against_conv3d(rows, shape):
    B, Cin, N, T, H, W = shape
    x, w, bias, res, ref = _random_case(shape)
    with _tile_rows(rows):
        got = _launch(shape, rows, x, w, bias, res)
    _close(_rows_to_ncthw(got, B, T, H, W), ref, what=f"{shape} at {rows}-row tiles")


@pytest.mark.parametrize("shape,rows", COLSTATS_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"rows{v}")
def test_cconv3_column_sums_past_one_tile(shape, rows):
    """rows through LDS and the epilogue's column sums on several row tiles per sample and more than one tile column: the statistics
    from the sums and those from the read pass against the fp64 mean and rstd of the fp16 rows the launch wrote"""
    from lkgd_amd import ops
    B, Cin, N, T, H, W = shape
    per = T * H * W
    x, w, bias = _conv_data(shape)
    with _tile_rows(rows):
        out = _launch(shape, rows, x, w, bias, None, colstats=per)
        assert getattr(out, "_lkgd_colstats", None) is not None and out._lkgd_colstats[1] == rows
        assert ops._stats_from_cols(out, None, B, per, 1e-6, False) is not None          # (what groupnorm_stats returns below)
        fast = ops.groupnorm_stats(out, None, B, per, 1e-6).cpu()
    slow = ops.groupnorm_stats(out.clone(), None, B, per, 1e-6).cpu()
    v = out.cpu().double().reshape(B, per, 32, N // 32).permute(0, 2, 1, 3).reshape(B, 32, -1)
    mean, var = v.mean(-1), v.var(-1, unbiased=False)
    truth = torch.stack([mean, (var + 1e-6).rsqrt()], dim=-1).float()
    for name, st in (("column sums", fast), ("read pass", slow)):
        err = (st - truth).abs().max().item()
        print(f"{shape} at {rows}-row tiles, statistics from the {name}: max abs error {err:.3e}")
        assert torch.allclose(st, truth, rtol=1e-4, atol=1e-5), name
    _close(_rows_to_ncthw(out, B, T, H, W), _conv_ref(x, w, bias), what=f"colstats launch {shape}")


# ------------------------------------------------------------------------------------------------------ the spatial norm
def _norm_case(C_, Tz, T, sh, H=8, Wd=16, B=2):
    """the recipe of test_cogvideox_vae_gpu._norm_case at f = [B, C, T, 8, 16], zq = [B, 16, Tz, 8 >> sh, 16 >> sh]"""
    torch.manual_seed(C_ + 10 * Tz + T + sh)
    mod = oc.SpatialNorm3D(C_, 16, 32, 1e-6, oc.Switches())
    with torch.no_grad():
        mod.norm_layer.weight.normal_(1.0, 0.3); mod.norm_layer.bias.normal_(0.0, 0.3)
        mod.conv_y.conv.bias.add_(1.0)
        for p in mod.parameters():
            p.copy_(p.half().float())
    f = (torch.randn(B, C_, T, H, Wd) * 1.5 + 0.3).half().float()
    zq = (torch.randn(B, 16, Tz, H >> sh, Wd >> sh) * (1.0 + torch.arange(Tz).float())[None, None, :, None, None]).half().float()
    return mod, f, zq


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("sh", [2, 3])
@pytest.mark.parametrize("C_", [192, 256, 512])
def test_spatial_norm_at_the_decoders_widths(C_, sh, silu):
    """6, 8 and 16 channels per group, the latent grid 4x and 8x coarser.  At C = 192 a group boundary falls inside a thread's 8-channel
    vector (channels 5 | 6 and 17 | 18): those channels are held to the reference each on its own"""
    for Tz, T in NORM_PAIRS:
        mod, f, zq = _norm_case(C_, Tz, T, sh)
        got = _norm_run(mod, f, zq, T, Tz, sh, silu)
        ref = _norm_ref(mod, f, zq, silu)
        r = rel(got, ref)
        print(f"spatial norm C={C_} sh={sh} silu={silu} (Tz, T)=({Tz}, {T}): rel L2 {r:.3e}")
        assert r < 3e-3, (Tz, T, r)
        assert torch.isfinite(got.float()).all()
        if T > 1 and T % 2 == 1 and T != Tz:             # the no-split decoy resizes another way: it must miss
            d = rel(got, _norm_ref(mod, f, zq, silu, no_split=True))
            assert d > 10 * 3e-3, (Tz, T, d)
        if C_ == 192:
            for ch in (5, 6, 17, 18):
                rc = rel(got[:, ch], ref[:, ch])
                assert rc < 3e-3, (Tz, T, ch, rc)


# ------------------------------------------------------------------------------------------------- the encoder's conv_in
def test_pixel_taps_and_gemm_on_the_real_launchs_program():
    """[1, 3, 2, 80, 90] -> 128 channels, 14 400 rows: the program the 480 x 720 launch (M = 8 * 480 * 720) gets on this device, where
    the small-integer test of the encoder file runs the few-row program; exact on integers"""
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import ops
    from test_kernels_gpu import _gemm_as
    B, Cin, T, H, W, N = 1, 3, 2, 80, 90, 128
    g = torch.Generator().manual_seed(8 + T + H + W)
    x = torch.randint(-2, 3, (B, Cin, T, H, W), generator=g).half()
    enc = pv.CogVideoXEncoder3D(pv.CogVAEConfig(block_out_channels=(N, 64, 64, 64), layers_per_block=1))
    with torch.no_grad():
        enc.conv_in.conv.weight.copy_(torch.randint(-2, 3, (N, Cin, 3, 3, 3), generator=g).float())
        enc.conv_in.conv.bias.copy_(torch.randint(-2, 3, (N,), generator=g).float())
    enc = enc.to(DEV)
    enc.pack()
    M, Mreal = B * T * H * W, 8 * 480 * 720
    e = lambda *s: torch.empty(*s, dtype=torch.float16)          # (the plan of CPU tensors reads strides, never memory)
    real = ops.gemm_plan(e(Mreal, 128), e(N, 128), e(Mreal, N), cus=_cus(), M=Mreal, N=N, K=128, bias=torch.empty(N), colstats=Mreal)
    form = {k: getattr(real, k) for k in ("program", "k_slices", "tile_m", "tile_n")}
    print(f"conv_in at 480 x 720 on {_cus()} CUs: {form}")
    taps = torch.full((M, 128), float("nan"), dtype=torch.float16, device=DEV)
    ops.cogvae_pixel_taps(x.to(DEV), 0, T, out=taps)
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device=DEV)
    _gemm_as(ops, form, taps, enc._w_in, out, M=M, N=N, K=128, bias=enc._b_in, colstats=M)
    xp = torch.cat([x[:, :, :1]] * 2 + [x], dim=2).float()
    ref = F.conv3d(xp, enc.conv_in.conv.weight.detach().float().cpu(), enc.conv_in.conv.bias.detach().float().cpu(), padding=(0, 1, 1))
    assert ref.abs().max().item() < 2048
    _bitwise(out, ref.permute(0, 2, 3, 4, 1).reshape(M, N).half(), "conv_in")


# ----------------------------------------------------------------------------------- real-width decode and encode
REAL = oc.CogVAEConfig()
DECODE_T = (1, 3, 5)
ENCODE_T = (1, 5, 9)                 # the oracle's frame batch is 8: nine frames are two frame groups


def _latents(T, h=2, w=3, seed=2):
    """oc.tiny_latents' recipe on an h x w grid"""
    g = torch.Generator().manual_seed(seed + T)
    z = torch.randn(1, 16, T, h, w, generator=g)
    z = z * (1.0 + 2.0 * torch.arange(T, dtype=torch.float32))[None, None, :, None, None]
    return z.half().float()


def _clip(T, H=16, W=24, seed=3):
    """eo.tiny_clip's recipe on an H x W grid"""
    g = torch.Generator().manual_seed(seed + T)
    x = 0.5 * torch.randn(1, 3, T, H, W, generator=g)
    x = x + torch.sin(0.9 * torch.arange(T, dtype=torch.float32))[None, None, :, None, None]
    return x.clamp(-1.0, 1.0).half().float()


def _torch_fp16(o, fn, x):
    """the oracle module itself in torch fp16 on the GPU (torch's own convolutions, not the vendor library's tuned ones: no search)"""
    o16 = copy.deepcopy(o).half().to(DEV)
    was, torch.backends.cudnn.enabled = torch.backends.cudnn.enabled, False
    try:
        return getattr(o16, fn)(x.half().to(DEV)).float().cpu()
    finally:
        torch.backends.cudnn.enabled = was


def _gate(r16):
    return GATE if r16 <= GATE else 2.0 * r16


@pytest.fixture(scope="module")
def real_decoder():
    from lkgd_amd import cogvideox_vae as pv
    assert REAL.block_out_channels == (128, 256, 256, 512) and REAL.layers_per_block == 3
    o = oc.tiny_pair_weights(cfg=REAL)
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**REAL.__dict__))
    m.load_state_dict(o.state_dict())
    return o, m.half().to(DEV)


@pytest.fixture(scope="module")
def real_encoder():
    from lkgd_amd import cogvideox_vae as pv
    o = eo.tiny_weights(cfg=REAL)
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**REAL.__dict__), encoder=True)
    m.load_state_dict(o.state_dict())
    return o, m.half().to(DEV)


@pytest.mark.parametrize("T", DECODE_T)
def test_real_width_decode_against_the_oracle(real_decoder, T):
    o, m = real_decoder
    z = _latents(T)
    truth = o.decode(z)
    got = m.decode(z.half().to(DEV)).sample
    assert tuple(got.shape) == tuple(truth.shape) == (1, 3, {1: 1, 3: 9, 5: 17}[T], 16, 24)
    assert got.dtype == torch.float16 and bool(torch.isfinite(got.float()).all())
    r, r16 = rel(got, truth), rel(_torch_fp16(o, "decode", z), truth)
    print(f"real-width decode T={T}: HIP vs fp32 oracle rel L2 {r:.3e}; torch fp16 vs fp32 oracle {r16:.3e}; gate {_gate(r16):.3e}")
    assert r < _gate(r16), (r, r16)


@pytest.mark.parametrize("T", ENCODE_T)
def test_real_width_encode_against_the_oracle(real_encoder, T):
    o, m = real_encoder
    x = _clip(T)
    truth = o.moments(x)
    dist = m.encode(x.half().to(DEV)).latent_dist
    got = torch.cat([dist.mean.float().cpu(), dist.logvar.float().cpu()], dim=1)
    assert tuple(got.shape) == tuple(truth.shape) == (1, 32, {1: 1, 5: 2, 9: 3}[T], 2, 3)
    assert dist.mean.dtype == torch.float16 and bool(torch.isfinite(got).all())
    r, r16 = rel(got, truth), rel(_torch_fp16(o, "moments", x), truth)
    print(f"real-width encode T={T}: HIP vs fp32 oracle rel L2 of the moments {r:.3e}; torch fp16 vs fp32 oracle {r16:.3e}; "
          f"gate {_gate(r16):.3e}")
    assert r <= _gate(r16), (r, r16)
