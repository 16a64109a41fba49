"""The CogVideoX 3-D causal VAE decoder on the GPU: the causal 3x3x3 A-operand mode of lkgd_gemm_f16 against ``F.conv3d`` (tolerance,
exact integers, causality, the zero-time-padding decoy), ``lkgd_spatial_norm3d`` against the oracle's statement (and the no-split
decoy), both launches on windowed operands, and the tiny decode against tests/cogvideox_vae_oracle.py with its four decoys.

Decoy distances of the tiny decode (relative L2 from the fp32 truth, this oracle, the recipe of ``oc.tiny_pair_weights`` /
``oc.tiny_latents``), measured on the CPU:
    whole clip in one pass   T = 5   0.51          caches dropped   T = 5   0.46
    no first-frame split     T = 3   0.67          T = 5   0.40
    zero time padding, FIRST output frame only   T = 3   1.05     T = 5   0.93     (whole clip at T = 5: 0.050 - below the bar, so
    the first frame is what is measured)
The gate is 1e-2 (the SVD decode's in tests/test_vae.py); every decoy must be >= 10x that from the truth (DECOY_MIN)."""
import pytest
import torch
import torch.nn.functional as F

import cogvideox_vae_oracle as oc
from cogvideox_support import DEV, rel
from footprint import run_case

pytestmark = pytest.mark.gpu

#: every name in lkgd_amd._lib.COGVAE_SYMBOLS -> its footprint tests in this module
FOOTPRINT = {
    "lkgd_spatial_norm3d": ["test_footprint_spatial_norm"],
}

GATE = 1e-2
DECOY_MIN = 10 * GATE


def _close(got, ref, what=""):
    from test_kernels_gpu import _close as c
    c(got, ref, what=what)


# ------------------------------------------------------------------------------------------------------ the convolution
CONV_SHAPES = [(1, 64, 64, 1, 5, 7), (2, 64, 192, 3, 5, 7), (1, 128, 64, 2, 9, 16), (1, 64, 4, 2, 6, 10)]


def _prefix(x, zero=False):
    """[B, C, T, H, W] -> the context-prefixed rows [B*(T+2)*H*W, C] the gather reads (first frame twice; zeros for the decoy)"""
    first = torch.zeros_like(x[:, :, :1]) if zero else x[:, :, :1]
    xp = torch.cat([first, first, x], dim=2)
    return xp.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1]).contiguous()


def _rows_to_ncthw(rows, B, T, H, W):
    return rows.float().cpu().reshape(B, T, H, W, -1).permute(0, 4, 1, 2, 3)


def _cconv(a_rows, w, bias, B, T, H, W, res1=None, out=None):
    from lkgd_amd import ops
    from lkgd_amd.packing import pack_cconv3
    N, Cin = w.shape[:2]
    wp = pack_cconv3(w).to(DEV)
    M = B * T * H * W
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.gemm(a_rows, wp, out, M=M, N=N, K=27 * Cin, bias=None if bias is None else bias.float().to(DEV), mode=ops.A_CCONV3, Cin=Cin,
             cconv=(T, H, W), res1=res1)
    return out


def _conv_data(shape, seed=0, ints=False):
    B, Cin, N, T, H, W = shape
    g = torch.Generator().manual_seed(seed + sum(shape))
    if ints:
        x = torch.randint(-2, 3, (B, Cin, T, H, W), generator=g).half()
        w = torch.randint(-2, 3, (N, Cin, 3, 3, 3), generator=g).half()
        return x, w, None
    x = torch.randn(B, Cin, T, H, W, generator=g).half()
    w = (torch.randn(N, Cin, 3, 3, 3, generator=g) * (27 * Cin) ** -0.5).half()
    return x, w, torch.randn(N, generator=g)


def _conv_ref(x, w, bias, zero=False):
    first = torch.zeros_like(x[:, :, :1]) if zero else x[:, :, :1]
    xp = torch.cat([first, first, x], dim=2).float()
    return F.conv3d(xp, w.float(), bias, padding=(0, 1, 1))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_cconv3_against_conv3d(shape, with_res):
    B, Cin, N, T, H, W = shape
    x, w, bias = _conv_data(shape)
    ref = _conv_ref(x, w, bias)
    res = None
    if with_res:
        res = torch.randn(B * T * H * W, N, generator=torch.Generator().manual_seed(9)).half()
        ref = ref + _rows_to_ncthw(res, B, T, H, W)
    got = _cconv(_prefix(x).to(DEV), w, bias, B, T, H, W, res1=None if res is None else res.to(DEV))
    _close(_rows_to_ncthw(got, B, T, H, W), ref, what=str(shape))
    # the zero-time-padding decoy is somebody else's convolution: it differs from the output on the first frame, and only there
    # where a later frame still sees the chunk's own frames
    decoy = _conv_ref(x, w, bias, zero=True)
    if with_res:
        decoy = decoy + _rows_to_ncthw(res, B, T, H, W)
    g0 = _rows_to_ncthw(got, B, T, H, W)[:, :, 0]
    assert ((g0 - decoy[:, :, 0]).norm() / decoy[:, :, 0].norm()).item() > 0.1
    if T > 2:
        assert torch.allclose(decoy[:, :, 2:], ref[:, :, 2:], atol=1e-5)


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_cconv3_exact_on_small_integers(shape):
    B, Cin, N, T, H, W = shape
    x, w, _ = _conv_data(shape, ints=True)
    ref = _conv_ref(x, w, None)
    assert ref.abs().max().item() < 2048                    # every sum is an integer fp16 holds exactly
    got = _cconv(_prefix(x).to(DEV), w, None, B, T, H, W)
    want = ref.permute(0, 2, 3, 4, 1).reshape(-1, N).half()
    assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def test_cconv3_is_causal():
    shape = (2, 64, 64, 4, 5, 7)
    B, Cin, N, T, H, W = shape
    x, w, bias = _conv_data(shape)
    base = _rows_to_ncthw(_cconv(_prefix(x).to(DEV), w, bias, B, T, H, W), B, T, H, W)
    for t in range(T - 1):
        y = x.clone()
        y[:, :, t + 1] += 1.0
        got = _rows_to_ncthw(_cconv(_prefix(y).to(DEV), w, bias, B, T, H, W), B, T, H, W)
        assert torch.equal(got[:, :, :t + 1], base[:, :, :t + 1]), t
        assert not torch.equal(got[:, :, t + 1], base[:, :, t + 1]), t


def test_cconv3_cache_context_equals_the_whole_clip():
    """the second chunk over (last two frames of the first chunk's buffer | its own frames) = the whole clip's convolution, bit for bit"""
    shape = (1, 64, 64, 5, 6, 10)
    B, Cin, N, T, H, W = shape
    x, w, bias = _conv_data(shape)
    whole = _cconv(_prefix(x).to(DEV), w, bias, B, T, H, W).reshape(T, H * W, N)
    second = x[:, :, 1:].permute(0, 2, 3, 4, 1).reshape(-1, Cin).contiguous().to(DEV)      # frames 1, 2 = the cache; 3, 4 = the chunk
    got = _cconv(second, w, bias, B, 2, H, W).reshape(2, H * W, N)
    assert torch.equal(got, whole[3:])


def test_cconv3_colstats_feed_the_groupnorm_statistics():
    """N = 256 on whole 256-row tiles: the epilogue's column sums give the statistics the read pass gives"""
    from lkgd_amd import ops
    from lkgd_amd.packing import pack_cconv3
    B, Cin, N, T, H, W = 1, 64, 256, 2, 16, 16
    x, w, bias = _conv_data((B, Cin, N, T, H, W))
    M = B * T * H * W
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.gemm(_prefix(x).to(DEV), pack_cconv3(w).to(DEV), out, M=M, N=N, K=27 * Cin, bias=bias.to(DEV), mode=ops.A_CCONV3, Cin=Cin,
             cconv=(T, H, W), colstats=M)
    assert getattr(out, "_lkgd_colstats", None) is not None
    fast = ops.groupnorm_stats(out, None, B, M, 1e-6).cpu()
    slow = ops.groupnorm_stats(out.clone(), None, B, M, 1e-6).cpu()
    assert torch.allclose(fast, slow, rtol=1e-4, atol=1e-5)
    _close(_rows_to_ncthw(out, B, T, H, W), _conv_ref(x, w, bias), what="colstats launch")


# ----------------------------------------------------------------------------------------------------- the spatial norm
NORM_PAIRS = [(1, 1), (2, 2), (2, 8), (3, 3), (3, 5), (3, 9)]


def _norm_case(C_, Tz, T, sh, seed=0, B=2):
    """inputs of one spatial norm at f = [B, C, T, 6, 10], zq = [B, 16, Tz, 6 >> sh, 10 >> sh] + the oracle module (fp16 values)"""
    torch.manual_seed(seed + C_ + 10 * Tz + T + sh)
    mod = oc.SpatialNorm3D(C_, 16, 32, 1e-6, oc.Switches())
    with torch.no_grad():
        mod.norm_layer.weight.normal_(1.0, 0.3); mod.norm_layer.bias.normal_(0.0, 0.3)
        mod.conv_y.conv.bias.add_(1.0)
        for p in mod.parameters():
            p.copy_(p.half().float())
    f = (torch.randn(B, C_, T, 6, 10) * 1.5 + 0.3).half().float()
    zq = (torch.randn(B, 16, Tz, 6 >> sh, 10 >> sh) * (1.0 + torch.arange(Tz).float())[None, None, :, None, None]).half().float()
    return mod, f, zq


def _norm_run(mod, f, zq, T, Tz, sh, silu, W=None):
    """the kernel on (f, zq): conv_y | conv_b on the latent grid in torch fp32 -> fp16 rows, statistics by lkgd_groupnorm_stats"""
    from lkgd_amd import ops
    from lkgd_amd.cogvideox_vae import spatial_norm_tmap
    B, C_ = f.shape[:2]
    H, Wd = f.shape[-2:]
    rows = f.permute(0, 2, 3, 4, 1).reshape(-1, C_).half()
    zr = zq.permute(0, 2, 3, 4, 1).reshape(-1, 16)
    wyb = torch.cat([mod.conv_y.conv.weight.reshape(C_, 16), mod.conv_b.conv.weight.reshape(C_, 16)])
    yb = (zr @ wyb.t() + torch.cat([mod.conv_y.conv.bias, mod.conv_b.conv.bias])).detach().half()
    tmap = torch.tensor(spatial_norm_tmap(Tz, T), dtype=torch.int32)
    if W is None:
        fr, ybr, out = rows.to(DEV), yb.to(DEV), torch.empty(rows.shape, dtype=torch.float16, device=DEV)
    else:
        fr, ybr, out = W.inp(rows, name="f"), W.inp(yb, name="yb"), W.out(rows.shape[0], C_, name="out")
    stats = ops.groupnorm_stats(fr, None, B, T * H * Wd, 1e-6)
    ops.spatial_norm3d(fr, stats, mod.norm_layer.weight.detach().float().to(DEV), mod.norm_layer.bias.detach().float().to(DEV), ybr,
                       tmap.to(DEV), out, B, T, H, Wd, Tz, sh, silu)
    return out


def _norm_ref(mod, f, zq, silu, no_split=False):
    mod.sw.no_split = no_split
    with torch.no_grad():
        y = mod(f, zq)
    mod.sw.no_split = False
    y = F.silu(y) if silu else y
    return y.permute(0, 2, 3, 4, 1).reshape(-1, f.shape[1])


@pytest.mark.parametrize("silu", [True, False])
@pytest.mark.parametrize("sh", [0, 1])
@pytest.mark.parametrize("C_", [64, 128])
def test_spatial_norm_against_the_oracles_statement(C_, sh, silu):
    for Tz, T in NORM_PAIRS:
        mod, f, zq = _norm_case(C_, Tz, T, sh)
        got = _norm_run(mod, f, zq, T, Tz, sh, silu)
        r = rel(got, _norm_ref(mod, f, zq, silu))
        print(f"spatial norm C={C_} sh={sh} silu={silu} (Tz, T)=({Tz}, {T}): rel L2 {r:.3e}")
        assert r < 3e-3, (Tz, T, r)
        assert torch.isfinite(got.float()).all()
        if T > 1 and T % 2 == 1 and T != Tz:             # the no-split decoy resizes another way: it must miss
            d = rel(got, _norm_ref(mod, f, zq, silu, no_split=True))
            assert d > 10 * 3e-3, (Tz, T, d)


def test_spatial_norm_writes_into_a_prefixed_buffer():
    """output rows at a frame offset: behind the two context frames of every batch entry, and nowhere else"""
    from lkgd_amd import ops
    from lkgd_amd.cogvideox_vae import spatial_norm_tmap
    C_, Tz, T, sh, B, H, Wd = 64, 3, 5, 1, 2, 6, 10
    mod, f, zq = _norm_case(C_, Tz, T, sh)
    compact = _norm_run(mod, f, zq, T, Tz, sh, True)
    rows = f.permute(0, 2, 3, 4, 1).reshape(-1, C_).half().to(DEV)
    zr = zq.permute(0, 2, 3, 4, 1).reshape(-1, 16)
    wyb = torch.cat([mod.conv_y.conv.weight.reshape(C_, 16), mod.conv_b.conv.weight.reshape(C_, 16)])
    yb = (zr @ wyb.t() + torch.cat([mod.conv_y.conv.bias, mod.conv_b.conv.bias])).detach().half().to(DEV)
    hw = H * Wd
    P = torch.full((B, T + 2, hw, C_), 7.0, dtype=torch.float16, device=DEV)
    stats = ops.groupnorm_stats(rows, None, B, T * hw, 1e-6)
    ops.spatial_norm3d(rows, stats, mod.norm_layer.weight.detach().float().to(DEV), mod.norm_layer.bias.detach().float().to(DEV), yb,
                       torch.tensor(spatial_norm_tmap(Tz, T), dtype=torch.int32).to(DEV), P.view(-1, C_)[2 * hw:], B, T, H, Wd, Tz, sh,
                       True, out_batch_rows=(T + 2) * hw)
    assert torch.equal(P[:, 2:].reshape(-1, C_), compact)
    assert bool((P[:, :2] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ footprint
def test_footprint_cconv3():
    for shape, with_res in (((2, 64, 192, 3, 5, 7), True), ((1, 64, 4, 2, 6, 10), False)):
        B, Cin, N, T, H, W = shape
        x, w, bias = _conv_data(shape)
        res = torch.randn(B * T * H * W, N, generator=torch.Generator().manual_seed(4)).half()
        ref = _conv_ref(x, w, bias).permute(0, 2, 3, 4, 1).reshape(-1, N) + (res.float() if with_res else 0.0)

        def case(Wn):
            a = Wn.inp(_prefix(x), name="a0")
            r = Wn.inp(res, pad=8 if N % 8 == 0 else 4, name="res1") if with_res else None
            out = Wn.out(B * T * H * W, N, pad=8 if N % 8 == 0 else 4, name="out")
            _cconv(a, w, bias, B, T, H, W, res1=r, out=out)
            return {"out": out}

        run_case(case, DEV, lambda: {"out": ref}, lambda g, r, n: _close(g, r, what=n), True, sync=torch.cuda.synchronize)


def test_footprint_spatial_norm():
    for C_, Tz, T, sh, silu in ((64, 3, 5, 1, True), (128, 2, 8, 0, False)):
        mod, f, zq = _norm_case(C_, Tz, T, sh)
        ref = _norm_ref(mod, f, zq, silu)

        def close(g, r, n):
            assert rel(g, r) < 3e-3, n

        run_case(lambda Wn: {"out": _norm_run(mod, f, zq, T, Tz, sh, silu, W=Wn)}, DEV, lambda: {"out": ref}, close, True,
                 sync=torch.cuda.synchronize)


# ---------------------------------------------------------------------------------------------------------- tiny decode
@pytest.fixture(scope="module")
def pair():
    """(fp32 oracle, HIP twin on the GPU) with the recipe's weights; the truth of every T is computed once"""
    from lkgd_amd import cogvideox_vae as pv
    o = oc.tiny_pair_weights()
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**oc.TINY.__dict__))
    m.load_state_dict(o.state_dict())
    m = m.half().to(DEV)
    truth = {T: o.decode(oc.tiny_latents(T)) for T in (1, 2, 3, 5)}
    return o, m, truth


@pytest.mark.parametrize("T", [1, 2, 3, 5])
def test_tiny_decode_against_the_oracle_and_its_decoys(pair, T):
    o, m, truth = pair
    z, t = oc.tiny_latents(T), truth[T]
    got = m.decode(z.half().to(DEV)).sample
    assert tuple(got.shape) == tuple(t.shape) == (1, 3, {1: 1, 2: 8, 3: 9, 5: 17}[T], 48, 80)
    assert got.dtype == torch.float16 and bool(torch.isfinite(got.float()).all())
    r = rel(got, t)
    print(f"tiny decode T={T}: HIP vs oracle rel L2 {r:.3e}")
    assert r < GATE, r
    decoys = {}
    if T >= 3:
        decoys["no split"] = (oc.with_switches(o, no_split=True).decode(z), slice(None))
        decoys["zero time padding (first frame)"] = (oc.with_switches(o, zero_time_pad=True).decode(z), slice(0, 1))
    if T == 5:                      # at T <= 3 there is one chunk: the chunk decoys are the truth itself
        decoys["whole clip in one pass"] = (o.decode(z, whole=True), slice(None))
        decoys["caches dropped"] = (oc.with_switches(o, drop_cache=True).decode(z), slice(None))
    for name, (d, fr) in decoys.items():
        dist, hip = rel(d[:, :, fr], t[:, :, fr]), rel(got[:, :, fr], t[:, :, fr])
        print(f"  decoy {name}: {dist:.3f} from the truth; HIP {hip:.3e}")
        assert dist >= DECOY_MIN, (name, dist)
        assert hip < GATE, (name, hip)
    assert T != 5 or len(decoys) == 4


def test_decode_latents_and_pretrained_round_trip(pair, tmp_path):
    from lkgd_amd import cogvideox_vae as pv
    o, m, _ = pair
    lat = oc.tiny_latents(3).permute(0, 2, 1, 3, 4).contiguous().half().to(DEV)              # [B, T, 16, h, w]
    a = pv.decode_latents(m, lat)
    b = m.decode((1 / m.config.scaling_factor * lat.permute(0, 2, 1, 3, 4))).sample
    assert torch.equal(a, b)
    assert rel(a, oc.decode_latents(o, lat.float().cpu())) < GATE
    m.save_pretrained(str(tmp_path / "vae"))
    m2 = pv.AutoencoderKLCogVideoX.from_pretrained(str(tmp_path), subfolder="vae", torch_dtype=torch.float16).to(DEV)
    assert torch.equal(pv.decode_latents(m2, lat), a)
    assert m.decode(lat.permute(0, 2, 1, 3, 4), return_dict=False)[0].shape == a.shape


def test_batch_of_two_equals_two_single_decodes(pair):
    """Every batch entry is normalised and convolved on its own, so B = 2 is two B = 1 decodes - up to the ORDER of fp32 sums: the
    GroupNorm statistics pass sizes its row chunks by the sample count and the few-row GEMMs cut K by the row count, so a sum may
    round differently in its last fp32 bit, which can move an fp16 rounding by one ulp somewhere downstream.  The bound is therefore
    one fp16 ulp in relative L2 (2^-10; a wrong batch stride, cache or statistic would be O(1)), and the entries must not be
    swapped: each is far from the other's decode."""
    o, m, _ = pair
    z = torch.cat([oc.tiny_latents(5), oc.tiny_latents(5, seed=11)]).half().to(DEV)
    both = m.decode(z).sample
    assert tuple(both.shape) == (2, 3, 17, 48, 80)
    ones = [m.decode(z[i:i + 1]).sample for i in range(2)]
    for i in range(2):
        r = rel(both[i:i + 1], ones[i])
        print(f"B = 2 entry {i} vs its B = 1 decode: rel L2 {r:.3e}")
        assert r < 2.0 ** -10, (i, r)
        assert rel(both[i:i + 1], ones[1 - i]) > DECOY_MIN
        assert rel(both[i:i + 1], o.decode(z[i:i + 1].float().cpu())) < GATE
