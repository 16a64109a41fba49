"""The CogVideoX 3-D causal VAE encoder on the GPU: ``lkgd_cogvae_pixel_taps`` against a torch gather of its statement (and, with the
GEMM behind it, against ``F.conv3d``), ``lkgd_cogvae_time_pool`` against ``avg_pool1d``, ``lkgd_cogvae_posterior`` against its fp32
statement, all three on windowed operands, the tiny encode against tests/cogvideox_vae_encoder_oracle.py with its six decoys, and
``prepare_latents`` -> ``denoise`` end to end.

Decoy distances of the tiny encode (relative L2 of the moments from the fp32 truth, this oracle, the recipe of ``eo.tiny_weights`` /
``eo.tiny_clip``), measured on the CPU:
    T                     1      2      5      9      16     17     25
    zero_time_pad         1.06   1.10   1.10   1.08   1.17   1.20   1.15
    pad_symmetric         1.20   1.19   1.21   1.20   1.15   1.18   1.20
    pool_split_last       =      =      0.70   0.77   =      0.75   0.75
    drop_cache            =      =      =      =      0.84   0.76   0.90
    remainder_last        =      =      =      =      =      0.77   0.81
    whole                 =      =      =      =      0.38   0.26   0.38
The gate is 1e-2 (the decoder's and T5's: fp16 activations, fp32 accumulation); every decoy that differs at a T must lie at least
10x that from the HIP result (DECOY_MIN)."""
import pytest
import torch
import torch.nn.functional as F

import cogvideox_vae_encoder_oracle as eo
from cogvideox_support import DEV, DIT_SEED, rel, tiny_cpu_model
from footprint import run_case

pytestmark = pytest.mark.gpu

GATE = 1e-2
DECOY_MIN = 10 * GATE

#: every name in lkgd_amd._lib.COGVAE_ENC_SYMBOLS -> its footprint tests in this module
FOOTPRINT = {
    "lkgd_cogvae_pixel_taps": ["test_footprint_pixel_taps"],
    "lkgd_cogvae_time_pool": ["test_footprint_time_pool"],
    "lkgd_cogvae_posterior": ["test_footprint_posterior"],
}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------- pixel taps
TAP_CASES = [(1, 3, 1, 8, 8, 0, 1), (2, 3, 5, 6, 10, 0, 5), (1, 3, 9, 6, 10, 3, 4), (1, 4, 3, 5, 7, 1, 2), (1, 1, 2, 8, 8, 0, 2)]


def _clip(B, Cin, T, H, W, seed=0, ints=False):
    g = torch.Generator().manual_seed(seed + B + 3 * Cin + 5 * T + 7 * H + 11 * W)
    if ints:
        return torch.randint(-2, 3, (B, Cin, T, H, W), generator=g).half()
    return torch.randn(B, Cin, T, H, W, generator=g).half()


def _taps_ref(x, t0, Tc):
    """the statement of include/lkgd_hip_cogvae_enc.h as a torch gather: fp16 [B*Tc*H*W, 128]"""
    B, Cin, T, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))                                    # zeros outside the image
    out = torch.zeros(B, Tc, H, W, 128, dtype=torch.float16)
    for kt in range(3):
        ts = (t0 + torch.arange(Tc) + kt - 2).clamp(min=0)         # frame 0 replicated in front of the clip
        for ky in range(3):
            for kx in range(3):
                k = ((kt * 3 + ky) * 3 + kx) * Cin
                out[..., k:k + Cin] = xp[:, :, ts, ky:ky + H, kx:kx + W].permute(0, 2, 3, 4, 1)
    return out.reshape(-1, 128)


def _taps(x_dev, t0, Tc, out=None):
    from lkgd_amd import ops
    B, _, _, H, W = x_dev.shape
    if out is None:
        out = torch.full((B * Tc * H * W, 128), float("nan"), dtype=torch.float16, device=DEV)
    return ops.cogvae_pixel_taps(x_dev, t0, Tc, out=out)


@pytest.mark.parametrize("case", TAP_CASES)
def test_pixel_taps_equal_the_gather(case):
    B, Cin, T, H, W, t0, Tc = case
    x = _clip(B, Cin, T, H, W)
    got = _taps(x.to(DEV), t0, Tc)
    want = _taps_ref(x, t0, Tc)
    assert torch.equal(_bits(got), _bits(want))
    assert bool((got[:, 27 * Cin:] == 0).all())                    # the columns behind the taps are written, as zeros


def test_pixel_taps_later_chunk_reads_its_context_from_the_clip():
    """t0 > 0 gives the rows the whole clip's launch gives at those frames: conv_in's cache is the clip"""
    B, Cin, T, H, W, t0, Tc = 1, 3, 9, 6, 10, 3, 4
    x = _clip(B, Cin, T, H, W).to(DEV)
    whole = _taps(x, 0, T).view(T, H * W, 128)
    part = _taps(x, t0, Tc).view(Tc, H * W, 128)
    assert torch.equal(part, whole[t0:t0 + Tc])
    assert not torch.equal(part[0], _taps(x[:, :, t0:].contiguous(), 0, Tc).view(Tc, H * W, 128)[0])      # not its own first frame


def test_pixel_taps_and_gemm_equal_conv3d_on_small_integers():
    """taps + one plain GEMM (the weight packed by the encoder's own ``pack``) = F.conv3d over the clip with its first frame twice in
    front: exact, every sum an integer fp16 holds"""
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import ops
    B, Cin, T, H, W, N = 1, 3, 5, 16, 24, 64
    x = _clip(B, Cin, T, H, W, ints=True)
    enc = pv.CogVideoXEncoder3D(pv.CogVAEConfig(**eo.TINY.__dict__))
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        enc.conv_in.conv.weight.copy_(torch.randint(-2, 3, (N, Cin, 3, 3, 3), generator=g).float())
        enc.conv_in.conv.bias.copy_(torch.randint(-2, 3, (N,), generator=g).float())
    enc = enc.to(DEV)
    enc.pack()
    M = B * T * H * W
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.gemm(_taps(x.to(DEV), 0, T), enc._w_in, out, M=M, N=N, K=128, bias=enc._b_in, colstats=M)
    xp = torch.cat([x[:, :, :1]] * 2 + [x], dim=2).float()
    ref = F.conv3d(xp, enc.conv_in.conv.weight.detach().float().cpu(), enc.conv_in.conv.bias.detach().float().cpu(), padding=(0, 1, 1))
    assert ref.abs().max().item() < 2048
    want = ref.permute(0, 2, 3, 4, 1).reshape(M, N).half()
    assert torch.equal(_bits(out), _bits(want))
    if getattr(out, "_lkgd_colstats", None) is not None:          # the column sums feed the first GroupNorm
        fast = ops.groupnorm_stats(out, None, B, M, 1e-6).cpu()
        slow = ops.groupnorm_stats(out.clone(), None, B, M, 1e-6).cpu()
        assert torch.allclose(fast, slow, rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------ time pool
def _pool_data(B, T, HW, C_, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * B + 10 * T + HW + C_)
    return (torch.randn(B * T * HW, C_, generator=g) * 3.0).half()


def _pool_ref(rows, B, T, HW):
    """fp32 avg_pool1d of the fp16 values as diffusers writes it, then rounded"""
    C_ = rows.shape[1]
    x = rows.float().view(B, T, HW, 1, C_).permute(0, 4, 1, 2, 3)                    # [B, C, T, HW, 1]
    y = eo.time_pool(x)
    return y.permute(0, 2, 3, 4, 1).reshape(-1, C_).half()


@pytest.mark.parametrize("shape", [(2, 15, 64), (1, 7, 128)])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 9])
def test_time_pool_exact_against_avg_pool1d(T, shape):
    from lkgd_amd import ops
    B, HW, C_ = shape
    rows = _pool_data(B, T, HW, C_)
    got = ops.cogvae_time_pool(rows.to(DEV), B, T, HW)
    want = _pool_ref(rows, B, T, HW)
    assert tuple(got.shape) == tuple(want.shape) == (B * ops.pooled_frames(T) * HW, C_)
    assert torch.equal(_bits(got), _bits(want))


def test_time_pool_row_stride_wider_than_the_channels():
    from lkgd_amd import ops
    B, T, HW, C_ = 2, 5, 15, 64
    rows = _pool_data(B, T, HW, C_)
    wide = torch.full((B * T * HW, C_ + 24), float("nan"), dtype=torch.float16, device=DEV)
    wide[:, 8:8 + C_] = rows.to(DEV)
    orows = B * ops.pooled_frames(T) * HW
    owide = torch.full((orows, C_ + 8), 7.0, dtype=torch.float16, device=DEV)
    ops.cogvae_time_pool(wide[:, 8:8 + C_], B, T, HW, out=owide[:, :C_])
    assert torch.equal(_bits(owide[:, :C_]), _bits(_pool_ref(rows, B, T, HW)))
    assert bool((owide[:, C_:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ posterior
LC = 16
POST_GEOS = [(1, 1, 6, 10), (2, 3, 4, 6)]


def _post_data(geo, ld, seed=0):
    """moment rows with log-variance columns 0 / 5 / 9 set to -40 / 0 / 30 (both clamps bite), |noise| within [0.05, 2] so that
    exp(10) * noise stays an fp16 number.  The mean (|mean| >= 0.1) and the noise of an element share a random sign: the sum
    mean + std * noise then never cancels.  One fp16 ulp of a CANCELLED sum would lie below the fp32 precision of its two terms - no
    fp32 evaluation, the reference's included, could be held to it."""
    B, T, h, w = geo
    g = torch.Generator().manual_seed(seed + B + 10 * T + ld)
    rows = B * T * h * w
    mom = torch.randn(rows, ld, generator=g)
    sign = torch.where(torch.rand(rows, LC, generator=g) < 0.5, -1.0, 1.0)
    mom[:, :LC] = sign * (mom[:, :LC].abs() + 0.1)
    mom[:, LC + 0], mom[:, LC + 5], mom[:, LC + 9] = -40.0, 0.0, 30.0
    noise = sign * (0.05 + 1.95 * torch.rand(rows, LC, generator=g))
    noise = noise.view(B, T, h, w, LC).permute(0, 4, 1, 2, 3).contiguous()
    return mom.half(), noise.half()


def _post_ref(mom, noise, geo, scale):
    """the fp32 statement: (mean, sample) [B, lc, T, h, w]"""
    B, T, h, w = geo
    m = mom.float().view(B, T, h, w, -1).permute(0, 4, 1, 2, 3)
    mean, logvar = m[:, :LC], torch.clamp(m[:, LC:2 * LC], -30.0, 20.0)
    return mean, scale * (mean + torch.exp(0.5 * logvar) * noise.float())


def _one_ulp(got, ref, what=""):
    """|got - ref| within one fp16 ulp of ref (ref fp32): 2^(e - 10) for a normal |ref| in [2^e, 2^(e+1)), 2^-24 below 2^-14"""
    ref = ref.float().cpu()
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14)))
    ulp = torch.exp2(e - 10)
    err = (got.float().cpu() - ref).abs()
    assert bool(torch.isfinite(got.float()).all()), what
    assert bool((err <= ulp).all()), (what, float((err / ulp).max()))


@pytest.mark.parametrize("ld", [32, 40])
@pytest.mark.parametrize("scale", [1.0, 0.7, 1 / 1.15258426])
@pytest.mark.parametrize("geo", POST_GEOS)
def test_posterior_against_the_fp32_statement(geo, scale, ld):
    from lkgd_amd import ops
    B, T, h, w = geo
    mom, noise = _post_data(geo, ld)
    rmean, rsample = _post_ref(mom, noise, geo, scale)
    assert rsample.abs().max().item() < 60000.0 and (rsample.abs() > 1000.0).any()          # exp(10) is reached and fp16 holds it
    mean, sample = ops.cogvae_posterior(mom.to(DEV), B, LC, T, h, w, noise=noise.to(DEV), scale=scale)
    assert torch.equal(_bits(mean), _bits(rmean.half()))                                   # the mean is a copy
    _one_ulp(sample, rsample, "sample")
    # clamps: the -40 column has std exp(-15), the 30 column std exp(10)
    s = sample.float().cpu()
    _one_ulp(s[:, 0], scale * (rmean[:, 0] + 3.059e-7 * noise[:, 0].float()), "low clamp")
    assert not torch.allclose(s[:, 9], scale * (rmean[:, 9] + 3269017.0 * noise[:, 9].float()), rtol=0.5)      # exp(15) unclamped: no
    # without noise: the mean only, `sample` untouched (none is allocated)
    mean2, none = ops.cogvae_posterior(mom.to(DEV), B, LC, T, h, w)
    assert none is None and torch.equal(mean2, mean)


# ------------------------------------------------------------------------------------------------------------ footprint
def _exact(got, ref, what):
    assert torch.equal(_bits(got), _bits(ref)), what


def test_footprint_pixel_taps():
    for B, Cin, T, H, W, t0, Tc in ((2, 3, 5, 6, 10, 1, 3), (1, 4, 3, 5, 7, 0, 3)):
        x = _clip(B, Cin, T, H, W)
        want = _taps_ref(x, t0, Tc)

        def case(Wn):
            # the clip's strides are fixed by the entry point: guard rows around it, no gaps
            xw = Wn.inp(x.reshape(-1, W), pad=0, gap=False, name="x")
            xw = xw.view(B, Cin, T, H, W)
            out = Wn.out(B * Tc * H * W, 128, name="out")
            from lkgd_amd import ops
            ops.cogvae_pixel_taps(xw, t0, Tc, out=out)
            return {"out": out}

        run_case(case, DEV, lambda: {"out": want}, _exact, True, sync=torch.cuda.synchronize)


def test_footprint_time_pool():
    from lkgd_amd import ops
    for B, T, HW, C_ in ((2, 5, 15, 64), (1, 4, 7, 128)):
        rows = _pool_data(B, T, HW, C_)
        want = _pool_ref(rows, B, T, HW)

        def case(Wn):
            out = Wn.out(B * ops.pooled_frames(T) * HW, C_, name="out")
            ops.cogvae_time_pool(Wn.inp(rows, name="in"), B, T, HW, out=out)
            return {"out": out}

        run_case(case, DEV, lambda: {"out": want}, _exact, True, sync=torch.cuda.synchronize)


def test_footprint_posterior():
    from lkgd_amd import _lib
    for geo, with_noise in (((2, 3, 4, 6), True), ((1, 1, 6, 10), False)):
        B, T, h, w = geo
        mom, noise = _post_data(geo, 32)
        rmean, rsample = _post_ref(mom, noise, geo, 0.7)
        thw = T * h * w

        def case(Wn):
            # the planar tensors are contiguous by contract: [B*lc, T*h*w] windows without gaps, guard rows around them
            mw = Wn.inp(mom, name="mom")
            nz = Wn.inp(noise.reshape(B * LC, thw), pad=0, gap=False, name="noise") if with_noise else None
            mean = Wn.out(B * LC, thw, pad=0, gap=False, name="mean")
            sample = Wn.out(B * LC, thw, pad=0, gap=False, name="sample") if with_noise else None
            rc = _lib.lib().lkgd_cogvae_posterior(mw.data_ptr(), mw.stride(0), nz.data_ptr() if with_noise else None, mean.data_ptr(),
                                                  sample.data_ptr() if with_noise else None, 0.7, B, LC, T, h, w,
                                                  torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            return {"mean": mean, "sample": sample} if with_noise else {"mean": mean}

        def close(g, r, n):
            if n.startswith("mean"):
                _exact(g, r.half(), n)
            else:
                _one_ulp(g, r, n)

        refs = {"mean": rmean.reshape(B * LC, thw)}
        if with_noise:
            refs["sample"] = rsample.reshape(B * LC, thw)
        run_case(case, DEV, lambda: refs, close, True, sync=torch.cuda.synchronize)


# ---------------------------------------------------------------------------------------------------------- tiny encode
FORWARD_T = (1, 2, 5, 9, 17)


@pytest.fixture(scope="module")
def pair():
    """(fp32 oracle, HIP twin on the GPU) with the recipe's weights; the truth of every T is computed once"""
    from lkgd_amd import cogvideox_vae as pv
    o = eo.tiny_weights()
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**eo.TINY.__dict__), encoder=True)
    m.load_state_dict(o.state_dict())
    m = m.half().to(DEV)
    truth = {T: o.moments(eo.tiny_clip(T)) for T in FORWARD_T}
    return o, m, truth


def _moments_of(dist):
    return torch.cat([dist.mean.float().cpu(), dist.logvar.float().cpu()], dim=1)


@pytest.mark.parametrize("T", FORWARD_T)
def test_tiny_encode_against_the_oracle_and_its_decoys(pair, T):
    o, m, truth = pair
    x, t = eo.tiny_clip(T), truth[T]
    out = m.encode(x.half().to(DEV))
    dist = out.latent_dist
    assert out[0] is dist and m.encode(x.half().to(DEV), return_dict=False)[0].mean.shape == dist.mean.shape
    Tl = {1: 1, 2: 1, 5: 2, 9: 3, 17: 5}[T]
    assert tuple(dist.mean.shape) == tuple(dist.logvar.shape) == tuple(dist.std.shape) == (1, 16, Tl, 6, 10)
    assert dist.mean.dtype == torch.float16 and dist.mode() is dist.mean
    got = _moments_of(dist)
    assert tuple(got.shape) == tuple(t.shape) and bool(torch.isfinite(got).all())
    r = rel(got, t)
    print(f"tiny encode T={T}: HIP vs oracle rel L2 of the moments {r:.3e}")
    assert r <= GATE, r
    assert rel(dist.std, torch.exp(0.5 * t[:, 16:])) <= GATE
    n = 0
    for name, where in eo.DECOYS.items():
        if T in where["differs"]:
            d = rel(got, eo.decoy_moments(o, name, x))
            print(f"  decoy {name}: HIP result {d:.3f} away")
            assert d >= DECOY_MIN, (name, d)
            n += 1
    assert n == {1: 2, 2: 2, 5: 3, 9: 3, 17: 6}[T]


def test_batch_of_two_equals_two_single_encodes_bitwise(pair):
    o, m, _ = pair
    x = torch.cat([eo.tiny_clip(9), eo.tiny_clip(9, seed=11)]).half().to(DEV)
    both = m.encode(x).latent_dist
    assert tuple(both.mean.shape) == (2, 16, 3, 6, 10)
    for i in range(2):
        one = m.encode(x[i:i + 1]).latent_dist
        assert torch.equal(both.mean[i:i + 1], one.mean) and torch.equal(both.logvar[i:i + 1], one.logvar), i
    assert rel(both.mean[0], both.mean[1]) > DECOY_MIN                # and the entries are not one another
    assert rel(_moments_of(both)[1:], o.moments(x[1:].float().cpu())) <= GATE


def test_sample_draws_like_dpm_noise_and_equals_the_oracles(pair):
    """a seeded CPU generator: the sample is the oracle's mean + std * noise for the same draw, and the generator is left where one
    randn of mean.shape leaves it"""
    o, m, _ = pair
    x = eo.tiny_clip(5)
    dist = m.encode(x.half().to(DEV)).latent_dist
    g = torch.Generator().manual_seed(1234)
    s = dist.sample(g)
    ref_g = torch.Generator().manual_seed(1234)
    noise = torch.randn(tuple(dist.mean.shape), generator=ref_g, dtype=torch.float16)
    assert torch.equal(g.get_state(), ref_g.get_state())
    assert s.dtype == torch.float16 and s.device == dist.mean.device and tuple(s.shape) == tuple(dist.mean.shape)
    mean, _, std = o.posterior(x)
    r = rel(s, mean + std * noise.float())
    print(f"sample vs the oracle's mean + std * noise: rel L2 {r:.3e}")
    assert r <= GATE, r
    assert rel(s, mean) > DECOY_MIN                                   # the noise took part
    # scale folds into the same launch
    s7 = dist.sample(torch.Generator().manual_seed(1234), scale=0.7)
    assert rel(s7, 0.7 * (mean + std * noise.float())) <= GATE
    # a device generator draws on the device
    gd = torch.Generator(device=DEV).manual_seed(5)
    assert dist.sample(gd).device == dist.mean.device


# ----------------------------------------------------------------------------------------------------------- end to end
def test_decode_of_encode_has_the_clips_shape(pair):
    _, m, _ = pair
    x = eo.tiny_clip(9).half().to(DEV)
    y = m.decode(m.encode(x).latent_dist.mode()).sample
    assert tuple(y.shape) == tuple(x.shape) and bool(torch.isfinite(y.float()).all())


def test_prepare_latents_feeds_denoise(pair):
    from lkgd_amd import cogvideox as pc
    o, m, _ = pair
    image = eo.tiny_clip(1)[:, :, 0].half().to(DEV)                                   # [1, 3, 48, 80]
    dit = tiny_cpu_model(seed=DIT_SEED, sample_height=6, sample_width=10).half().to(DEV)
    sched = pc.CogVideoXDDIMScheduler()
    g = torch.Generator().manual_seed(77)
    lat, img = pc.prepare_latents(m, sched, dit.config, image, batch_size=1, num_channels_latents=16, num_frames=9, height=48, width=80,
                                  dtype=torch.float16, device=DEV, generator=g)
    assert tuple(lat.shape) == tuple(img.shape) == (1, 3, 16, 6, 10)
    assert lat.dtype == img.dtype == torch.float16 and lat.device == img.device == m.device
    # the first frame is scaling_factor * sample (the same draw), the rest zero; the latents are the generator's next draw
    ref_g = torch.Generator().manual_seed(77)
    sample = m.encode(image[:, :, None]).latent_dist.sample(ref_g)
    sf = m.config.scaling_factor
    assert rel(img[:, 0], sf * sample[:, :, 0].float()) < 2.0 ** -10                   # one rounding apart: the scale is in the launch
    mean, _, std = o.posterior(eo.tiny_clip(1))
    noise = torch.randn((1, 16, 1, 6, 10), generator=torch.Generator().manual_seed(77), dtype=torch.float16).float()
    assert rel(img[:, 0], sf * (mean + std * noise)[:, :, 0]) <= GATE
    assert bool((img[:, 1:] == 0).all())
    assert torch.equal(lat.cpu(), torch.randn((1, 3, 16, 6, 10), generator=ref_g, dtype=torch.float16) * sched.init_noise_sigma)
    # and both feed the loop
    gi = torch.Generator().manual_seed(6)
    c = dit.config
    pe = torch.randn(2, c.max_text_seq_length, c.text_embed_dim, generator=gi).half().to(DEV)
    dom, flow = torch.randn(1, 1, 1000, generator=gi).to(DEV), torch.randn(1, 1, 1000, generator=gi).to(DEV)
    out = pc.denoise(dit, sched, lat, img, pe, dom, flow, 2, 6.0, True)
    assert tuple(out.shape) == (1, 3, 16, 6, 10) and out.dtype == torch.float16 and bool(torch.isfinite(out.float()).all())
