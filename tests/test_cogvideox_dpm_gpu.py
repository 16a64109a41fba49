"""The CogVideoX DPM-Solver++ path on the MI355X: ``lkgd_dit_cfg_dpm_step`` / ``lkgd_dit_cfg_dpm_step_t`` (include/lkgd_hip_dit_dpm.h) bit
for bit against the torch statements they replace (tests/dpm_oracle.py::aten_dpm_step), what they must NOT read, four decoys they
must miss, their footprint cases (tests/footprint.py); ``denoise`` with a ``CogVideoXDPMScheduler`` bit for bit and step by step
against ``forward_tokens`` + ``CogVideoXDPMScheduler.step`` written out here, for the tiny 2B twin and the tiny 1.5 model."""
import pytest
import torch

import cogvideox15_oracle as vo
import dpm_oracle as do
from cogvideox_support import DEV, DIT_SEED, P, glue_data, hip_twin, loop_inputs, tiny_oracle
from footprint import run_case

gpu = pytest.mark.gpu
PT = 2

#: every name in lkgd_amd._lib.DIT_DPM_SYMBOLS -> its footprint tests in this module (the rule REGISTRY keeps for _lib.SYMBOLS in
#: tests/test_footprint_gpu.py)
FOOTPRINT = {
    "lkgd_dit_cfg_dpm_step": ["test_dit_cfg_dpm_step_footprint"],
    "lkgd_dit_cfg_dpm_step_t": ["test_dit_cfg_dpm_step_t_footprint"],
}

GLUE_SHAPES = [(1, 3, 16, 8, 12), (2, 2, 16, 6, 10), (1, 1, 4, 2, 4)]   # (B, F, C, H, W) of the 2-D file; the second has an odd w = 5
#: the grid of the 1.5 file: a frame-in-patch (F = 2, 4), channel (C = 2, 16), batch or x / y (w = 2 against 3) transposition shows
GLUE_SHAPES_T = [(B, F, C_, H, W) for B in (1, 2) for F in (2, 4) for C_ in (2, 16) for H, W in ((4, 4), (4, 6))]
G = 6.0


def _coef():
    """the 6-step schedule's t = 499 after t = 666: m3 = 1.43, m4 = 0.43, mn = 0.72 - every statement of the second-order step moves
    the result"""
    from lkgd_amd import cogvideox as pc
    s = pc.CogVideoXDPMScheduler()
    s.set_timesteps(6)
    k = s.coefficients(499, 666)
    assert k.order == 2 and k.mn != 0.0
    return k


def _step_data(shape, seed, p_t=None):
    """(fp32 latents, fp16 rows of both CFG entries, fp32 x0 of the step before, fp32 noise) of a clip, on the CPU"""
    lat, _, noise = glue_data(shape, seed, p_t)
    g = torch.Generator().manual_seed(seed + 1000)
    return lat, noise, torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def _run(noise_rows, lat0, x0_old, eps, cfg, order, k, p_t=None):
    """one launch on clones -> (latents, x0_state)"""
    from lkgd_amd import ops
    lat, x0 = lat0.clone(), x0_old.clone()
    glue = {} if p_t is None else {"p_t": p_t}
    assert ops.dit_cfg_dpm_step(noise_rows, lat, x0, eps, P, cfg, order, G, k, **glue) is lat
    return lat, x0


def _bitwise(shape, p_t):
    k2 = _coef()
    lat32, noise, old, eps32 = (t.to(DEV) for t in _step_data(shape, 4, p_t))
    rows = noise.shape[0] // 2
    for lat0 in (lat32, lat32.half()):
        eps = eps32.to(lat0.dtype)
        for cfg in (1, 2):
            n = noise[:cfg * rows].contiguous()
            wide = torch.full((cfg * rows, n.shape[1] + 8), float("nan"), dtype=torch.float16, device=DEV)      # ldn wider than the row
            wide[:, :n.shape[1]] = n
            for order in (1, 2):
                for k, e in ((k2._replace(order=order), eps), (k2._replace(order=order, mn=0.0), None)):
                    ref, ref0 = do.aten_dpm_step(n, lat0, old, e, cfg, G, k, p_t)
                    for src in (n, wide[:, :n.shape[1]]):
                        lat, x0 = _run(src, lat0, old, e, cfg, order, k, p_t)
                        what = (shape, lat0.dtype, cfg, order, k.mn)
                        assert lat.dtype == lat0.dtype and torch.equal(lat, ref), (what, (lat.float() - ref.float()).abs().max().item())
                        assert x0.dtype == torch.float32 and torch.equal(x0, ref0), (what, (x0 - ref0).abs().max().item())


# ---------------------------------------------------------------------------------------------------------- the step kernel
@gpu
@pytest.mark.parametrize("shape", GLUE_SHAPES)
def test_dit_cfg_dpm_step_bitwise(shape):
    """latents fp16 / fp32 x cfg 1 / 2 x order 1 / 2 x (mn != 0 with eps | mn == 0 with eps = NULL) x (ldn == | > the row width):
    both outputs, the latents and x0_state"""
    _bitwise(shape, None)


@gpu
@pytest.mark.parametrize("shape", GLUE_SHAPES_T)
def test_dit_cfg_dpm_step_t_bitwise(shape):
    _bitwise(shape, PT)


@gpu
@pytest.mark.parametrize("shape,p_t", [(GLUE_SHAPES[0], None), ((1, 4, 16, 4, 6), PT)])
def test_mn_zero_never_reads_eps(shape, p_t):
    k = _coef()._replace(mn=0.0)
    lat32, noise, old, eps32 = (t.to(DEV) for t in _step_data(shape, 5, p_t))
    for lat0 in (lat32, lat32.half()):
        nan = torch.full_like(lat0, float("nan"))
        for order in (1, 2):
            a, a0 = _run(noise, lat0, old, None, 2, order, k, p_t)
            b, b0 = _run(noise, lat0, old, nan, 2, order, k, p_t)
            assert torch.equal(a, b) and torch.equal(a0, b0) and bool(torch.isfinite(b.float()).all())
            ref, ref0 = do.aten_dpm_step(noise, lat0, old, None, 2, G, k._replace(order=order), p_t)
            assert torch.equal(b, ref) and torch.equal(b0, ref0)


@gpu
@pytest.mark.parametrize("shape,p_t", [(GLUE_SHAPES[0], None), ((1, 4, 16, 4, 6), PT)])
def test_order_one_never_reads_x0_state(shape, p_t):
    k = _coef()._replace(order=1)
    lat32, noise, old, eps32 = (t.to(DEV) for t in _step_data(shape, 6, p_t))
    for lat0 in (lat32, lat32.half()):
        eps = eps32.to(lat0.dtype)
        lat, x0 = _run(noise, lat0, torch.full_like(old, float("nan")), eps, 2, 1, k, p_t)
        ref, ref0 = do.aten_dpm_step(noise, lat0, None, eps, 2, G, k, p_t)
        assert torch.equal(lat, ref) and torch.equal(x0, ref0) and bool(torch.isfinite(x0).all()) and bool(torch.isfinite(lat.float()).all())


@gpu
@pytest.mark.parametrize("f32", [0, 1])
def test_dit_cfg_dpm_step_misses_the_decoys(f32):
    """a second-order step that were first order, had m3 and m4 exchanged, dropped the noise, or took x0 from the unconditional entry:
    precondition (on the CPU, a condition on the data, not a measurement) - each decoy differs from the true ATen result in at least
    90 % of the elements; the kernel equals the true result and differs from every decoy"""
    k = _coef()
    for shape, p_t in ((GLUE_SHAPES[0], None), ((1, 4, 16, 4, 6), PT)):
        lat, noise, old, eps = _step_data(shape, 7, p_t)
        if not f32:
            lat, eps = lat.half(), eps.half()
        true, _ = do.aten_dpm_step(noise, lat, old, eps, 2, G, k, p_t)
        decoys = {d: do.aten_dpm_step(noise, lat, old, eps, 2, G, k, p_t, decoy=d)[0] for d in do.DECOYS}
        for d, wrong in decoys.items():
            frac = (wrong != true).float().mean().item()
            assert frac >= 0.9, (shape, d, frac)
        dv = [t.to(DEV) for t in (noise, lat, old, eps)]
        got, _ = _run(dv[0], dv[1], dv[2], dv[3], 2, 2, k, p_t)
        assert torch.equal(got, do.aten_dpm_step(dv[0], dv[1], dv[2], dv[3], 2, G, k, p_t)[0])
        for d in do.DECOYS:
            on_dev = do.aten_dpm_step(dv[0], dv[1], dv[2], dv[3], 2, G, k, p_t, decoy=d)[0]
            frac = (on_dev != got).float().mean().item()
            assert frac >= 0.9, (shape, d, frac)


# --------------------------------------------------------------------------------------------------------- footprint cases
def _footprint(shape, f32, cfg, order, noisy, p_t):
    """the noise rows between NaN guards and gaps, eps between NaN guards, the latents and x0_state - inputs AND outputs - between
    pattern guards: the call writes the two and nothing else, and NaN next to every operand changes nothing"""
    from test_footprint_gpu import _lib_, _ok, _st, flat_in, flat_inout
    lib = _lib_()
    B, F, C_, H, W_ = shape
    lat, noise, old, eps = _step_data(shape, 12, p_t)
    if not f32:
        lat, eps = lat.half(), eps.half()
    noise = noise[:cfg * noise.shape[0] // 2].contiguous()
    k = _coef()._replace(order=order)
    if not noisy:
        k = k._replace(mn=0.0)
    fn, pt = (lib.lkgd_dit_cfg_dpm_step, ()) if p_t is None else (lib.lkgd_dit_cfg_dpm_step_t, (p_t,))

    def case(W):
        nv = W.inp(noise, pad=8, col0=8, name="noise_rows")
        lv = flat_inout(W, lat, "latents")
        xv = flat_inout(W, old, "x0_state")
        ev = flat_in(W, eps, "eps") if noisy else None
        _ok(fn(nv.data_ptr(), nv.stride(0), lv.data_ptr(), f32, xv.data_ptr(), ev.data_ptr() if noisy else None, B, F, C_, H, W_, P, *pt,
               cfg, order, G, k.sqrt_alpha, k.sqrt_beta, k.m1, k.m2, k.m3, k.m4, k.mn, _st()), "dit_cfg_dpm_step")
        return {"latents": lv, "x0_state": xv}

    def refs():
        a, b = do.aten_dpm_step(noise.to(DEV), lat.to(DEV), old.to(DEV), eps.to(DEV) if noisy else None, cfg, G, k, p_t)
        return {"latents": a.reshape(1, -1), "x0_state": b.reshape(1, -1)}

    def close(got, ref, what):
        assert torch.equal(got, ref), (what, (got.float() - ref.float()).abs().max().item())
    run_case(case, DEV, refs, close, True, sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("shape,f32,cfg,order,noisy", [((1, 3, 16, 8, 12), 0, 2, 2, 1), ((2, 2, 16, 6, 10), 1, 2, 1, 1),
                                                       ((1, 1, 4, 2, 4), 0, 1, 2, 0)])
def test_dit_cfg_dpm_step_footprint(shape, f32, cfg, order, noisy):
    _footprint(shape, f32, cfg, order, noisy, None)


@gpu
@pytest.mark.parametrize("shape,f32,cfg,order,noisy", [((1, 4, 16, 8, 12), 0, 2, 2, 1), ((2, 2, 16, 4, 6), 1, 2, 1, 1),
                                                       ((1, 2, 2, 4, 4), 0, 1, 2, 0)])
def test_dit_cfg_dpm_step_t_footprint(shape, f32, cfg, order, noisy):
    _footprint(shape, f32, cfg, order, noisy, PT)


# ------------------------------------------------------------------------------------------------------------------ the loop
def aten_dpm_denoise(pc, m, sched, latents, image_latents, prompt_embeds, dom, flow, steps, guidance_scale, callback, generator,
                     rope=None, ofs=None):
    """the DPM branch of pipeline_cogvideox_image2video.py:829-885 without the glue kernels: ``forward_tokens`` on the CFG-duplicated,
    channel-concatenated batch, the CFG statements, ``CogVideoXDPMScheduler.step`` with the previous step's x0 and timestep, the cast
    back (:884)"""
    sched.set_timesteps(steps)
    cfg = guidance_scale > 1.0
    text = m.fused_text(prompt_embeds, dom, flow)
    latents = latents.to(torch.float16)
    img = image_latents.to(torch.float16)
    img2 = torch.cat([img] * 2) if cfg else img
    timesteps = sched.timesteps.tolist()
    old_pred_original_sample = None
    for i, t in enumerate(timesteps):
        x = torch.cat([latents] * 2) if cfg else latents
        x = torch.cat([x, img2], dim=2)
        noise = m.forward_tokens(x, text, float(t), image_rotary_emb=rope, ofs=ofs).float()
        g = pc.dynamic_guidance(guidance_scale, steps, t)
        if cfg:
            u, c = noise.chunk(2)
            noise = u + g * (c - u)
        latents, old_pred_original_sample = sched.step(noise, old_pred_original_sample, t, timesteps[i - 1] if i > 0 else None, latents,
                                                       generator=generator, return_dict=False)
        latents = latents.to(torch.float16)
        callback(i, t, latents)
    return latents


@pytest.fixture(scope="module")
def twin2b():
    """the HIP twin of the tiny 2B oracle; not modified by a test"""
    return hip_twin(tiny_oracle(4242), dev=DEV)


@pytest.fixture(scope="module")
def tiny15():
    """the tiny 1.5 model of tests/test_cogvideox15_gpu.py (same configuration and seed); not modified by a test"""
    cfg = vo.TINY_V15_DIT
    return hip_twin(vo.seeded_model(cfg, DIT_SEED), cfg, DEV)


def _both_loops(pc, m, dv, steps, guidance_scale, seed, **aten_kw):
    old_steps, new_steps = [], []
    old = aten_dpm_denoise(pc, m, pc.CogVideoXDPMScheduler(), *dv, steps, guidance_scale, lambda i, t, l: old_steps.append((i, t, l)),
                           torch.Generator().manual_seed(seed), **aten_kw)
    new = pc.denoise(m, pc.CogVideoXDPMScheduler(), *dv, steps, guidance_scale, True, callback=lambda i, t, l: new_steps.append((i, t, l)),
                     generator=torch.Generator().manual_seed(seed))
    assert len(new_steps) == len(old_steps) == steps and new.dtype == torch.float16
    for (i, t, a), (j, u, b) in zip(new_steps, old_steps):
        assert (i, t) == (j, u) and a.dtype == torch.float16 and a.shape == b.shape
        assert torch.equal(a, b), (i, (a.float() - b.float()).abs().max().item())
    assert torch.equal(new, old) and torch.equal(new, new_steps[-1][2]) and bool(torch.isfinite(new.float()).all())
    return new


@gpu
@pytest.mark.parametrize("guidance_scale", [6.0, 1.0])
@pytest.mark.parametrize("steps", [4, 6])
def test_dpm_denoise_equals_the_aten_loop_bitwise(twin2b, steps, guidance_scale):
    """3 latent frames; 4 steps end first order onto final_alpha_cumprod (x' = x0), 6 steps end second order; dynamic CFG and no
    CFG: every step of ``denoise`` has the bits of the loop written out above, and the callbacks see the same (i, t)"""
    from lkgd_amd import cogvideox as pc
    lat, img, pe, dom, flow = loop_inputs(cfg=guidance_scale > 1.0)
    dv = [t.to(DEV) for t in (lat.half(), img, pe, dom, flow)]
    lat_in = dv[0].clone()
    _both_loops(pc, twin2b, dv, steps, guidance_scale, 31)
    assert torch.equal(dv[0], lat_in)                                # the caller's latents are not the loop's in-place operand


@gpu
def test_dpm_denoise_15_equals_the_aten_loop_bitwise(tiny15):
    """the tiny 1.5 model: 4 latent frames (two temporal patches), the _t step, ofs = 2.0 as the pipeline sets it, 4 steps"""
    from lkgd_amd import cogvideox as pc
    cfg = vo.TINY_V15_DIT
    lat, img, pe, dom, flow = loop_inputs(cfg, f=4)
    dv = [t.to(DEV) for t in (lat.half(), img, pe, dom, flow)]
    rope = pc.rotary_tables(tiny15.config, 4 // PT, cfg.sample_height // P, cfg.sample_width // P)
    _both_loops(pc, tiny15, dv, 4, 6.0, 32, rope=rope, ofs=2.0)


@gpu
def test_dpm_denoise_seeds_and_the_ddim_fallback(twin2b):
    """the same seed twice gives the same bits (a CPU and a device generator each), another seed other latents; and the result is
    not the DDIM loop's: a DPM scheduler does not get DDIM updates any more"""
    from lkgd_amd import cogvideox as pc
    dv = [t.to(DEV) for t in loop_inputs()]
    dv[0] = dv[0].half()

    def run(gen, cls=pc.CogVideoXDPMScheduler):
        return pc.denoise(twin2b, cls(), *dv, 4, 6.0, True, generator=gen)
    a = run(torch.Generator().manual_seed(5))
    assert torch.equal(run(torch.Generator().manual_seed(5)), a)
    b = run(torch.Generator().manual_seed(6))
    assert (a != b).float().mean().item() > 0.9 and bool(torch.isfinite(b.float()).all())
    on_dev = run(torch.Generator(device=DEV).manual_seed(5))
    assert torch.equal(run(torch.Generator(device=DEV).manual_seed(5)), on_dev) and bool(torch.isfinite(on_dev.float()).all())
    ddim = run(None, pc.CogVideoXDDIMScheduler)
    assert torch.equal(run(torch.Generator().manual_seed(5), pc.CogVideoXDDIMScheduler), ddim)       # DDIM draws nothing
    assert (a != ddim).float().mean().item() > 0.9
