"""The CogVideoX 1.5 path on the MI355X: ``lkgd_dit_patch_rows_t`` / ``lkgd_dit_cfg_ddim_step_t`` (include/lkgd_hip_dit_tpatch.h) bit
for bit against the torch statements they replace, their refusals and footprint cases (tests/footprint.py); ``denoise`` of the tiny
1.5 model, loaded by ``from_pretrained``, bit for bit and step by step against ``forward_tokens`` + the ATen glue written out here;
the HIP forward against tests/golden/cogvideox15.safetensors (the reference's own in-tree forward, make_goldens_cogvideox15.py)
and its two decoys."""
import os

import pytest
import torch
from safetensors.torch import load_file

import cogvideox15_oracle as vo
from cogvideox_support import DEV, DIT_SEED, P, aten_denoise, aten_step, dit_inputs as _inputs, glue_data, hip_twin, loop_inputs, patchify, \
    rel as _rel, unpatchify
from c_interface import ALIGN, NULL, SHAPE, entry
from footprint import run_case

gpu = pytest.mark.gpu
PT = 2

#: every name in lkgd_amd._lib.DIT_TPATCH_SYMBOLS -> its footprint tests in this module (the rule REGISTRY keeps for _lib.SYMBOLS
#: in tests/test_footprint_gpu.py)
FOOTPRINT = {
    "lkgd_dit_patch_rows_t": ["test_dit_patch_rows_t_footprint"],
    "lkgd_dit_cfg_ddim_step_t": ["test_dit_cfg_ddim_step_t_footprint"],
}

#: (B, F, C, H, W): the smallest shapes where a frame-in-patch (F = 2: one temporal patch, 4: two), channel (C = 2, 16), batch or
#: x / y (4 x 4 against 4 x 6: w = 2 against 3, odd) transposition shows
GLUE_SHAPES = [(B, F, C_, H, W) for B in (1, 2) for F in (2, 4) for C_ in (2, 16) for H, W in ((4, 4), (4, 6))]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_file(os.path.join(golden_dir, "cogvideox15.safetensors"))


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """(twin, HIP model) of the fixture's tiny 1.5 DiT; the HIP model went through save_pretrained / from_pretrained.  Neither is
    modified by a test"""
    from lkgd_amd import cogvideox as pc
    cfg = vo.TINY_V15_DIT
    o = vo.seeded_model(cfg, DIT_SEED)
    m = hip_twin(o, cfg)
    d = str(tmp_path_factory.mktemp("cogvideox15") / "transformer")
    m.save_pretrained(d)
    r = pc.CogVideoXTransformer3DModel.from_pretrained(d, torch_dtype=torch.float16)
    assert r.config.patch_size_t == 2 and r.config.ofs_embed_dim == 64 and r.ofs_embedding is not None
    return o, r.to(DEV)


# ------------------------------------------------------------------------------------------------------------- the glue
def test_the_two_torch_statements_are_inverse():
    """the available cross-check of the unpinned column order: the in-tree un-patchify undoes the restated patch reshape"""
    x = torch.randn(2, 4, 6, 4, 6)
    assert torch.equal(unpatchify(patchify(x, PT), 2, 4, 4, 6, PT), x)
    # column ((c * p_t + pt) * p + py) * p + px of row (b, ft, y, x)
    r = patchify(x, PT).reshape(2, 2, 2, 3, 6, 2, 2, 2)
    assert r[1, 1, 0, 2, 4, 1, 0, 1] == x[1, 1 * 2 + 1, 4, 0 * 2 + 0, 2 * 2 + 1]
    assert torch.equal(patchify(x, p_t=1), patchify(x))          # one frame per patch is the 2-D statement, bit for bit


@gpu
@pytest.mark.parametrize("shape", GLUE_SHAPES)
def test_dit_patch_rows_t_bitwise(shape):
    from lkgd_amd import ops
    lat32, img, _ = (t.to(DEV) for t in glue_data(shape, 3, PT))
    for lat in (lat32, lat32.half()):
        for im in (img, None):
            x = lat.half() if im is None else torch.cat([lat.half(), im], 2)
            ref = patchify(x, PT)
            got = ops.dit_patch_rows(lat, im, p_t=PT)
            assert got.dtype == torch.float16 and got.shape == ref.shape and torch.equal(got, ref), (shape, lat.dtype, im is None)
            buf = torch.full((ref.shape[0], ref.shape[1] + 24), float("nan"), dtype=torch.float16, device=DEV)   # ldp wider than the row
            ops.dit_patch_rows(lat, im, out=buf[:, 8:8 + ref.shape[1]], p_t=PT)
            assert torch.equal(buf[:, 8:8 + ref.shape[1]], ref) and int(torch.isnan(buf).sum()) == ref.shape[0] * 24


@gpu
@pytest.mark.parametrize("shape", GLUE_SHAPES)
def test_dit_cfg_ddim_step_t_bitwise(shape):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ops
    lat32, _, noise = (t.to(DEV) for t in glue_data(shape, 4, PT))
    sched = pc.CogVideoXDDIMScheduler()
    sched.set_timesteps(4)
    rows = noise.shape[0] // 2
    for t in sched.timesteps.tolist()[:2]:
        g, coef = pc.dynamic_guidance(6.0, 4, t), sched.coefficients(t)
        for lat0 in (lat32, lat32.half()):
            for cfg in (1, 2):
                n = noise[:cfg * rows].contiguous()
                ref = aten_step(n, lat0, cfg, g, coef, PT)
                wide = torch.full((cfg * rows, n.shape[1] + 8), float("nan"), dtype=torch.float16, device=DEV)      # ldn wider than the row
                wide[:, :n.shape[1]] = n
                for src in (n, wide[:, :n.shape[1]]):
                    lat = lat0.clone()
                    assert ops.dit_cfg_ddim_step(src, lat, P, cfg, g, *coef, p_t=PT) is lat
                    assert torch.equal(lat, ref), (shape, t, lat0.dtype, cfg, (lat.float() - ref.float()).abs().max().item())


@gpu
def test_dit_tpatch_refusals():
    """every refusal returns its code and launches nothing: rows and latents come back untouched"""
    from test_footprint_gpu import _st
    from lkgd_amd import ops
    from lkgd_amd._lib import LkgdHipError
    shape = (1, 4, 16, 8, 12)
    lat, img, noise = (t.to(DEV) for t in glue_data(shape, 5, PT))
    lat = lat.half()
    rows = torch.full((48, 256), 7.0, dtype=torch.float16, device=DEV)
    lat0, rows0 = lat.clone(), rows.clone()
    odd = torch.zeros(96 * 128 + 8, dtype=torch.float16, device=DEV)[1:]                 # 2 bytes off a 16-byte boundary

    patch = entry("lkgd_dit_patch_rows_t", latents=lat.data_ptr(), latents_is_f32=0, image_latents=img.data_ptr(), B=1, F=4, C=16, H=8,
                  W=12, p=2, p_t=2, rows_out=rows.data_ptr(), ldp=256, stream=_st())
    step = entry("lkgd_dit_cfg_ddim_step_t", noise_rows=noise.data_ptr(), ldn=128, latents=lat.data_ptr(), latents_is_f32=0, B=1, F=4,
                 C=16, H=8, W=12, p=2, p_t=2, cfg=2, guidance=3.0, a=0.9, b=0.1, sqrt_alpha=0.8, sqrt_beta=0.6, stream=_st())
    assert patch(latents=None) == NULL and patch(rows_out=None) == NULL and step(noise_rows=None) == NULL and step(latents=None) == NULL
    for name, fn, ld in (("patch", patch, "ldp"), ("step", step, "ldn")):
        for kw in (dict(p_t=1), dict(p_t=3), dict(p_t=4), dict(F=3), dict(F=5), dict(F=0), dict(p=1), dict(p=4), dict(W=13), dict(H=7),
                   dict(B=0), dict(C=0), dict(C=3), {ld: 120}, {ld: 260}):
            assert fn(**kw) == SHAPE, (name, kw)
    assert patch(ldp=128) == SHAPE and step(cfg=0) == SHAPE and step(cfg=3) == SHAPE
    assert patch(rows_out=odd.data_ptr()) == ALIGN and step(noise_rows=odd.data_ptr()) == ALIGN
    torch.cuda.synchronize()
    assert torch.equal(lat, lat0) and torch.equal(rows, rows0)
    # the Python side's own errors
    for bad in (lambda: ops.dit_patch_rows(lat[:, :3].contiguous(), None, p_t=2),                     # F % p_t
                lambda: ops.dit_patch_rows(lat, img, p_t=3),
                lambda: ops.dit_patch_rows(lat, img, out=rows[:, :128], p_t=2),                          # the 2-D width
                lambda: ops.dit_cfg_ddim_step(noise[:96, :64].contiguous(), lat, 2, 2, 3.0, 0.9, 0.1, 0.8, 0.6, p_t=2),
                lambda: ops.dit_cfg_ddim_step(noise, lat[:, :3].contiguous(), 2, 2, 3.0, 0.9, 0.1, 0.8, 0.6, p_t=2)):
        with pytest.raises(LkgdHipError):
            bad()
    assert torch.equal(lat, lat0) and torch.equal(rows, rows0)


# --------------------------------------------------------------------------------------------------------- footprint cases
@gpu
@pytest.mark.parametrize("shape,f32,with_img", [((1, 4, 16, 8, 12), 0, 1), ((2, 2, 16, 4, 6), 1, 1), ((1, 2, 2, 4, 4), 0, 0)])
def test_dit_patch_rows_t_footprint(shape, f32, with_img):
    from test_footprint_gpu import _lib_, _ok, _st, flat_in
    lib = _lib_()
    B, F, C_, H, W_ = shape
    lat, img, _ = glue_data(shape, 11, PT)
    lat = lat if f32 else lat.half()
    rows, width = B * (F // PT) * (H // P) * (W_ // P), (2 if with_img else 1) * C_ * PT * P * P

    def case(W):
        lv = flat_in(W, lat, "latents")
        iv = flat_in(W, img, "image_latents")
        ov = W.out(rows, width, torch.float16, pad=16, col0=8, name="rows")
        _ok(lib.lkgd_dit_patch_rows_t(lv.data_ptr(), f32, iv.data_ptr() if with_img else None, B, F, C_, H, W_, P, PT, ov.data_ptr(),
                                      ov.stride(0), _st()), "dit_patch_rows_t")
        return {"rows": ov}

    def refs():
        x = torch.cat([lat.half(), img], 2) if with_img else lat.half()
        return {"rows": patchify(x, PT).to(DEV)}

    def close(got, ref, what):
        assert torch.equal(got, ref), what
    run_case(case, DEV, refs, close, True, sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("shape,f32,cfg", [((1, 4, 16, 8, 12), 0, 2), ((2, 2, 16, 4, 6), 1, 2), ((1, 2, 2, 4, 4), 0, 1)])
def test_dit_cfg_ddim_step_t_footprint(shape, f32, cfg):
    """the noise rows between NaN guards and gaps, the latents - input AND output - between pattern guards"""
    from test_footprint_gpu import _lib_, _ok, _st, flat_inout
    from lkgd_amd import cogvideox as pc
    lib = _lib_()
    B, F, C_, H, W_ = shape
    lat, _, noise = glue_data(shape, 12, PT)
    lat = lat if f32 else lat.half()
    noise = noise[:cfg * noise.shape[0] // 2].contiguous()
    sched = pc.CogVideoXDDIMScheduler()
    sched.set_timesteps(4)
    t = sched.timesteps.tolist()[1]
    g, coef = pc.dynamic_guidance(6.0, 4, t), sched.coefficients(t)

    def case(W):
        nv = W.inp(noise, pad=8, col0=8, name="noise_rows")
        lv = flat_inout(W, lat, "latents")
        _ok(lib.lkgd_dit_cfg_ddim_step_t(nv.data_ptr(), nv.stride(0), lv.data_ptr(), f32, B, F, C_, H, W_, P, PT, cfg, g, *coef, _st()),
            "dit_cfg_ddim_step_t")
        return {"latents": lv}

    def refs():
        return {"latents": aten_step(noise.to(DEV), lat.to(DEV), cfg, g, coef, PT).reshape(1, -1)}

    def close(got, ref, what):
        assert torch.equal(got, ref), (what, (got.float() - ref.float()).abs().max().item())
    run_case(case, DEV, refs, close, True, sync=torch.cuda.synchronize)


# ------------------------------------------------------------------------------------------------------------------ the loop
@gpu
@pytest.mark.parametrize("guidance_scale", [6.0, 1.0])
def test_denoise_equals_the_aten_loop_bitwise(tiny, guidance_scale):
    """4 latent frames (two temporal patches), 3 steps, dynamic CFG (and no CFG), ofs = 2.0 by default as the pipeline sets it:
    every step of ``denoise`` (the _t glue pair around forward_rows, ofs embedded once) has the bits of the loop written out
    above.  No bound against the fp32 twin's loop is asserted: with this fixture's weights (q / k norms x 4, CFG up to 7) the three
    steps sit 7.2e-4, 6.1e-3 and 3.6e-2 (relative L2) from a twin that never rounds its latents to fp16 - the first figure is that
    rounding, the loop then amplifies it ~8 x per step; parity of the forward itself is the golden test's"""
    from lkgd_amd import cogvideox as pc
    _, m = tiny
    cfg = vo.TINY_V15_DIT
    lat, img, pe, dom, flow = loop_inputs(cfg, f=4, cfg=guidance_scale > 1.0)
    dv = [t.to(DEV) for t in (lat.half(), img, pe, dom, flow)]
    lat_in = dv[0].clone()
    rope = pc.rotary_tables(m.config, 4 // PT, cfg.sample_height // P, cfg.sample_width // P)
    old_steps, new_steps = [], []
    old = aten_denoise(pc, m, pc.CogVideoXDDIMScheduler(), *dv, 3, guidance_scale, lambda i, t, l: old_steps.append(l), rope, 2.0)
    new = pc.denoise(m, pc.CogVideoXDDIMScheduler(), *dv, 3, guidance_scale, True, callback=lambda i, t, l: new_steps.append(l))
    assert torch.equal(dv[0], lat_in)                                # the caller's latents are not the loop's in-place operand
    assert len(new_steps) == len(old_steps) == 3 and new.dtype == torch.float16 and new.shape == lat.shape
    for i, (a, b) in enumerate(zip(new_steps, old_steps)):
        assert a.dtype == torch.float16 and torch.equal(a, b), (i, (a.float() - b.float()).abs().max().item())
    assert torch.equal(new, old) and torch.equal(new, new_steps[-1]) and bool(torch.isfinite(new.float()).all())
    assert torch.equal(pc.denoise(m, pc.CogVideoXDDIMScheduler(), *dv, 3, guidance_scale, True, ofs=torch.full((1,), 2.0)), new)
    other = pc.denoise(m, pc.CogVideoXDDIMScheduler(), *dv, 3, guidance_scale, True, ofs=0.0)
    assert not torch.equal(other, new)                                # ofs reaches the loop


@gpu
def test_denoise_refuses_an_odd_frame_count_and_pads(tiny):
    """3 latent frames: ``denoise`` raises; padded by the pipeline's rule (one frame at the front) it runs, and the padding is
    dropped afterwards"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    _, m = tiny
    lat, img, pe, dom, flow = (t.to(DEV) for t in loop_inputs(vo.TINY_V15_DIT, seed=6, f=3))
    with pytest.raises(LkgdHipError, match="patch_size_t"):
        pc.denoise(m, pc.CogVideoXDDIMScheduler(), lat.half(), img, pe, dom, flow, 2)
    add = pc.temporal_padding_frames(3, m.config.patch_size_t)
    lat_p, img_p = pc.pad_for_temporal_patches(lat.half(), img, m.config.patch_size_t)
    assert add == 1 and lat_p.shape[1] == img_p.shape[1] == 4
    out = pc.drop_temporal_padding(pc.denoise(m, pc.CogVideoXDDIMScheduler(), lat_p, img_p, pe, dom, flow, 2), add)
    assert out.shape == lat.shape and bool(torch.isfinite(out.float()).all())


# ------------------------------------------------------------------------------------------------------------------ the forward
@gpu
def test_hip_15_dit_forward_vs_reference_golden(golden, tiny):
    """the bounds of test_hip_rotary_dit_forward_vs_reference_golden (rel L2 1e-2, max abs 5e-2) against the reference's output,
    and the same forward MISSES both decoys - ofs = 0, and the frames of every temporal patch exchanged - by at least half the
    distance the generator recorded (0.396 and 1.256 of ||out||): neither ofs nor the frame order inside a patch is lost in the
    tolerance.  Fed the decoys' inputs, it meets them"""
    o, m = tiny
    i = {k: v.to(DEV) for k, v in _inputs(vo.TINY_V15_DIT).items()}
    cos, sin = golden["cos"], golden["sin"]

    def run(hidden, ofs):
        return m(hidden, i["text"], i["t"], i["domain"], i["flow"], ofs=ofs, image_rotary_emb=(cos, sin), return_dict=False)[0]
    out = run(i["hidden"], 2.0)
    r, a = _rel(out, golden["out"]), (out.float().cpu() - golden["out"]).abs().max().item()
    print(f"\nHIP CogVideoX 1.5 DiT forward vs the reference: rel L2 {r:.3e}, max abs {a:.3e}")
    assert out.shape == golden["out"].shape == (2, 4, 16, 8, 12) and out.dtype == torch.float16
    assert r < 1e-2 and a < 5e-2
    assert torch.equal(run(i["hidden"], torch.full((2,), 2.0, device=DEV)), out)           # a [B] tensor is the same ofs
    norm = golden["out"].norm()
    for name, k in (("out_ofs0", 0), ("out_swapped", 1)):
        recorded = golden["decoy_distance"][k].item()
        miss = ((out.float().cpu() - golden[name]).norm() / norm).item()
        print(f"{name}: {miss:.3f} of ||out|| away (the generator recorded {recorded:.3f})")
        assert recorded >= 0.1 and miss >= 0.5 * recorded, (name, miss, recorded)
    assert _rel(run(i["hidden"], 0.0), golden["out_ofs0"]) < 1e-2
    assert _rel(run(vo.swap_frames_in_patches(i["hidden"]), 2.0), golden["out_swapped"]) < 1e-2


@gpu
def test_hip_15_t2v_forward_vs_twin():
    """the text-to-video form: 16 input channels would give K = 128 patch columns; here 32 channels without the ofs embedding"""
    from lkgd_amd import cogvideox as pc
    cfg = vo.V15DiTConfig(**{**vo.TINY_V15_DIT.__dict__, "ofs_embed_dim": None})
    o = vo.seeded_model(cfg, DIT_SEED + 3)
    m = hip_twin(o, cfg, DEV)
    i = _inputs(cfg, seed=9)
    rope = vo.rotary_tables(cfg, 4, 4, 6)
    with torch.no_grad():
        ref = o(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], image_rotary_emb=rope)[0]
    out = m(*(i[k].to(DEV) for k in ("hidden", "text", "t", "domain", "flow")), image_rotary_emb=pc.rotary_tables(m.config, 2, 4, 6),
            return_dict=False)[0]
    r = _rel(out, ref)
    print(f"\ntiny 1.5 DiT without ofs vs twin: rel L2 {r:.3e}")
    assert out.shape == ref.shape and r < 1e-2
