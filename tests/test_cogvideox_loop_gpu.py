"""The CogVideoX loop kernels on the GPU (include/lkgd_hip_dit_loop.h): ``lkgd_lk_fuse_tokens`` against the fp32 oracle and the
reference pin, row independence bit for bit; ``lkgd_dit_patch_rows`` / ``lkgd_dit_cfg_ddim_step`` bit for bit against the torch
statements they replace; ``denoise`` bit for bit against the loop it was (``forward_tokens`` + the ATen glue, written out here);
the footprint cases of the three entry points (tests/footprint.py)."""
import ctypes as C
import os

import pytest
import torch
from safetensors.torch import load_file

from cogvideox_support import (DEV, DIT_SEED, aten_denoise, aten_step as _aten_step, dit_inputs as _pin_inputs, glue_data as _glue_data,
                               hip_twin, loop_inputs as _loop_inputs, patchify as _patchify, rel as _rel, tiny_oracle as _oracle,
                               unpatchify as _unpatchify)
from footprint import run_case

gpu = pytest.mark.gpu
LK_SEED = 4242                       # weights of the fuse tests

#: every name in lkgd_amd._lib.DIT_LOOP_SYMBOLS -> its footprint tests in this module (the rule REGISTRY keeps for _lib.SYMBOLS in
#: tests/test_footprint_gpu.py)
FOOTPRINT = {
    "lkgd_lk_fuse_tokens": ["test_lk_fuse_tokens_footprint"],
    "lkgd_dit_patch_rows": ["test_dit_patch_rows_footprint"],
    "lkgd_dit_cfg_ddim_step": ["test_dit_cfg_ddim_step_footprint"],
}

FUSE_CASES = [(2, 1, 1), (2, 5, 2), (2, 16, 1), (3, 7, 3)]        # (B, L, Bd): one row, a ragged tail, broadcast, per-entry features
GLUE_SHAPES = [(1, 3, 16, 8, 12), (2, 2, 16, 6, 10), (1, 1, 4, 2, 4)]   # (B, F, C, H, W); the second has an odd w = 5


@pytest.fixture(scope="module")
def lk():
    """(oracle, HIP model) with the fuse tests' weights; neither is modified by a test"""
    o = _oracle(LK_SEED)
    return o, hip_twin(o, dev=DEV)


@pytest.fixture(scope="module")
def pinned():
    """(oracle, HIP model) with the weights of the reference fixture"""
    o = _oracle(DIT_SEED)
    return o, hip_twin(o, dev=DEV)


def _fuse_inputs(seed):
    """one generator per seed draws the four cases in order"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for B, L, Bd in FUSE_CASES:
        e = torch.randn(B, L, 4096, generator=g).half().float()
        d = 3 * torch.randn(Bd, 1, 1000, generator=g)
        f = 3 * torch.randn(Bd, 1, 1000, generator=g)
        out.append((e, d, f))
    return out


def _fuse_preconditions(o, e, d, f):
    """the block is discontinuous where a spectrum bin crosses the negative real axis (phase +-pi): (smallest |Im X| / ||x|| over
    the bins 1..127 with Re X < 0 of low, low_d, low_f; whether a DC or Nyquist bin is negative), from the oracle's values"""
    import torch.nn.functional as F
    low = o.quaternion_lora_lconv(e.permute(0, 2, 1)).permute(0, 2, 1)
    low_d = o.quaternion_lora_dconv(F.interpolate(d, size=1024, mode="linear").permute(0, 2, 1)).permute(0, 2, 1)
    low_f = o.quaternion_lora_fconv(F.interpolate(f, size=1024, mode="linear").permute(0, 2, 1)).permute(0, 2, 1)
    margin, negative = float("inf"), False
    for x in (low, low_d, low_f):
        X = torch.fft.rfft(x.double(), dim=-1)
        inner = X[..., 1:128]
        rel = (inner.imag.abs() / x.double().norm(dim=-1, keepdim=True))[inner.real < 0]
        margin = min(margin, rel.min().item())
        negative = negative or bool((X[..., 0].real < 0).any() or (X[..., 128].real < 0).any())
    return margin, negative


# ------------------------------------------------------------------------------------------------------------- the fuse
@gpu
@pytest.mark.parametrize("seed", [13, 14])
def test_lk_fuse_tokens_vs_oracle(lk, seed):
    """the bound of test_lk_fuse_kernel_vs_oracle.  Seeds 13 and 14 keep every bin with a negative real part >= 2.1e-4 ||x|| away
    from the real axis in all four cases (seed 11: 2.5e-5), and every case has a negative DC or Nyquist bin (the +pi convention)"""
    o, m = lk
    for (B, L, Bd), (e, d, f) in zip(FUSE_CASES, _fuse_inputs(seed)):
        with torch.no_grad():
            margin, negative = _fuse_preconditions(o, e, d, f)
            ref = o.lk_fuse(e, d, f)
        assert margin >= 1e-4 and negative, (seed, (B, L, Bd), margin, negative)
        got = m.fused_text(e.to(DEV), d.to(DEV), f.to(DEV))
        assert got.shape == (B, L, 4096) and got.dtype == torch.float16
        err = (got.float().cpu() - ref).abs().max().item()
        print(f"\nlk_fuse_tokens seed {seed} (B, L, Bd) = {(B, L, Bd)}: max err {err:.3e}, max |ref| {ref.abs().max().item():.3f}, "
              f"margin {margin:.2e}")
        assert err <= 2e-3 * ref.abs().max().item() + 1e-3, (seed, (B, L, Bd), err)


@gpu
def test_lk_fuse_tokens_rows_are_independent(lk):
    """(2, 16, 1): two workgroups of 8 rows per entry == the 32 single-row calls == the call with Bd == B and expanded feature rows
    == a second call, bit for bit; and a row stride wider than 4096 changes nothing"""
    from lkgd_amd import lk_fuse
    _, m = lk
    e, d, f = (t.to(DEV) for t in _fuse_inputs(13)[2])
    full = m.fused_text(e, d, f)
    for b in range(2):
        for r in range(16):
            one = m.fused_text(e[b:b + 1, r:r + 1], d, f)
            assert torch.equal(one[0, 0], full[b, r]), (b, r)
    assert torch.equal(m.fused_text(e, d.expand(2, 1, 1000), f.expand(2, 1, 1000)), full)
    assert torch.equal(m.fused_text(e, d, f), full)
    assert torch.equal(m.fused_text(e[:, :13], d, f), full[:, :13])                       # a ragged tail next to other company
    wide = torch.full((2, 16, 4096 + 8), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, :, :4096] = e
    outw = torch.full((2, 16, 4096 + 16), float("nan"), dtype=torch.float16, device=DEV)
    lk_fuse.lk_fuse_tokens(m._pk.lk_tokens, wide[:, :, :4096], d, f, out=outw[:, :, :4096])
    assert torch.equal(outw[:, :, :4096], full) and bool(torch.isnan(outw[:, :, 4096:]).all())


def _no_aten_fuse(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the DiT path called rocFFT / ATen interpolation")
    monkeypatch.setattr(torch.fft, "rfft", refuse)
    monkeypatch.setattr(torch.fft, "irfft", refuse)
    monkeypatch.setattr(torch.nn.functional, "interpolate", refuse)


@gpu
def test_fused_text_vs_reference_pin_without_aten(pinned, golden_dir, monkeypatch):
    """``fused_text`` against the reference's own forward (tests/golden/cogvideox.safetensors) at the existing bound, and a 2-step
    ``denoise``, with torch.fft.rfft / irfft and F.interpolate patched to raise"""
    from lkgd_amd import cogvideox as pc
    from oracle import cogvideox as oc
    golden = load_file(os.path.join(golden_dir, "cogvideox.safetensors"))
    _, m = pinned
    i = _pin_inputs(oc.TINY_DIT)
    _no_aten_fuse(monkeypatch)
    fused = m.fused_text(i["text"].to(DEV), i["domain"].to(DEV), i["flow"].to(DEV))
    r = _rel(fused, golden["fused_text"])
    print(f"\nfused_text vs the reference: rel L2 {r:.3e}")
    assert r < 2e-3
    lat, img, pe, dom, flow = _loop_inputs()
    out = pc.denoise(m, pc.CogVideoXDDIMScheduler(), lat.half().to(DEV), img.to(DEV), pe.to(DEV), dom.to(DEV), flow.to(DEV), 2, 6.0, True)
    assert out.dtype == torch.float16 and bool(torch.isfinite(out.float()).all())


# -------------------------------------------------------------------------------------------------------------- the glue
@gpu
@pytest.mark.parametrize("shape", GLUE_SHAPES)
def test_dit_patch_rows_bitwise(shape):
    from lkgd_amd import ops
    lat32, img, _ = (t.to(DEV) for t in _glue_data(shape, 3))
    for lat in (lat32, lat32.half()):
        for im in (img, None):
            x = lat.half() if im is None else torch.cat([lat.half(), im], 2)
            ref = _patchify(x)
            got = ops.dit_patch_rows(lat, im)
            assert got.dtype == torch.float16 and torch.equal(got, ref), (shape, lat.dtype, im is None)
            buf = torch.full((ref.shape[0], ref.shape[1] + 24), float("nan"), dtype=torch.float16, device=DEV)   # ldp wider than the row
            ops.dit_patch_rows(lat, im, out=buf[:, 8:8 + ref.shape[1]])
            assert torch.equal(buf[:, 8:8 + ref.shape[1]], ref) and int(torch.isnan(buf).sum()) == ref.shape[0] * 24


@gpu
@pytest.mark.parametrize("shape", GLUE_SHAPES)
def test_dit_cfg_ddim_step_bitwise(shape):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ops
    lat32, _, noise = (t.to(DEV) for t in _glue_data(shape, 4))
    sched = pc.CogVideoXDDIMScheduler()
    sched.set_timesteps(4)
    rows = noise.shape[0] // 2
    for t in sched.timesteps.tolist():
        g, coef = pc.dynamic_guidance(6.0, 4, t), sched.coefficients(t)
        for lat0 in (lat32, lat32.half()):
            for cfg in (1, 2):
                n = noise[:cfg * rows].contiguous()
                ref = _aten_step(n, lat0, cfg, g, coef)
                wide = torch.full((cfg * rows, n.shape[1] + 8), float("nan"), dtype=torch.float16, device=DEV)      # ldn wider than the row
                wide[:, :n.shape[1]] = n
                for src in (n, wide[:, :n.shape[1]]):
                    lat = lat0.clone()
                    assert ops.dit_cfg_ddim_step(src, lat, 2, cfg, g, *coef) is lat
                    assert torch.equal(lat, ref), (shape, t, lat0.dtype, cfg, (lat.float() - ref.float()).abs().max().item())


@gpu
@pytest.mark.parametrize("guidance_scale", [6.0, 1.0])
def test_denoise_equals_the_aten_loop_bitwise(lk, guidance_scale):
    """3 latent frames, 4 steps, dynamic CFG (and no CFG): every step of the new loop has the bits of the old one; with CFG it
    also meets the oracle's loop at test_hip_dit_loop_vs_oracle's bound"""
    from lkgd_amd import cogvideox as pc
    from oracle import cogvideox as oc
    o, m = lk
    lat, img, pe, dom, flow = _loop_inputs(cfg=guidance_scale > 1.0)
    dv = [t.to(DEV) for t in (lat.half(), img, pe, dom, flow)]
    lat_in = dv[0].clone()
    old_steps, new_steps = [], []
    old = aten_denoise(pc, m, pc.CogVideoXDDIMScheduler(), *dv, 4, guidance_scale, lambda i, t, l: old_steps.append(l))
    new = pc.denoise(m, pc.CogVideoXDDIMScheduler(), *dv, 4, guidance_scale, True, callback=lambda i, t, l: new_steps.append(l))
    assert torch.equal(dv[0], lat_in)                                # the caller's latents are not the loop's in-place operand
    assert len(new_steps) == len(old_steps) == 4 and new.dtype == torch.float16
    for i, (a, b) in enumerate(zip(new_steps, old_steps)):
        assert a.dtype == torch.float16 and torch.equal(a, b), (i, (a.float() - b.float()).abs().max().item())
    assert torch.equal(new, old) and torch.equal(new, new_steps[-1])
    if guidance_scale > 1.0:
        ref_steps = []
        ref = oc.denoise(o, oc.CogVideoXDDIMScheduler(), lat.half().float(), img, pe, dom, flow, 4, guidance_scale, True,
                         callback=lambda i, t, l: ref_steps.append(l.clone()))
        for i, (a, b) in enumerate(zip(new_steps, ref_steps)):
            assert _rel(a, b) < 2e-2, (i, _rel(a, b))
        assert _rel(new, ref) < 2e-2


@gpu
def test_forward_rows_shares_one_copy_of_the_patch_rows(lk):
    """forward_rows on ONE copy of the rows (Bv = 1) == forward_tokens on the duplicated batch, bit for bit"""
    from lkgd_amd import ops
    _, m = lk
    lat, img, pe, dom, flow = (t.to(DEV) for t in _loop_inputs())
    text = m.fused_text(pe, dom, flow)
    x = torch.cat([torch.cat([lat.half()] * 2), torch.cat([img.half()] * 2)], dim=2)
    ref = m.forward_tokens(x, text, 721.0)
    rows = ops.dit_patch_rows(lat.half(), img.half())
    out = m.forward_rows(rows, (3, 4, 6), text, 721.0)
    assert out.shape == (2 * 72, 64) and torch.equal(_unpatchify(out, 2, 3, 8, 12), ref)


# --------------------------------------------------------------------------------------------------------- footprint cases
@gpu
@pytest.mark.parametrize("B,L,Bd", [(2, 5, 2), (1, 9, 1)])
def test_lk_fuse_tokens_footprint(B, L, Bd):
    """e between NaN guard rows and gaps (lde > 4096), d / f and the 18 operands between NaN guards, out between pattern guards
    and gaps: nothing outside the [B L, 4096] window is written, NaN next to every operand changes nothing, the result meets the
    oracle and equals the run on compact copies bit for bit"""
    from test_footprint_gpu import _lib_, _ok, _st, flat_in
    from lkgd_amd import lk_fuse
    lib = _lib_()
    o = _oracle(LK_SEED)
    ws_cpu, _ = lk_fuse.pack_lk_tokens(hip_twin(o, dev="cpu").float())
    g = torch.Generator().manual_seed(100 * B + L)
    e = torch.randn(B, L, 4096, generator=g).half().float()
    d, f = 3 * torch.randn(Bd, 1, 1000, generator=g), 3 * torch.randn(Bd, 1, 1000, generator=g)

    def case(W):
        ev = W.inp(e.reshape(B * L, 4096), pad=4, name="e")
        dv = W.inp(d.reshape(Bd, 1000), pad=0, gap=False, name="d")
        fv = W.inp(f.reshape(Bd, 1000), pad=0, gap=False, name="f")
        wv = [flat_in(W, w, f"w[{i}]") for i, w in enumerate(ws_cpu)]
        ptrs = (C.c_void_p * 18)(*[w.data_ptr() for w in wv])
        ov = W.out(B * L, 4096, torch.float16, pad=8, name="out")
        _ok(lib.lkgd_lk_fuse_tokens(ev.data_ptr(), ev.stride(0), dv.data_ptr(), fv.data_ptr(), B, L, Bd, ptrs, ov.data_ptr(),
                                    ov.stride(0), _st()), "lk_fuse_tokens")
        torch.cuda.synchronize()                 # `wv` lives until the launch has run
        return {"out": ov}

    def refs():
        with torch.no_grad():
            return {"out": o.lk_fuse(e, d, f).reshape(B * L, 4096)}

    def close(got, ref, what):
        ref = ref.float().cpu()
        err = (got.float().cpu() - ref).abs().max().item()
        assert err <= 2e-3 * ref.abs().max().item() + 1e-3, (what, err)
    run_case(case, DEV, refs, close, True, sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("shape,f32,with_img", [((1, 3, 16, 8, 12), 0, 1), ((2, 2, 16, 6, 10), 1, 1), ((1, 1, 4, 2, 4), 0, 0)])
def test_dit_patch_rows_footprint(shape, f32, with_img):
    from test_footprint_gpu import _lib_, _ok, _st, flat_in
    lib = _lib_()
    B, F, C_, H, W_ = shape
    lat, img, _ = _glue_data(shape, 11)
    lat = lat if f32 else lat.half()
    rows, width = B * F * (H // 2) * (W_ // 2), (2 if with_img else 1) * C_ * 4

    def case(W):
        lv = flat_in(W, lat, "latents")
        iv = flat_in(W, img, "image_latents")
        ov = W.out(rows, width, torch.float16, pad=16, col0=8, name="rows")
        _ok(lib.lkgd_dit_patch_rows(lv.data_ptr(), f32, iv.data_ptr() if with_img else None, B, F, C_, H, W_, 2, ov.data_ptr(),
                                    ov.stride(0), _st()), "dit_patch_rows")
        return {"rows": ov}

    def refs():
        x = torch.cat([lat.half(), img], 2) if with_img else lat.half()
        return {"rows": _patchify(x).to(DEV)}

    def close(got, ref, what):
        assert torch.equal(got, ref), what
    run_case(case, DEV, refs, close, True, sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("shape,f32,cfg", [((1, 3, 16, 8, 12), 0, 2), ((2, 2, 16, 6, 10), 1, 2), ((1, 1, 4, 2, 4), 0, 1)])
def test_dit_cfg_ddim_step_footprint(shape, f32, cfg):
    """the noise rows between NaN guards and gaps, the latents - input AND output - between pattern guards"""
    from test_footprint_gpu import _lib_, _ok, _st, flat_inout
    from lkgd_amd import cogvideox as pc
    lib = _lib_()
    B, F, C_, H, W_ = shape
    lat, _, noise = _glue_data(shape, 12)
    lat = lat if f32 else lat.half()
    noise = noise[:cfg * noise.shape[0] // 2].contiguous()
    sched = pc.CogVideoXDDIMScheduler()
    sched.set_timesteps(4)
    t = sched.timesteps.tolist()[1]
    g, coef = pc.dynamic_guidance(6.0, 4, t), sched.coefficients(t)

    def case(W):
        nv = W.inp(noise, pad=8, col0=8, name="noise_rows")
        lv = flat_inout(W, lat, "latents")
        _ok(lib.lkgd_dit_cfg_ddim_step(nv.data_ptr(), nv.stride(0), lv.data_ptr(), f32, B, F, C_, H, W_, 2, cfg, g, *coef, _st()),
            "dit_cfg_ddim_step")
        return {"latents": lv}

    def refs():
        return {"latents": _aten_step(noise.to(DEV), lat.to(DEV), cfg, g, coef).reshape(1, -1)}

    def close(got, ref, what):
        assert torch.equal(got, ref), (what, (got.float() - ref.float()).abs().max().item())
    run_case(case, DEV, refs, close, True, sync=torch.cuda.synchronize)
