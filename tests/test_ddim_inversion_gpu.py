"""DDIM inversion and reference-guided sampling on the GPU (lkgd_amd/ddim_inversion.py).

The two kernel regimes the feature adds no entry point for: ``lkgd_attn_spatial(_qk)`` with ``nbatch`` 1 on row windows of larger
buffers (Sq = L queries against the 2L adjacent key rows of a [sample, reference] pair), and ``lkgd_dit_cfg_ddim_step`` with the
inverse scheduler's ``(A, -M, 0, 1)``.  Then the guided forward against the fp32 oracle with the restated processor
(tests/ddim_inversion_oracle.py) and its four decoys, the duplicate-key property, the launch list, ``sample`` against the stages called
by hand, and one ``ddim_inversion`` call end to end.

The model is the tiny rotary stock transformer (``dio.TINY``): 3 latent frames x 4 x 6 tokens + 16 text rows, L = 88 - a sample entry
runs Sq = 88 against S = 176, neither a multiple of the 32-row query block nor of the 64- / 128-key stage."""
import math

import pytest
import torch
import torch.nn.functional as F

import cogvideox_pipeline_oracle as po
import cogvideox_vae_encoder_oracle as eo
import ddim_inversion_oracle as dio
from cogvideox_support import DEV, hip_twin, patchify, unpatchify
from test_attn_pipe_gpu import _close as attn_close
from test_cogvideox_launches_gpu import _expected as plain_launches
from test_cogvideox_launches_gpu import _recorded

pytestmark = pytest.mark.gpu
SEQ = 16
LAT = (1, 3, 16, 8, 12)
#: measured relative L2 of the guided forward against the oracle x 3 (the docstring of test_guided_forward_vs_oracle)
GATE = dio.GATE
#: measured relative L2 of the end-to-end trajectories against the composed oracle x 3 (test_ddim_inversion_end_to_end)
E2E_GATE_INVERSE, E2E_GATE_RECON = 3.3e-3, 2.0e-2


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm()).item()


@pytest.fixture(scope="module")
def tiny():
    o = dio.seeded_model()
    return o, hip_twin(o, dio.TINY, DEV)


@pytest.fixture(scope="module")
def rope():
    from lkgd_amd import cogvideox as pc
    return pc.rotary_tables(dio.TINY, *dio.GRID)


# ------------------------------------------------------------------------------------------------ 5. regime A: row windows
@pytest.mark.parametrize("Sq,S", [(88, 176), (4100, 8200)])
def test_attn_spatial_on_row_windows(Sq, S):
    """one batch entry, q / out windows of Sq rows and k / v windows of S rows inside larger buffers (rows before and after) against
    fp32 SDPA over the window's keys, to the bound of the spatial-attention tests (test_attn_pipe_gpu.py); the rows of ``out`` outside
    the window keep their sentinel.  (4100, 8200) takes the software-pipelined program (S, Sq >= 4096) in its masked form (S % 128 =
    8) with Sq != S; (88, 176) the compiler-scheduled one with a masked tail on both axes.  Then the block's second call: Sq = S on
    the reference's window"""
    from lkgd_amd import ops
    heads = 2
    C = heads * 64
    g = torch.Generator().manual_seed(Sq + S)
    q0, k0 = Sq, 2 * Sq                                         # the windows' first rows
    q = torch.randn(3 * Sq, C, generator=g).half().to(DEV)
    k = torch.randn(k0 + S + Sq, C, generator=g).half().to(DEV)
    v = torch.randn(k0 + S + Sq, C, generator=g).half().to(DEV)
    out = torch.full((3 * Sq, C), -3.0, dtype=torch.float16, device=DEV)
    ops.attn_spatial(q[q0:q0 + Sq], k[k0:k0 + S], v[k0:k0 + S], out[q0:q0 + Sq], 1, S, heads, Sq=Sq)

    def ref(qw, kw, vw):
        qf, kf, vf = (t.float().cpu().reshape(1, -1, heads, 64).transpose(1, 2) for t in (qw, kw, vw))
        return F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(-1, C)
    attn_close(out[q0:q0 + Sq], ref(q[q0:q0 + Sq], k[k0:k0 + S], v[k0:k0 + S]), f"window Sq={Sq} S={S}")
    assert (out[:q0] == -3).all() and (out[q0 + Sq:] == -3).all()
    # a reference entry: its own Sq rows, the second half of the pair's keys
    out.fill_(-3.0)
    r0 = k0 + S - Sq
    ops.attn_spatial(q[q0:q0 + Sq], k[r0:r0 + Sq], v[r0:r0 + Sq], out[q0:q0 + Sq], 1, Sq, heads)
    attn_close(out[q0:q0 + Sq], ref(q[q0:q0 + Sq], k[r0:r0 + Sq], v[r0:r0 + Sq]), f"window Sq=S={Sq}")
    assert (out[:q0] == -3).all() and (out[q0 + Sq:] == -3).all()


# ------------------------------------------------------------------------------------------------ 6. regime B: the inverse step
def _fp16_spacing(v: torch.Tensor) -> torch.Tensor:
    """the distance between neighbouring fp16 values at |v| (fp64), 2^-24 in the subnormal range"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


@pytest.mark.parametrize("cfg", [1, 2])
def test_inverse_step_kernel_vs_host_and_fp64(cfg):
    """``lkgd_dit_cfg_ddim_step`` with ``DDIMInverseScheduler.coefficients`` = (A, -M, 0, 1) on the tiny latent shape, first step
    (cur = -1, at = 1) and last step (ap = 0) included:

    * equal TO THE BIT to the host statements: un-patchify, ``.float()``, the CFG statements, ``DDIMInverseScheduler.step``, ``.half()``;
    * within ONE fp16 ulp of the scheduler's literal fp64 statements (``dio.inverse_step_fp64``) on the model output the step is
      handed (the fp32 CFG combine), and within the tighter derived bound: with e = 2^-24 the step rounds A and M to fp32, the two
      products and the sum (|y32 - y| <= 3e (|A x| + |M n|) + O(e^2), 4e used =: Es), then once to fp16: |got - y| <= Es + half an
      fp16 spacing at |y| + Es.  Measured: at most 0.61 ulp;
    * with the CFG statements in fp64 as well (fp64 guidance) only the derived bound holds: the combine adds roundings of g, c - u,
      g * diff and u + gd, collected E = 8e (|A x| + |M| (|u| + |g (c - u)|)), and |got - y| <= E + half a spacing.  One fp16 ulp is
      NOT a bound of that chain: where A x and M n cancel, E exceeds the spacing at y - of the 64 512 elements here one sits at 1.23
      ulp (|y| = 1.7e-4, spacing 1.2e-7, error 1.5e-7: the fp32 rounding of O(1) operands), every other below 0.75."""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ddim_inversion as di
    from lkgd_amd import ops
    ac = dio.alphas_cumprod()
    gen = torch.Generator().manual_seed(40 + cfg)
    B, Fr, C, H, W = LAT
    guidance = 6.0 if cfg == 2 else 1.0
    e32 = 2.0 ** -24
    cases = [(3, t) for t in dio.inverse_timesteps(3)] + [(50, t) for t in (19, 499, 999)] + [(7, 142)]
    for n, t in cases:
        s = di.DDIMInverseScheduler(**pc.CogVideoXDDIMScheduler(snr_shift_scale=1.0).config)
        s.set_timesteps(n)
        lat = torch.randn(LAT, generator=gen).half()
        rows = (2 * torch.randn(cfg * Fr * (H // 2) * (W // 2), C * 4, generator=gen)).half()
        g = pc.dynamic_guidance(guidance, n, t) if cfg == 2 else 1.0
        got = ops.dit_cfg_ddim_step(rows.to(DEV), lat.to(DEV).clone(), 2, cfg, g, *s.coefficients(t)).cpu()
        # the host statements
        noise = unpatchify(rows, cfg, Fr, H, W).float()
        if cfg == 2:
            u, c = noise.chunk(2)
            noise = u + g * (c - u)
        host = s.step(noise, t, lat.float())[0].half()
        assert torch.equal(got, host), (n, t, (got.float() - host.float()).abs().max().item())
        # the scheduler's fp64 statements on the step's own model output
        A, M = s.linear_coefficients(t)
        y = dio.inverse_step_fp64(ac, t, n, lat, noise)
        err = (got.double() - y).abs()
        Es = 4 * e32 * (abs(A) * lat.double().abs() + abs(M) * noise.double().abs())
        print(f"cfg {cfg} n {n} t {t}: max error {(err / _fp16_spacing(y)).max().item():.3f} fp16 ulp of the fp64 statements")
        assert (err < _fp16_spacing(y)).all(), (n, t, (err / _fp16_spacing(y)).max().item())
        assert (err <= Es + 0.5 * _fp16_spacing(y.abs() + Es)).all(), (n, t)
        # the CFG statements in fp64 too
        n64 = unpatchify(rows, cfg, Fr, H, W).double()
        u64, c64 = n64.chunk(2) if cfg == 2 else (n64, n64)
        if cfg == 2:
            n64 = u64 + g * (c64 - u64)
        y = dio.inverse_step_fp64(ac, t, n, lat, n64)
        E = 8 * e32 * (abs(A) * lat.double().abs() + abs(M) * (u64.abs() + abs(g) * (c64 - u64).abs()))
        err = (got.double() - y).abs()
        assert (err <= E + 0.5 * _fp16_spacing(y.abs() + E)).all(), (n, t, (err / _fp16_spacing(y)).max().item())


# ------------------------------------------------------------------------------------------------ 7. the guided forward
def _hip_guided(m, hidden, text, rope, t=721.0):
    from lkgd_amd import ddim_inversion as di
    with di.OverrideAttnProcessors(m):
        return m.forward_tokens(hidden.half().to(DEV), text.half().to(DEV), t, image_rotary_emb=rope)


@pytest.mark.parametrize("cfg", [True, False])
def test_guided_forward_vs_oracle(tiny, rope, cfg):
    """``forward_tokens`` under ``OverrideAttnProcessors`` in the script's order [u, c, ref_u, ref_c] against the fp32 oracle with the
    restated processor: relative L2 of the sample half and of the reference half (which equals those entries' plain prediction).
    Measured on an MI355X: sample half 9.77e-4 (guidance) / 9.51e-4 (none), reference half 1.212e-3 / 1.186e-3.  The reference half is
    bit for bit the plain forward of those entries, so 1.2e-3 is where the plain forward of THIS model sits against the rope oracle
    (the I2V fixture with its learned table and 32 input channels sits at 7e-4); the sample half is no further.  Gate: three times
    the largest measured distance, 3.6e-3 (``dio.GATE``).  The four wrong processors stay 35 - 53 gates from the HIP result (at
    least ten are asked)"""
    o, m = tiny
    hidden, text = dio.guided_inputs(cfg=cfg)
    out = _hip_guided(m, hidden, text, rope)
    ro_ = dio.rope_for(o.config, hidden)
    with dio.override(o, "true"):
        want = dio.dit_forward(o, hidden, text, 721, ro_)
    n = hidden.shape[0] // 2
    assert out.shape == want.shape and out.dtype == torch.float16 and torch.isfinite(out.float()).all()
    ds, dr = _rel(out[:n], want[:n]), _rel(out[n:], want[n:])
    print(f"guided forward cfg={cfg}: rel L2 sample half {ds:.3e}, reference half {dr:.3e}; gate {GATE:.1e}")
    assert ds < GATE and dr < GATE
    plain = m.forward_tokens(hidden[n:].half().to(DEV), text[n:].half().to(DEV), 721.0, image_rotary_emb=rope)
    assert torch.equal(out[n:], plain)                      # a reference entry attends itself: its plain prediction, to the bit
    for mode in dio.DECOYS:
        with dio.override(o, mode):
            wrong = dio.dit_forward(o, hidden, text, 721, ro_)
        d = _rel(out, wrong)
        print(f"  decoy {mode}: rel L2 {d:.3e} ({d / GATE:.1f} gates)")
        assert d >= 10 * GATE, (mode, d)


# ------------------------------------------------------------------------------------------------ 8. duplicate keys
def test_duplicate_keys_leave_the_softmax_unchanged(tiny, rope):
    """reference latents and text identical to the sample's: every key appears twice with the same value, the softmax weights halve
    and the output is the plain forward of the sample - within the gate of the guided forward (the kernel sums 2L terms instead of
    L, so not to the bit; measured 4.2e-4)"""
    o, m = tiny
    hidden, text = dio.guided_inputs(same=True)
    out = _hip_guided(m, hidden, text, rope)
    plain = m.forward_tokens(hidden[:2].half().to(DEV), text[:2].half().to(DEV), 721.0, image_rotary_emb=rope)
    d = _rel(out[:2], plain)
    print(f"duplicate keys: rel L2 {d:.3e} from the plain forward; gate {GATE:.1e}")
    assert d < GATE and torch.equal(out[2:], plain)


# ------------------------------------------------------------------------------------------------ 9. the launch list
def _guided_launches(layers, B):
    prologue = ["lkgd_timestep_embedding", "lkgd_gemm_f16", "lkgd_silu", "lkgd_gemm_f16", "lkgd_silu", "lkgd_gemm_f16"]
    prologue += ["lkgd_gemm_f16", "lkgd_gemm_f16"] * B                                       # text, video embedding per entry
    block = ["lkgd_layernorm"] * (2 * B) + ["lkgd_gemm_f16"] * 3 + ["lkgd_qk_norm_rope"] \
        + ["lkgd_attn_spatial_qk", "lkgd_attn_spatial"] * (B // 2) \
        + ["lkgd_gemm_f16", "lkgd_gated_add"] \
        + ["lkgd_layernorm"] * (2 * B) + ["lkgd_gemm_f16", "lkgd_gelu_tanh", "lkgd_gemm_f16", "lkgd_gated_add"]
    head = ["lkgd_layernorm", "lkgd_layernorm", "lkgd_gemm_f16"] * (B // 2)                  # the sample entries only
    return prologue + block * layers + head


def test_guided_forward_rows_launch_list(tiny, rope):
    """the entry points one guided ``forward_rows`` issues at [u, ref_u, c, ref_c]: per block one q, k and v GEMM over all 4L rows, one
    ``lkgd_qk_norm_rope``, per pair the two attention calls on row windows, and no other entry point - nothing gathers, copies or
    concatenates K or V (between recorded launches the block makes no ATen call on them either: ``CogVideoXBlock.run`` hands the
    kernels views).  The head runs for the two sample entries.  Without the override the same model issues the plain list that
    test_cogvideox_launches_gpu.py pins (at that file's batch of 2)"""
    from lkgd_amd import ddim_inversion as di
    o, m = tiny
    hidden, text = dio.guided_inputs()
    pair = [0, 2, 1, 3]                                          # [u, c, ref_u, ref_c] -> [u, ref_u, c, ref_c]
    rows = patchify(hidden[[0, 2]].half()).to(DEV)               # Bv = 2: [sample rows | reference rows]
    txt = text[pair].half().to(DEV)

    def run():
        return m.forward_rows(rows, dio.GRID, txt, 721.0, image_rotary_emb=rope)
    with di.OverrideAttnProcessors(m):
        got = _recorded(run)
        out = run()
    want = _guided_launches(m.config.num_layers, 4)
    first = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (len(got), len(want), first, got[first:first + 6], want[first:first + 6])
    Tv = math.prod(dio.GRID)
    assert out.shape == (2 * Tv, 64) and out.is_contiguous()
    # the rows are the sample half of forward_tokens' output
    full = _hip_guided(m, hidden, text, rope)
    assert torch.equal(out, patchify(full[:2].cpu()).to(DEV))
    # no override: the plain list
    plain = _recorded(lambda: m.forward_rows(rows[:Tv], dio.GRID, txt[[0, 2]].contiguous(), 721.0, image_rotary_emb=rope))
    assert plain == plain_launches(m.config.num_layers, rotary=True)


# ------------------------------------------------------------------------------------------------ 10. sample() against the stages
@pytest.fixture(scope="module")
def parts(tiny):
    """the tiny pipeline: the T5 and VAE of the pipeline tests' support, the rotary DiT above, the 5B scheduler config"""
    pytest.importorskip("transformers")
    from types import SimpleNamespace

    from lkgd_amd import cogvideox as pc
    from lkgd_amd.pipeline_cogvideox import CogVideoXPipeline
    from t5_support import StubTokenizer, hf_model
    from t5_support import hip_twin as t5_twin

    class TinyPipeline(CogVideoXPipeline):
        def encode_prompt(self, *args, **kw):              # the tiny DiT's 16 text rows instead of the default 226
            kw.setdefault("max_sequence_length", SEQ)
            return super().encode_prompt(*args, **kw)
    t5_ref = hf_model(po.T5_CFG)
    te = t5_twin(t5_ref, po.T5_CFG, DEV)
    vae_o, dec_o, vae = po._vae_pair()
    tok = StubTokenizer(po.T5_CFG["vocab_size"])
    o, m = tiny
    pipe = TinyPipeline(tok, te, vae, m, pc.CogVideoXDDIMScheduler(snr_shift_scale=1.0))
    return SimpleNamespace(pipe=pipe, t5_ref=t5_ref, te=te, tok=tok, vae_o=vae_o, dec_o=dec_o, vae=vae, o=o, m=m)


def _text(parts, prompt, negative, cfg):
    from lkgd_amd import cogvideox as pc
    pe, ne = pc.encode_prompt(parts.te, parts.tok, prompt, negative, cfg, 1, None, None, SEQ, DEV)
    return torch.cat([ne, pe]) if cfg else pe


def _by_hand(parts, lat0, sched, prompt, *, steps, guidance_scale, use_dynamic_cfg=False, reference=None, rope=None, override=True):
    """the script's loop over the public stages, in the script's batch order: ``forward_tokens`` on [u, c, ref_u, ref_c] (under the
    override, or with ``override`` False as the plain doubled batch), the first half of its output patchified into the step kernel's
    rows"""
    import contextlib
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ddim_inversion as di
    from lkgd_amd import ops
    m = parts.m
    cfg = guidance_scale > 1.0
    text = _text(parts, prompt, None, cfg).half()
    sched.set_timesteps(steps)
    lat = lat0.to(DEV, torch.float16).clone()
    traj = []
    for i, t in enumerate(sched.timesteps.tolist()):
        x = torch.cat([lat] * 2) if cfg else lat
        if reference is None:
            noise = m.forward_tokens(x, text, float(t), image_rotary_emb=rope)
        else:
            r = reference[i].to(DEV, torch.float16)
            x = torch.cat([x, torch.cat([r] * 2) if cfg else r])
            with (di.OverrideAttnProcessors(m) if override else contextlib.nullcontext()):
                noise = m.forward_tokens(x, torch.cat([text] * 2), float(t), image_rotary_emb=rope).chunk(2)[0]
        g = pc.dynamic_guidance(guidance_scale, steps, t) if use_dynamic_cfg else guidance_scale
        ops.dit_cfg_ddim_step(patchify(noise).contiguous(), lat, 2, 2 if cfg else 1, g, *sched.coefficients(int(t)))
        traj.append(lat.clone())
    return torch.stack(traj)


def _inverse_scheduler(parts):
    from lkgd_amd import ddim_inversion as di
    return di.DDIMInverseScheduler(**parts.pipe.scheduler.config)


def test_sample_inverse_equals_stages(parts, rope):
    from lkgd_amd import ddim_inversion as di
    g = torch.Generator().manual_seed(8)
    lat0 = torch.randn(LAT, generator=g).half()
    got = di.sample(parts.pipe, lat0.to(DEV), _inverse_scheduler(parts), prompt="", num_inference_steps=3, guidance_scale=6.0)
    want = _by_hand(parts, lat0, _inverse_scheduler(parts), "", steps=3, guidance_scale=6.0, rope=rope)
    assert got.shape == (3,) + LAT and got.dtype == torch.float16 and torch.isfinite(got.float()).all()
    assert torch.equal(got, want)
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0], lat0.to(DEV))


@pytest.mark.parametrize("guidance_scale,dynamic", [(6.0, False), (1.0, False), (6.0, True)])
def test_sample_guided_equals_stages(parts, rope, guidance_scale, dynamic):
    """guided sampling, 3 steps: equal to the bit to the stages called by hand; the trajectory's last entry is what a caller reads as
    the final latents; reference latents in the wrong step order miss it; without the override the doubled batch runs plain
    attention, which is the plain loop of the sample"""
    from lkgd_amd import ddim_inversion as di
    pipe = parts.pipe
    g = torch.Generator().manual_seed(9)
    lat0, start = torch.randn(LAT, generator=g).half(), torch.randn(LAT, generator=g).half()
    inverse = di.sample(pipe, lat0.to(DEV), _inverse_scheduler(parts), prompt="", num_inference_steps=3, guidance_scale=guidance_scale)
    kw = dict(num_inference_steps=3, guidance_scale=guidance_scale, use_dynamic_cfg=dynamic)
    with di.OverrideAttnProcessors(pipe.transformer):
        got = di.sample(pipe, start.to(DEV), pipe.scheduler, prompt="a cat", reference_latents=reversed(inverse), **kw)
        wrong = di.sample(pipe, start.to(DEV), pipe.scheduler, prompt="a cat", reference_latents=inverse, **kw)
    assert not di.reference_attention_installed(pipe.transformer)
    want = _by_hand(parts, start, pipe.scheduler, "a cat", steps=3, guidance_scale=guidance_scale, use_dynamic_cfg=dynamic,
                    reference=inverse.flip(0), rope=rope)
    assert got.shape == (3,) + LAT and torch.equal(got, want)
    assert not torch.equal(wrong[-1], got[-1])
    as_list = [inverse[2], inverse[1], inverse[0]]
    with di.OverrideAttnProcessors(pipe.transformer):
        assert torch.equal(di.sample(pipe, start.to(DEV), pipe.scheduler, prompt="a cat", reference_latents=as_list, **kw), got)
    if dynamic:
        from lkgd_amd import cogvideox as pc
        assert pipe.guidance_scale == pc.dynamic_guidance(6.0, 3, int(pipe.scheduler.timesteps[-1]))
    # no override: plain attention at the doubled batch, the reference half discarded (the script's behaviour)
    plain = di.sample(pipe, start.to(DEV), pipe.scheduler, prompt="a cat", reference_latents=reversed(inverse), **kw)
    doubled = _by_hand(parts, start, pipe.scheduler, "a cat", steps=3, guidance_scale=guidance_scale, use_dynamic_cfg=dynamic,
                       reference=inverse.flip(0), rope=rope, override=False)
    alone = _by_hand(parts, start, pipe.scheduler, "a cat", steps=3, guidance_scale=guidance_scale, use_dynamic_cfg=dynamic, rope=rope)
    assert torch.equal(plain, doubled) and torch.equal(plain, alone) and not torch.equal(plain[-1], got[-1])


# ------------------------------------------------------------------------------------------------ 11. end to end
def test_ddim_inversion_end_to_end(parts):
    """one ``ddim_inversion`` call - a 9-frame in-memory clip at 96 x 64, 3 steps, guidance 6 - against the composed fp32 oracle:
    the script's host normalisation, the VAE encoder oracle's posterior with the call's own draw, transformers' T5, the rope oracle
    with the restated processor, the fp64 scheduler statements (latents rounded to fp16 after every step, as the script casts them).
    Measured on an MI355X: inversion trajectory rel L2 1.108e-3, reconstruction trajectory 6.715e-3 (three more forwards, each
    reading the inversion's own deviation through the reference keys); gates three times those, 3.3e-3 and 2.0e-2.
    The tiny model's inversion -> reconstruction round trip is printed, not gated: |recon[-1] - encoded| / |encoded| = 1.516 for the
    oracle and for the HIP path alike - random weights reconstruct nothing"""
    from lkgd_amd import ddim_inversion as di
    pipe = parts.pipe
    g = torch.Generator().manual_seed(12)
    clip = torch.randint(0, 256, (11, 64, 96, 3), generator=g, dtype=torch.uint8)        # 11 frames: the first 9 = 4 * 2 + 1 are kept
    torch.manual_seed(1234)
    inv, rec, f_inv, f_rec = di.ddim_inversion(pipe, "a cat", clip, num_inference_steps=3, width=96, height=64, guidance_scale=6.0)
    assert inv.shape == rec.shape == (3,) + LAT and inv.dtype == torch.float16
    assert len(f_inv) == len(f_rec) == 9 and f_inv[0].size == (96, 64)
    assert not di.reference_attention_installed(pipe.transformer)
    # the call's two draws from the global RNG, replayed: the posterior's noise, then randn_like of the transposed latents
    torch.manual_seed(1234)
    n_post = torch.randn((1, 16, 3, 8, 12), device=DEV, dtype=torch.float16)
    n_start = torch.randn_like(torch.empty((1, 16, 3, 8, 12), device=DEV, dtype=torch.float16).transpose(1, 2))
    frames = di.get_video_frames(clip, 96, 64, 0, 0, 81, None).half().float()              # [9, 3, 64, 96]
    mean, _, std = parts.vae_o.posterior(frames.unsqueeze(0).permute(0, 2, 1, 3, 4))
    lat0 = ((mean + std * n_post.float().cpu()) * eo.TINY.scaling_factor).permute(0, 2, 1, 3, 4)

    def t5(prompt):
        return parts.t5_ref(input_ids=parts.tok([prompt], padding="max_length", max_length=SEQ, truncation=True, add_special_tokens=True,
                                                return_tensors="pt").input_ids).last_hidden_state
    with torch.no_grad():
        empty, cat = t5(""), t5("a cat")
    inv_o = dio.sample(parts.o, lat0, torch.cat([empty, empty]), steps=3, guidance_scale=6.0, inverse=True)
    rec_o = dio.sample(parts.o, n_start.float().cpu(), torch.cat([empty, cat]), steps=3, guidance_scale=6.0, inverse=False,
                       reference=inv_o.flip(0))
    di_, dr = _rel(inv, inv_o), _rel(rec, rec_o)
    print(f"ddim_inversion end to end: rel L2 inversion trajectory {di_:.3e} (gate {E2E_GATE_INVERSE:.1e}), reconstruction "
          f"{dr:.3e} (gate {E2E_GATE_RECON:.1e})")
    print(f"  first latents {_rel(inv[0], inv_o[0]):.3e}; round trip |recon[-1] - encoded| / |encoded| = {_rel(rec_o[-1], lat0):.3f} "
          f"(oracle), {_rel(rec[-1], lat0):.3f} (HIP)")
    assert di_ < E2E_GATE_INVERSE and dr < E2E_GATE_RECON
