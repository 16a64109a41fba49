"""``CogVideoXPipeline`` (text-to-video) and ``CogVideoXVideoToVideoPipeline`` on the GPU ([EXT] diffusers' classes, parity unpinned;
tests/cogvideox_t2v_v2v_support.py holds the tiny components and the two independent statements of each call).

* ``preprocess_video``: the GPU path (one ``lkgd_image_preprocess`` launch per clip on the [1, T * H, W, C] view) equals the host chain
  followed by the cast, to the bit.
* Composition, to the bit: ``pipe(...)`` equals the HIP stage functions called by hand in diffusers' order with the same generator - both
  schedulers, guidance on and off, dynamic guidance, two prompts with two generators, ``num_videos_per_prompt``, given latents, a
  ``patch_size_t`` model, every output type; video-to-video at strength 1.0 / 0.8 / 0.2; the five wrong calls of ``V2V_DECOYS`` miss.
* ``denoise``: ``start_step = 0`` with both features is the call it was; the truncated loop equals the loop written over the launches.
* One call of each class against the composed fp32 CPU oracle."""
import numpy as np
import pytest
import torch

import cogvideox_pipeline_oracle as po
import cogvideox_t2v_v2v_support as sp
from cogvideox_support import DEV, loop_inputs, rel, tiny_oracle, hip_twin

pytestmark = pytest.mark.gpu

PROMPT, NEGATIVE = "a red kite over the dunes", "blurry"
T2V, V2V = "CogVideoXPipeline", "CogVideoXVideoToVideoPipeline"
H, W, SEQ = sp.H, sp.W, sp.SEQ


@pytest.fixture(scope="module")
def parts():
    pytest.importorskip("transformers")
    return sp.build()


def _gen(seed, n=None):
    return torch.Generator().manual_seed(seed) if n is None else [torch.Generator().manual_seed(seed + i) for i in range(n)]


def _same_state(a, b):
    a, b = (a if isinstance(a, list) else [a]), (b if isinstance(b, list) else [b])
    return all(torch.equal(x.get_state(), y.get_state()) for x, y in zip(a, b))


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------------------------------ preprocess_video
def _pil(u):
    import PIL.Image
    return PIL.Image.fromarray(u[..., 0], mode="L") if u.shape[-1] == 1 else PIL.Image.fromarray(u)


#: (clips, T, C, source (w, h), target (height, width)); T * H * W % 8 == 0 takes the wide path, otherwise one pixel per thread
VIDEO_CASES = {"wide_rgb": (1, 5, 3, (80, 48), (48, 80)), "narrow_rgb": (1, 5, 3, (9, 7), (7, 9)), "narrow_one_frame": (1, 1, 3, (9, 7), (7, 9)),
               "wide_one_frame_rgba": (1, 1, 4, (16, 8), (8, 16)), "narrow_grey": (1, 5, 1, (9, 7), (7, 9)),
               "wide_grey_batch": (2, 5, 1, (16, 8), (8, 16)), "narrow_rgba_batch": (2, 5, 4, (3, 5), (5, 3)),
               "resized_batch": (2, 5, 3, (96, 60), (48, 80))}


@pytest.mark.parametrize("case", list(VIDEO_CASES))
def test_preprocess_video_gpu_path_equals_the_host_chain_bitwise(case):
    from lkgd_amd import replay
    from lkgd_amd.video_processor import VideoProcessor
    B, T, C, (w, h), (th, tw) = VIDEO_CASES[case]
    vp = VideoProcessor(vae_scale_factor=1)                 # factor 1: odd sizes stay what they are
    values = torch.arange(B * T * h * w * C, dtype=torch.int64)
    u = ((values * 37 + values // 256) % 256).to(torch.uint8).reshape(B, T, h, w, C).numpy()        # every byte value, when there is room
    assert B * T * h * w * C < 256 or len(np.unique(u)) == 256
    clips = [[_pil(u[b, t]) for t in range(T)] for b in range(B)]
    video = clips if B > 1 else clips[0]
    want = torch.stack([vp.preprocess(c, th, tw) for c in clips]).permute(0, 2, 1, 3, 4).to(torch.float16)
    assert (T * th * tw % 8 == 0) == case.startswith(("wide", "resized"))
    with replay.strict(False):
        with replay.record() as rec:
            got = vp.preprocess_video(video, th, tw, device=DEV, dtype=torch.float16)
    torch.cuda.synchronize()
    names = [name for _, _, name, _ in rec.calls]
    rec.release()
    assert names == ["lkgd_image_preprocess"] * B                                   # one launch per clip, nothing else
    assert got.is_cuda and got.dtype == torch.float16 and got.is_contiguous() and tuple(got.shape) == (B, C, T, th, tw)
    assert torch.equal(_bits(got), _bits(want))
    if case == "resized_batch":
        assert (h, w) != (th, tw) and not torch.equal(got[0], got[1])
    # the host form on a GPU target is the same tensor (tensor input: no GPU path)
    t = torch.from_numpy(u[0]).permute(0, 3, 1, 2).float() / 255
    assert torch.equal(vp.preprocess_video(t, device=DEV, dtype=torch.float16).cpu(), (2 * t - 1).half().permute(1, 0, 2, 3)[None])


# ---------------------------------------------------------------------------------------------------------- text-to-video
#: name -> (model, scheduler, prompts, generators, call keywords)
T2V_CASES = {
    "ddim_cfg": ("sincos", "ddim", 1, None, dict(num_frames=9, steps=2, guidance_scale=6.0)),
    "dpm_cfg_dynamic": ("sincos", "dpm", 1, None, dict(num_frames=9, steps=3, guidance_scale=6.0, use_dynamic_cfg=True)),
    "ddim_no_cfg": ("sincos", "ddim", 1, None, dict(num_frames=5, steps=2, guidance_scale=1.0)),
    "dpm_two_prompts_two_generators": ("sincos", "dpm", 2, 2, dict(num_frames=5, steps=2, guidance_scale=6.0)),
    "ddim_two_videos_per_prompt": ("sincos", "ddim", 1, None, dict(num_frames=5, steps=2, guidance_scale=6.0, num_videos_per_prompt=2)),
    "v15_dpm_odd_latent_frames": ("v15", "dpm", 1, None, dict(num_frames=9, steps=2, guidance_scale=6.0)),
}


def _t2v(pipe, prompt, negative, kw, generator, output_type, **more):
    kw = dict(kw)
    return pipe(prompt, negative, height=H, width=W, num_frames=kw.pop("num_frames"), num_inference_steps=kw.pop("steps"),
                generator=generator, output_type=output_type, max_sequence_length=SEQ, **kw, **more)


@pytest.mark.parametrize("case", list(T2V_CASES))
def test_t2v_call_equals_the_stages_by_hand_bitwise(parts, case):
    kind, sched, n_prompts, n_gen, kw = T2V_CASES[case]
    prompt, negative = (PROMPT, NEGATIVE) if n_prompts == 1 else ([PROMPT, "a second prompt"], [NEGATIVE, "dull"])
    pipe = parts.pipe(T2V, kind, sched)
    g0, g = _gen(5, n_gen), _gen(5, n_gen)
    want = sp.by_hand_t2v(parts, kind, sched, prompt, negative, generator=g0, **kw)
    B = n_prompts * kw.get("num_videos_per_prompt", 1)
    latent_frames = (kw["num_frames"] - 1) // 4 + 1
    padded = latent_frames + (latent_frames % 2 if kind == "v15" else 0)
    assert tuple(want.shape) == (B, padded, 16, 6, 10)
    out = _t2v(pipe, prompt, negative, kw, g, "latent")
    assert type(out).__name__ == "CogVideoXPipelineOutput" and out.frames.dtype == torch.float16
    assert torch.equal(out.frames, want) and _same_state(g, g0)
    assert pipe.num_timesteps == kw["steps"] and pipe.current_timestep is None
    if B == 2:
        assert not torch.equal(out.frames[0], out.frames[1])


def test_t2v_given_latents_and_output_types(parts):
    kw = dict(num_frames=9, steps=2, guidance_scale=6.0)
    pipe = parts.pipe(T2V, "v15", "ddim")                   # 3 latent frames + 1 padding frame, which leaves before the decode
    lat0 = torch.randn(1, 4, 16, 6, 10, generator=_gen(8)).half()
    want = sp.by_hand_t2v(parts, "v15", "ddim", PROMPT, NEGATIVE, latents=lat0, **kw)
    got = _t2v(pipe, PROMPT, NEGATIVE, kw, None, "latent", latents=lat0).frames
    assert torch.equal(got, want) and not torch.equal(got, _t2v(pipe, PROMPT, NEGATIVE, kw, _gen(6), "latent").frames)
    clip = sp.by_hand_t2v(parts, "v15", "ddim", PROMPT, NEGATIVE, latents=lat0, latent=False, **kw)
    assert tuple(clip.shape) == (1, 3, 9, H, W)
    pt = _t2v(pipe, PROMPT, NEGATIVE, kw, None, "pt", latents=lat0, return_dict=False)
    assert isinstance(pt, tuple) and len(pt) == 1 and torch.equal(_bits(pt[0]), _bits(po.torch_frames(clip, "pt")))
    arr = _t2v(pipe, PROMPT, NEGATIVE, kw, None, "np", latents=lat0).frames
    assert isinstance(arr, np.ndarray) and np.array_equal(arr, po.torch_frames(clip, "np").cpu().numpy())
    pil = _t2v(pipe, PROMPT, NEGATIVE, kw, None, "pil", latents=lat0).frames
    u8 = po.torch_frames(clip, "pil").cpu().numpy()
    assert len(pil) == 1 and len(pil[0]) == 9 and all(np.array_equal(np.asarray(f), u8[0, t]) for t, f in enumerate(pil[0]))


# --------------------------------------------------------------------------------------------------------- video-to-video
def _v2v(pipe, video, prompt, negative, kw, generator, output_type, **more):
    kw = dict(kw)
    return pipe(video, prompt, negative, height=H, width=W, num_inference_steps=kw.pop("steps"), generator=generator,
                output_type=output_type, max_sequence_length=SEQ, **kw, **more)


@pytest.mark.parametrize("sched", ["ddim", "dpm"])
@pytest.mark.parametrize("strength,frames", [(1.0, 5), (0.8, 9), (0.2, 9)])
def test_v2v_call_equals_the_stages_by_hand_bitwise(parts, sched, strength, frames):
    """5 steps: strength 1.0 / 0.8 / 0.2 start at step 0 / 1 / 4.  The 9-frame clip crosses the encoder's 1 | 8 frame batches"""
    kw = dict(strength=strength, steps=5, guidance_scale=6.0, use_dynamic_cfg=strength == 0.8)
    pipe, video = parts.pipe(V2V, "sincos", sched), sp.pil_clip(frames)
    g0, g = _gen(5), _gen(5)
    want = sp.by_hand_v2v(parts, "sincos", sched, video, PROMPT, NEGATIVE, generator=g0, **kw)
    assert tuple(want.shape) == (1, (frames - 1) // 4 + 1, 16, 6, 10)
    got = _v2v(pipe, video, PROMPT, NEGATIVE, kw, g, "latent", num_frames=frames).frames
    assert torch.equal(got, want) and _same_state(g, g0)
    assert pipe.num_timesteps == {1.0: 5, 0.8: 4, 0.2: 1}[strength]
    # the loop written over the launches is the same loop
    hand = sp.by_hand_v2v(parts, "sincos", sched, video, PROMPT, NEGATIVE, generator=_gen(5), loop="hand", **kw)
    assert torch.equal(hand, want)


def test_v2v_batch_output_types_and_callback(parts):
    kw = dict(strength=0.8, steps=3, guidance_scale=6.0)
    pipe = parts.pipe(V2V, "sincos", "dpm")
    videos, prompts = [sp.pil_clip(5, 51), sp.pil_clip(5, 71)], [PROMPT, "a second prompt"]
    g0, g = _gen(40, 2), _gen(40, 2)
    want = sp.by_hand_v2v(parts, "sincos", "dpm", videos, prompts, None, generator=g0, **kw)
    seen = []
    got = _v2v(pipe, videos, prompts, None, kw, g, "latent",
               callback_on_step_end=lambda p, i, t, d: seen.append((i, int(t), int(p.current_timestep)))).frames
    assert tuple(got.shape) == (2, 2, 16, 6, 10) and torch.equal(got, want) and _same_state(g, g0) and not torch.equal(got[0], got[1])
    assert seen == [(0, 666, 666), (1, 332, 332)]           # executed steps count from 0; 3 steps (999, 666, 332) at strength 0.8 skip 999
    one = _v2v(pipe, videos[0], prompts[0], None, kw, _gen(40), "latent").frames
    assert torch.equal(one[0], got[0])                      # a list of generators is per batch entry
    clip = sp.by_hand_v2v(parts, "sincos", "dpm", videos[0], PROMPT, NEGATIVE, generator=_gen(7), latent=False, **kw)
    assert tuple(clip.shape) == (1, 3, 8, H, W)             # 2 latent frames decode to 8: an even chunk doubles whole
    pt = _v2v(pipe, videos[0], PROMPT, NEGATIVE, kw, _gen(7), "pt").frames
    assert torch.equal(_bits(pt), _bits(po.torch_frames(clip, "pt")))
    arr = _v2v(pipe, videos[0], PROMPT, NEGATIVE, kw, _gen(7), "np").frames
    assert np.array_equal(arr, po.torch_frames(clip, "np").cpu().numpy())
    pil = _v2v(pipe, videos[0], PROMPT, NEGATIVE, kw, _gen(7), "pil").frames
    u8 = po.torch_frames(clip, "pil").cpu().numpy()
    assert len(pil[0]) == 8 and all(np.array_equal(np.asarray(f), u8[0, t]) for t, f in enumerate(pil[0]))


def test_v2v_given_latents_skip_the_encode(parts):
    class NoEncode:
        config, device, dtype = parts.vae.config, parts.vae.device, parts.vae.dtype

        def encode(self, *a, **k):
            raise AssertionError("the video was encoded")
    kw = dict(strength=0.8, steps=3, guidance_scale=6.0)
    lat0 = torch.randn(1, 3, 16, 6, 10, generator=_gen(8)).half()
    want = sp.by_hand_v2v(parts, "sincos", "ddim", None, PROMPT, NEGATIVE, latents=lat0, **kw)
    got = _v2v(parts.pipe(V2V, "sincos", "ddim", vae=NoEncode()), None, PROMPT, NEGATIVE, kw, None, "latent", latents=lat0).frames
    assert torch.equal(got, want)
    with pytest.raises(AssertionError, match="the video was encoded"):
        _v2v(parts.pipe(V2V, "sincos", "ddim", vae=NoEncode()), sp.pil_clip(5), PROMPT, NEGATIVE, kw, None, "latent")


@pytest.mark.parametrize("decoy", sp.V2V_DECOYS)
def test_v2v_wrong_calls_miss_the_equality(parts, decoy):
    kw = dict(strength=0.8, steps=4, guidance_scale=6.0, use_dynamic_cfg=True)
    video = sp.pil_clip(9)
    wrong = sp.by_hand_v2v(parts, "sincos", "dpm", video, PROMPT, NEGATIVE, generator=_gen(5), decoy=decoy, **kw)
    got = _v2v(parts.pipe(V2V, "sincos", "dpm"), video, PROMPT, NEGATIVE, kw, _gen(5), "latent").frames
    right = sp.by_hand_v2v(parts, "sincos", "dpm", video, PROMPT, NEGATIVE, generator=_gen(5), loop="hand", **kw)
    assert torch.equal(got, right) and not torch.equal(got, wrong), decoy
    print(f"decoy {decoy}: misses the class's latents by rel L2 {rel(wrong, right):.3e}")


# ----------------------------------------------------------------------------------------------------- denoise's defaults
@pytest.mark.parametrize("sched", ["ddim", "dpm"])
def test_denoise_start_step_zero_with_both_features_is_the_existing_call(sched):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    from cogvideox_support import aten_denoise
    m = hip_twin(tiny_oracle(), dev=DEV)
    lat, img, pe, dom, flow = loop_inputs()
    mk = pc.CogVideoXDDIMScheduler if sched == "ddim" else pc.CogVideoXDPMScheduler
    args = (lat, img, pe, dom.to(DEV), flow.to(DEV), 3, 6.0, True)
    a = pc.denoise(m, mk(), *args, generator=_gen(3))
    b = pc.denoise(m, mk(), *args, generator=_gen(3), start_step=0)
    assert torch.equal(a, b)
    if sched == "ddim":                                     # the parent's loop, statement by statement in ATen (cogvideox_support)
        want = aten_denoise(pc, m, mk(), lat.to(DEV), img.to(DEV), pe.to(DEV), dom.to(DEV), flow.to(DEV), 3, 6.0, lambda *a: None)
        assert torch.equal(a, want)
    for features, name in (((None, flow.to(DEV)), "domain_features"), ((dom.to(DEV), None), "flow_features")):
        with pytest.raises(LkgdHipError, match=f"`{name}` is None"):
            pc.denoise(m, mk(), lat, img, pe, *features, 3, 6.0, True)


# ------------------------------------------------------------------------------------------------- end to end, fp32 oracle
#: relative L2 of the HIP calls against the composed fp32 oracle, measured on the MI355X (see the tests' docstrings); each quantity is
#: gated at three times its measured value - the margin test_cogvideox_pipeline_gpu.py gives the I2V call's 3.9e-3
MEASURED = {"t2v_latents": 4.002e-3, "t2v_frames": 3.947e-3, "v2v_latents": 1.670e-3, "v2v_frames": 1.735e-3}


def _gate(name):
    return 3 * MEASURED[name]


def _ids(parts):
    tok = dict(padding="max_length", max_length=SEQ, truncation=True, add_special_tokens=True, return_tensors="pt")
    return parts.tok([PROMPT], **tok).input_ids, parts.tok([NEGATIVE], **tok).input_ids


def test_t2v_call_against_the_fp32_oracle(parts):
    """One DDIM call (9 frames, 2 steps, guidance 6, given initial noise) against ``sp.oracle_t2v``: transformers' T5, the DiT oracle
    without its fuse line, the oracle's DDIM scheduler, the VAE decoder oracle.  Prints the relative L2 of the final latents and of
    the ``pt`` frames.  Measured: latents 4.002e-3, ``pt`` frames 3.947e-3 (the I2V call's 3.9e-3 / 3.6e-3: the same two fp16 loop steps
    behind the same one-layer T5); the gates are 3 x those, 1.201e-2 and 1.184e-2."""
    kw = dict(num_frames=9, steps=2, guidance_scale=6.0)
    lat0 = torch.randn(1, 3, 16, 6, 10, generator=_gen(8)).half()
    pipe = parts.pipe(T2V, "sincos", "ddim")
    got_lat = _t2v(pipe, PROMPT, NEGATIVE, kw, None, "latent", latents=lat0).frames
    got_pt = _t2v(pipe, PROMPT, NEGATIVE, kw, None, "pt", latents=lat0).frames
    ref_lat, ref_pt = sp.oracle_t2v(parts, *_ids(parts), lat0.float(), steps=2, guidance_scale=6.0)
    r_lat, r_pt = rel(got_lat, ref_lat), rel(got_pt, ref_pt)
    print(f"T2V HIP call vs the fp32 oracle: rel L2 latents {r_lat:.3e}, pt frames {r_pt:.3e}")
    assert bool(torch.isfinite(got_lat.float()).all()) and tuple(got_pt.shape) == tuple(ref_pt.shape) == (1, 9, 3, H, W)
    assert r_lat <= _gate("t2v_latents") and r_pt <= _gate("t2v_frames"), (r_lat, r_pt)


#: the video-to-video oracle case runs the DPM scheduler on the 5B models' tables (``snr_shift_scale`` 1.0 of their scheduler_config.json:
#: inference/cli_demo.py:134-140 installs the DPM class for the 5B models and recommends DDIM for the 2B).  See the test's docstring for
#: what the 2B tables (3.0) give
V2V_SHIFT = 1.0


def test_v2v_call_against_the_fp32_oracle(parts):
    """One DPM call (a 9-frame clip, strength 0.8 of 4 steps: 3 executed, guidance 6, dynamic) against ``sp.oracle_v2v``: the VAE
    encoder oracle's posterior with the pipeline's draw, ``add_noise`` in fp32, the DiT oracle without its fuse line, dpm_oracle's
    fp64 step with the pipeline's draws, the VAE decoder oracle.  Prints the relative L2 of the final latents and of the ``pt``
    frames, and the distance of the HIP result from each of the five decoys run through the oracle: every one lies at least ten times
    the gate away.
    Measured (``snr_shift_scale`` 1.0): latents 1.670e-3, ``pt`` frames 1.735e-3; the gates are 3 x those, 5.01e-3 and 5.21e-3, and ten
    times the gates 5.01e-2 and 5.21e-2.  The oracle's decoys lie 0.61 / 0.42 (noise drawn before the posterior sample), 0.79 / 0.47
    (``start_step`` off by one), 8.12e-2 / 7.82e-2 (``dynamic_guidance`` fed the untruncated step count), 1.10 / 0.60 (a second-order
    first step) and 1.06e-1 / 1.06e-1 (``add_noise`` at the schedule's first timestep) from the HIP result.
    Why the 5B tables: with the 2B tables (``snr_shift_scale`` 3.0) the call measured 1.602e-3 / 1.700e-3 and four decoys as far as
    here, but ``add_noise`` at the first timestep only 3.94e-2 / 3.96e-2 - 8.2 times that gate, not ten.  That is the schedule, not
    the code: the oracle's own decoy lies 3.93e-2 from the oracle's own result.  At strength 0.8 of 4 steps the clip enters with
    weight sqrt(alphas_cumprod[749]) = 0.105 (3.0) or 0.182 (1.0), and the tiny VAE's scaled latents have an rms of 0.23 against the
    noise's 1: noising at t = 999 instead removes 2 % or 4 % of the start.  The bit-level decoy test above runs on the 2B tables."""
    kw = dict(strength=0.8, steps=4, guidance_scale=6.0, use_dynamic_cfg=True)
    video = sp.pil_clip(9)
    pipe = parts.pipe(V2V, "sincos", "dpm", snr_shift_scale=V2V_SHIFT)
    got_lat = _v2v(pipe, video, PROMPT, NEGATIVE, kw, _gen(9), "latent").frames
    got_pt = _v2v(pipe, video, PROMPT, NEGATIVE, kw, _gen(9), "pt").frames
    ids, neg_ids = _ids(parts)
    clip = sp.host_video(video).half().float()
    post_shape, lat_shape = (1, 16, 3, 6, 10), (1, 3, 16, 6, 10)

    def oracle(decoy=None):
        start = 2 if decoy == "start_off_by_one" else 1
        orders = sp.dpm_orders(4, start, 999 if decoy == "second_order_first" else None)
        shapes = (lat_shape, post_shape) if decoy == "noise_first" else (post_shape, lat_shape)
        first, eps = sp.host_draws(_gen(9), shapes, orders, lat_shape)
        post, noise = (first[1], first[0]) if decoy == "noise_first" else first
        return sp.oracle_v2v(parts, clip, ids, neg_ids, post, noise, steps=4, strength=0.8, guidance_scale=6.0, eps=eps,
                             use_dynamic_cfg=True, decoy=None if decoy == "noise_first" else decoy, snr_shift_scale=V2V_SHIFT)
    assert sp.dpm_orders(4, 1) == [1, 2, 1] and sp.dpm_orders(4, 1, 999) == [2, 2, 1]
    ref_lat, ref_pt = oracle()
    r_lat, r_pt = rel(got_lat, ref_lat), rel(got_pt, ref_pt)
    print(f"V2V HIP call vs the fp32 oracle: rel L2 latents {r_lat:.3e}, pt frames {r_pt:.3e}")
    far = {}
    for decoy in sp.V2V_DECOYS:
        d_lat, d_pt = oracle(decoy)
        far[decoy] = (rel(got_lat, d_lat), rel(got_pt, d_pt))
        print(f"  oracle decoy {decoy}: HIP result rel L2 latents {far[decoy][0]:.3e}, pt frames {far[decoy][1]:.3e}")
    assert bool(torch.isfinite(got_lat.float()).all()) and tuple(got_pt.shape) == tuple(ref_pt.shape) == (1, 9, 3, H, W)
    assert r_lat <= _gate("v2v_latents") and r_pt <= _gate("v2v_frames"), (r_lat, r_pt)
    for decoy, (a, b) in far.items():
        assert a >= 10 * _gate("v2v_latents") and b >= 10 * _gate("v2v_frames"), (decoy, a, b)
