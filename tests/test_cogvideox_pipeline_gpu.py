"""``CogVideoXImageToVideoPipeline.__call__`` on the GPU (tests/cogvideox_pipeline_oracle.py holds the tiny components and the two
independent statements of the call).

* Composition, to the bit - the gate on the orchestration: ``pipe(...)`` equals the HIP stage functions called by hand in the
  reference's order with the same generator, for every output type, both schedulers, guidance on and off, a batch of two with two
  generators, given latents, given prompt embeddings and a ``patch_size_t`` model; every wrong order of ``DECOYS`` misses it.
* End to end against the composed fp32 CPU oracle (one DDIM case, the image-posterior draw and the initial noise handed to it).
* Launch accounting with the launch recorder, and the callback contract."""
import numpy as np
import pytest
import torch

import cogvideox_pipeline_oracle as po
from cogvideox_support import DEV, rel
from t5_support import GATE

pytestmark = pytest.mark.gpu

PROMPT, NEGATIVE = "a red kite over the dunes", "blurry"


@pytest.fixture(scope="module")
def parts():
    pytest.importorskip("transformers")
    return po.build()


def _gen(seed, n=None):
    return torch.Generator().manual_seed(seed) if n is None else [torch.Generator().manual_seed(seed + i) for i in range(n)]


def _state(g):
    return [x.get_state() for x in g] if isinstance(g, list) else [g.get_state()]


def _same_state(a, b):
    return all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))


def _bits(t):
    return t.detach().cpu().reshape(-1).contiguous().view(torch.uint8)


# --------------------------------------------------------------------------------------------------------- composition
#: name -> (model, scheduler, call keywords); generators and tensors are made per call from the seeds
CASES = {
    "ddim_cfg": ("sincos", "ddim", dict(num_frames=9, steps=2, guidance_scale=6.0)),
    "dpm_cfg_dynamic": ("sincos", "dpm", dict(num_frames=9, steps=3, guidance_scale=6.0, use_dynamic_cfg=True)),
    "ddim_no_cfg": ("sincos", "ddim", dict(num_frames=5, steps=2, guidance_scale=1.0)),
    "dpm_no_cfg": ("sincos", "dpm", dict(num_frames=5, steps=2, guidance_scale=1.0)),
    "v15_ddim": ("v15", "ddim", dict(num_frames=9, steps=2, guidance_scale=6.0)),
    "v15_dpm": ("v15", "dpm", dict(num_frames=9, steps=2, guidance_scale=6.0)),
}


def _call(pipe, image, prompt, negative, kw, generator, output_type, **more):
    kw = dict(kw)
    return pipe(image, prompt, negative, height=po.H, width=po.W, num_frames=kw.pop("num_frames"), num_inference_steps=kw.pop("steps"),
                generator=generator, output_type=output_type, max_sequence_length=po.SEQ, **kw, **more)


@pytest.mark.parametrize("case", list(CASES))
def test_call_equals_the_stages_by_hand_bitwise(parts, case):
    kind, sched, kw = CASES[case]
    pipe, image = parts.pipe(kind, sched), po.pil_image()
    g0 = _gen(5)
    want_lat = po.by_hand(parts, kind, sched, image, PROMPT, NEGATIVE, generator=g0, latent=True, **kw)
    want_clip = po.by_hand(parts, kind, sched, image, PROMPT, NEGATIVE, generator=_gen(5), **kw)
    latent_frames = (kw["num_frames"] - 1) // 4 + 1
    padded = latent_frames + (latent_frames % 2 if kind == "v15" else 0)
    # 3 latent frames decode to 9 frames (the v15 padding frame gone); 2 latent frames to 8: an even chunk doubles whole, as diffusers
    frames = {9: 9, 5: 8}[kw["num_frames"]]
    assert tuple(want_lat.shape) == (1, padded, 16, 6, 10) and tuple(want_clip.shape) == (1, 3, frames, po.H, po.W)

    g = _gen(5)
    out = _call(pipe, image, PROMPT, NEGATIVE, kw, g, "latent")
    assert type(out).__name__ == "CogVideoXPipelineOutput" and out.frames.dtype == torch.float16
    assert torch.equal(out.frames, want_lat) and _same_state(g, g0)          # :905-911: the latents keep their padding frames
    assert pipe.num_timesteps == kw["steps"] and pipe.current_timestep is None

    pt = _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "pt", return_dict=False)
    assert isinstance(pt, tuple) and len(pt) == 1 and pt[0].is_cuda and tuple(pt[0].shape) == (1, frames, 3, po.H, po.W)
    assert torch.equal(_bits(pt[0]), _bits(po.torch_frames(want_clip, "pt")))
    arr = _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "np").frames
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and arr.shape == (1, frames, po.H, po.W, 3)
    assert np.array_equal(arr, po.torch_frames(want_clip, "np").cpu().numpy())
    pil = _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "pil").frames
    u8 = po.torch_frames(want_clip, "pil").cpu().numpy()
    assert len(pil) == 1 and len(pil[0]) == frames
    for t, frame in enumerate(pil[0]):
        assert frame.size == (po.W, po.H) and np.array_equal(np.asarray(frame), u8[0, t]), t


@pytest.mark.parametrize("sched", ["ddim", "dpm"])
def test_two_prompts_with_two_generators(parts, sched):
    """without guidance: under it the reference hands the fuse 2B text rows and B feature rows, which neither it nor
    ``lkgd_lk_fuse_tokens`` takes for B > 1"""
    kw = dict(num_frames=5, steps=2, guidance_scale=1.0)
    images, prompts, negs = [po.pil_image(31), po.pil_image(32)], [PROMPT, "a second prompt"], None
    g0, g = _gen(40, 2), _gen(40, 2)
    want = po.by_hand(parts, "sincos", sched, images, prompts, negs, generator=g0, latent=True, **kw)
    got = _call(parts.pipe("sincos", sched), images, prompts, negs, kw, g, "latent").frames
    assert tuple(got.shape) == (2, 2, 16, 6, 10) and torch.equal(got, want) and _same_state(g, g0)
    assert not torch.equal(got[0], got[1])
    # entry 0 is the single call with generator 0: a list of generators is per batch entry
    one = _call(parts.pipe("sincos", sched), images[0], prompts[0], None, kw, _gen(40), "latent").frames
    assert torch.equal(one[0], got[0])


def test_given_latents_and_given_prompt_embeddings(parts):
    from lkgd_amd import cogvideox as pc
    kw = dict(num_frames=9, steps=2, guidance_scale=6.0)
    pipe, image = parts.pipe(), po.pil_image()
    lat0 = torch.randn(1, 3, 16, 6, 10, generator=_gen(8)).half()
    want = po.by_hand(parts, "sincos", "ddim", image, PROMPT, NEGATIVE, generator=_gen(6), latents=lat0, latent=True, **kw)
    got = _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(6), "latent", latents=lat0).frames
    assert torch.equal(got, want)
    assert not torch.equal(got, _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(6), "latent").frames)      # the given latents took part
    # embeddings in place of the prompts: the same result as the prompts they were encoded from
    pe, ne = pc.encode_prompt(parts.te, parts.tok, PROMPT, NEGATIVE, True, 1, None, None, po.SEQ, DEV)
    emb = _call(pipe, image, None, None, kw, _gen(6), "latent", latents=lat0, prompt_embeds=pe, negative_prompt_embeds=ne).frames
    assert torch.equal(emb, want)
    hand = po.by_hand(parts, "sincos", "ddim", image, generator=_gen(6), latents=lat0, prompt_embeds=pe, negative_prompt_embeds=ne,
                      latent=True, **kw)
    assert torch.equal(hand, want)


# -------------------------------------------------------------------------------------------------------------- decoys
@pytest.mark.parametrize("decoy", po.DECOYS)
def test_wrong_orders_miss_the_equality(parts, decoy):
    kind = "v15" if decoy == "keep_padding" else "sincos"
    kw = dict(num_frames=9, steps=2, guidance_scale=6.0)
    image = po.pil_image()
    latent = decoy in ("positive_first", "noise_first", "fp32_image")
    right = po.by_hand(parts, kind, "ddim", image, PROMPT, NEGATIVE, generator=_gen(5), latent=latent, **kw)
    wrong = po.by_hand(parts, kind, "ddim", image, PROMPT, NEGATIVE, generator=_gen(5), latent=latent, decoy=decoy, **kw)
    got = _call(parts.pipe(kind, "ddim"), image, PROMPT, NEGATIVE, kw, _gen(5), "latent" if latent else "pt").frames
    if latent:
        assert torch.equal(got, right) and not torch.equal(got, wrong), decoy
    else:
        assert torch.equal(_bits(got), _bits(po.torch_frames(right, "pt")))
        w = po.torch_frames(wrong, "pt")
        assert tuple(w.shape) != tuple(got.shape) or not torch.equal(_bits(got), _bits(w)), decoy
    print(f"decoy {decoy}: misses the class's result" + ("" if tuple(wrong.shape) != tuple(right.shape) else
                                                         f" by rel L2 {rel(wrong, right):.3e}"))


# ------------------------------------------------------------------------------------------------- end to end, fp32 oracle
#: relative L2 of the HIP call against the fp32 oracle, measured on the MI355X (see the test's docstring).  Neither leaves the project's
#: 1e-2 (t5_support.GATE) three times its size in headroom, so each quantity is gated at three times its measured value
MEASURED = {"latents": 3.858e-3, "frames": 3.603e-3}
assert max(MEASURED.values()) * 3 > GATE
E2E_GATE = {k: 3 * v for k, v in MEASURED.items()}


def test_call_against_the_fp32_oracle(parts):
    """One DDIM call (9 frames, 2 steps, guidance 6) against ``po.oracle_call`` on the same image with the same posterior draw and
    initial noise.  Prints the relative L2 of the final latents and of the ``pt`` frames, and of three decoys run through the oracle.
    Measured: latents 3.858e-3, ``pt`` frames 3.603e-3 - two fp16 loop steps behind a one-layer T5 at d_model 4096, each a few 1e-3 by
    the stages' own tests; the gates are 3 x those, 1.157e-2 and 1.081e-2.  The oracle's decoys lie 0.60 / 0.37 (positive prompt
    first), 0.67 / 0.42 (noise drawn before the image sample) and 3.9e-3 / 9.2e-2 (scaling factor omitted: the latents do not see
    it, the frames do) from the HIP result: all three outside."""
    kw = dict(num_frames=9, steps=2, guidance_scale=6.0)
    image = po.pil_image()
    lat0 = torch.randn(1, 3, 16, 6, 10, generator=_gen(8)).half()
    pipe = parts.pipe()
    got_lat = _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(9), "latent", latents=lat0).frames
    got_pt = _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(9), "pt", latents=lat0).frames
    tok = dict(padding="max_length", max_length=po.SEQ, truncation=True, add_special_tokens=True, return_tensors="pt")
    ids, neg_ids = parts.tok([PROMPT], **tok).input_ids, parts.tok([NEGATIVE], **tok).input_ids
    image_noise = torch.randn((1, 16, 1, 6, 10), generator=_gen(9), dtype=torch.float16).float()
    x = po.host_image(image).half().float()

    def oracle(decoy=None):
        return po.oracle_call(parts, x, ids, neg_ids, image_noise, lat0.float(), steps=2, guidance_scale=6.0, decoy=decoy)
    ref_lat, ref_pt = oracle()
    r_lat, r_pt = rel(got_lat, ref_lat), rel(got_pt, ref_pt)
    print(f"HIP call vs the fp32 oracle: rel L2 latents {r_lat:.3e}, pt frames {r_pt:.3e} (gates {E2E_GATE['latents']:.3e}, {E2E_GATE['frames']:.3e})")
    outside = 0
    for decoy in ("positive_first", "noise_first", "no_scaling"):
        d_lat, d_pt = oracle(decoy)
        a, b = rel(got_lat, d_lat), rel(got_pt, d_pt)
        print(f"  oracle decoy {decoy}: HIP result rel L2 latents {a:.3e}, pt frames {b:.3e}")
        outside += a > E2E_GATE["latents"] or b > E2E_GATE["frames"]
    assert bool(torch.isfinite(got_lat.float()).all()) and tuple(got_pt.shape) == tuple(ref_pt.shape)
    assert r_lat <= E2E_GATE["latents"] and r_pt <= E2E_GATE["frames"], (r_lat, r_pt)
    assert outside >= 2, outside


# ------------------------------------------------------------------------------------------------------ launch accounting
def _recorded(run):
    """one eager warm-up, then a recorded call (tests/test_cogvideox_launches_gpu.py): the entry-point names, in order"""
    from lkgd_amd import replay
    run()
    torch.cuda.synchronize()
    with replay.strict(False):
        with replay.record() as p:
            run()
    torch.cuda.synchronize()
    names = [name for _, _, name, _ in p.calls]
    p.release()
    return names


def test_frames_out_and_image_in_are_one_launch_each(parts):
    from lkgd_amd.video_processor import VideoProcessor
    vp = VideoProcessor(vae_scale_factor=8)
    clip = (1.2 * torch.randn(1, 3, 5, po.H, po.W, generator=_gen(3))).half().to(DEV)
    for output_type in ("pil", "np", "pt"):
        assert _recorded(lambda: vp.postprocess_video(clip, output_type)) == ["lkgd_video_postprocess"], output_type
    image = po.pil_image()
    assert _recorded(lambda: vp.preprocess(image, po.H, po.W, device=DEV, dtype=torch.float16)) == ["lkgd_image_preprocess"]
    assert _recorded(lambda: vp.preprocess([image, image], po.H, po.W, device=DEV, dtype=torch.float16)) == ["lkgd_image_preprocess"]


@pytest.mark.parametrize("sched", ["ddim", "dpm"])
def test_call_adds_two_launches_to_the_stages(parts, sched):
    kw = dict(num_frames=9, steps=2, guidance_scale=6.0)
    pipe, image = parts.pipe("sincos", sched), po.pil_image()
    stages = _recorded(lambda: po.by_hand(parts, "sincos", sched, image, PROMPT, NEGATIVE, generator=_gen(5), **kw))
    call = _recorded(lambda: _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "pil"))
    assert call.count("lkgd_image_preprocess") == 1 and call.count("lkgd_video_postprocess") == 1 and call[-1] == "lkgd_video_postprocess"
    assert not {"lkgd_image_preprocess", "lkgd_video_postprocess"} & set(stages)
    assert [n for n in call if n not in ("lkgd_image_preprocess", "lkgd_video_postprocess")] == stages
    # the image kernel comes behind the prompt's launches and in front of the ViTs'
    assert call.index("lkgd_image_preprocess") < call.index("lkgd_vit_patchify")
    assert "lkgd_t5_embed_rows" in call[:call.index("lkgd_image_preprocess")]


# --------------------------------------------------------------------------------------------------------------- callbacks
def test_callbacks_observe_and_may_not_replace(parts):
    from lkgd_amd._lib import LkgdHipError
    kw = dict(num_frames=5, steps=2, guidance_scale=6.0)
    pipe, image = parts.pipe(), po.pil_image()
    plain = _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "latent").frames
    seen = []

    def observe(p, i, t, tensors):
        seen.append((p, i, int(t), int(p.current_timestep), {k: v.clone() for k, v in tensors.items()}))
        return tensors

    got = _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "latent", callback_on_step_end=observe,
                callback_on_step_end_tensor_inputs=["latents", "prompt_embeds", "negative_prompt_embeds"]).frames
    assert torch.equal(got, plain) and [s[1] for s in seen] == [0, 1] and all(s[0] is pipe for s in seen)
    assert [s[2] for s in seen] == pipe.scheduler.timesteps.tolist() == [s[3] for s in seen]
    assert set(seen[0][4]) == {"latents", "prompt_embeds", "negative_prompt_embeds"}
    assert tuple(seen[0][4]["prompt_embeds"].shape) == (2, po.SEQ, 4096) and tuple(seen[0][4]["negative_prompt_embeds"].shape) == (1, po.SEQ, 4096)
    assert torch.equal(seen[1][4]["latents"], plain) and not torch.equal(seen[0][4]["latents"], plain)
    # a callback that returns nothing only observes, with the default tensor inputs
    names = []
    _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "latent", callback_on_step_end=lambda p, i, t, d: names.append(sorted(d)))
    assert names == [["latents"], ["latents"]]
    for name in ("latents", "prompt_embeds"):
        with pytest.raises(LkgdHipError, match=f"`{name}`"):
            _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "latent", callback_on_step_end=lambda p, i, t, d: {name: d[name] * 2},
                  callback_on_step_end_tensor_inputs=["latents", "prompt_embeds"])
    with pytest.raises(ValueError, match="callback_on_step_end_tensor_inputs"):
        _call(pipe, image, PROMPT, NEGATIVE, kw, _gen(5), "latent", callback_on_step_end=observe, callback_on_step_end_tensor_inputs=["image"])
