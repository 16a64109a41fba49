"""``CogVideoXPipeline`` (text-to-video) and ``CogVideoXVideoToVideoPipeline`` without a GPU ([EXT] diffusers' classes, parity unpinned):
``get_timesteps`` against a literal table, ``add_noise`` against its formula, ``denoise``'s truncated loop seen through spies (the
launches replaced by recorders: which timesteps run, with which ``coefficients`` arguments, guidance values, draws and callback
indices), the ``check_inputs`` errors, exports and signatures, ``from_pretrained`` of a directory of tiny components, and the host form
of ``preprocess_video`` for every accepted input."""
import inspect
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cogvideox_vae_encoder_oracle as eo
from cogvideox_support import tiny_cpu_model
from t5_support import TINY_A


# ---------------------------------------------------------------------------------------------------------- get_timesteps
#: num_inference_steps = 5: strength -> t_start.  int(5 * s) is 5, 4, 2, 1 and 0 for these s (checked below: no product lands under
#: its integer)
T_START = {1.0: 0, 0.8: 1, 0.5: 3, 0.2: 4}


def test_get_timesteps_against_the_table():
    from lkgd_amd import cogvideox as pc
    assert [int(5 * s) for s in (1.0, 0.8, 0.5, 0.2, 0.1)] == [5, 4, 2, 1, 0]
    for cls in (pc.CogVideoXDDIMScheduler, pc.CogVideoXDPMScheduler):
        s = cls()
        s.set_timesteps(5)
        assert s.timesteps.tolist() == [999, 799, 599, 399, 199]
        for strength, t_start in T_START.items():
            times, n, start = pc.get_timesteps(s, 5, strength)
            assert (times.tolist(), n, start) == ([999, 799, 599, 399, 199][t_start:], 5 - t_start, t_start), strength
        with pytest.raises(ValueError, match=r"`strength`=0\.1 with `num_inference_steps`=5"):
            pc.get_timesteps(s, 5, 0.1)
        with pytest.raises(ValueError, match="`strength`=0.0"):
            pc.get_timesteps(s, 5, 0.0)


# -------------------------------------------------------------------------------------------------------------- add_noise
@pytest.mark.parametrize("cls", ["CogVideoXDDIMScheduler", "CogVideoXDPMScheduler"])
def test_add_noise_is_its_formula(cls):
    from lkgd_amd import cogvideox as pc
    s = getattr(pc, cls)()
    g = torch.Generator().manual_seed(3)
    x, n = torch.randn(2, 3, 16, 6, 10, generator=g), torch.randn(2, 3, 16, 6, 10, generator=g)
    t = torch.tensor([799, 199])                                    # a per-entry timestep vector
    ac = s.alphas_cumprod
    assert ac.dtype == torch.float64 and float(ac[999]) == 0.0
    # fp32: exact
    a32, s32 = ac.float()[t] ** 0.5, (1 - ac.float()[t]) ** 0.5
    want = a32.view(2, 1, 1, 1, 1) * x + s32.view(2, 1, 1, 1, 1) * n
    got = s.add_noise(x, n, t)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert not torch.equal(got[0], s.add_noise(x, n, torch.tensor([199, 199]))[0])
    assert torch.equal(s.add_noise(x[:1], n[:1], torch.tensor([999])), n[:1])           # zero terminal SNR: the noise alone
    # fp16: the table cast to fp16, then both products and the sum each rounded to fp16
    xh, nh, ach = x.half(), n.half(), ac.half()
    a16, s16 = (ach[t] ** 0.5).view(2, 1, 1, 1, 1), ((1 - ach[t]) ** 0.5).view(2, 1, 1, 1, 1)
    assert a16.dtype == torch.float16
    p1 = (a16.float() * xh.float()).half()
    p2 = (s16.float() * nh.float()).half()
    want16 = (p1.float() + p2.float()).half()
    got16 = s.add_noise(xh, nh, t)
    assert got16.dtype == torch.float16 and torch.equal(got16, want16)
    fused = (a16.float() * xh.float() + s16.float() * nh.float()).half()                # one rounding: not the statement
    assert not torch.equal(fused, want16)
    # one timestep for the whole batch, as ``timesteps[:1].repeat(B)`` hands it over
    assert torch.equal(s.add_noise(x, n, torch.tensor([599]).repeat(2)), ac.float()[599] ** 0.5 * x + (1 - ac.float()[599]) ** 0.5 * n)


# ------------------------------------------------------------------------------------------------- the truncated loop, spied
class _Spy:
    """``denoise`` with its launches replaced by recorders: a transformer stub, ``ops.dit_patch_rows`` / the two step launches as
    functions that note their arguments"""

    def __init__(self, monkeypatch, dpm=True):
        from lkgd_amd import cogvideox as pc
        self.pc, self.coef, self.steps, self.times, self.draws = pc, [], [], [], []
        spy = self
        base = pc.CogVideoXDPMScheduler if dpm else pc.CogVideoXDDIMScheduler

        class Sched(base):
            def coefficients(self, t, *back):
                spy.coef.append((t,) + back)
                return super().coefficients(t, *back)
        self.sched = Sched()
        cfg = SimpleNamespace(patch_size=2, patch_size_t=None, use_rotary_positional_embeddings=False)

        def forward_rows(rows, grid, text, t, **kw):
            spy.times.append(t)
            spy.text = text
            return rows
        self.transformer = SimpleNamespace(config=cfg, device=torch.device("cpu"), ofs_embedding=None, forward_rows=forward_rows,
                                           fused_text=lambda *a: pytest.fail("fused_text was called"))
        monkeypatch.setattr(pc.ops, "dit_patch_rows", lambda lat, img, p, out=None, **kw: torch.zeros(1))
        monkeypatch.setattr(pc.ops, "dit_cfg_dpm_step", lambda rows, lat, x0, eps, p, n, order, g, k, **kw: spy.steps.append((order, g)))
        monkeypatch.setattr(pc.ops, "dit_cfg_ddim_step", lambda rows, lat, p, n, g, *coef, **kw: spy.steps.append((1, g)))
        real = pc.dpm_noise
        monkeypatch.setattr(pc, "dpm_noise", lambda shape, dtype, dev, gen, order: (spy.draws.append(order), real(shape, dtype, dev, gen, order))[1])

    def run(self, steps, start_step=0, dynamic=False, features=(None, None), **kw):
        lat, pe = torch.zeros(1, 2, 16, 6, 10), torch.ones(2, 4, 4096)
        return self.pc.denoise(self.transformer, self.sched, lat, None, pe, features[0], features[1], steps, 6.0, dynamic,
                               start_step=start_step, **kw)


def test_first_executed_dpm_step_after_truncation_is_first_order(monkeypatch):
    spy = _Spy(monkeypatch)
    seen = []
    spy.run(5, start_step=2, callback=lambda i, t, lat: seen.append((i, t)))
    assert spy.times == [599.0, 399.0, 199.0]
    assert spy.coef == [(599, None), (399, 599), (199, 399)]            # no previous timestep: t_back None, not the skipped 799
    assert [o for o, _ in spy.steps] == [1, 2, 1] and spy.draws == [1, 2, 1]     # one draw, two draws; the last step is first order
    assert seen == [(0, 599), (1, 399), (2, 199)]                       # the callback counts executed steps
    assert spy.text.dtype == torch.float16 and spy.text.is_contiguous() and torch.equal(spy.text, torch.ones(2, 4, 4096).half())
    # the whole schedule: what the loop did before ``start_step`` existed
    full = _Spy(monkeypatch)
    full.run(5)
    assert full.coef == [(999, None), (799, 999), (599, 799), (399, 599), (199, 399)] and full.draws == [1, 2, 2, 2, 1]


def test_dynamic_guidance_takes_the_truncated_step_count(monkeypatch):
    from lkgd_amd import cogvideox as pc
    spy = _Spy(monkeypatch, dpm=False)
    spy.run(5, start_step=2, dynamic=True)
    assert [g for _, g in spy.steps] == [pc.dynamic_guidance(6.0, 3, t) for t in (599, 399, 199)]
    assert [g for _, g in spy.steps] != [pc.dynamic_guidance(6.0, 5, t) for t in (599, 399, 199)]
    full = _Spy(monkeypatch, dpm=False)
    full.run(5, dynamic=True)
    assert [g for _, g in full.steps] == [pc.dynamic_guidance(6.0, 5, t) for t in (999, 799, 599, 399, 199)]


def test_denoise_refuses_a_start_step_outside_the_schedule_and_one_feature(monkeypatch):
    from lkgd_amd._lib import LkgdHipError
    spy = _Spy(monkeypatch)
    for bad in (-1, 5, 6):
        with pytest.raises(ValueError, match=f"start_step={bad}"):
            spy.run(5, start_step=bad)
    f = torch.zeros(1, 1, 1000)
    with pytest.raises(LkgdHipError, match="`domain_features` is None"):
        spy.run(5, features=(None, f))
    with pytest.raises(LkgdHipError, match="`flow_features` is None"):
        spy.run(5, features=(f, None))
    assert spy.steps == []


# ---------------------------------------------------------------------------------------------------------- the pipelines
def _stub_pipe(cls, patch_size_t=None, ofs_embed_dim=None):
    """a pipeline of configuration stubs: everything up to the first use of a module runs on the CPU"""
    from lkgd_amd import pipeline_cogvideox as pp
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(64, 64, 128, 128), temporal_compression_ratio=4, scaling_factor=0.7))
    tr = SimpleNamespace(config=SimpleNamespace(sample_height=6, sample_width=10, sample_frames=9, patch_size=2, patch_size_t=patch_size_t,
                                                in_channels=16, use_rotary_positional_embeddings=patch_size_t is not None,
                                                ofs_embed_dim=ofs_embed_dim),
                         device=torch.device("cpu"))
    return getattr(pp, cls)(tokenizer=None, text_encoder=None, vae=vae, transformer=tr, scheduler=None)


COMMON = dict(prompt=None, negative_prompt=None, height=None, width=None, num_frames=None, num_inference_steps=50, timesteps=None,
              guidance_scale=6, use_dynamic_cfg=False, num_videos_per_prompt=1, eta=0.0, generator=None, latents=None, prompt_embeds=None,
              negative_prompt_embeds=None, output_type="pil", return_dict=True, attention_kwargs=None, callback_on_step_end=None,
              callback_on_step_end_tensor_inputs=["latents"], max_sequence_length=226)


def test_exports_and_signatures():
    from lkgd_amd import pipeline_cogvideox as pp
    t2v, v2v, i2v = pp.CogVideoXPipeline, pp.CogVideoXVideoToVideoPipeline, pp.CogVideoXImageToVideoPipeline
    for cls in (t2v, v2v):
        assert list(inspect.signature(cls.__init__).parameters) == ["self", "tokenizer", "text_encoder", "vae", "transformer", "scheduler"]
        p = _stub_pipe(cls.__name__)
        assert (p.vae_scale_factor_spatial, p.vae_scale_factor_temporal, p.vae_scaling_factor_image) == (8, 4, 0.7)
        assert set(p.components) == {"tokenizer", "text_encoder", "vae", "transformer", "scheduler"}
        assert p.enable_model_cpu_offload() is None and p.guidance_scale is None and p.interrupt is False
        for name in ("load_lora_weights", "fuse_lora", "unfuse_lora", "set_adapters", "unload_lora_weights", "encode_prompt",
                     "decode_latents", "to", "from_pretrained", "check_inputs", "prepare_latents"):
            assert callable(getattr(cls, name)), name
    sig = inspect.signature(t2v.__call__)
    assert list(sig.parameters) == ["self"] + list(COMMON) and {k: sig.parameters[k].default for k in COMMON} == COMMON
    sig = inspect.signature(v2v.__call__)
    want = {**COMMON, "strength": 0.8}
    assert list(sig.parameters)[:2] == ["self", "video"] and set(list(sig.parameters)[2:]) == set(want)
    assert {k: sig.parameters[k].default for k in want} == want
    # the three classes share one base, and the I2V class keeps its own components
    assert t2v.__mro__[2] is v2v.__mro__[2] and i2v.__mro__[1] is t2v.__mro__[2]
    assert "domain_model" in inspect.signature(i2v.__init__).parameters
    assert "CogVideoXPipeline" in pp.__doc__ and "CogVideoXVideoToVideoPipeline" in pp.__doc__


def _frames(T, size=(80, 48)):
    import PIL.Image
    return [PIL.Image.fromarray(np.full((size[1], size[0], 3), 10 * t, dtype=np.uint8)) for t in range(T)]


def test_check_inputs_of_the_text_to_video_class():
    p = _stub_pipe("CogVideoXPipeline")
    pe = torch.zeros(1, 4, 8)
    ok = dict(prompt="a", height=48, width=80, negative_prompt=None, callback_on_step_end_tensor_inputs=["latents"])
    p.check_inputs(**ok)
    p.check_inputs(**{**ok, "prompt": None, "prompt_embeds": pe, "negative_prompt_embeds": pe})
    for over, msg in ((dict(height=50), "divisible by 8 but are 50 and 80"),
                      (dict(callback_on_step_end_tensor_inputs=["video"]), r"has to be in .*but found \['video'\]"),
                      (dict(prompt_embeds=pe), "Cannot forward both `prompt`: a and `prompt_embeds`"),
                      (dict(prompt=None), "Provide either `prompt` or `prompt_embeds`"),
                      (dict(prompt=3), "`prompt` has to be of type `str` or `list`"),
                      (dict(prompt=None, prompt_embeds=pe, negative_prompt_embeds=torch.zeros(1, 5, 8)), "must have the same shape")):
        with pytest.raises(ValueError, match=msg):
            p.check_inputs(**{**ok, **over})


def test_check_inputs_of_the_video_to_video_class():
    p = _stub_pipe("CogVideoXVideoToVideoPipeline")
    ok = dict(prompt="a", height=48, width=80, strength=0.8, negative_prompt=None, callback_on_step_end_tensor_inputs=["latents"],
              video=_frames(9))
    p.check_inputs(**ok)
    p.check_inputs(**{**ok, "num_frames": 9})
    p.check_inputs(**{**ok, "video": None, "latents": torch.zeros(1, 3, 16, 6, 10)})
    p.check_inputs(**{**ok, "video": torch.zeros(5, 3, 48, 80), "num_frames": 5})          # a tensor clip is [T, C, H, W]
    p.check_inputs(**{**ok, "video": [_frames(5), _frames(5)], "prompt": ["a", "b"], "num_frames": 5})
    for over, msg in ((dict(strength=1.5), r"strength should in \[0.0, 1.0\] but is 1.5"),
                      (dict(strength=-0.1), r"strength should in \[0.0, 1.0\] but is -0.1"),
                      (dict(latents=torch.zeros(1, 3, 16, 6, 10)), "Only one of `video` or `latents`"),
                      (dict(video=None), "Provide either `video` or `latents`"),
                      (dict(num_frames=49), "`num_frames`=49 differs from the 9 frames of `video`"),
                      (dict(height=50), "divisible by 8"),
                      (dict(prompt=None), "Provide either `prompt` or `prompt_embeds`")):
        with pytest.raises(ValueError, match=msg):
            p.check_inputs(**{**ok, **over})
    # a temporal-patch model: the class does not pad
    q = _stub_pipe("CogVideoXVideoToVideoPipeline", patch_size_t=2)
    q.check_inputs(**{**ok, "video": _frames(5)})                                           # 2 latent frames
    with pytest.raises(ValueError, match="`patch_size_t`=2 does not divide the 3 latent frames"):
        q.check_inputs(**ok)
    with pytest.raises(ValueError, match="`patch_size_t`=2 does not divide the 3 latent frames"):
        q.check_inputs(**{**ok, "video": None, "latents": torch.zeros(1, 3, 16, 6, 10)})
    # through __call__: the checks come before anything touches a module
    with pytest.raises(ValueError, match="`num_frames`=49"):
        p(_frames(9), "a", height=48, width=80, num_frames=49)
    with pytest.raises(ValueError, match="strength"):
        p(_frames(9), "a", height=48, width=80, strength=2)


@pytest.mark.parametrize("cls", ["CogVideoXPipeline", "CogVideoXVideoToVideoPipeline"])
@pytest.mark.parametrize("kw,name", [(dict(timesteps=[999, 500]), "timesteps"), (dict(eta=0.5), "eta"),
                                     (dict(attention_kwargs={"scale": 1.0}), "attention_kwargs")])
def test_arguments_the_loop_cannot_honour_raise_and_name_themselves(cls, kw, name):
    from lkgd_amd._lib import LkgdHipError
    p = _stub_pipe(cls)
    first = (_frames(5),) if "VideoToVideo" in cls else ()
    with pytest.raises(LkgdHipError, match=f"{cls}: .*`{name}`"):
        p(*first, "a", height=48, width=80, **kw)
    with pytest.raises(LkgdHipError, match=f"{cls}: .*`ofs_embed_dim`"):
        _stub_pipe(cls, patch_size_t=2, ofs_embed_dim=64)(*first, "a", height=48, width=80)


# ------------------------------------------------------------------------------------------------------- from_pretrained
SCHED = dict(_class_name="CogVideoXDDIMScheduler", prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True,
             set_alpha_to_one=True, beta_schedule="scaled_linear", snr_shift_scale=3.0, num_train_timesteps=1000)


def _checkpoint(root, encoder):
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import t5
    torch.manual_seed(4)
    te = t5.T5EncoderModel(t5.T5Config(**TINY_A))
    vae = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**eo.TINY.__dict__), encoder=encoder)
    dit = tiny_cpu_model(seed=9, in_channels=16)
    te.save_pretrained(os.path.join(root, "text_encoder"))
    vae.save_pretrained(os.path.join(root, "vae"))
    dit.save_pretrained(os.path.join(root, "transformer"))
    os.makedirs(os.path.join(root, "scheduler"))
    with open(os.path.join(root, "scheduler", "scheduler_config.json"), "w") as fh:
        json.dump(SCHED, fh)
    index = {"_class_name": "CogVideoXPipeline", "_diffusers_version": "0.32.0", "scheduler": ["diffusers", SCHED["_class_name"]],
             "text_encoder": ["transformers", "T5EncoderModel"], "tokenizer": ["transformers", "T5Tokenizer"],
             "transformer": ["diffusers", "CogVideoXTransformer3DModel"], "vae": ["diffusers", "AutoencoderKLCogVideoX"]}
    with open(os.path.join(root, "model_index.json"), "w") as fh:
        json.dump(index, fh)
    return te, vae, dit


def test_from_pretrained_takes_a_decoder_only_vae_for_text_to_video_only(tmp_path):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    from lkgd_amd.pipeline_cogvideox import CogVideoXPipeline, CogVideoXVideoToVideoPipeline
    te, vae, dit = _checkpoint(str(tmp_path), encoder=False)
    tok = object()
    p = CogVideoXPipeline.from_pretrained(str(tmp_path), torch_dtype=torch.float32, tokenizer=tok)
    assert type(p) is CogVideoXPipeline and not p.vae.has_encoder and p.tokenizer is tok
    assert type(p.scheduler) is pc.CogVideoXDDIMScheduler and p.transformer.config.in_channels == 16
    for got, want in ((p.text_encoder, te), (p.vae, vae), (p.transformer, dit)):
        a, b = got.state_dict(), want.state_dict()
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    with pytest.raises(LkgdHipError, match=r"CogVideoXVideoToVideoPipeline\.from_pretrained.*vae/ holds no encoder\.\* keys.*encoder"):
        CogVideoXVideoToVideoPipeline.from_pretrained(str(tmp_path), torch_dtype=torch.float32)


def test_from_pretrained_builds_the_video_to_video_class_with_the_whole_vae(tmp_path):
    from lkgd_amd.pipeline_cogvideox import CogVideoXVideoToVideoPipeline
    _checkpoint(str(tmp_path), encoder=True)
    p = CogVideoXVideoToVideoPipeline.from_pretrained(str(tmp_path), torch_dtype=torch.float32)
    assert type(p) is CogVideoXVideoToVideoPipeline and p.vae.has_encoder and p.tokenizer is None


# ------------------------------------------------------------------------------------------------------ preprocess_video
def test_preprocess_video_on_the_host_for_every_accepted_input():
    import PIL.Image
    from lkgd_amd.video_processor import VideoProcessor
    vp = VideoProcessor(vae_scale_factor=8)
    g = torch.Generator().manual_seed(5)

    def clip(T, size=(72, 40)):
        return [PIL.Image.fromarray(torch.randint(0, 256, (size[1], size[0], 3), generator=g, dtype=torch.uint8).numpy()) for _ in range(T)]

    def want(clips):
        return torch.stack([vp.preprocess(c, 48, 80) for c in clips]).permute(0, 2, 1, 3, 4)
    a, b = clip(5), clip(5)
    t5 = torch.rand(2, 5, 3, 48, 80, generator=g)                       # [B, T, C, H, W]
    n5 = t5.permute(0, 1, 3, 4, 2).numpy()                              # [B, T, H, W, C]
    cases = {"pil frames": (a, [a], (1, 3, 5, 48, 80)), "lists of pil frames": ([a, b], [a, b], (2, 3, 5, 48, 80)),
             "5-D tensor": (t5, list(t5), (2, 3, 5, 48, 80)), "4-D tensor": (t5[0], [t5[0]], (1, 3, 5, 48, 80)),
             "list of 4-D tensors": ([t5[0], t5[1]], [t5[0], t5[1]], (2, 3, 5, 48, 80)),
             "5-D ndarray": (n5, list(n5), (2, 3, 5, 48, 80)), "4-D ndarray": (n5[1], [n5[1]], (1, 3, 5, 48, 80)),
             "list of 4-D ndarrays": ([n5[0], n5[1]], [n5[0], n5[1]], (2, 3, 5, 48, 80))}
    for name, (video, clips, shape) in cases.items():
        got = vp.preprocess_video(video, height=48, width=80)
        assert got.dtype == torch.float32 and tuple(got.shape) == shape and torch.equal(got, want(clips)), name
    assert torch.equal(vp.preprocess_video(t5, 48, 80)[1, :, 2], 2 * t5[1, 2] - 1)
    # a single frame, the default size (rounded down to the VAE's factor), and a CPU target: the host form with the cast
    assert tuple(vp.preprocess_video(clip(1)).shape) == (1, 3, 1, 40, 72)
    got = vp.preprocess_video(a, 48, 80, device="cpu", dtype=torch.float16)
    assert got.dtype == torch.float16 and torch.equal(got, want([a]).half())
    for bad in ("clip.mp4", [], [a, t5[0]], torch.zeros(3, 48, 80)):
        with pytest.raises(ValueError, match="incorrect format"):
            vp.preprocess_video(bad)
