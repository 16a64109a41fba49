"""``CogVideoXImageToVideoPipeline`` and ``VideoProcessor`` without a GPU: both entry points of include/lkgd_hip_video.h
refuse before launching; ``check_inputs`` raises the reference's errors
(pipeline_cogvideox_image2video.py:465-527); the 1.5 frame padding (:779-786); every argument the loop cannot honour raises and names
itself; ``from_pretrained`` of a directory assembled from tiny components; ``VideoProcessor`` on CPU data is ``VaeImageProcessor`` /
``tensor2vid``."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cogvideox_vae_encoder_oracle as eo
from c_interface import ALIGN, MODE, NULL, SHAPE, Host, entry
from cogvideox_support import tiny_cpu_model
from t5_support import TINY_A


# -------------------------------------------------------------------------------------------------------------- refusals
def test_postprocess_refuses_before_launching():
    """every refusal include/lkgd_hip_video.h lists; host pointers: a refused call launches nothing"""
    h = Host()
    call = entry("lkgd_video_postprocess", x=h.p, out=h.p + 2048, mode=0, B=1, C=3, T=2, H=4, W=8)
    for k in ("x", "out"):
        assert call(**{k: None}) == NULL, k
    for kw in (dict(B=0), dict(C=0), dict(T=0), dict(H=0), dict(W=0), dict(B=-1), dict(C=-3), dict(T=-1), dict(H=-4), dict(W=-8),
               dict(C=5), dict(B=1 << 20, T=1 << 10, H=1 << 10, W=1 << 10), dict(T=1 << 20, H=1 << 20, W=1 << 20)):
        assert call(**kw) == SHAPE, kw
    for m in (-1, 3, 7):
        assert call(mode=m) == MODE, m
    assert call(x=h.p + 1) == ALIGN
    assert call(mode=1, out=h.p + 2048 + 2) == ALIGN and call(mode=2, out=h.p + 2048 + 1) == ALIGN


def test_preprocess_refuses_before_launching():
    h = Host()
    call = entry("lkgd_image_preprocess", u=h.p, out=h.p + 2048, N=1, H=4, W=8, C=3)
    for k in ("u", "out"):
        assert call(**{k: None}) == NULL, k
    for kw in (dict(N=0), dict(H=0), dict(W=0), dict(C=0), dict(N=-1), dict(H=-4), dict(W=-8), dict(C=-3), dict(C=5),
               dict(N=1 << 20, H=1 << 10, W=1 << 10)):
        assert call(**kw) == SHAPE, kw
    assert call(out=h.p + 2048 + 1) == ALIGN


# ---------------------------------------------------------------------------------------------------------- the pipeline
def _stub_pipe(patch_size_t=None, **kw):
    """a pipeline of configuration stubs: everything up to the first use of a module runs on the CPU"""
    from lkgd_amd.pipeline_cogvideox import CogVideoXImageToVideoPipeline
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(64, 64, 128, 128), temporal_compression_ratio=4, scaling_factor=0.7))
    tr = SimpleNamespace(config=SimpleNamespace(sample_height=6, sample_width=10, sample_frames=9, patch_size=2, patch_size_t=patch_size_t,
                                                in_channels=32, use_rotary_positional_embeddings=False, ofs_embed_dim=None),
                         device=torch.device("cpu"))
    parts = dict(tokenizer=None, text_encoder=None, vae=vae, transformer=tr, scheduler=None, domain_model=object(), flow_model=object())
    parts.update(kw)
    return CogVideoXImageToVideoPipeline(**parts)


def test_constructor_carries_the_reference_attributes():
    p = _stub_pipe()
    assert (p.vae_scale_factor_spatial, p.vae_scale_factor_temporal, p.vae_scaling_factor_image) == (8, 4, 0.7)
    assert p.video_processor.config.vae_scale_factor == 8 and p.video_processor.config.do_normalize
    assert p._callback_tensor_inputs == ["latents", "prompt_embeds", "negative_prompt_embeds"]
    assert p.guidance_scale is None and p.num_timesteps is None and p.current_timestep is None and p.interrupt is False
    assert p.enable_model_cpu_offload() is None and p.enable_sequential_cpu_offload() is None
    for f in (p.enable_model_cpu_offload, p.enable_sequential_cpu_offload):
        assert "does nothing" in f.__doc__
    import inspect
    sig = inspect.signature(type(p).__call__)
    want = dict(prompt=None, negative_prompt=None, height=None, width=None, num_frames=49, num_inference_steps=50, timesteps=None,
                guidance_scale=6, use_dynamic_cfg=False, num_videos_per_prompt=1, eta=0.0, generator=None, latents=None,
                prompt_embeds=None, negative_prompt_embeds=None, output_type="pil", return_dict=True, attention_kwargs=None,
                callback_on_step_end=None, callback_on_step_end_tensor_inputs=["latents"], max_sequence_length=226)
    assert list(sig.parameters)[:2] == ["self", "image"] and list(sig.parameters)[2:] == list(want)
    assert {k: sig.parameters[k].default for k in want} == want


def test_check_inputs_raises_the_reference_errors():
    p = _stub_pipe()
    img, pe = torch.zeros(1, 3, 48, 80), torch.zeros(1, 4, 8)
    ok = dict(image=img, prompt="a", height=48, width=80, negative_prompt=None, callback_on_step_end_tensor_inputs=["latents"])
    p.check_inputs(**ok)
    p.check_inputs(**{**ok, "prompt": None, "prompt_embeds": pe, "negative_prompt_embeds": pe})
    p.check_inputs(**{**ok, "image": [img], "prompt": ["a", "b"]})
    for over, msg in ((dict(image=np.zeros((48, 80, 3))), "`image` has to be of type"),
                      (dict(height=50), "divisible by 8 but are 50 and 80"),
                      (dict(width=81), "divisible by 8 but are 48 and 81"),
                      (dict(callback_on_step_end_tensor_inputs=["latents", "image"]), r"has to be in .*but found \['image'\]"),
                      (dict(prompt_embeds=pe), "Cannot forward both `prompt`: a and `prompt_embeds`"),
                      (dict(prompt=None), "Provide either `prompt` or `prompt_embeds`"),
                      (dict(prompt=3), "`prompt` has to be of type `str` or `list` but is <class 'int'>"),
                      (dict(negative_prompt_embeds=pe), "Cannot forward both `prompt`: a and `negative_prompt_embeds`"),
                      (dict(prompt=None, prompt_embeds=pe, negative_prompt="n", negative_prompt_embeds=pe),
                       "Cannot forward both `negative_prompt`: n and `negative_prompt_embeds`"),
                      (dict(prompt=None, prompt_embeds=pe, negative_prompt_embeds=torch.zeros(1, 5, 8)), "must have the same shape")):
        with pytest.raises(ValueError, match=msg):
            p.check_inputs(**{**ok, **over})


@pytest.mark.parametrize("frames,p_t,want", [(49, None, (13, 0, 49)), (81, None, (21, 0, 81)), (161, None, (41, 0, 161)),
                                             (49, 2, (13, 1, 53)), (81, 2, (21, 1, 85)), (161, 2, (41, 1, 165)),
                                             (45, 2, (12, 0, 45)), (9, 2, (3, 1, 13))])
def test_frame_padding_arithmetic(frames, p_t, want):
    """:779-786 with temporal factor 4: (latent frames, additional latent frames, pixel frames handed to prepare_latents)"""
    from lkgd_amd.pipeline_cogvideox import additional_latent_frames
    assert additional_latent_frames(frames, 4, p_t) == want
    latent, extra, padded = want
    assert (padded - 1) // 4 + 1 == latent + extra and (p_t is None or (latent + extra) % p_t == 0)


@pytest.mark.parametrize("kw,name", [(dict(timesteps=[999, 500]), "timesteps"), (dict(eta=0.5), "eta"),
                                     (dict(attention_kwargs={"scale": 1.0}), "attention_kwargs"),
                                     (dict(domain_model=None), "domain_model"), (dict(flow_model=None), "flow_model")])
def test_arguments_the_loop_cannot_honour_raise_and_name_themselves(kw, name):
    from lkgd_amd._lib import LkgdHipError
    ctor = {k: v for k, v in kw.items() if k.endswith("_model")}
    call = {k: v for k, v in kw.items() if k not in ctor}
    p = _stub_pipe(**ctor)
    with pytest.raises(LkgdHipError, match=f"`{name}`"):
        p(torch.zeros(1, 3, 48, 80), prompt="a", height=48, width=80, num_frames=9, **call)
    # the reference's own checks come first
    with pytest.raises(ValueError, match="divisible by 8"):
        p(torch.zeros(1, 3, 48, 80), prompt="a", height=50, width=80, **call)


# ------------------------------------------------------------------------------------------------------- from_pretrained
SCHED = dict(_class_name="CogVideoXDPMScheduler", prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True,
             set_alpha_to_one=True, beta_schedule="scaled_linear", snr_shift_scale=1.0, num_train_timesteps=1000)


def _checkpoint(root, encoder=True):
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import t5
    torch.manual_seed(4)
    te = t5.T5EncoderModel(t5.T5Config(**TINY_A))
    vae = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**eo.TINY.__dict__), encoder=encoder)
    dit = tiny_cpu_model(seed=9)
    te.save_pretrained(os.path.join(root, "text_encoder"))
    vae.save_pretrained(os.path.join(root, "vae"))
    dit.save_pretrained(os.path.join(root, "transformer"))
    os.makedirs(os.path.join(root, "scheduler"))
    with open(os.path.join(root, "scheduler", "scheduler_config.json"), "w") as fh:
        json.dump(SCHED, fh)
    index = {"_class_name": "CogVideoXImageToVideoPipeline", "_diffusers_version": "0.32.0",
             "scheduler": ["diffusers", SCHED["_class_name"]], "text_encoder": ["transformers", "T5EncoderModel"],
             "tokenizer": ["transformers", "T5Tokenizer"], "transformer": ["diffusers", "CogVideoXTransformer3DModel"],
             "vae": ["diffusers", "AutoencoderKLCogVideoX"]}
    with open(os.path.join(root, "model_index.json"), "w") as fh:
        json.dump(index, fh)
    return te, vae, dit


def _equal_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


def test_from_pretrained_reads_a_directory_of_tiny_components(tmp_path):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd.pipeline_cogvideox import CogVideoXImageToVideoPipeline
    te, vae, dit = _checkpoint(str(tmp_path))
    tok, dom, flow = object(), object(), object()
    p = CogVideoXImageToVideoPipeline.from_pretrained(str(tmp_path), torch_dtype=torch.float32, tokenizer=tok, domain_model=dom,
                                                      flow_model=flow)
    _equal_state(p.text_encoder, te)
    _equal_state(p.vae, vae)
    _equal_state(p.transformer, dit)
    assert p.vae.has_encoder and type(p.scheduler) is pc.CogVideoXDPMScheduler
    assert p.tokenizer is tok and p.domain_model is dom and p.flow_model is flow
    assert (p.vae_scale_factor_spatial, p.vae_scale_factor_temporal) == (8, 4) and p.vae_scaling_factor_image == vae.config.scaling_factor
    # no tokenizer given and no tokenizer/ directory: None, and id prompts still pass check_inputs
    q = CogVideoXImageToVideoPipeline.from_pretrained(str(tmp_path), torch_dtype=torch.float32)
    assert q.tokenizer is None and q.domain_model is None
    q.check_inputs(torch.zeros(1, 3, 48, 80), torch.zeros(1, 16, dtype=torch.int64), 48, 80, None, ["latents"])
    # the other scheduler class the config may name
    with open(os.path.join(str(tmp_path), "scheduler", "scheduler_config.json"), "w") as fh:
        json.dump({**SCHED, "_class_name": "CogVideoXDDIMScheduler"}, fh)
    assert type(CogVideoXImageToVideoPipeline.from_pretrained(str(tmp_path), torch_dtype=torch.float32).scheduler) is pc.CogVideoXDDIMScheduler


def test_from_pretrained_refuses_a_vae_without_its_encoder(tmp_path):
    from lkgd_amd._lib import LkgdHipError
    from lkgd_amd.pipeline_cogvideox import CogVideoXImageToVideoPipeline
    _checkpoint(str(tmp_path), encoder=False)
    with pytest.raises(LkgdHipError, match=r"vae/ holds no encoder\.\* keys"):
        CogVideoXImageToVideoPipeline.from_pretrained(str(tmp_path), torch_dtype=torch.float32)
    os.remove(os.path.join(str(tmp_path), "model_index.json"))
    with pytest.raises(OSError, match="model_index.json"):
        CogVideoXImageToVideoPipeline.from_pretrained(str(tmp_path))


# -------------------------------------------------------------------------------------------------------- VideoProcessor
def _clip(B=2, C=3, T=3, H=5, W=7, seed=2):
    return (1.2 * torch.randn(B, C, T, H, W, generator=torch.Generator().manual_seed(seed))).half()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_video_processor_on_cpu_clips_is_tensor2vid(dtype):
    from lkgd_amd.image_processor import VaeImageProcessor, tensor2vid
    from lkgd_amd.video_processor import VideoProcessor
    vp, ip = VideoProcessor(vae_scale_factor=8), VaeImageProcessor(vae_scale_factor=8)
    v = _clip().to(dtype)
    got, want = vp.postprocess_video(v, "np"), tensor2vid(v, ip, "np")
    assert got.dtype == np.float32 and got.shape == (2, 3, 5, 7, 3) and np.array_equal(got, want)
    got, want = vp.postprocess_video(v, "pt"), tensor2vid(v, ip, "pt")
    assert got.dtype == dtype and tuple(got.shape) == (2, 3, 3, 5, 7) and torch.equal(got, want)
    got, want = vp.postprocess_video(v, "pil"), tensor2vid(v, ip, "pil")
    assert len(got) == 2 and all(len(c) == 3 for c in got)
    for a, b in zip(got, want):
        for fa, fb in zip(a, b):
            assert fa.size == (7, 5) and fa.mode == "RGB" and np.array_equal(np.asarray(fa), np.asarray(fb))
    for bad in ("latent", "mp4"):
        with pytest.raises(ValueError, match="does not exist"):
            vp.postprocess_video(v, bad)
    assert vp.postprocess_video(v).dtype == np.float32              # diffusers' default output type


def test_video_processor_preprocess_on_the_host_is_the_image_processors():
    import PIL.Image
    from lkgd_amd.image_processor import VaeImageProcessor
    from lkgd_amd.video_processor import VideoProcessor
    vp, ip = VideoProcessor(vae_scale_factor=8), VaeImageProcessor(vae_scale_factor=8)
    g = torch.Generator().manual_seed(5)
    pix = torch.randint(0, 256, (40, 72, 3), generator=g, dtype=torch.uint8).numpy()
    pil = PIL.Image.fromarray(pix)
    t = torch.rand(2, 3, 48, 80, generator=g)
    for image in (pil, [pil, pil], t, [t[0], t[1]], t.permute(0, 2, 3, 1).numpy()):
        got, want = vp.preprocess(image, height=48, width=80), ip.preprocess(image, height=48, width=80)
        assert got.dtype == torch.float32 and tuple(got.shape)[1:] == (3, 48, 80) and torch.equal(got, want)
    # with a target the result is the pipeline's cast; a CPU target keeps the host form
    got = vp.preprocess(pil, 48, 80, device="cpu", dtype=torch.float16)
    assert got.dtype == torch.float16 and torch.equal(got, ip.preprocess(pil, 48, 80).to(torch.float16))
