"""Host side of the trans-ControlNet pipeline without a GPU: argument validation of the fused direct-fusion Euler step's C
entry point, and the pipeline class's ``__call__`` parameters against the reference's list
(pipeline_stable_video_diffusion_trans_controlnet.py:354-380)."""
import inspect

from c_interface import ALIGN, MODE, NULL, SHAPE, entry

#: the reference's __call__ parameters, in order (pipeline_stable_video_diffusion_trans_controlnet.py:354-380)
REFERENCE_PARAMS = [
    "image", "controlnet_condition", "height", "width", "num_frames", "num_inference_steps", "min_guidance_scale",
    "max_guidance_scale", "fps", "motion_bucket_id", "noise_aug_strength", "decode_chunk_size", "num_videos_per_prompt",
    "generator", "latents", "output_type", "callback_on_step_end", "callback_on_step_end_tensor_inputs", "return_dict",
    "controlnet_cond_scale", "original_latents", "start_step", "direct_fusion", "controlnet_scale",
]


def test_cfg_fusion_euler_step_validation_without_gpu():
    """argument errors are reported before anything touches the device (no pointer below is ever dereferenced)"""
    p = 4096                                                      # aligned dummy addresses
    f = entry("lkgd_cfg_fusion_euler_step", noise_tokens=p, latents=p, latents_is_f32=0, guidance=p, weight=p, B=2, F=4, H=8, W=8,
              cfg=2, sigma=1.0, sigma_next=0.5, prediction_type=1)
    assert f(noise_tokens=None) == NULL and f(latents=None) == NULL and f(weight=None) == NULL
    assert f(guidance=None) == NULL                               # cfg == 2 needs the per-frame guidance
    for bad in (dict(B=3), dict(B=1), dict(B=0), dict(B=-2), dict(cfg=0), dict(cfg=3), dict(sigma=0.0),
                dict(sigma=float("nan"))):
        assert f(**bad) == SHAPE, bad
    assert f(prediction_type=2) == MODE
    assert f(noise_tokens=p + 2) == ALIGN


def test_trans_controlnet_call_signature_matches_reference():
    from lkgd_amd import pipeline
    cls = pipeline.StableVideoDiffusionPipelineTransControlNet
    assert issubclass(cls, pipeline.StableVideoDiffusionPipeline)
    sig = inspect.signature(cls.__call__)
    named = [n for n, p in sig.parameters.items() if n != "self" and p.kind != p.VAR_KEYWORD]
    assert named == REFERENCE_PARAMS
    d = {n: p.default for n, p in sig.parameters.items()}
    assert (d["original_latents"], d["start_step"], d["direct_fusion"], d["controlnet_scale"]) == (None, 0, False, 1.0)
    assert (d["controlnet_cond_scale"], d["height"], d["width"], d["num_inference_steps"]) == (1.0, 576, 1024, 25)
    # the loop's new keywords default to today's behaviour
    den = inspect.signature(pipeline.StableVideoDiffusionPipeline.denoise).parameters
    assert (den["start_step"].default, den["direct_fusion"].default, den["controlnet_scale"].default) == (0, False, 1.0)
