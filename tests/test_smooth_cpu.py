"""Host side of the long-video smoothing pipeline without a GPU: the frame windows (``smooth_chunks`` against the windows the
reference's ``get_chunks`` drew, pipeline_stable_video_diffusion_smooth.py:526-533, and their partition properties), the
pipeline class's ``__call__`` parameters against the reference's list (:320-341), argument validation of the two windowed entry
points."""
import inspect
import os

import numpy as np
import pytest
import torch
from safetensors import safe_open

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "smooth.safetensors")
TOTAL, NUM_FRAMES = 7, 3                                         # tests/golden/make_goldens_smooth.py


@pytest.fixture(scope="module")
def golden():
    with safe_open(GOLDEN, "pt") as f:
        return {"meta": f.metadata(), "a_windows": f.get_tensor("a_windows"), "b_windows": f.get_tensor("b_windows")}


def _windows(t):
    return [[(int(f0), int(n)) for f0, n in step if n > 0] for step in t.tolist()]


def test_smooth_chunks_reproduce_the_reference_windows(golden):
    from lkgd_amd.pipeline import smooth_chunks
    ref = _windows(golden["a_windows"])
    assert ref == _windows(golden["b_windows"]) and len(ref) == 3
    assert {n for step in ref for _, n in step} == {1, 2, 3}     # every window length 1..num_frames occurs in the fixture
    np.random.seed(int(golden["meta"]["numpy_seed"]))
    assert [smooth_chunks(TOTAL, NUM_FRAMES) for _ in ref] == ref
    rng = np.random.RandomState(int(golden["meta"]["numpy_seed"]))
    assert [smooth_chunks(TOTAL, NUM_FRAMES, rng) for _ in ref] == ref


@pytest.mark.parametrize("total,num_frames", [(7, 3), (1, 14), (14, 14), (30, 14)])
def test_smooth_chunks_partition_the_frames(total, num_frames):
    from lkgd_amd.pipeline import smooth_chunks

    class Rng:                                                   # np.random's interface, counting the draws
        def __init__(self, seed):
            self.state, self.calls = np.random.RandomState(seed), []

        def randint(self, lo, hi):
            self.calls.append((lo, hi))
            return self.state.randint(lo, hi)
    rng = Rng(1000 * total + num_frames)
    firsts = set()
    for k in range(200):
        chunks = smooth_chunks(total, num_frames, rng)
        assert rng.calls == [(0, num_frames)] * (k + 1)          # one draw per call, as get_chunks draws it
        assert chunks[0][0] == 0 and sum(n for _, n in chunks) == total
        for (f0, n), (g0, _) in zip(chunks, chunks[1:]):
            assert g0 == f0 + n                                  # contiguous, in order: frames 0..T-1 exactly once
        assert all(1 <= n <= num_frames for _, n in chunks)
        assert all(n == num_frames for _, n in chunks[1:-1])     # only the first and the last may be shorter
        firsts.add(chunks[0][1])
    assert firsts == set(range(1, min(num_frames, total) + 1))   # the first window takes every length it can


def test_smooth_call_signature_matches_reference(golden):
    from lkgd_amd import pipeline
    cls = pipeline.StableVideoDiffusionPipelineSmooth
    assert issubclass(cls, pipeline.StableVideoDiffusionPipeline)
    ref = golden["meta"]["call_params"].split(",")
    assert ref[0] == "image" and ref[-1] == "start_step" and len(ref) == 19
    sig = inspect.signature(cls.__call__)
    named = [n for n in sig.parameters if n != "self"]
    assert named[:len(ref)] == ref
    assert named[len(ref):] == ["image_embeddings", "image_latents", "noise", "controlnet_condition"]
    d = {n: p.default for n, p in sig.parameters.items()}
    assert (d["height"], d["width"], d["num_inference_steps"], d["start_step"], d["num_videos_per_prompt"]) == (576, 1024, 25, 0, 1)
    assert all(d[n] is None for n in named[len(ref):])
    den = inspect.signature(cls.denoise_smooth).parameters
    assert list(den)[1:6] == ["latents", "image_latents", "image_embeddings", "added_time_ids", "num_frames"]


def test_window_entry_points_validate_without_gpu():
    """argument errors are reported before anything touches the device (no pointer below is ever dereferenced)"""
    from c_interface import ALIGN, MODE, NULL, SHAPE, entry
    p = 4096                                                     # aligned dummy addresses
    prep = entry("lkgd_window_prepare_input", latents=p, latents_is_f32=0, image_latents=p, T=7, f0=2, L=3, H=8, W=8, cfg=2,
                 sigma=1.0, tokens_out=p)
    step = entry("lkgd_window_cfg_euler_step", noise_tokens=p, latents=p, latents_is_f32=0, guidance=p, T=7, f0=2, L=3, H=8, W=8,
                 cfg=2, sigma=1.0, sigma_next=0.5, prediction_type=1)
    assert prep(latents=None) == NULL and prep(image_latents=None) == NULL and prep(tokens_out=None) == NULL
    assert step(noise_tokens=None) == NULL and step(latents=None) == NULL and step(guidance=None) == NULL   # cfg == 2 needs the guidance
    for name, f in (("prep", prep), ("step", step)):
        for bad in (dict(cfg=0), dict(cfg=3), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(f0=-1),
                    dict(L=0), dict(L=-3), dict(f0=5, L=3), dict(f0=7, L=1), dict(f0=0, L=8), dict(T=0),
                    dict(f0=2 ** 31 - 1, L=2 ** 31 - 1)):
            assert f(**bad) == SHAPE, (name, bad)
    assert step(prediction_type=2) == MODE and step(prediction_type=-1) == MODE
    assert prep(tokens_out=p + 8) == ALIGN and step(noise_tokens=p + 4) == ALIGN


def test_smooth_refusals_need_no_gpu():
    from lkgd_amd.pipeline import StableVideoDiffusionPipelineSmooth
    pipe = StableVideoDiffusionPipelineSmooth()
    for kw in (dict(max_guidance_scale=1.0), dict(num_videos_per_prompt=2), dict(num_frames=17), dict(num_frames=0),
               dict(controlnet_condition=torch.zeros(1))):
        full = dict(num_frames=3, max_guidance_scale=3.0)
        full.update(kw)
        with pytest.raises(ValueError):
            pipe._refuse(**full)
    pipe._refuse(16, 3.0)
