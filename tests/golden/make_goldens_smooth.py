#!/usr/bin/env python3
"""Generate tests/golden/smooth.safetensors by EXECUTING THE REFERENCE'S OWN long-video smoothing pipeline.

Runs only where the reference tree is mounted (build container, CPU, fp32).  Uses make_goldens.py's name-only stubs and
stand-in boundary stages, then calls ``pipeline_stable_video_diffusion_smooth.StableVideoDiffusionPipeline.__call__``
(output_type="latent") at the tiny config: an input video of T = 7 frames of 8x8 latents, windows of num_frames = 3, 4 steps,
start_step = 1, on

* a = the stock UNet (models/unet_spatio_temporal_condition_controlnet.py), seeded, weights rounded to fp16;
* b = the same UNet patched as run_models/run_inference_svd_smooth.py has it (utils/util.py:408-438): ``apply_patch(flip=True)``
  + ``initialize_joint_layers``, joint layers seeded (lora_cases.seed_joint_and_lora_) so the joint branch is not an identity,
  joint mask [0, 1, 0, 1] over the UNet batch [window, reversed window] x [uncond, cond].

``torch.randn_like`` is replaced by a recorded tensor so that the noise ``add_noise`` uses is stored, and ``np.random.seed`` is
called just before ``__call__`` so that ``get_chunks`` (:526-533) draws recorded first-window lengths.  Recorded: the per-frame
boundary outputs (CLIP embeddings, VAE image latents; the rows of the UNet's first call are checked against them), the added
time ids of the UNet's first call, the noisy start, every executed step's window list and latents, the final latents, weight
checksums, and - as file metadata - the parameter names of the reference's ``__call__``.

Weights are NOT stored: the tests regenerate them from the seeds (checksums are stored).

Usage:  python tests/golden/make_goldens_smooth.py
"""
from __future__ import annotations

import inspect
import os
import sys

sys.dont_write_bytecode = True

import numpy as np                                        # noqa: E402
import torch                                              # noqa: E402
from safetensors.torch import save_file                   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as mg                                  # noqa: E402
from make_goldens import REF, TINY, WSEED, _FakeCLIP, _FakeVAE, _mod, checksum, install_stubs, load_ref   # noqa: E402
from lora_cases import seed_joint_and_lora_               # noqa: E402
from oracle import unet as ou                              # noqa: E402

UNET_SEED = WSEED + 31        # tests/test_smooth_gpu.py regenerates the weights from these seeds
JOINT_SEED = WSEED + 32
INPUT_SEED = 251
NUMPY_SEED = 3                # first-window lengths 3, 1, 2 over the three executed steps: every length 1..NUM_FRAMES occurs
JOINT_MASK = [0, 1, 0, 1]     # utils/util.py:408-438
TOTAL, NUM_FRAMES, HW, STEPS, START = 7, 3, 8, 4, 1


def inputs():
    g = torch.Generator().manual_seed(INPUT_SEED)
    return dict(image=torch.rand(TOTAL, 3, 8 * HW, 8 * HW, generator=g),
                noise=torch.randn(1, TOTAL, 4, HW, HW, generator=g))


def _round16_(m):
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    return m


def main():
    assert os.path.isdir(REF), "runs only where the reference tree is mounted"
    install_stubs()
    sys.path.insert(0, REF)
    for m in ("models", "utils"):
        _mod(m)
    sched_mod = load_ref("utils/scheduling_euler_discrete_karras_fix.py", "utils.scheduling_euler_discrete_karras_fix")
    ref_stock = load_ref("models/unet_spatio_temporal_condition_controlnet.py",
                         "models.unet_spatio_temporal_condition_controlnet")
    load_ref("models/controlnet_sdv.py", "models.controlnet_sdv")          # the pipeline module imports it
    _mod("patch")
    load_ref("patch/utils.py", "patch.utils")
    patch_mod = load_ref("patch/patch.py", "patch.patch")
    sys.modules["patch"].patch = patch_mod
    pipe_mod = load_ref("pipeline/pipeline_stable_video_diffusion_smooth.py", "ref_pipeline_smooth")
    from oracle.scheduler import SchedulerConfig

    kw = dict(TINY.__dict__)
    inp = inputs()
    out = {"noise": inp["noise"], "image": inp["image"]}
    with torch.no_grad():
        unet = _round16_(ou.init_weights_(ref_stock.UNetSpatioTemporalConditionControlNetModel(**kw), UNET_SEED))
    out["checksum_unet_base"] = torch.tensor(checksum(unet), dtype=torch.float64)

    def patch_for_case_b():
        with torch.no_grad():
            patch_mod.apply_patch(unet, flip=True)
            patch_mod.initialize_joint_layers(unet)
            names = seed_joint_and_lora_(unet, JOINT_SEED)
        out["n_joint_seeded"] = torch.tensor(len(names))
        out["checksum_unet"] = torch.tensor(checksum(unet), dtype=torch.float64)
        patch_mod.set_joint_attention_mask(unet, JOINT_MASK)

    real_randn_like = torch.randn_like
    for name in ("a", "b"):
        if name == "b":
            patch_for_case_b()
        sched = sched_mod.EulerDiscreteScheduler(**SchedulerConfig().__dict__)
        fe = lambda images, **k: mg.SimpleNamespace(pixel_values=images)   # noqa: E731
        pipe = pipe_mod.StableVideoDiffusionPipeline(vae=_FakeVAE(), image_encoder=_FakeCLIP(), unet=unet,
                                                     scheduler=sched, feature_extractor=fe)
        rec = {"lens": [], "vae": []}
        orig_forward = unet.forward

        def spy(sample, t, _f=orig_forward, **k):
            rec["lens"].append(sample.shape[1])
            if "ids" not in rec:
                rec["ids"], rec["enc0"] = k["added_time_ids"].clone(), k["encoder_hidden_states"].clone()
                rec["img0"] = sample[:, 0, 4:].clone()
            return _f(sample, t, **k)
        unet.forward = spy
        enc_image, enc_vae, add_noise = pipe._encode_image, pipe._encode_vae_image, sched.add_noise

        def spy_clip(*a, **k):
            rec["emb"] = enc_image(*a, **k).clone()
            return rec["emb"]

        def spy_vae(*a, **k):
            rec["vae"].append(enc_vae(*a, **k).clone())
            return rec["vae"][-1]

        def spy_add_noise(*a, **k):
            rec["start"] = add_noise(*a, **k).clone()
            return rec["start"]
        pipe._encode_image, pipe._encode_vae_image, sched.add_noise = spy_clip, spy_vae, spy_add_noise
        steps, idx = [], []
        torch.randn_like = lambda x, **k: inp["noise"].to(dtype=x.dtype).clone()
        try:
            np.random.seed(NUMPY_SEED)
            res = pipe(inp["image"], height=8 * HW, width=8 * HW, num_frames=NUM_FRAMES, num_inference_steps=STEPS,
                       noise_aug_strength=0.02, output_type="latent", generator=torch.Generator().manual_seed(INPUT_SEED + 1),
                       callback_on_step_end=lambda p, i, t, kw_: (steps.append(kw_["latents"].clone()), idx.append(i), {})[2],
                       start_step=START)
        finally:
            torch.randn_like = real_randn_like
            unet.forward = orig_forward
        assert idx == list(range(START, STEPS)), idx
        # the window list of every executed step, from the lengths the UNet saw: windows are contiguous and cover 0..T-1
        windows, cur, f0 = [], [], 0
        for n in rec["lens"]:
            cur.append((f0, n))
            f0 += n
            if f0 == TOTAL:
                windows.append(cur)
                cur, f0 = [], 0
        assert not cur and len(windows) == STEPS - START, rec["lens"]
        assert {n for w in windows for _, n in w} == set(range(1, NUM_FRAMES + 1)), windows
        wt = torch.full((len(windows), max(len(w) for w in windows), 2), -1, dtype=torch.int32)
        for s, w in enumerate(windows):
            wt[s, :len(w)] = torch.tensor(w, dtype=torch.int32)
        emb = rec["emb"]                                             # [2T, 1, 1024]: zeros, then one row per input frame
        assert emb.shape[0] == 2 * TOTAL and not emb[:TOTAL].any()
        img = torch.cat(rec["vae"])                                  # [T, 4, h, w], encoded in slices of decode_chunk_size
        f0, n = windows[0][0]
        assert torch.equal(rec["enc0"], torch.stack([emb[f0], emb[f0 + n - 1], emb[TOTAL + f0], emb[TOTAL + f0 + n - 1]]))
        assert torch.equal(rec["img0"][2:], torch.stack([img[f0], img[f0 + n - 1]])) and not rec["img0"][:2].any()
        case = {"windows": wt, "start": rec["start"].float(), "step_latents": torch.stack(steps).float(),
                "final": res.frames.float()}
        if name == "a":
            out["image_embeddings"], out["image_latents"], out["added_time_ids"] = emb[TOTAL:], img, rec["ids"]
        else:       # the boundary stages do not see the patch
            assert torch.equal(out["image_embeddings"], emb[TOTAL:]) and torch.equal(out["image_latents"], img)
            assert torch.equal(out["a_windows"], wt) and torch.equal(out["a_start"], case["start"])
        out.update({f"{name}_{k}": v for k, v in case.items()})
        print("case %s: windows %s, final std %.4f, dtype %s" % (name, windows, res.frames.std(), res.frames.dtype))
    rel = ((out["a_final"] - out["b_final"]).norm() / out["a_final"].norm()).item()
    print("a vs b final rel L2 %.4f" % rel)
    assert rel > 0.1
    params = [n for n in inspect.signature(pipe_mod.StableVideoDiffusionPipeline.__call__).parameters if n != "self"]
    save_file({k: v.contiguous() for k, v in out.items()}, os.path.join(HERE, "smooth.safetensors"),
              metadata={"call_params": ",".join(params), "numpy_seed": str(NUMPY_SEED)})


if __name__ == "__main__":
    main()
