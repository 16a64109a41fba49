#!/usr/bin/env python3
"""Generate tests/golden/trans_controlnet.safetensors by EXECUTING THE REFERENCE'S OWN trans-ControlNet pipeline.

Runs only where the reference tree is mounted (build container, CPU, fp32).  Uses make_goldens.py's name-only stubs and
stand-in boundary stages, then calls ``pipeline_stable_video_diffusion_trans_controlnet.StableVideoDiffusionPipeline.__call__``
(output_type="latent") at the tiny config on:

* the stock UNet (models/unet_spatio_temporal_condition_controlnet.py), seeded, weights rounded to fp16, patched with the
  reference's ``patch.apply_patch`` (spatial + temporal) + ``initialize_joint_layers``, joint layers seeded
  (lora_cases.seed_joint_and_lora_) so the joint branch is not an identity, joint mask [1, 0, 1, 0] (utils/util.py:695);
* models/controlnet_sdv.py ``ControlNetSDVModel`` with conditioning_channels=2, seeded, rounded to fp16;
* two images (two clips, a CFG batch of 4), 4 frames of 8x8 latents, a list of two 2-channel conditions, 4 steps.

``torch.randn_like`` is replaced by a recorded tensor so that the noise ``add_noise`` uses is stored.  Every executed step's
latents are recorded through ``callback_on_step_end``; the UNet's first call records the boundary-stage outputs (image
embeddings, image latents, added time ids), so the tests need no CLIP / VAE.

Cases:  a = direct_fusion, start_step 1, original_latents, controlnet_cond_scale 0.8, controlnet_scale 0.5
        b = joint attention on (no fusion), same ControlNet scales, from the start

Weights are NOT stored: the tests regenerate them from the seeds (checksums are stored).

Usage:  python tests/golden/make_goldens_trans_controlnet.py
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import torch                                              # noqa: E402
from safetensors.torch import save_file                   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_goldens as mg                                  # noqa: E402
from make_goldens import REF, TINY, WSEED, _FakeCLIP, _FakeVAE, _mod, checksum, install_stubs, load_ref   # noqa: E402
from lora_cases import seed_joint_and_lora_               # noqa: E402
from oracle import unet as ou                              # noqa: E402

UNET_SEED = WSEED + 21        # tests/test_trans_controlnet_gpu.py regenerates the weights from these seeds
CTRL_SEED = WSEED + 22
JOINT_SEED = WSEED + 23
INPUT_SEED = 241
JOINT_MASK = [1, 0, 1, 0]     # utils/util.py:695
FRAMES, HW, STEPS = 4, 8, 4
CASES = {
    "a": dict(direct_fusion=True, start_step=1, original=True, controlnet_cond_scale=0.8, controlnet_scale=0.5),
    "b": dict(direct_fusion=False, start_step=0, original=False, controlnet_cond_scale=0.8, controlnet_scale=0.5),
}


def inputs():
    g = torch.Generator().manual_seed(INPUT_SEED)
    return dict(
        image=torch.rand(2, 3, 8 * HW, 8 * HW, generator=g),
        latents0=torch.randn(2, FRAMES, 4, HW, HW, generator=g),
        original_latents=torch.randn(2, FRAMES, 4, HW, HW, generator=g),
        noise=torch.randn(2, FRAMES, 4, HW, HW, generator=g),
        cond0=torch.rand(FRAMES, 2, 8 * HW, 8 * HW, generator=g),
        cond1=torch.rand(FRAMES, 2, 8 * HW, 8 * HW, generator=g),
    )


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
    ref_ctrl = load_ref("models/controlnet_sdv.py", "models.controlnet_sdv")
    _mod("patch")
    load_ref("patch/utils.py", "patch.utils")
    patch_mod = load_ref("patch/patch.py", "patch.patch")
    sys.modules["patch"].patch = patch_mod
    pipe_mod = load_ref("pipeline/pipeline_stable_video_diffusion_trans_controlnet.py", "ref_pipeline_trans_controlnet")
    from oracle.scheduler import SchedulerConfig

    kw = dict(TINY.__dict__)
    inp = inputs()
    out = {k: v for k, v in inp.items() if k != "image"}
    with torch.no_grad():
        unet = _round16_(ou.init_weights_(ref_stock.UNetSpatioTemporalConditionControlNetModel(**kw), UNET_SEED))
        out["checksum_unet_base"] = torch.tensor(checksum(unet), dtype=torch.float64)
        patch_mod.apply_patch(unet, flip=False, with_temporal_block=True, with_spatial_block=True)
        patch_mod.initialize_joint_layers(unet)
        names = seed_joint_and_lora_(unet, JOINT_SEED)
        out["n_joint_seeded"] = torch.tensor(len(names))
        out["checksum_unet"] = torch.tensor(checksum(unet), dtype=torch.float64)
        patch_mod.set_joint_attention_mask(unet, JOINT_MASK)
        ctrl = ref_ctrl.ControlNetSDVModel(**kw, conditioning_channels=2,
                                           conditioning_embedding_out_channels=(16, 32, 96, 256))
        _round16_(ou.init_weights_(ctrl, CTRL_SEED))
        out["checksum_controlnet"] = torch.tensor(checksum(ctrl), dtype=torch.float64)

    rec = {}
    orig_forward = unet.forward

    def spy(sample, t, **k):
        if "enc" not in rec:
            rec["enc"], rec["ids"] = k["encoder_hidden_states"].clone(), k["added_time_ids"].clone()
            rec["img"] = sample[:, :, 4:].clone()
        return orig_forward(sample, t, **k)
    unet.forward = spy

    real_randn_like = torch.randn_like
    for name, case in CASES.items():
        sched = sched_mod.EulerDiscreteScheduler(**SchedulerConfig().__dict__)
        fe = lambda images, **k: mg.SimpleNamespace(pixel_values=images)   # noqa: E731
        pipe = pipe_mod.StableVideoDiffusionPipeline(vae=_FakeVAE(), image_encoder=_FakeCLIP(), unet=unet,
                                                     controlnet=ctrl, scheduler=sched, feature_extractor=fe)
        steps, idx = [], []
        torch.randn_like = lambda x, **k: inp["noise"].to(dtype=x.dtype).clone()
        try:
            res = pipe(inp["image"], [inp["cond0"], inp["cond1"]], height=8 * HW, width=8 * HW, num_frames=FRAMES,
                       num_inference_steps=STEPS, latents=inp["latents0"].clone(), output_type="latent",
                       generator=torch.Generator().manual_seed(INPUT_SEED + 1),
                       callback_on_step_end=lambda p, i, t, kw_: (steps.append(kw_["latents"].clone()), idx.append(i),
                                                                  {})[2],
                       controlnet_cond_scale=case["controlnet_cond_scale"],
                       original_latents=inp["original_latents"].clone() if case["original"] else None,
                       start_step=case["start_step"], direct_fusion=case["direct_fusion"],
                       controlnet_scale=case["controlnet_scale"])
        finally:
            torch.randn_like = real_randn_like
        assert idx == list(range(case["start_step"], STEPS)), idx
        out[f"{name}_step_latents"] = torch.stack(steps).float()
        out[f"{name}_final"] = res.frames.float()
        print("case %s: %d steps, final std %.4f, dtype %s" % (name, len(steps), res.frames.std(), res.frames.dtype))
    out["image_embeddings"], out["added_time_ids"], out["image_latents"] = rec["enc"], rec["ids"], rec["img"]
    print("a vs b final max delta %.4f" % (out["a_final"] - out["b_final"]).abs().max())
    save_file({k: v.contiguous() for k, v in out.items()}, os.path.join(HERE, "trans_controlnet.safetensors"))


if __name__ == "__main__":
    main()
