#!/usr/bin/env python3
"""Timing of the trans-ControlNet pipeline loop (lkgd_amd.pipeline.StableVideoDiffusionPipelineTransControlNet) on one GPU.

The pair: 2 clips x 14 frames x 576x1024 (latents 72x128), CFG (UNet batch 4), 25 Euler steps, the ControlNet-SVD encoder
with conditioning_channels=2 every step, the joint-attention patch (spatial + temporal, mask [1, 0, 1, 0]) on the real-width
UNet; random-init fp16 weights, synthetic inputs, output_type="latent" (CLIP / VAE excluded).  Configurations:
direct_fusion off (joint hooks on) / on  x  start_step 0 / 10 (with original_latents).  Prints one JSON line per
configuration: ms per pipeline call (device events around a synchronised window of --steps calls, after --warmup calls) and
denoised frames/s.

    python tools/trans_controlnet_bench.py [--steps 3] [--warmup 1]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402


def build(dev, F, H, W):
    import bench
    from lkgd_amd import controlnet as pc
    from lkgd_amd import patch
    from lkgd_amd import unet as pu
    from lkgd_amd.pipeline import StableVideoDiffusionPipelineTransControlNet
    unet = bench.build_unet(dev, tiny=False)
    patch.apply_patch(unet, flip=False, with_temporal_block=True, with_spatial_block=True)
    patch.initialize_joint_layers(unet)
    g = torch.Generator(device=dev).manual_seed(11)
    with torch.no_grad():            # the zero-initialised joint projections would make the joint branch an identity
        for name, p in unet.named_parameters():
            if "attn1n" in name or "conv1n" in name:
                p.copy_((torch.randn(p.shape, generator=g, device=dev) * (0.5 / max(p.shape[-1], 1) ** 0.5)).to(p.dtype))
    unet.invalidate()
    patch.set_joint_attention_mask(unet, [1, 0, 1, 0])
    with torch.device("meta"):
        cn = pc.ControlNetSDVModel(pu.UNetConfig(**{k: v for k, v in unet.config.__dict__.items()
                                                    if k in pu.UNetConfig.__dataclass_fields__}), conditioning_channels=2)
    cn = cn.to(torch.float16).to_empty(device=dev)
    pu.init_synthetic_weights_(cn, seed=1)
    pipe = StableVideoDiffusionPipelineTransControlNet(unet=unet, controlnet=cn)
    gen = torch.Generator().manual_seed(12345)
    lat0 = torch.randn(2, F, 4, H, W, generator=gen).to(dev)
    img = torch.randn(2, 4, H, W, generator=gen) * 0.18215
    img = torch.cat([torch.zeros_like(img), img]).unsqueeze(1).repeat(1, F, 1, 1, 1).half().to(dev).contiguous()
    emb = torch.cat([torch.zeros(2, 1, 1024), torch.randn(2, 1, 1024, generator=gen)]).half().to(dev)
    conds = [torch.rand(F, 2, 8 * H, 8 * W, generator=gen) for _ in range(2)]
    return pipe, lat0, img, emb, conds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3, help="timed pipeline calls per configuration")
    ap.add_argument("--warmup", type=int, default=1, help="untimed pipeline calls per configuration")
    ap.add_argument("--frames", type=int, default=14)
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--inference-steps", type=int, default=25)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    F, H, W = a.frames, a.height // 8, a.width // 8
    pipe, lat0, img, emb, conds = build(dev, F, H, W)
    for direct_fusion in (False, True):
        for start_step in (0, 10):
            def call():
                return pipe(None, conds, height=8 * H, width=8 * W, num_frames=F, num_inference_steps=a.inference_steps,
                            latents=lat0, output_type="latent", image_embeddings=emb, image_latents=img,
                            original_latents=lat0 if start_step else None, start_step=start_step,
                            direct_fusion=direct_fusion, controlnet_cond_scale=1.0, controlnet_scale=1.0).frames
            for _ in range(a.warmup):
                out = call()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                out = call()
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.steps
            print(json.dumps({
                "workload": f"trans-ControlNet pair: 2 clips x {F}f x {8 * H}x{8 * W}, CFG, {a.inference_steps}-step Euler, "
                            "ControlNet (2-channel condition) + joint patch (spatial+temporal)",
                "direct_fusion": direct_fusion, "start_step": start_step,
                "euler_steps_run": a.inference_steps - start_step,
                "ms_per_call": round(ms, 2), "frames_per_s": round(2 * F * 1000.0 / ms, 4),
                "timed_calls": a.steps, "warmup_calls": a.warmup, "finite": bool(torch.isfinite(out).all()),
                "latents_dtype": str(out.dtype).replace("torch.", ""),
            }), flush=True)
    pipe.release_arena()


if __name__ == "__main__":
    main()
