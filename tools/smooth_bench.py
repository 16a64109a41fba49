#!/usr/bin/env python3
"""Timing of the long-video smoothing loop (lkgd_amd.pipeline.StableVideoDiffusionPipelineSmooth.denoise_smooth) on one GPU.

The video: T = 56 frames x 576x1024 (latents 72x128), windows of 14 frames, CFG (UNet batch 4 = [window, reversed window] x
[uncond, cond]), start_step 15 of 25 Euler steps, the joint-attention patch with flip=True and mask [0, 1, 0, 1] on the
real-width UNet; random-init fp16 weights, synthetic inputs, latents in and out (CLIP / VAE excluded).  Three loops over the same
windows (np.random is seeded alike before each):

    baseline      the window forwards (module walk) with the loop glue as the reference writes it - gather, flip, cat, repeat,
                  scatter of the forward clip's noise - done by torch ops around the existing lkgd_prepare_unet_input (per window)
                  and lkgd_cfg_euler_step (once per step on the assembled [1, T] tensor).  This loop exists in this tool only.
    windowed      denoise_smooth with use_replay off: lkgd_window_prepare_input / lkgd_window_cfg_euler_step, module walk
    windowed+replay   denoise_smooth as shipped: full windows replay the recorded forward

Prints one JSON line: ms per loop for each (device events around --steps synchronised calls after --warmup calls), denoised
frames/s, and whether the three results are bit-equal.

    python tools/smooth_bench.py [--steps 1] [--warmup 1]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(dev, T, H, W, patched=True):
    import bench
    from lkgd_amd import patch
    from lkgd_amd.pipeline import StableVideoDiffusionPipelineSmooth
    unet = bench.build_unet(dev, tiny=False)
    if patched:
        patch.apply_patch(unet, flip=True)
        patch.initialize_joint_layers(unet)
        g = torch.Generator(device=dev).manual_seed(11)
        with torch.no_grad():            # the zero-initialised joint projections would make the joint branch an identity
            for name, p in unet.named_parameters():
                if "attn1n" in name or "conv1n" in name:
                    p.copy_((torch.randn(p.shape, generator=g, device=dev) * (0.5 / max(p.shape[-1], 1) ** 0.5)).to(p.dtype))
        unet.invalidate()
        patch.set_joint_attention_mask(unet, [0, 1, 0, 1])
    pipe = StableVideoDiffusionPipelineSmooth(unet=unet)
    gen = torch.Generator().manual_seed(12345)
    img = (torch.randn(T, 4, H, W, generator=gen) * 0.18215).half().to(dev)
    emb = torch.randn(T, 1, 1024, generator=gen).half().to(dev)
    noise = torch.randn(1, T, 4, H, W, generator=gen)
    ids = torch.tensor([[6.0, 127.0, 0.02]])
    return pipe, img, emb, noise, ids


@torch.no_grad()
def baseline_loop(pipe, latents, img, emb, ids, nf, steps, gmin, gmax, start_step):
    """the reference's loop :545-594 with torch ops for the glue, around the kernels the other pipelines use"""
    from lkgd_amd import ops
    from lkgd_amd.pipeline import smooth_chunks
    unet, sch = pipe.unet, pipe.scheduler
    dev = unet.device
    _, T, _, H, W = latents.shape
    sch.set_timesteps(steps, device=None)
    image_latents = torch.cat([torch.zeros_like(img), img], dim=0)             # :470-471
    embs = torch.cat([torch.zeros_like(emb), emb], dim=0)
    ids4 = ids.to(device=dev, dtype=torch.float32).repeat(4, 1)
    for i, t in enumerate(sch.timesteps_host):
        if i < start_step:
            continue
        sigma, sigma_next = sch.sigmas_host[i], sch.sigmas_host[i + 1]
        noise_pred = torch.empty(2, T, H * W, 4, dtype=torch.float16, device=dev)     # [uncond | cond] of the forward clips
        gs = torch.empty(T, dtype=torch.float32)
        for f0, n in smooth_chunks(T, nf):
            chunk = latents[:, f0:f0 + n]
            lc = torch.cat([chunk, chunk.flip(dims=[1])], dim=0).contiguous()          # :551
            first = [f0, f0 + n - 1, f0 + T, f0 + n - 1 + T]                           # :554
            cur = image_latents[first].unsqueeze(1).repeat(1, n, 1, 1, 1).contiguous() # :557-559
            tok = ops.prepare_unet_input(lc, cur, 2, sigma)                            # :565-568
            out, _ = unet.forward_tokens(tok, 4, n, H, W, t, embs[first].contiguous(), ids4)
            out = out.view(4, n, H * W, 4)
            noise_pred[0, f0:f0 + n] = out[0]                                          # :587-591, CFG deferred to the step
            noise_pred[1, f0:f0 + n] = out[2]
            gs[f0:f0 + n] = torch.linspace(gmin, gmax, n)
        ops.cfg_euler_step(noise_pred.view(-1, 4), latents, gs.to(dev), 2, sigma, sigma_next,
                           v_prediction=sch.config.prediction_type == "v_prediction")  # :594
    return latents


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1, help="timed loops per variant")
    ap.add_argument("--warmup", type=int, default=1, help="untimed loops per variant")
    ap.add_argument("--total-frames", type=int, default=56)
    ap.add_argument("--frames", type=int, default=14, help="window length (num_frames)")
    ap.add_argument("--height", type=int, default=576)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--inference-steps", type=int, default=25)
    ap.add_argument("--start-step", type=int, default=15)
    ap.add_argument("--no-patch", action="store_true", help="stock UNet (no joint attention)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = torch.device("cuda:0")
    T, nf, H, W = a.total_frames, a.frames, a.height // 8, a.width // 8
    pipe, img, emb, noise, ids = build(dev, T, H, W, patched=not a.no_patch)
    pipe.scheduler.set_timesteps(a.inference_steps)
    start = pipe._noisy_start(img, noise, a.start_step)

    def variant(name):
        np.random.seed(7)
        lat = start.clone()
        if name == "baseline":
            return baseline_loop(pipe, lat, img, emb, ids, nf, a.inference_steps, 1.0, 3.0, a.start_step)
        pipe.use_replay = name == "windowed+replay"
        return pipe.denoise_smooth(lat, img, emb, ids, nf, a.inference_steps, 1.0, 3.0, start_step=a.start_step)
    res, outs = {}, {}
    for name in ("baseline", "windowed", "windowed+replay"):
        for _ in range(a.warmup):
            variant(name)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            outs[name] = variant(name)
        t1.record()
        torch.cuda.synchronize()
        res[name] = t0.elapsed_time(t1) / a.steps
    pipe.use_replay = True
    pipe.release_arena()
    np.random.seed(7)
    from lkgd_amd.pipeline import smooth_chunks
    windows = sum(len(smooth_chunks(T, nf)) for _ in range(a.inference_steps - a.start_step))
    print(json.dumps({
        "workload": f"smoothing loop: {T}f x {8 * H}x{8 * W}, windows of {nf}, CFG, Euler steps {a.start_step}..{a.inference_steps - 1}, "
                    + ("stock UNet" if a.no_patch else "joint patch (flip, mask [0,1,0,1])"),
        "euler_steps_run": a.inference_steps - a.start_step, "window_forwards": windows,
        "ms_per_loop": {k: round(v, 2) for k, v in res.items()},
        "frames_per_s": {k: round(T * 1000.0 / v, 4) for k, v in res.items()},
        "ms_saved_per_window": {k: round((res["baseline"] - res[k]) / windows, 3) for k in ("windowed", "windowed+replay")},
        "bit_equal": {k: bool(torch.equal(outs[k], outs["baseline"])) for k in ("windowed", "windowed+replay")},
        "finite": bool(torch.isfinite(outs["windowed+replay"]).all()), "timed_loops": a.steps, "warmup_loops": a.warmup,
    }), flush=True)


if __name__ == "__main__":
    main()
