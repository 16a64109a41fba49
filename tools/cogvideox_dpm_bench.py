#!/usr/bin/env python3
"""The DPM-Solver++ step kernel (include/lkgd_hip_dit_dpm.h) against the ATen sequence it replaces, on one MI355X.

    python tools/cogvideox_dpm_bench.py [--rounds 20] [--warmup 3] [--inner 200] [--out FILE]
        one JSON line (also written to FILE): medians, in one process with the forms alternating, of the per-step work after
        proj_out at
        * the 2B / 5B-I2V geometry: 13 x 60 x 90 latents, C = 16, cfg = 2, fp16 latents - lkgd_dit_cfg_dpm_step, first and second order;
        * the 1.5 I2V geometry of tools/cogvideox_fuse_bench.py --v15: 22 x 96 x 170 latents, C = 16, p_t = 2 -
          lkgd_dit_cfg_dpm_step_t, second order;
        each as (a) the launch alone on noise drawn beforehand, (b) ``dpm_noise`` + the launch, which is what ``denoise`` runs per
        step, and (c) the ATen form: un-patchify, .float(), chunk, the CFG statements, ``CogVideoXDPMScheduler.step`` (which draws
        its own noise, once or twice), .half().  (b) and (c) do the same work; (a) is the kernel's share of (b).  Every form is
        checked bit for bit against (c)'s statements on the same noise first.

A window is ``--inner`` calls of one form between two device events, divided by ``--inner``: a single launch is too short for
the event clock.  Times include the host's launch overhead - this is a latency-bound launch - and are not kernel times.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner          # us per call


def _unpatchify(rows, B, F_, H, W, p_t, p=2):
    """cogvideox_transformer_3d.py:624-625, or with ``p_t`` :626-630"""
    h, w = H // p, W // p
    if p_t is None:
        return rows.reshape(B, F_, h, w, -1, p, p).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4).contiguous()
    return rows.reshape(B, F_ // p_t, h, w, -1, p_t, p, p).permute(0, 1, 5, 4, 2, 6, 3, 7).flatten(6, 7).flatten(4, 5).flatten(1, 2) \
        .contiguous()


def _aten(sched, noise_rows, lat, old, t, t_back, g, gen, p_t):
    """the loop body of pipeline_cogvideox_image2video.py:860-884 on proj_out's rows"""
    B, F_, _, H, W = lat.shape
    noise = _unpatchify(noise_rows, 2 * B, F_, H, W, p_t).float()
    u, c = noise.chunk(2)
    noise = u + g * (c - u)
    prev, x0 = sched.step(noise, old, t, t_back, lat, generator=gen)
    return prev.to(torch.float16), x0


def measure(args, dev, name, shape, p_t, order):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ops
    B, F_, C_, H, W = shape
    pt = p_t or 1
    g0 = torch.Generator().manual_seed(1)
    lat = torch.randn(shape, generator=g0).half().to(dev)
    old = torch.randn(shape, generator=g0).to(dev)
    noise_rows = torch.randn(2 * B * (F_ // pt) * (H // 2) * (W // 2), C_ * pt * 4, generator=g0).half().to(dev)
    sched = pc.CogVideoXDPMScheduler()
    sched.set_timesteps(50)
    ts = sched.timesteps.tolist()
    t, t_back = ts[10], (ts[9] if order == 2 else None)
    gd, k = pc.dynamic_guidance(6.0, 50, t), sched.coefficients(t, t_back)
    assert k.order == order
    glue = {} if p_t is None else {"p_t": p_t}
    gen = torch.Generator(device=dev)
    # bit for bit first: the same seed gives both forms the same draws
    gen.manual_seed(3)
    ref, ref0 = _aten(sched, noise_rows, lat, old if order == 2 else None, t, t_back, gd, gen, p_t)
    gen.manual_seed(3)
    work, state = lat.clone(), old.clone()
    ops.dit_cfg_dpm_step(noise_rows, work, state, pc.dpm_noise(shape, lat.dtype, dev, gen, order), 2, 2, order, gd, k, **glue)
    same = bool(torch.equal(work, ref) and torch.equal(state, ref0))
    eps = pc.dpm_noise(shape, lat.dtype, dev, gen, order)

    def launch():
        ops.dit_cfg_dpm_step(noise_rows, work, state, eps, 2, 2, order, gd, k, **glue)

    def launch_with_draw():
        ops.dit_cfg_dpm_step(noise_rows, work, state, pc.dpm_noise(shape, lat.dtype, dev, gen, order), 2, 2, order, gd, k, **glue)

    def aten():
        _aten(sched, noise_rows, lat, old if order == 2 else None, t, t_back, gd, gen, p_t)
    forms = {"launch": launch, "draw_and_launch": launch_with_draw, "aten": aten}
    times = {n: [] for n in forms}
    for i in range(args.warmup + args.rounds):
        for n, fn in forms.items():
            work.copy_(lat)                       # the in-place operand stays in range over thousands of calls
            us = _timed(fn, args.inner)
            if i >= args.warmup:
                times[n].append(us)
    med = statistics.median
    elements = B * F_ * C_ * H * W
    # the bytes the launch moves (at these sizes largely through the 256-MB Infinity Cache, not HBM): both CFG entries of the rows (fp16), latents and eps read, latents written (fp16), x0 written (and
    # read when order is 2) in fp32
    traffic = elements * (2 * 2 + 2 + 2 + 2 + 4 + (4 if order == 2 else 0))
    return {"geometry": name, "order": order, "elements": elements, "bitwise_equal_to_aten": same,
            "launch_us_median": round(med(times["launch"]), 1), "launch_us_min": round(min(times["launch"]), 1),
            "draw_and_launch_us_median": round(med(times["draw_and_launch"]), 1),
            "draw_and_launch_us_min": round(min(times["draw_and_launch"]), 1),
            "aten_sequence_us_median": round(med(times["aten"]), 1), "aten_sequence_us_min": round(min(times["aten"]), 1),
            "launch_bytes": traffic, "not_slower": med(times["draw_and_launch"]) <= med(times["aten"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="alternations of the forms (>= 20 for a reported median)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=200, help="calls of one form per timed window")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cogvideox_dpm_bench needs the MI355X: there is nothing to time without it")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g2b = "13 x 60 x 90 latents, C = 16, cfg = 2, fp16: the 2B-I2V and the 5B-I2V loop alike"
    g15 = "22 x 96 x 170 latents, C = 16, cfg = 2, fp16, p_t = 2: the 1.5 I2V loop"
    with torch.no_grad():
        cases = [measure(args, dev, g2b, (1, 13, 16, 60, 90), None, 1), measure(args, dev, g2b, (1, 13, 16, 60, 90), None, 2),
                 measure(args, dev, g15, (1, 22, 16, 96, 170), 2, 2)]
    line = {"tool": "cogvideox_dpm_bench", "rounds": args.rounds, "warmup": args.warmup, "inner": args.inner,
            "timing": "device events around `inner` calls, per call; host launch overhead included", "step": cases,
            "valid": args.rounds >= 20 and all(c["bitwise_equal_to_aten"] for c in cases)}
    text = json.dumps(line)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
