#!/usr/bin/env python3
"""One loop step of lkgd_amd/ddim_inversion.py at the CogVideoX-5B text-to-video geometry, on one MI355X.

    python tools/cogvideox_ddim_inversion_bench.py [--rounds 3] [--warmup 1] [--layers 42] [--out FILE]
        one JSON line (also written to FILE): ms per step, medians over ``--rounds`` alternations in one process, of
        * ``inverse``: a ``DDIMInverseScheduler`` step under guidance - ``lkgd_dit_patch_rows``, ``forward_rows`` on [u, c],
          ``lkgd_dit_cfg_ddim_step`` with (A, -M, 0, 1);
        * ``plain``: the same step with ``CogVideoXDDIMScheduler`` (the text-to-video loop's step);
        * ``guided``: the step under ``OverrideAttnProcessors`` with reference latents - the rows of sample and reference,
          ``forward_rows`` on [u, ref_u, c, ref_c] (per pair Sq = L queries against 2L keys + the reference's own L x L), the head
          for [u, c], the step.
        Geometry: 48 heads x 64, 42 layers, rotary without a learned table, 16 latent channels; 49 x 480 x 720 pixels = 13 x 60 x 90
        latents = 17 550 video + 226 text rows per batch entry.  Random weights.

By FLOPs a guided step's attention is about 3x a plain step's (L x 2L + L x L against L x L per CFG entry) and everything else about
2x (twice the rows, except the head).  The number is recorded, nothing is gated on it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _model(dev, layers):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import unet as pu
    with torch.device("meta"):
        m = pc.CogVideoXTransformer3DModel(pc.DiTConfig(num_attention_heads=48, num_layers=layers, in_channels=16,
                                                        use_rotary_positional_embeddings=True))
    m = m.to(torch.float16).to_empty(device=dev)
    pu.init_synthetic_weights_(m, seed=0)
    return m


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=42)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cogvideox_ddim_inversion_bench needs the MI355X: there is nothing to time without it")
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ddim_inversion as di
    from lkgd_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with torch.no_grad():
        m = _model(dev, args.layers)
        g = torch.Generator().manual_seed(1)
        shape = (1, 13, 16, 60, 90)
        lat0 = torch.randn(shape, generator=g).half().to(dev)
        ref = torch.randn(shape, generator=g).half().to(dev)
        text = torch.randn(2, 226, 4096, generator=g).half().to(dev)
        text_pairs = text.repeat_interleave(2, dim=0).contiguous()
        grid = (13, 30, 45)
        Tv = 13 * 30 * 45
        rope = tuple(t.to(dev) for t in pc.rotary_tables(m.config, *grid))
        fwd = pc.CogVideoXDDIMScheduler(snr_shift_scale=1.0)
        inv = di.DDIMInverseScheduler(**fwd.config)
        fwd.set_timesteps(50)
        inv.set_timesteps(50)
        t_inv, t_fwd = int(inv.timesteps[25]), int(fwd.timesteps[25])
        gd = 6.0
        lat = lat0.clone()
        rows1 = torch.empty(Tv, 64, dtype=torch.float16, device=dev)
        rows2 = torch.empty(2 * Tv, 64, dtype=torch.float16, device=dev)

        def step(sched, t):
            ops.dit_patch_rows(lat, None, 2, out=rows1)
            noise = m.forward_rows(rows1, grid, text, float(t), image_rotary_emb=rope)
            ops.dit_cfg_ddim_step(noise, lat, 2, 2, gd, *sched.coefficients(t))

        def guided():
            ops.dit_patch_rows(lat, None, 2, out=rows2[:Tv])
            ops.dit_patch_rows(ref, None, 2, out=rows2[Tv:])
            noise = m.forward_rows(rows2, grid, text_pairs, float(t_fwd), image_rotary_emb=rope)
            ops.dit_cfg_ddim_step(noise, lat, 2, 2, gd, *fwd.coefficients(t_fwd))

        def guided_step():
            with di.OverrideAttnProcessors(m):
                guided()
        forms = {"inverse": lambda: step(inv, t_inv), "plain": lambda: step(fwd, t_fwd), "guided": guided_step}
        times = {n: [] for n in forms}
        finite = True
        for i in range(args.warmup + args.rounds):
            for n, fn in forms.items():
                lat.copy_(lat0)                   # the in-place operand stays in range
                ms = _timed(fn)
                finite = finite and bool(torch.isfinite(lat.float()).all())
                if i >= args.warmup:
                    times[n].append(ms)
    med = {n: statistics.median(v) for n, v in times.items()}
    line = {"tool": "cogvideox_ddim_inversion_bench", "geometry": "CogVideoX-5B T2V: 48 heads, %d layers, 13 x 60 x 90 latents, "
            "17 550 + 226 rows per entry, guidance 6, random weights" % args.layers, "rounds": args.rounds, "warmup": args.warmup,
            "timing": "device events around one step (patch rows, forward_rows, step kernel); host launch overhead included",
            "ms_per_step": {n: round(v, 2) for n, v in med.items()},
            "ms_per_step_all": {n: [round(x, 2) for x in v] for n, v in times.items()},
            "guided_over_plain": round(med["guided"] / med["plain"], 3), "inverse_over_plain": round(med["inverse"] / med["plain"], 3),
            "finite_output": finite}
    out = json.dumps(line)
    print(out, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(out + "\n")


if __name__ == "__main__":
    main()
