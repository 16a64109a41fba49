#!/usr/bin/env python3
"""The CogVideoX 3-D causal VAE decode (lkgd_amd/cogvideox_vae.py) at the real geometry on one MI355X, against the ATen form a user
without the module would run.

    python tools/cogvideox_vae_bench.py [--rounds 3] [--frames 13] [--height 60] [--width 90] [--no-baseline] [--out FILE]

Random weights at the real ``vae/config.json`` (there is no checkpoint on a GPU box), z = [1, 16, 13, 60, 90] -> 49 x 480 x 720 frames.
One JSON line (also written to ``profiles/cogvideox_vae_bench.json``):
    * ms per decode of the HIP path and of the baseline, by device events around whole decodes after one warm-up decode of each, the
      two alternating in one process; the baseline is the tests' oracle (tests/cogvideox_vae_oracle.py: the torch restatement of
      diffusers' decoder) in fp16 on the GPU;
    * peak allocated device memory of either;
    * per kernel family (causal 3x3x3 conv, upsampler 3x3 conv, plain GEMMs, spatial norm, GroupNorm statistics) the time of one
      instrumented decode (events around every launch), with the FLOP / bytes this tool counts for the family and the rate they give;
    * the causal gather against LKGD_A_CONV3X3 at the same Cin / N / row count (256 -> 256 channels, 8 frames of 240 x 360).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)          # ms


class _Families:
    """events around every launch of one decode, grouped by kernel family, with the work this tool counts for it"""

    def __init__(self, ops):
        self.ops, self.rec, self.saved = ops, {}, {}

    def _add(self, fam, fn, flop=0.0, nbytes=0.0):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.rec.setdefault(fam, []).append((a, b, flop, nbytes))
        return r

    def __enter__(self):
        ops = self.ops
        self.saved = dict(gemm=ops.gemm, spatial_norm3d=ops.spatial_norm3d, groupnorm_stats=ops.groupnorm_stats)
        fam_of = {ops.A_CCONV3: "causal conv 3x3x3", ops.A_CONV3X3: "upsampler conv 3x3", ops.A_PLAIN: "plain GEMM (conv_y|conv_b, shortcut)"}

        def gemm(a0, w, out, **kw):
            M, N, K = kw["M"], kw["N"], kw["K"]
            return self._add(fam_of[kw.get("mode", ops.A_PLAIN)], lambda: self.saved["gemm"](a0, w, out, **kw), flop=2.0 * M * N * K)

        def spatial_norm3d(f, stats, gamma, beta, yb, tmap, out, *a, **kw):
            return self._add("spatial norm", lambda: self.saved["spatial_norm3d"](f, stats, gamma, beta, yb, tmap, out, *a, **kw),
                             nbytes=4.0 * f.numel())                      # f read + out written, fp16

        def groupnorm_stats(x0, *a, **kw):
            cols = getattr(x0, "_lkgd_colstats", None) is not None
            return self._add("GroupNorm statistics" + (" (from column sums)" if cols else " (read pass)"),
                             lambda: self.saved["groupnorm_stats"](x0, *a, **kw), nbytes=0.0 if cols else 2.0 * x0.numel())

        ops.gemm, ops.spatial_norm3d, ops.groupnorm_stats = gemm, spatial_norm3d, groupnorm_stats
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.ops, k, v)

    def report(self):
        torch.cuda.synchronize()
        out = {}
        for fam, evs in self.rec.items():
            ms = sum(a.elapsed_time(b) for a, b, _, _ in evs)
            flop, nbytes = sum(e[2] for e in evs), sum(e[3] for e in evs)
            out[fam] = dict(launches=len(evs), ms=round(ms, 3), tflop=round(flop / 1e12, 3), gbytes=round(nbytes / 1e9, 3),
                            tflops_per_s=round(flop / ms / 1e9, 1) if flop and ms else None,
                            tbytes_per_s=round(nbytes / ms / 1e9, 2) if nbytes and ms else None)
        return out


def _gather_pair(rounds):
    """the causal gather against LKGD_A_CONV3X3 at the same Cin / N / rows: 256 -> 256 channels, 8 frames of 240 x 360"""
    from lkgd_amd import ops
    Cin, N, T, H, W = 256, 256, 8, 240, 360
    M = T * H * W
    g = torch.Generator(device="cuda").manual_seed(0)
    a3 = torch.randn((T + 2) * H * W, Cin, generator=g, device="cuda", dtype=torch.float16)
    w3 = torch.randn(N, 27 * Cin, generator=g, device="cuda", dtype=torch.float16) * 0.01
    w2 = w3[:, :9 * Cin].contiguous()
    bias = torch.zeros(N, device="cuda")
    out = torch.empty(M, N, device="cuda", dtype=torch.float16)

    def causal():
        ops.gemm(a3, w3, out, M=M, N=N, K=27 * Cin, bias=bias, mode=ops.A_CCONV3, Cin=Cin, cconv=(T, H, W))

    def spatial():
        ops.gemm(a3, w2, out, M=M, N=N, K=9 * Cin, bias=bias, mode=ops.A_CONV3X3, Cin=Cin, conv=(H, W, H, W, 1, 0))

    causal(); spatial()
    tc, ts = [], []
    for _ in range(max(rounds, 5)):
        tc.append(_timed(causal)); ts.append(_timed(spatial))
    mc, ms = statistics.median(tc), statistics.median(ts)
    return dict(shape=f"Cin {Cin} N {N} M {M}", cconv3_ms=round(mc, 3), cconv3_tflops=round(2.0 * M * N * 27 * Cin / mc / 1e9, 1),
                conv3x3_ms=round(ms, 3), conv3x3_tflops=round(2.0 * M * N * 9 * Cin / ms / 1e9, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--height", type=int, default=60)
    ap.add_argument("--width", type=int, default=90)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cogvideox_vae_bench.json"))
    args = ap.parse_args()

    import cogvideox_vae_oracle as oc
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import ops

    cfg = oc.CogVAEConfig()
    torch.manual_seed(0)
    o = oc.AutoencoderKLCogVideoX(cfg)
    with torch.no_grad():
        for n, p in o.named_parameters():
            if n.endswith("conv_y.conv.bias"):
                p.add_(1.0)
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**cfg.__dict__))
    m.load_state_dict(o.state_dict())
    m = m.half().to("cuda")
    o = o.half().to("cuda")
    z = torch.randn(1, 16, args.frames, args.height, args.width, generator=torch.Generator().manual_seed(1)).half().to("cuda")

    res = dict(tool="cogvideox_vae_bench", latents=list(z.shape), rounds=args.rounds, device=torch.cuda.get_device_name(0))
    torch.cuda.reset_peak_memory_stats()
    got = m.decode(z).sample                                    # warm-up (packs the weights)
    res["frames_out"] = list(got.shape)
    res["hip_peak_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    ref = None
    if not args.no_baseline:
        torch.cuda.reset_peak_memory_stats()
        ref = o.decode(z)                                       # warm-up
        res["aten_peak_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        res["hip_vs_aten_fp16_rel_l2"] = round(((got.float() - ref.float()).norm() / ref.float().norm()).item(), 5)
    del got, ref
    hip, aten = [], []
    for _ in range(args.rounds):
        hip.append(_timed(lambda: m.decode(z)))
        if not args.no_baseline:
            aten.append(_timed(lambda: o.decode(z)))
    res["hip_ms"] = round(statistics.median(hip), 2)
    res["hip_ms_all"] = [round(t, 2) for t in hip]
    if aten:
        res["aten_fp16_ms"] = round(statistics.median(aten), 2)
        res["aten_fp16_ms_all"] = [round(t, 2) for t in aten]
        res["speedup"] = round(res["aten_fp16_ms"] / res["hip_ms"], 2)
    with _Families(ops) as fam:
        m.decode(z)
    res["families"] = fam.report()
    res["gather_pair"] = _gather_pair(args.rounds)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
