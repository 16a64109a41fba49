#!/usr/bin/env python3
"""The CogVideoX 3-D causal VAE encode (lkgd_amd/cogvideox_vae.py) at the real geometry on one MI355X, against the ATen form a user
without the module would run.

    python tools/cogvideox_vae_encode_bench.py [--rounds 3] [--height 480] [--width 720] [--no-baseline] [--out FILE]

Random weights at the real ``vae/config.json`` (there is no checkpoint on a GPU box), two clips: x = [1, 3, 1, 480, 720] (the image the
I2V pipeline's ``prepare_latents`` encodes) and [1, 3, 49, 480, 720] (the clip of inference/cli_vae_demo.py).  One JSON line (also
written to ``profiles/cogvideox_vae_encode_bench.json``), per clip:
    * ms per encode of the HIP path and of the baseline, by device events around whole encodes (the posterior's mean included) after
      one warm-up encode of each, the two alternating in one process; the baseline is the tests' oracle
      (tests/cogvideox_vae_encoder_oracle.py: the torch restatement of diffusers' encoder) in fp16 on the GPU;
    * peak allocated device memory of either, and the relative L2 between the two sets of moments;
    * per kernel family (conv_in = pixel taps + its GEMM, causal 3x3x3 conv, downsampler 3x3 conv, shortcut GEMMs, temporal pool,
      GroupNorm statistics and apply, posterior) the time of one instrumented encode (events around every launch), with the FLOP /
      bytes this tool counts for the family and the rate they give.
The alternative for conv_in - pixels padded to 64 channels through LKGD_A_CCONV3, K = 1728 - is NOT measured here: the choice of the
tap rows rests on the arithmetic (81 real taps of 1728) alone.
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
    """events around every launch of one encode, grouped by kernel family, with the work this tool counts for it"""

    NAMES = ("gemm", "cogvae_pixel_taps", "cogvae_time_pool", "cogvae_posterior", "groupnorm_stats", "groupnorm_apply")

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
        self.saved = {n: getattr(ops, n) for n in self.NAMES}
        s = self.saved

        def gemm(a0, w, out, **kw):
            M, N, K = kw["M"], kw["N"], kw["K"]
            mode = kw.get("mode", ops.A_PLAIN)
            if mode == ops.A_CCONV3:
                fam = "causal conv 3x3x3"
            elif mode == ops.A_CONV3X3:
                fam = "downsampler conv 3x3 stride 2"
            else:
                fam = "conv_in: GEMM on the tap rows" if getattr(a0, "_bench_taps", False) else "plain GEMM (shortcut)"
            return self._add(fam, lambda: s["gemm"](a0, w, out, **kw), flop=2.0 * M * N * K)

        def pixel_taps(x, t0, Tc, out=None):
            rows = x.shape[0] * Tc * x.shape[3] * x.shape[4]
            taps = self._add("conv_in: pixel taps", lambda: s["cogvae_pixel_taps"](x, t0, Tc, out=out),
                             nbytes=2.0 * rows * (128 + x.shape[1]))          # rows written + each pixel read once from HBM
            taps._bench_taps = True                                           # (the GEMM that reads them is conv_in's)
            return taps

        def time_pool(x, B, T, HW, out=None):
            nb = 2.0 * x.shape[1] * B * HW * (T + ops.pooled_frames(T))
            return self._add("temporal pool", lambda: s["cogvae_time_pool"](x, B, T, HW, out=out), nbytes=nb)

        def posterior(mom, B, lc, T, h, w, noise=None, scale=1.0):
            n = B * T * h * w * lc
            return self._add("posterior", lambda: s["cogvae_posterior"](mom, B, lc, T, h, w, noise=noise, scale=scale),
                             nbytes=2.0 * n * (2 if noise is None else 5))

        def groupnorm_stats(x0, *a, **kw):
            cols = getattr(x0, "_lkgd_colstats", None) is not None
            return self._add("GroupNorm statistics" + (" (from column sums)" if cols else " (read pass)"),
                             lambda: s["groupnorm_stats"](x0, *a, **kw), nbytes=0.0 if cols else 2.0 * x0.numel())

        def groupnorm_apply(x0, *a, **kw):
            return self._add("GroupNorm apply + SiLU", lambda: s["groupnorm_apply"](x0, *a, **kw), nbytes=4.0 * x0.numel())

        for n, f in zip(self.NAMES, (gemm, pixel_taps, time_pool, posterior, groupnorm_stats, groupnorm_apply)):
            setattr(ops, n, f)
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
        taps, gemm_in = out.get("conv_in: pixel taps"), out.get("conv_in: GEMM on the tap rows")
        if taps and gemm_in:
            out["conv_in: taps + GEMM"] = dict(launches=taps["launches"] + gemm_in["launches"], ms=round(taps["ms"] + gemm_in["ms"], 3))
        return out


def _moments(dist):
    return torch.cat([dist.mean.float(), dist.logvar.float()], dim=1)


def _one_clip(m, o, ops, frames, args):
    g = torch.Generator().manual_seed(1 + frames)
    x = (0.5 * torch.randn(1, 3, frames, args.height, args.width, generator=g)).clamp(-1, 1).half().to("cuda")
    res = dict(clip=list(x.shape))
    torch.cuda.reset_peak_memory_stats()
    got = _moments(m.encode(x).latent_dist)                     # warm-up (packs the weights)
    res["moments"] = list(got.shape)
    res["hip_peak_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    if not args.no_baseline:
        torch.cuda.reset_peak_memory_stats()
        ref = o.moments(x)                                      # warm-up
        res["aten_peak_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
        ref = torch.cat([ref[:, :16].float(), ref[:, 16:].float().clamp(-30, 20)], dim=1)
        res["hip_vs_aten_fp16_rel_l2"] = round(((got - ref).norm() / ref.norm()).item(), 5)
        del ref
    del got
    hip, aten = [], []
    for _ in range(args.rounds):
        hip.append(_timed(lambda: m.encode(x)))
        if not args.no_baseline:
            aten.append(_timed(lambda: o.moments(x)))
    res["hip_ms"] = round(statistics.median(hip), 2)
    res["hip_ms_all"] = [round(t, 2) for t in hip]
    if aten:
        res["aten_fp16_ms"] = round(statistics.median(aten), 2)
        res["aten_fp16_ms_all"] = [round(t, 2) for t in aten]
        res["speedup"] = round(res["aten_fp16_ms"] / res["hip_ms"], 2)
    with _Families(ops) as fam:
        m.encode(x).latent_dist.sample(torch.Generator(device="cuda").manual_seed(0))
    res["families"] = fam.report()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=720)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 49])
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cogvideox_vae_encode_bench.json"))
    args = ap.parse_args()

    import cogvideox_vae_encoder_oracle as eo
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("cogvideox_vae_encode_bench measures on the MI355X: no GPU found")
    cfg = eo.CogVAEConfig()
    torch.manual_seed(0)
    o = eo.AutoencoderKLCogVideoX(cfg)
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**cfg.__dict__), encoder=True)
    m.load_state_dict(o.state_dict())
    m = m.half().to("cuda")
    o = o.half().to("cuda")
    res = dict(tool="cogvideox_vae_encode_bench", rounds=args.rounds, device=torch.cuda.get_device_name(0),
               conv_in_pad_to_64_alternative="not measured", clips=[_one_clip(m, o, ops, f, args) for f in args.frames])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
