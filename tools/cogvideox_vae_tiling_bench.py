#!/usr/bin/env python3
"""The TILED decode and encode of the CogVideoX 3-D causal VAE (lkgd_amd/cogvideox_vae.py, ``enable_tiling``) at the real geometry on
one MI355X: tiles of equal shape as one batch against one tile at a time, against the untiled HIP path, and against the ATen form a
user without the module would run.

    python tools/cogvideox_vae_tiling_bench.py [--rounds 3] [--no-baseline] [--skip-encode] [--out FILE]

Random weights at the real ``vae/config.json`` (there is no checkpoint on a GPU box).  Decode: z = [1, 16, 13, 60, 90] (49 frames of
480 x 720: 3 x 3 tiles of 30 x 45 latents); encode: x = [1, 3, 1, 480, 720] and [1, 3, 49, 480, 720].  One JSON line (also written to
``profiles/cogvideox_vae_tiling_bench.json``), per input:
    * ms per pass of the tiled HIP path tile by tile (the default) and with equal-shaped tiles as one batch
      (``LKGD_COGVAE_TILE_BATCH=1``), of the untiled HIP path, and of the baseline - the tests' tiled oracle
      (tests/cogvideox_vae_tiling_oracle.py: the torch restatement of diffusers' tiled passes with its Python blend loops) in fp16 on
      the GPU - by device events around whole passes after one warm-up of each, the forms alternating in one process;
    * peak allocated device memory of each, the relative L2 between the tiled HIP result and the baseline, and whether the two HIP
      tile orders agree to the bit;
    * the seam launches of one instrumented pass: their count, summed time, the bytes this tool counts for them (the tile read and
      written, the neighbours' blended rows / columns read, the crop written) and the rate that gives.
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

SWITCH = "LKGD_COGVAE_TILE_BATCH"


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)          # ms


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    return r, round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)


class _Seams:
    """events around every seam launch of one pass, with the bytes this tool counts for it"""

    NAMES = ("cogvae_tile_blend_planar", "cogvae_tile_blend_rows")

    def __init__(self, ops):
        self.ops, self.rec, self.saved = ops, [], {}

    def __enter__(self):
        ops = self.ops
        self.saved = {n: getattr(ops, n) for n in self.NAMES}

        def wrap(name, planar):
            def f(tile, up, left, out, y0, x0, e_y, e_x, c_y, c_x):
                if planar:
                    Yt, Xt = tile.shape[-2:]
                    per = tile.numel() // (Yt * Xt)                    # elements per (y, x): the planes
                    Yu, Xl = (up.shape[-2] if up is not None else 0), (left.shape[-1] if left is not None else 0)
                else:
                    Yt, Xt = tile.shape[1:3]
                    per = tile.shape[0] * tile.shape[3]
                    Yu, Xl = (up.shape[1] if up is not None else 0), (left.shape[2] if left is not None else 0)
                ey, ex = min(Yu, Yt, e_y), min(Xl, Xt, e_x)
                n = 2 * Yt * Xt + ey * Xt + Yt * ex + min(c_y, Yt) * min(c_x, Xt)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                r = self.saved[name](tile, up, left, out, y0, x0, e_y, e_x, c_y, c_x)
                b.record()
                self.rec.append((a, b, 2.0 * per * n))
                return r
            return f

        ops.cogvae_tile_blend_planar = wrap("cogvae_tile_blend_planar", True)
        ops.cogvae_tile_blend_rows = wrap("cogvae_tile_blend_rows", False)
        return self

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            setattr(self.ops, k, v)

    def report(self):
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b, _ in self.rec)
        nbytes = sum(e[2] for e in self.rec)
        return dict(launches=len(self.rec), ms=round(ms, 4), mbytes=round(nbytes / 1e6, 2),
                    tbytes_per_s=round(nbytes / ms / 1e9, 3) if ms else None)


def _measure(forms, rounds):
    """``forms``: name -> callable; one warm-up of each has run; they alternate within every round"""
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(_timed(fn))
    out = {}
    for k, v in ms.items():
        out[k + "_ms"] = round(statistics.median(v), 2)
        out[k + "_ms_all"] = [round(t, 2) for t in v]
    return out


def _with_switch(value, fn):
    old = os.environ.get(SWITCH)
    os.environ[SWITCH] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[SWITCH]
        else:
            os.environ[SWITCH] = old


def _rel(a, b):
    a, b = a.float(), b.float()
    return round(((a - b).norm() / b.norm()).item(), 5)


def _one(name, shape, hip, aten, m, ops, args):
    """``hip()`` runs the HIP pass on the module as it is switched, ``aten()`` the tiled oracle; both return the result tensor"""
    res = {name: shape}

    def untiled():
        m.disable_tiling()
        try:
            return hip()
        finally:
            m.enable_tiling()

    forms = {"tiled_batched": lambda: _with_switch("1", hip), "tiled_one_by_one": lambda: _with_switch("0", hip), "untiled": untiled}
    got, res["tiled_batched_peak_gb"] = _peak(forms["tiled_batched"])            # the warm-ups (the first packs the weights)
    one, res["tiled_one_by_one_peak_gb"] = _peak(forms["tiled_one_by_one"])
    res["tile_orders_bit_identical"] = bool(torch.equal(got, one))
    whole, res["untiled_peak_gb"] = _peak(forms["untiled"])
    res["tiled_vs_untiled_rel_l2"] = _rel(got, whole)
    del one, whole
    if not args.no_baseline:
        forms["aten_fp16_tiled"] = aten
        ref, res["aten_fp16_tiled_peak_gb"] = _peak(aten)
        res["hip_vs_aten_fp16_rel_l2"] = _rel(got, ref)
        del ref
    del got
    res.update(_measure(forms, args.rounds))
    with _Seams(ops) as seams:
        _with_switch("1", hip)
    res["seams"] = seams.report()
    res["faster"] = "tiled_batched" if res["tiled_batched_ms"] <= res["tiled_one_by_one_ms"] else "tiled_one_by_one"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--latent-frames", type=int, default=13)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 49])
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--skip-encode", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cogvideox_vae_tiling_bench.json"))
    args = ap.parse_args()

    import cogvideox_vae_encoder_oracle as eo
    import cogvideox_vae_oracle as oc
    import cogvideox_vae_tiling_oracle as to
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import ops

    if not torch.cuda.is_available():
        raise SystemExit("cogvideox_vae_tiling_bench measures on the MI355X: no GPU found")
    cfg = eo.CogVAEConfig()
    torch.manual_seed(0)
    o = eo.AutoencoderKLCogVideoX(cfg)
    with torch.no_grad():
        for n, p in o.named_parameters():
            if n.endswith("conv_y.conv.bias"):
                p.add_(1.0)
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**cfg.__dict__), encoder=True)
    m.load_state_dict(o.state_dict())
    m = m.half().to("cuda")
    o = o.half().to("cuda")
    od = oc.AutoencoderKLCogVideoX(cfg)                         # the decoder oracle's ``decode`` around the same decoder
    od.decoder = o.decoder
    m.enable_tiling()
    tiling = to.Tiling()                                        # 240 x 360, 1/6, 1/5: the real defaults

    def moments(dist):
        return torch.cat([dist.mean.float(), dist.logvar.float()], dim=1)

    def aten_moments(x):
        r = to.tiled_moments(o, x, tiling)
        return torch.cat([r[:, :16].float(), r[:, 16:].float().clamp(-30, 20)], dim=1)

    g = torch.Generator().manual_seed(7)
    z = torch.randn(1, 16, args.latent_frames, 60, 90, generator=g).half().to("cuda")
    runs = [_one("decode", list(z.shape), lambda: m.decode(z).sample, lambda: to.tiled_decode(od, z, tiling), m, ops, args)]
    if not args.skip_encode:
        for f in args.frames:
            x = (0.5 * torch.randn(1, 3, f, 480, 720, generator=g)).clamp(-1, 1).half().to("cuda")
            runs.append(_one("encode", list(x.shape), lambda: moments(m.encode(x).latent_dist), lambda: aten_moments(x), m, ops, args))
    res = dict(tool="cogvideox_vae_tiling_bench", rounds=args.rounds, device=torch.cuda.get_device_name(0),
               tile=[m.tile_sample_min_height, m.tile_sample_min_width],
               default="tiled_one_by_one: a batch entry is not bit-identical to a single run (tile_orders_bit_identical below)", runs=runs)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
