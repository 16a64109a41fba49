#!/usr/bin/env python3
"""Fingerprints of the CogVideoX VAE (lkgd_amd/cogvideox_vae.py) on one MI355X, to show that a change of its host code changed nothing:
per case the SHA-256 of the result's fp16 bytes, the ordered C-ABI launches with their arguments, and the peak allocated memory.

    python tools/cogvideox_vae_fingerprint.py [--out FILE]

One JSON line per case.  The tiny configuration with the oracles' weights and inputs (the shapes of the GPU tests): the untiled decode
and encode, a batch of two, slicing, and the tiled decode and encode at 48 x 80 pixels with ``LKGD_COGVAE_TILE_BATCH`` unset and = 1.
A case runs three times: a warm-up, a pass whose result is hashed and whose peak is read, and a recorded pass (as
``tools/gemm_census.record_launches``) whose launches are listed - ``lkgd_gemm_f16`` by ``gemm_census.signature``, every other entry
point by its integer arguments below 2^31 and its float arguments (device addresses lie above and are left out).  The record holds
that list's SHA-256, its length and the count per entry point - the lists themselves come to megabytes.  Only the public surface of
the module is used, so the same file runs against another commit's tree."""
import argparse
import hashlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

SWITCH = "LKGD_COGVAE_TILE_BATCH"
DEV = "cuda:0"


def _launches(run):
    from gemm_census import signature
    from lkgd_amd import replay
    from lkgd_amd._lib import GemmDesc
    with replay.strict(False):                 # only the launch list is of interest: nothing is replayed
        with replay.record() as p:
            run()
    torch.cuda.synchronize()
    out, by_name = [], {}
    for _, args, name, _ in p.calls:
        if name == "lkgd_gemm_f16":
            out.append([name, signature(GemmDesc.from_buffer_copy(args[0]._obj))])
        else:
            out.append([name, [a for a in args if isinstance(a, float) or (isinstance(a, int) and a < 2 ** 31)]])
        by_name[name] = by_name.get(name, 0) + 1
    p.release()
    # the list of a tiled case runs to hundreds of kilobytes: the record carries its hash, and the counts to start a search from
    return {"sha256": hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest(), "count": len(out), "by_name": by_name}


def fingerprint(name, run, tensors):
    """``run()`` -> the result; ``tensors(result)`` -> the fp16 tensors that are hashed"""
    run()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    r = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    h = hashlib.sha256()
    for t in tensors(r):
        assert t.dtype == torch.float16, t.dtype
        h.update(t.contiguous().cpu().numpy().tobytes())
    del r
    return {"case": name, "sha256": h.hexdigest(), "peak_bytes": peak, "launches": _launches(run)}


def _decoded(r):
    return [r.sample]


def _posterior(r):
    d = r.latent_dist
    return [d.mean, d.logvar, d.sample(torch.Generator().manual_seed(21))]


def cases():
    import cogvideox_vae_encoder_oracle as eo
    import cogvideox_vae_oracle as oc
    import cogvideox_vae_tiling_oracle as to
    from lkgd_amd import cogvideox_vae as pv

    def module(o, cfg, **kw):
        m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**cfg.__dict__), **kw)
        m.load_state_dict(o.state_dict())
        return m.half().to(DEV)

    def both_tile_orders(name, run, tensors):
        for v in (None, "1"):
            os.environ.pop(SWITCH, None)
            if v is not None:
                os.environ[SWITCH] = v
            try:
                yield fingerprint(f"{name} {SWITCH}={v or 'unset'}", run, tensors)
            finally:
                os.environ.pop(SWITCH, None)

    dec = module(oc.tiny_pair_weights(), oc.TINY)
    for B, T in ((1, 1), (1, 2), (1, 3), (1, 5), (2, 5)):
        z = oc.tiny_latents(T, B=B).half().to(DEV)
        yield fingerprint(f"decode B={B} T={T} 6x10", lambda: dec.decode(z), _decoded)
    dec.enable_slicing()
    yield fingerprint("decode B=2 T=5 6x10 sliced", lambda: dec.decode(z), _decoded)
    dec.disable_slicing()
    dec.enable_tiling(48, 80)
    for T, h, w in ((1, 14, 22), (5, 14, 22), (3, 12, 20), (1, 11, 17)):
        z = to.grid_latents(T, h, w).half().to(DEV)
        yield from both_tile_orders(f"tiled decode T={T} {h}x{w}", lambda: dec.decode(z), _decoded)
    del dec

    enc = module(eo.tiny_weights(), eo.TINY, encoder=True)
    for B, T in ((1, 1), (1, 2), (1, 5), (1, 9), (1, 17), (2, 5)):
        x = eo.tiny_clip(T, B=B).half().to(DEV)
        yield fingerprint(f"encode B={B} T={T} 48x80", lambda: enc.encode(x), _posterior)
    enc.enable_slicing()
    enc.enable_tiling(48, 80)
    for T in (1, 9, 17):
        x = to.grid_clip(T, 112, 176).half().to(DEV)
        yield from both_tile_orders(f"tiled encode T={T} 112x176", lambda: enc.encode(x), _posterior)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = [json.dumps(rec, sort_keys=True) for rec in cases()]
    for rec in lines:
        print(rec[:200])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
