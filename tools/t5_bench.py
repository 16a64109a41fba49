#!/usr/bin/env python3
"""One prompt encode of the T5 text encoder (lkgd_amd/t5.py) at the geometry of CogVideoX's ``text_encoder/`` on one MI355X:
24 layers, d_model 4096, 64 heads of 64, d_ff 10240, ids [2, 226] (the prompt and the negative prompt of one clip).

    python tools/t5_bench.py [--rounds 20] [--warmup 3] [--layers 24] [--out profiles/t5_bench.json]

Weights are random and generated on the device (the released checkpoint is not needed); the ids are random.  Reported: milliseconds per
encode on the HIP path and, where transformers imports, of its own fp16 ``T5EncoderModel`` holding the same weights on the same GPU -
medians over ``rounds`` alternations in one process after ``warmup`` untimed ones, between device events - and the relative L2 distance
of each of the two outputs from transformers' fp32 forward of the same weights on that GPU (the yardstick both fp16 forms are read
against; ``--layers`` shows how the distances grow with depth).  The algorithmic FLOP of the encode (linears and attention) over the HIP
time is an end-to-end rate, not a kernel's share of peak.  There is no gate: the encoder runs once per clip.  One JSON line on stdout,
the same object in ``--out``.
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

B, S = 2, 226


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)                 # ms


def _random_weights_(model, dev, seed=0):
    """every parameter drawn on the device with the deviations of transformers' own T5 initialisation - linears fan_in ** -0.5, ``q``
    another d_kv ** -0.5 smaller (T5 does not scale its scores, so its ``q`` carries the factor) - norm weights near one, and the
    bias table with deviation 2.  Random weights of unit-size ``q`` make 24 layers of near-one-hot attention, which amplifies any
    rounding difference between two forwards beyond use as a comparison"""
    d_kv = model.config.d_kv
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("layer_norm.weight"):
                p.copy_(0.7 + 0.6 * torch.rand(p.shape, generator=g, device=dev))
            elif "relative_attention_bias" in n:
                p.copy_(2.0 * torch.randn(p.shape, generator=g, device=dev))
            elif n in ("shared.weight", "encoder.embed_tokens.weight"):
                p.copy_(torch.randn(p.shape, generator=g, device=dev))
            else:
                std = p.shape[1] ** -0.5 * (d_kv ** -0.5 if n.endswith("SelfAttention.q.weight") else 1.0)
                p.copy_(torch.randn(p.shape, generator=g, device=dev) * std)


def _transformers_twin(ours, cfg, dev, dtype=torch.float16):
    """transformers' module in ``dtype`` with ``ours``' weights on ``dev``, or (None, reason)"""
    try:
        import transformers
    except Exception as e:                   # not installed, or its import fails on this box: the HIP number stands alone
        return None, f"{type(e).__name__}: {e}"
    c = transformers.T5Config(feed_forward_proj="gated-gelu", **{k: v for k, v in cfg.__dict__.items() if k != "feed_forward_proj"})
    with torch.device("meta"):
        hf = transformers.T5EncoderModel(c)
    hf = hf.to(dtype).to_empty(device=dev).eval()
    hf.load_state_dict(ours.state_dict(), strict=True)            # (copies: the fp16 values, whatever ``dtype`` holds them)
    return hf, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="alternations of the two forms (>= 20 for a reported median)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=24, help="depth (24 = the released encoder; fewer: how the distances below grow)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "t5_bench.json"))
    args = ap.parse_args()
    from lkgd_amd import t5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = t5.T5Config(num_layers=args.layers)
    with torch.device("meta"):
        ours = t5.T5EncoderModel(cfg)
    ours = ours.to(torch.float16).to_empty(device=dev)
    _random_weights_(ours, dev)
    ours.invalidate()
    ids = torch.randint(2, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(1))
    ids_dev = ids.to(dev)
    hf, why_not = _transformers_twin(ours, cfg, dev)

    def hip():
        return ours(ids)[0]

    def theirs():
        with torch.no_grad():
            return hf(input_ids=ids_dev)[0]
    out = hip()
    torch.cuda.synchronize()
    res = {"tool": "t5_bench", "geometry": cfg.__dict__, "ids": [B, S], "rounds": args.rounds, "warmup": args.warmup,
           "finite": bool(torch.isfinite(out.float()).all())}
    if hf is not None:
        # the yardstick: transformers' fp32 forward of the same weights on this GPU (ATen's fp32 GEMMs; the checker, not the product)
        hf32, _ = _transformers_twin(ours, cfg, dev, torch.float32)
        with torch.no_grad():
            ref32 = hf32(input_ids=ids_dev)[0]
        del hf32
        torch.cuda.empty_cache()
        ref = theirs()

        def rel(a):
            return float(f"{float((a.float() - ref32).norm() / ref32.norm()):.3e}")
        res["hip_rel_l2_vs_transformers_fp32"] = rel(out)
        res["transformers_fp16_rel_l2_vs_transformers_fp32"] = rel(ref)
        res["transformers_fp16_finite"] = bool(torch.isfinite(ref.float()).all())
    else:
        res["transformers"] = f"not measured ({why_not})"
    t_hip, t_hf = [], []
    for i in range(args.warmup + args.rounds):
        a = _timed(hip)
        b = _timed(theirs) if hf is not None else None
        if i >= args.warmup:
            t_hip.append(a)
            if b is not None:
                t_hf.append(b)
    T, D, inner, F_ = B * S, cfg.d_model, cfg.num_heads * cfg.d_kv, cfg.d_ff
    flop = cfg.num_layers * (2.0 * T * D * (4 * inner + 3 * F_) + 4.0 * B * cfg.num_heads * S * S * cfg.d_kv)
    med = statistics.median(t_hip)
    res.update({"hip_ms": round(med, 3), "hip_ms_min_max": [round(min(t_hip), 3), round(max(t_hip), 3)],
                "algorithmic_tflop": round(flop * 1e-12, 3), "hip_end_to_end_tflops": round(flop / med * 1e-9, 1)})
    if t_hf:
        res.update({"transformers_fp16_ms": round(statistics.median(t_hf), 3),
                    "transformers_fp16_ms_min_max": [round(min(t_hf), 3), round(max(t_hf), 3)]})
    res["valid"] = args.rounds >= 20 and res["finite"]
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
