#!/usr/bin/env python3
"""LoRA adapters on the CogVideoX-5B-I2V DiT at full size on one MI355X (42 layers x 3072 channels, 13 x 60 x 90 latents, CFG batch 2):
what folding the adapters costs when the model packs, and that a step costs what it costs without them.  Random weights and random
adapters (rank 128, the trainer's default, and rank 256) on the four attention projections of every block, initialised on the device.

    python tools/cogvideox_lora_bench.py [--forwards 3] [--warmup 1] [--packs 3] [--out profiles/cogvideox_lora_bench.json]
        one JSON line, also written to --out:
          * ms of ``prepare()`` without adapters, and with them per rank (the fold: one fp32 [3072, r] x [r, 3072] product per wrapped
            linear, added to the fp32 weight, rounded once to fp16) - median and all of ``--packs`` packs, each after ``invalidate()``;
          * ms per ``forward_rows`` without and with adapters (min and all of ``--forwards`` calls between device events), and whether
            the two outputs of the same inputs differ (they must: the adapters are not zero);
          * peak device memory of a pack above what was allocated before it (median and all; the process's first fold also
            initialises the fp32 GEMM library, which shows in that pack's time and peak).

--layers / --frames shrink the model for a smoke run of the tool itself (marked INVALID in the line).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RANKS = (128, 256)
TARGETS = ("to_q", "to_k", "to_v", "to_out.0")


def _events(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _packs(m, n):
    """n packs, each after ``invalidate()`` -> (ms of each by the host clock around a synchronised ``prepare()``, each pack's peak
    bytes above the allocation before it)"""
    ms, peak = [], []
    for _ in range(n):
        m.invalidate()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        m.prepare()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        peak.append(torch.cuda.max_memory_allocated() - before)
    return ms, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forwards", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--packs", type=int, default=3)
    ap.add_argument("--layers", type=int, default=42)
    ap.add_argument("--frames", type=int, default=13, help="latent frames")
    ap.add_argument("--out", default=os.path.join("profiles", "cogvideox_lora_bench.json"))
    args = ap.parse_args()
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import lora
    from lkgd_amd import unet as pu
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = pc.DiTConfig(num_attention_heads=48, num_layers=args.layers, in_channels=32, sample_frames=4 * (args.frames - 1) + 1,
                       use_rotary_positional_embeddings=True, use_learned_positional_embeddings=True)
    with torch.device("meta"):
        m = pc.CogVideoXTransformer3DModel(cfg)
    m = m.to(torch.float16).to_empty(device=dev)
    pu.init_synthetic_weights_(m, seed=0)
    g = torch.Generator(device=dev).manual_seed(1)
    with torch.no_grad():
        for n, p in m.named_parameters():      # adaLN modulation / gates small, as in a trained model's range
            if ".linear." in n and ("norm1" in n or "norm2" in n or "norm_out" in n):
                p.mul_(0.1)
        m.patch_embed.pos_embedding.copy_(0.02 * torch.randn(m.patch_embed.pos_embedding.shape, generator=g, device=dev))
    f, h, w = args.frames, cfg.sample_height // 2, cfg.sample_width // 2
    x = torch.randn(1, f, 32, cfg.sample_height, cfg.sample_width, generator=g, device=dev).half()
    rows = x.permute(0, 1, 3, 4, 2).reshape(1, f, 1, h, 2, w, 2, 32).permute(0, 1, 3, 5, 7, 2, 4, 6).flatten(4, 7).flatten(1, 3) \
        .reshape(f * h * w, 32 * 4).contiguous()                    # one copy of the patch rows serves both CFG entries
    pe = torch.randn(2, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g, device=dev).half()
    dom, flow = torch.randn(1, 1, 1000, generator=g, device=dev), torch.randn(1, 1, 1000, generator=g, device=dev)
    rope = tuple(t.to(dev) for t in pc.rotary_tables(m.config, f, h, w))
    out = None

    def one():
        nonlocal out
        out = m.forward_rows(rows, (f, h, w), text, 500.0, image_rotary_emb=rope)

    def measure():
        nonlocal text
        pack_ms, pack_peak = _packs(m, args.packs)
        text = m.fused_text(pe, dom, flow)
        for _ in range(args.warmup):
            one()
        torch.cuda.synchronize()
        ms = _events(one, args.forwards)
        return {"prepare_ms": round(statistics.median(pack_ms), 1), "prepare_ms_all": [round(v, 1) for v in pack_ms],
                "pack_peak_memory_gb": round(statistics.median(pack_peak) / 2 ** 30, 3),
                "pack_peak_memory_gb_all": [round(v / 2 ** 30, 3) for v in pack_peak], "forward_rows_ms": round(min(ms), 2),
                "forward_rows_ms_all": [round(v, 2) for v in ms], "finite": bool(torch.isfinite(out.float()).all().item())}

    text = None
    res = {"no_adapters": measure()}
    base_out = out.clone()
    for r in RANKS:
        name = f"r{r}"
        wrapped = lora.add_adapter(m, name, r=r, lora_alpha=r, target_modules=TARGETS, init_lora_weights=False)
        with torch.no_grad():
            for _, lin in lora.lora_layers(m):
                a, b = lin.lora_A[name].weight, lin.lora_B[name].weight
                a.copy_(torch.randn(a.shape, generator=g, device=dev) / a.shape[1] ** 0.5)
                b.copy_(0.02 * torch.randn(b.shape, generator=g, device=dev))
        m.set_adapters([name], [0.5])
        res[name] = dict(measure(), rank=r, wrapped_linears=len(wrapped), adapter_parameters=sum(
            lin.lora_A[name].weight.numel() + lin.lora_B[name].weight.numel() for _, lin in lora.lora_layers(m)),
            output_differs_from_no_adapters=not torch.equal(out, base_out))
        m.unload_lora()
    full = args.layers == 42 and args.frames == 13
    line = {"tool": "cogvideox_lora_bench",
            "metric": "prepare() and forward_rows of the CogVideoX-5B-I2V DiT (42 x 3072, 13x60x90 latents, CFG batch 2) without and "
                      "with LoRA adapters on the four attention projections" + ("" if full else " [SHRUNK - INVALID]"),
            "layers": cfg.num_layers, "latent_frames": f, "joint_rows": 2 * (cfg.max_text_seq_length + f * h * w), "forwards": args.forwards,
            "warmup": args.warmup, "packs": args.packs, "dtype": "f16", "data": "synthetic weights, adapters and inputs", **res,
            "valid": full}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(line, indent=1) + "\n")


if __name__ == "__main__":
    main()
