#!/usr/bin/env python3
"""CogVideoX-5B-I2V DiT at full size on one MI355X: 42 layers x 3072 channels (48 heads), rotary embeddings + the learned joint
position table, 13 x 60 x 90 latents (17 550 video + 226 text tokens) with CFG (batch 2: 35 552 joint rows).  Random weights,
initialised on the device (there is no checkpoint on a GPU box): the numbers are a forward's cost, and ``finite`` says only that
THIS synthetic forward stayed inside fp16 - the released weights were trained in bf16 while this path is fp16 (as the
reference's own ``--mixed_precision "fp16"`` launchers), and overflow behaviour on the real weights is not measured here.

    python tools/cogvideox5b_bench.py [--forwards 3] [--warmup 1]            one JSON line: ms per forward, TFLOP/s, peak memory
    python tools/cogvideox5b_bench.py --kernel [--rounds 20]                one JSON line: lkgd_qk_norm_rope against the composed
                                                                            form (two lkgd_layernorm + the rotation in torch),
                                                                            alternating in one process, at the full-size rows
    python tools/cogvideox5b_bench.py --kernel-only N                        N launches of the fused kernel and N of lkgd_layernorm
                                                                            on the same rows and nothing else: the run to put
                                                                            under a kernel trace for device-side durations

--layers / --frames shrink the model for a smoke run of the tool itself (marked INVALID in the line).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_TBS = 8.0          # MI355X HBM3E peak, TB/s
MFMA_PEAK_TFLOPS = 2500.0   # dense fp16 MFMA


def _events(fn, n):
    """n calls, each between device events -> list of ms"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def forward_bench(args):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import unet as pu
    dev = torch.device("cuda", 0)
    frames = 4 * (args.frames - 1) + 1
    cfg = pc.DiTConfig(num_attention_heads=48, num_layers=args.layers, in_channels=32, sample_frames=frames,
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
    x = torch.randn(2, f, 32, cfg.sample_height, cfg.sample_width, generator=g, device=dev).half()
    pe = torch.randn(2, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g, device=dev).half()
    dom, flow = torch.randn(1, 1, 1000, generator=g, device=dev), torch.randn(1, 1, 1000, generator=g, device=dev)
    text = m.fused_text(pe, dom, flow)
    rope = tuple(t.to(dev) for t in pc.rotary_tables(m.config, f, h, w))
    out = None

    def one():
        nonlocal out
        out = m.forward_tokens(x, text, 500.0, image_rotary_emb=rope)
    for _ in range(args.warmup):
        one()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = _events(one, args.forwards)
    L = cfg.max_text_seq_length + f * h * w
    D = 3072
    tflop = 2 * cfg.num_layers * (2.0 * L * D * D * 12 + 4.0 * L * L * D) / 1e12      # CFG batch 2: projections + FF, attention
    best = min(ms)
    full = args.layers == 42 and args.frames == 13
    print(json.dumps({
        "metric": "ms per forward of the CogVideoX-5B-I2V DiT (42 x 3072, rotary + learned table, 13x60x90 latents, CFG batch 2)"
                  + ("" if full else " [SHRUNK - INVALID]"),
        "value": round(best, 2), "unit": "ms", "higher_is_better": False, "ms_per_forward_all": [round(v, 2) for v in ms],
        "forwards": args.forwards, "warmup": args.warmup, "layers": cfg.num_layers, "joint_rows": 2 * L,
        "tflop_per_forward": round(tflop, 2), "tflops": round(tflop / (best / 1e3), 1),
        "frac_of_mfma_peak": round(tflop / (best / 1e3) / MFMA_PEAK_TFLOPS, 3),
        "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
        "finite": bool(torch.isfinite(out.float()).all().item()), "dtype": "f16", "data": "synthetic weights and inputs"}), flush=True)


def _kernel_operands(args):
    from lkgd_amd import cogvideox as pc
    dev = torch.device("cuda", 0)
    heads, D = 48, 3072
    f, h, w = args.frames, 30, 45
    Tt, Tv = 226, f * h * w
    L, T = Tt + Tv, 2 * (Tt + Tv)
    g = torch.Generator(device=dev).manual_seed(2)
    q0 = torch.randn(T, D, generator=g, device=dev).half()
    k0 = torch.randn(T, D, generator=g, device=dev).half()
    nq = (1 + 0.1 * torch.randn(64, generator=g, device=dev), 0.1 * torch.randn(64, generator=g, device=dev))
    nk = (1 + 0.1 * torch.randn(64, generator=g, device=dev), 0.1 * torch.randn(64, generator=g, device=dev))
    cfg = pc.DiTConfig(num_attention_heads=48, use_rotary_positional_embeddings=True)
    rope = tuple(t.to(dev) for t in pc.rotary_tables(cfg, f, h, w))
    return heads, D, Tt, Tv, L, T, q0, k0, nq, nk, rope


def kernel_bench(args):
    """the fused kernel against the composed form, alternating in one process; both run in place on their own copies (the norm
    of a normalised row is again a valid input, so repeated launches do the same work)"""
    from lkgd_amd import ops
    heads, D, Tt, Tv, L, T, q0, k0, nq, nk, (cos, sin) = _kernel_operands(args)
    qa, ka, qb, kb = q0.clone(), k0.clone(), q0.clone(), k0.clone()

    def fused():
        ops.qk_norm_rope(qa, ka, heads, nq, nk, 1e-6, (cos, sin), L, Tt)

    def rotate_(x):     # the reference's apply_rotary_emb on the video rows of [T, heads * 64], in place
        v = x.view(2, L, heads, 64)[:, Tt:]
        real, imag = v.reshape(2, Tv, heads, 32, 2).unbind(-1)
        rot = torch.stack([-imag, real], dim=-1).flatten(3)
        v.copy_((v.float() * cos[None, :, None, :] + rot.float() * sin[None, :, None, :]).half())

    def composed():
        for x, (ga, be) in ((qb, nq), (kb, nk)):
            ops.layernorm(x.view(T * heads, 64), ga, be, 1e-6, out=x.view(T * heads, 64))
            rotate_(x)

    def norms():
        for x, (ga, be) in ((qb, nq), (kb, nk)):
            ops.layernorm(x.view(T * heads, 64), ga, be, 1e-6, out=x.view(T * heads, 64))
    # same results first (the composition is the kernel's definition)
    fused(), composed()
    same = bool(torch.equal(qa, qb) and torch.equal(ka, kb))
    tf, tc, tn = [], [], []
    for _ in range(args.rounds):
        tf += _events(fused, 1)
        tc += _events(composed, 1)
        tn += _events(norms, 1)
    nbytes = 4 * T * D * 2 + 2 * Tv * 64 * 4          # q and k read + written, the two tables once
    med = lambda v: sorted(v)[len(v) // 2]            # noqa: E731
    print(json.dumps({
        "metric": "lkgd_qk_norm_rope vs two lkgd_layernorm + torch rotation, 5B-I2V rows, alternating in one process, device events",
        "rows": T, "channels": D, "rounds": args.rounds, "bitwise_equal": same,
        "fused_ms_median": round(med(tf), 3), "fused_ms_min": round(min(tf), 3),
        "composed_ms_median": round(med(tc), 3), "composed_ms_min": round(min(tc), 3),
        "two_layernorms_ms_median": round(med(tn), 3), "two_layernorms_ms_min": round(min(tn), 3),
        "fused_bytes": nbytes, "fused_tb_per_s_from_events": round(nbytes / (med(tf) / 1e3) / 1e12, 3),
        "fused_frac_of_hbm_peak_from_events": round(nbytes / (med(tf) / 1e3) / 1e12 / HBM_PEAK_TBS, 3),
        "two_layernorms_tb_per_s_from_events": round(4 * T * D * 2 / (med(tn) / 1e3) / 1e12, 3),
        "speedup_vs_composed": round(med(tc) / med(tf), 2)}), flush=True)


def kernel_only(args):
    from lkgd_amd import ops
    heads, D, Tt, Tv, L, T, q, k, nq, nk, rope = _kernel_operands(args)
    for _ in range(args.kernel_only):
        ops.qk_norm_rope(q, k, heads, nq, nk, 1e-6, rope, L, Tt)
    for _ in range(args.kernel_only):
        ops.layernorm(q.view(T * heads, 64), nq[0], nq[1], 1e-6, out=q.view(T * heads, 64))
        ops.layernorm(k.view(T * heads, 64), nk[0], nk[1], 1e-6, out=k.view(T * heads, 64))
    torch.cuda.synchronize()
    print(json.dumps({"launches_each": args.kernel_only, "rows": T, "channels": D,
                      "fused_bytes_per_launch": 4 * T * D * 2 + 2 * Tv * 64 * 4, "layernorm_bytes_per_launch": 2 * T * D * 2}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--forwards", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--layers", type=int, default=42)
    ap.add_argument("--frames", type=int, default=13, help="latent frames")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--kernel-only", type=int, default=0)
    args = ap.parse_args()
    if args.forwards < 3 and args.layers == 42:
        ap.error("--forwards: at least 3 timed forwards")
    if args.kernel_only:
        return kernel_only(args)
    return kernel_bench(args) if args.kernel else forward_bench(args)


if __name__ == "__main__":
    main()
