#!/usr/bin/env python3
"""The FP8 block linears (include/lkgd_hip_fp8.h) against the fp16 GEMM they stand beside, on one MI355X, at the shapes of the 2B
and the 5B DiT clip: M = 35 552 rows (2 x (226 + 17 550)), (N, K) = (1920, 1920), (7680, 1920), (1920, 7680), (3072, 3072),
(12288, 3072), (3072, 12288).

    python tools/cogvideox_fp8_bench.py [--rounds 20] [--warmup 3] [--rows 35552]
        one JSON line.  Per shape, checked first (the FP8 linear against the fp16 GEMM's output, relative L2), then medians over
        ``rounds`` alternations in one process of
          * lkgd_gemm_f16;
          * the quantiser that feeds this linear in ``forward_rows`` + lkgd_gemm_fp8:
              N == 4 K (ff.0)      lkgd_layernorm_quant_fp8   (one launch also feeds q, k, v at N == K; it replaces lkgd_layernorm)
              K == 4 N (ff.2)      lkgd_gelu_tanh_quant_fp8   (replaces lkgd_gelu_tanh)
              N == K   (attn out)  lkgd_quant_rows_fp8        (an extra pass: the fp16 path has no kernel here)
          * lkgd_gemm_fp8 alone, with its TFLOP/s and its share of the 5 PFLOP/s dense FP8 peak;
          * the fp16 kernel the fused quantiser replaces (lkgd_layernorm / lkgd_gelu_tanh), so that both columns can be read with
            their producer: [producer + fp16 GEMM] against [quantiser + FP8 GEMM].
    python tools/cogvideox_fp8_bench.py --kernel-only N
        N launches of each FP8 kernel at the 2B shapes and nothing else: the run to put under a kernel trace.

Random operands (zero-filled ones read high); times are wall-clock between device events around each form.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1920, 1920), (7680, 1920), (1920, 7680), (3072, 3072), (12288, 3072), (3072, 12288)]
FP8_PEAK_TFLOPS = 5000.0


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def _operands(M, N, K, dev):
    from lkgd_amd import fp8
    g = torch.Generator().manual_seed(N * 7 + K)
    x = torch.randn(M, K, generator=g).half().to(dev)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half().to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    wq, ws = fp8.quantize_weight(w)
    return x, w, bias, wq, ws


def _forms(M, N, K, dev):
    """(name of the quantiser, fp16 producer or None, quantiser, fp16 GEMM, FP8 GEMM, check) as closures over one set of buffers"""
    from lkgd_amd import ops
    from lkgd_amd._lib import check
    x, w, bias, wq, ws = _operands(M, N, K, dev)
    out16 = torch.empty(M, N, dtype=torch.float16, device=dev)
    out8 = torch.empty_like(out16)
    q = torch.empty(M, K, dtype=torch.uint8, device=dev)
    s = torch.empty(M, dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    if N == 4 * K:
        gamma, beta = torch.ones(K, device=dev), torch.zeros(K, device=dev)
        name = "lkgd_layernorm_quant_fp8"

        def quant():
            ops.layernorm_quant_fp8(x, gamma, beta, 1e-5, q=q, scale=s)

        def producer():
            ops.layernorm(x, gamma, beta, 1e-5, out=y)
    elif K == 4 * N:
        name = "lkgd_gelu_tanh_quant_fp8"

        def quant():
            ops.gelu_tanh_quant_fp8(x, q=q, scale=s)

        def producer():
            check(ops._L().lkgd_gelu_tanh(x.data_ptr(), y.data_ptr(), x.numel(), ops._stream()), "lkgd_gelu_tanh")
    else:
        name, producer = "lkgd_quant_rows_fp8", None

        def quant():
            ops.quant_rows_fp8(x, q=q, scale=s)

    def gemm16():
        ops.gemm(y if producer is not None else x, w, out16, M=M, N=N, K=K, bias=bias)

    def gemm8():
        ops.gemm_fp8(q, s, wq, ws, bias, out=out8)

    def verify():
        if producer is not None:
            producer()
        gemm16()
        quant()
        gemm8()
        torch.cuda.synchronize()
        a, b = out8.float(), out16.float()
        return ((a - b).norm() / b.norm()).item()
    return name, producer, quant, gemm16, gemm8, verify


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="alternations of the forms (>= 20 for a reported median)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int, default=35552)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M = args.rows
    if args.kernel_only:
        for N, K in SHAPES[:3]:
            _, _, quant, _, gemm8, _ = _forms(M, N, K, dev)
            for _ in range(args.kernel_only):
                quant()
                gemm8()
            torch.cuda.synchronize()
        print(json.dumps({"kernel_only": args.kernel_only, "rows": M, "shapes": SHAPES[:3]}))
        return
    med = statistics.median
    shapes, ok = [], True
    for N, K in SHAPES:
        name, producer, quant, gemm16, gemm8, verify = _forms(M, N, K, dev)
        rel = verify()
        t16, t8, tq, tp = [], [], [], []
        for i in range(args.warmup + args.rounds):
            a, b, c = _timed(gemm16), _timed(gemm8), _timed(quant)
            d = _timed(producer) if producer is not None else 0.0
            if i >= args.warmup:
                t16.append(a); t8.append(b); tq.append(c); tp.append(d)
        flop = 2.0 * M * N * K
        g16, g8, gq, gp = med(t16), med(t8), med(tq), med(tp)
        ok = ok and rel < 5e-2
        shapes.append({"N": N, "K": K, "rel_l2_fp8_vs_fp16": float(f"{rel:.3e}"), "quantiser": name,
                       "gemm_f16_us": round(g16, 1), "gemm_f16_us_min_max": [round(min(t16), 1), round(max(t16), 1)],
                       "gemm_fp8_us": round(g8, 1), "gemm_fp8_us_min_max": [round(min(t8), 1), round(max(t8), 1)],
                       "quantiser_us": round(gq, 1), "fp16_producer_us": round(gp, 1) if producer is not None else None,
                       "gemm_f16_tflops": round(flop / g16 * 1e-6, 1), "gemm_fp8_tflops": round(flop / g8 * 1e-6, 1),
                       "gemm_fp8_share_of_fp8_peak": round(flop / g8 * 1e-6 / FP8_PEAK_TFLOPS, 3),
                       "quantiser_plus_fp8_us": round(gq + g8, 1),
                       "faster_than_gemm_f16": gq + g8 < g16,
                       "producer_plus_f16_us": round(gp + g16, 1),
                       "faster_than_producer_plus_f16": gq + g8 < gp + g16})
        del name, producer, quant, gemm16, gemm8, verify
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "cogvideox_fp8_bench", "rows": M, "rounds": args.rounds, "warmup": args.warmup, "shapes": shapes,
                      "valid": args.rounds >= 20 and ok}), flush=True)


if __name__ == "__main__":
    main()
