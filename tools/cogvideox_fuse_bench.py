#!/usr/bin/env python3
"""The CogVideoX loop kernels (include/lkgd_hip_dit_loop.h) against the ATen sequences they replaced, on one MI355X.

    python tools/cogvideox_fuse_bench.py [--rounds 20] [--warmup 3]     one JSON line: medians, in one process with the two forms
                                                                         alternating, of
        * the fused text at B = 2, L = 226: one launch of lkgd_lk_fuse_tokens against the ATen chain (interpolate, grouped-conv
          sums, matmuls, rfft / irfft, abs / angle - rocFFT + hipBLASLt).  The chain lives in THIS tool only;
        * the per-step glue at the 2B-I2V and 5B-I2V geometries (13 x 60 x 90 latents, C = 16; both have 32 input channels, so
          the glue is the same work - the line says so instead of timing it twice): lkgd_dit_patch_rows +
          lkgd_dit_cfg_ddim_step against cat / cat / permute-copy, permute-copy / float / chunk / CFG / DDIM / half.
    python tools/cogvideox_fuse_bench.py --v15 [--rounds 20] [--warmup 3]   one JSON line: the per-step glue of the 1.5 I2V loop
                                                                         (include/lkgd_hip_dit_tpatch.h) at its geometry, 22 latent
                                                                         frames x 96 x 170, C = 16 (+ 16 image channels), p_t = 2:
                                                                         lkgd_dit_patch_rows_t + lkgd_dit_cfg_ddim_step_t against
                                                                         cat / cat / permute-copy / permute-copy / float / CFG / DDIM /
                                                                         half, alternating in one process; checks both bit for bit first
    python tools/cogvideox_fuse_bench.py --kernel-only N                 N launches of the fuse and of the two glue kernels and
                                                                         nothing else: the run to put under a kernel trace
                                                                         (rocprofv3 --kernel-trace --stats -- python tools/...)

Random weights (there is no checkpoint on a GPU box); times are wall-clock between device events around each form.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3          # us


def aten_fused_text(m, encoder_hidden_states, domain_features, flow_features):
    """``fused_text`` as it was before lkgd_lk_fuse_tokens (cogvideox_transformer_3d.py:519-582 in torch ops)"""
    from lkgd_amd.lk_fuse import hamilton
    dev = m.device
    e = encoder_hidden_states.to(device=dev, dtype=torch.float32)

    def dw(conv, x, per):
        w = conv.weight.detach().float().reshape(256, per)
        return (x.reshape(*x.shape[:-1], 256, per) * w).sum(-1)

    def qlin(q, x):
        return x @ hamilton(q) + q.bias.detach().float()
    low = dw(m.quaternion_lora_lconv, e, 16)
    d = F.interpolate(domain_features.to(device=dev, dtype=torch.float32), size=1024, mode="linear")
    f = F.interpolate(flow_features.to(device=dev, dtype=torch.float32), size=1024, mode="linear")
    low_d = dw(m.quaternion_lora_dconv, d, 4).expand_as(low)
    low_f = dw(m.quaternion_lora_fconv, f, 4).expand_as(low)
    ctx = m.quaternion_lora_texts.detach().float().expand_as(low)
    spatial = qlin(m.quaternion_lora_fuse, torch.cat([low, low_d, low_f, ctx], -1))
    hf, df, ff = (torch.fft.rfft(t.contiguous(), dim=-1) for t in (low, low_d, low_f))
    mags = [hf.abs(), df.abs(), ff.abs(), m.quaternion_lora_texts_fft_mag.detach().float().expand_as(hf.real)]
    phas = [hf.angle(), df.angle(), ff.angle(), m.quaternion_lora_texts_fft_pha.detach().float().expand_as(hf.real)]
    mag = qlin(m.quaternion_lora_fuse_fft_mag, torch.cat([x[..., :-1] for x in mags], -1))
    pha = qlin(m.quaternion_lora_fuse_fft_pha, torch.cat([x[..., :-1] for x in phas], -1))
    l0m, l0p = m.quaternion_lora_fuse_fft_mag0, m.quaternion_lora_fuse_fft_pha0
    mag0 = torch.cat([x[..., -1:] for x in mags], -1) @ l0m.weight.detach().float().T + l0m.bias.detach().float()
    pha0 = torch.cat([x[..., -1:] for x in phas], -1) @ l0p.weight.detach().float().T + l0p.bias.detach().float()
    spec = torch.cat([torch.complex(mag * torch.cos(pha), mag * torch.sin(pha)),
                      torch.complex(mag0 * torch.cos(pha0), mag0 * torch.sin(pha0))], -1)
    freq = torch.fft.irfft(spec, dim=-1)
    sf = m.quaternion_lora_fuse_sf
    x = torch.cat([spatial, freq], -1)
    x = F.leaky_relu(x @ sf[0].weight.detach().float().T + sf[0].bias.detach().float(), 0.1)
    x = x @ sf[2].weight.detach().float().T + sf[2].bias.detach().float()
    return x.to(torch.float16)


def _model(dev):
    """the LK modules only matter here: a 1-layer DiT with the 2B width"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import unet as pu
    with torch.device("meta"):
        m = pc.CogVideoXTransformer3DModel(pc.DiTConfig(in_channels=32, num_layers=1))
    m = m.to(torch.float16).to_empty(device=dev)
    pu.init_synthetic_weights_(m, seed=0)
    return m


def _glue_operands(dev, C_=16, F_=13, H=60, W=90):
    g = torch.Generator().manual_seed(1)
    lat = torch.randn(1, F_, C_, H, W, generator=g).half().to(dev)
    img = (0.5 * torch.randn(1, F_, C_, H, W, generator=g)).half().to(dev)
    noise_rows = torch.randn(2 * F_ * (H // 2) * (W // 2), C_ * 4, generator=g).half().to(dev)
    return lat, img, noise_rows


def _aten_glue(lat, img2, noise_rows, g, coef, p=2):
    """the per-step glue before the kernels: CFG duplicate, channel concat, patch unfold; un-patchify, .float(), CFG, DDIM, .half()"""
    B, F_, C_, H, W = lat.shape
    h, w = H // p, W // p
    x = torch.cat([lat] * 2)
    x = torch.cat([x, img2], dim=2)
    patches = x.reshape(2 * B, F_, 2 * C_, h, p, w, p).permute(0, 1, 3, 5, 2, 4, 6).reshape(2 * B * F_ * h * w, 2 * C_ * p * p).contiguous()
    noise = noise_rows.reshape(2 * B, F_, h, w, -1, p, p).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4).contiguous().float()
    u, c = noise.chunk(2)
    noise = u + g * (c - u)
    a, b, sa, sb = coef
    s = lat.float()
    x0 = sa * s - sb * noise
    return patches, (a * s + b * x0).to(torch.float16)


def _aten_glue_t(lat, img2, noise_rows, g, coef, p=2, pt=2):
    """the per-step glue of a patch_size_t model without the kernels: CFG duplicate, channel concat, the 3-D patch unfold; the 3-D
    un-patchify (cogvideox_transformer_3d.py:626-630), .float(), CFG, DDIM, .half()"""
    B, F_, C_, H, W = lat.shape
    h, w = H // p, W // p
    x = torch.cat([lat] * 2)
    x = torch.cat([x, img2], dim=2)
    patches = x.permute(0, 1, 3, 4, 2).reshape(2 * B, F_ // pt, pt, h, p, w, p, 2 * C_).permute(0, 1, 3, 5, 7, 2, 4, 6) \
        .flatten(4, 7).flatten(1, 3).contiguous()
    noise = noise_rows.reshape(2 * B, F_ // pt, h, w, -1, pt, p, p).permute(0, 1, 5, 4, 2, 6, 3, 7).flatten(6, 7).flatten(4, 5) \
        .flatten(1, 2).contiguous().float()
    u, c = noise.chunk(2)
    noise = u + g * (c - u)
    a, b, sa, sb = coef
    s = lat.float()
    x0 = sa * s - sb * noise
    return patches, (a * s + b * x0).to(torch.float16)


def main_v15(args):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F_, H, W, C_ = 22, 96, 170, 16
    g = torch.Generator().manual_seed(1)
    lat = torch.randn(1, F_, C_, H, W, generator=g).half().to(dev)
    img = (0.5 * torch.randn(1, F_, C_, H, W, generator=g)).half().to(dev)
    noise_rows = torch.randn(2 * (F_ // 2) * (H // 2) * (W // 2), C_ * 8, generator=g).half().to(dev)
    img2 = torch.cat([img] * 2)
    sched = pc.CogVideoXDDIMScheduler()
    sched.set_timesteps(50)
    t = sched.timesteps.tolist()[10]
    gd, coef = pc.dynamic_guidance(6.0, 50, t), sched.coefficients(t)
    rows = ops.dit_patch_rows(lat, img, p_t=2)
    work = lat.clone()
    ref_rows, ref_lat = _aten_glue_t(lat, img2, noise_rows, gd, coef)
    ops.dit_cfg_ddim_step(noise_rows, work, 2, 2, gd, *coef, p_t=2)
    # one copy of the rows serves both CFG entries: the ATen form holds them twice
    same = bool(torch.equal(rows, ref_rows[0]) and torch.equal(rows, ref_rows[1]) and torch.equal(work, ref_lat))

    def hip_glue():
        ops.dit_patch_rows(lat, img, out=rows, p_t=2)
        ops.dit_cfg_ddim_step(noise_rows, work, 2, 2, gd, *coef, p_t=2)
    g_hip, g_aten = [], []
    for i in range(args.warmup + args.rounds):
        c = _timed(hip_glue)
        d = _timed(lambda: _aten_glue_t(lat, img2, noise_rows, gd, coef))
        if i >= args.warmup:
            g_hip.append(c); g_aten.append(d)
    med = statistics.median
    print(json.dumps({"tool": "cogvideox_fuse_bench --v15", "rounds": args.rounds, "warmup": args.warmup,
                      "step_glue_t": {"geometry": "22 x 96 x 170 latents, C = 16 (+ 16 image channels), p_t = 2: the 1.5 I2V loop",
                                      "bitwise_equal_to_aten": same,
                                      "two_launches_us_median": round(med(g_hip), 1), "aten_sequence_us_median": round(med(g_aten), 1),
                                      "two_launches_us_min": round(min(g_hip), 1), "aten_sequence_us_min": round(min(g_aten), 1),
                                      "not_slower": med(g_hip) <= med(g_aten)},
                      "valid": args.rounds >= 20 and same}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20, help="alternations of the two forms (>= 20 for a reported median)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", type=int, default=0, metavar="N")
    ap.add_argument("--v15", action="store_true", help="the _t glue pair at the 1.5 I2V geometry instead")
    args = ap.parse_args()
    if args.v15:
        return main_v15(args)
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    m = _model(dev)
    g = torch.Generator().manual_seed(2)
    B, L = 2, 226
    pe = torch.randn(B, L, 4096, generator=g).half().to(dev)
    dom, flow = (3 * torch.randn(1, 1, 1000, generator=g)).to(dev), (3 * torch.randn(1, 1, 1000, generator=g)).to(dev)
    lat, img, noise_rows = _glue_operands(dev)
    img2 = torch.cat([img] * 2)
    sched = pc.CogVideoXDDIMScheduler()
    sched.set_timesteps(50)
    t = sched.timesteps.tolist()[10]
    gd, coef = pc.dynamic_guidance(6.0, 50, t), sched.coefficients(t)
    rows = ops.dit_patch_rows(lat, img)
    work = lat.clone()

    def hip_glue():
        ops.dit_patch_rows(lat, img, out=rows)
        ops.dit_cfg_ddim_step(noise_rows, work, 2, 2, gd, *coef)

    if args.kernel_only:
        with torch.no_grad():
            for _ in range(args.kernel_only):
                m.fused_text(pe, dom, flow)
                hip_glue()
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": args.kernel_only, "B": B, "L": L, "rows_per_workgroup": 8, "grid": B * ((L + 7) // 8),
                          "threads": 512}))
        return
    with torch.no_grad():
        ref = aten_fused_text(m, pe, dom, flow)
        got = m.fused_text(pe, dom, flow)
        rel = ((got.float() - ref.float()).norm() / ref.float().norm()).item()
        t_hip, t_aten, g_hip, g_aten = [], [], [], []
        for i in range(args.warmup + args.rounds):
            a = _timed(lambda: m.fused_text(pe, dom, flow))
            b = _timed(lambda: aten_fused_text(m, pe, dom, flow))
            c = _timed(hip_glue)
            d = _timed(lambda: _aten_glue(lat, img2, noise_rows, gd, coef))
            if i >= args.warmup:
                t_hip.append(a); t_aten.append(b); g_hip.append(c); g_aten.append(d)
    med = statistics.median
    line = {"tool": "cogvideox_fuse_bench", "rounds": args.rounds, "warmup": args.warmup,
            "fused_text": {"B": B, "L": L, "rows_per_workgroup": 8, "grid": B * ((L + 7) // 8), "threads": 512,
                           "launch_us_median": round(med(t_hip), 1), "aten_chain_us_median": round(med(t_aten), 1),
                           "launch_us_min": round(min(t_hip), 1), "aten_chain_us_min": round(min(t_aten), 1),
                           "rel_l2_vs_aten": float(f"{rel:.3e}"), "not_slower": med(t_hip) <= med(t_aten)},
            "step_glue": {"geometry": "13 x 60 x 90 latents, C = 16 (+ 16 image channels): the 2B-I2V and the 5B-I2V loop alike",
                          "two_launches_us_median": round(med(g_hip), 1), "aten_sequence_us_median": round(med(g_aten), 1),
                          "two_launches_us_min": round(min(g_hip), 1), "aten_sequence_us_min": round(min(g_aten), 1),
                          "not_slower": med(g_hip) <= med(g_aten)},
            "valid": args.rounds >= 20}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
