"""What the CogVideoX DPM-Solver++ tests share (test_cogvideox_dpm_*.py), independent of lkgd_amd: the coefficient formulas of
DESIGN.md section 15 ([EXT] diffusers scheduling_dpm_cogvideox.py, PARITY UNPINNED) once more in Python floats (= fp64) with the
infinite cases written out as limits instead of left to IEEE arithmetic, the step in fp64, and ``aten_dpm_step``: the torch
statements ``lkgd_dit_cfg_dpm_step`` replaces, one torch op per operation, with the four decoys of the GPU file."""
import math
from collections import namedtuple

import torch

from cogvideox_support import unpatchify

Coef = namedtuple("Coef", "sqrt_alpha sqrt_beta m1 m2 m3 m4 mn order")
INF = float("inf")
DECOYS = ("first_order", "m3_m4_swapped", "eps_dropped", "x0_from_uncond")


def _lam(a: float) -> float:
    """log(sqrt(a / (1 - a))): -inf at a = 0 (the zero terminal SNR of t = 999), +inf at a = 1 (final_alpha_cumprod)"""
    if a == 0.0:
        return -INF
    if a == 1.0:
        return INF
    return math.log(math.sqrt(a / (1.0 - a)))


def coefficients(alphas_cumprod, t: int, t_back, num_inference_steps: int, num_train_timesteps: int = 1000) -> Coef:
    """``alphas_cumprod``: a sequence of Python floats (the table the DDIM tests pin); ``t_back`` the previous loop timestep or None"""
    prev = t - num_train_timesteps // num_inference_steps
    at = float(alphas_cumprod[t])
    ap = float(alphas_cumprod[prev]) if prev >= 0 else 1.0
    lam, lam_next = _lam(at), _lam(ap)
    h = lam_next - lam
    assert h > 0
    if h == INF:                        # exp(-h) = 0, expm1(-2 h) = -1
        m1, m2, mn = 0.0, -math.sqrt(ap), math.sqrt(1.0 - ap)
    else:
        m1 = math.sqrt((1.0 - ap) / (1.0 - at)) * math.exp(-h)
        m2 = math.expm1(-2.0 * h) * math.sqrt(ap)
        mn = math.sqrt(1.0 - ap) * math.sqrt(1.0 - math.exp(-2.0 * h))
    m3, m4, order = 1.0, 0.0, 1
    if t_back is not None and prev >= 0:
        order = 2
        lam_back = _lam(float(alphas_cumprod[t_back]))
        if lam_back != -INF:            # r = inf after the t = 999 step: m3 = 1, m4 = 0
            r = (lam - lam_back) / h
            m3, m4 = 1.0 + 1.0 / (2.0 * r), 1.0 / (2.0 * r)
    return Coef(math.sqrt(at), math.sqrt(1.0 - at), m1, m2, m3, m4, mn, order)


def step_fp64(noise, x0_old, sample, eps, coef):
    """the update in fp64 -> (x', x0, S', S0): S' / S0 the sums of the absolute values of the terms x' / x0 expand into, the scale of
    the rounding bound"""
    k = coef
    n, x, e = noise.double(), sample.double(), eps.double()
    x0 = k.sqrt_alpha * x - k.sqrt_beta * n
    s0 = abs(k.sqrt_alpha) * x.abs() + abs(k.sqrt_beta) * n.abs()
    if k.order == 2:
        old = x0_old.double()
        d = k.m3 * x0 - k.m4 * old
        sd = abs(k.m3) * s0 + abs(k.m4) * old.abs()
    else:
        d, sd = x0, s0
    out = k.m1 * x - k.m2 * d + k.mn * e
    return out, x0, abs(k.m1) * x.abs() + abs(k.m2) * sd + abs(k.mn) * e.abs(), s0


def aten_dpm_step(noise_rows, lat, x0_old, eps, cfg, g, coef, p_t=None, decoy=None):
    """the loop body the step kernel replaces, on the tensors' device: the un-patchify, .float(), the CFG statements, the fp32
    statements of CogVideoXDPMScheduler.step one torch op per operation, the cast back -> (latents', x0 fp32).  ``eps`` may be None
    when coef.mn == 0 (the term is then not evaluated).  ``decoy``: one of DECOYS - a step that is wrong in that one way"""
    assert decoy is None or decoy in DECOYS
    B, F, C_, H, W = lat.shape
    noise = unpatchify(noise_rows, cfg * B, F, H, W, p_t).float()
    uncond = noise
    if cfg == 2:
        u, c = noise.chunk(2)
        uncond = u
        diff = c - u
        gd = g * diff
        noise = u + gd
    if decoy == "x0_from_uncond":
        noise = uncond
    sa, sb, m1, m2, m3, m4, mn, order = coef
    if decoy == "m3_m4_swapped":
        m3, m4 = m4, m3
    if decoy == "first_order":
        order = 1
    if decoy == "eps_dropped":
        mn = 0.0
    x = lat.float()
    sx = sa * x
    sn = sb * noise
    x0 = sx - sn
    d = x0
    if order == 2:
        d3 = m3 * x0
        d4 = m4 * x0_old
        d = d3 - d4
    ax = m1 * x
    bd = m2 * d
    out = ax - bd
    if mn != 0.0:
        ne = mn * eps.float()
        out = out + ne
    return out.to(lat.dtype), x0
