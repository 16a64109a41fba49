"""The opt-in FP8 mode of the CogVideoX DiT (include/lkgd_hip_fp8.h).

The reference's quantised demo (CogVideo-main/inference/cli_demo_quantization.py:42-47, default ``quantization_scheme="fp8"``) calls
``quantize_to_float8(transformer, QuantConfig(ActivationCasting.DYNAMIC))`` of torchao [EXT]; here the one call is
``quantize_to_float8(transformer)``.  It switches the six linears of every ``CogVideoXBlock`` (q, k, v, out, ff.0, ff.2) to e4m3fn:
weights with one fp32 scale per output channel, quantised once when the model packs; activations with one fp32 scale per token
row, quantised on the device in every call; fp32 accumulation, fp16 output.  Everything else of the model stays fp16.
PARITY UNPINNED: torchao scales per TENSOR; the per-row / per-channel scheme here is the finer one and is not compared with it.
"""
from __future__ import annotations

import os
from typing import Tuple

import torch

from ._lib import LkgdHipError

E4M3_MAX = 448.0


def quantize_weight(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[N, K] weight -> (e4m3fn bytes uint8 [N, K], fp32 scale [N]): the statement Q of include/lkgd_hip_fp8.h on every output
    channel of the weight's fp16 values (the values the fp16 path multiplies with).  Torch code, on the weight's device."""
    if w.dim() != 2:
        raise LkgdHipError(f"quantize_weight: a Linear's [out, in] weight is expected, got {tuple(w.shape)}")
    x = w.detach().to(torch.float16).to(torch.float32)
    amax = x.abs().amax(dim=1)
    zero = amax == 0
    safe = torch.where(zero, torch.ones_like(amax), amax)
    top = torch.full_like(amax, E4M3_MAX)
    inv = torch.where(zero, torch.ones_like(amax), top / safe)
    scale = torch.where(zero, torch.ones_like(amax), safe / top)
    q = (x * inv[:, None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.contiguous(), scale.contiguous()


def env_on() -> bool:
    """LKGD_DIT_FP8=1: every DiT packs in the FP8 mode (read when a model packs, so ``bench.py --cogvideox`` runs both ways)"""
    return os.environ.get("LKGD_DIT_FP8", "0") == "1"


def active(model) -> bool:
    """whether ``model`` packs its block linears as FP8: ``quantize_to_float8`` was called on it, or LKGD_DIT_FP8=1"""
    return getattr(model, "quantization", None) == "fp8" or env_on()


def quantize(model, quantization_scheme: str = "fp8"):
    """the reference's ``quantize_model(part, quantization_scheme)``: "fp8" is built, every other name raises"""
    if quantization_scheme != "fp8":
        raise LkgdHipError(f"quantization scheme {quantization_scheme!r} is not built: the HIP path has \"fp8\" (e4m3 block linears) "
                           "only")
    if not hasattr(model, "transformer_blocks") or not hasattr(model, "invalidate"):
        raise LkgdHipError(f"quantize_to_float8: a CogVideoXTransformer3DModel is expected, got {type(model).__name__}")
    d = model.inner_dim
    if d % 128:
        raise LkgdHipError(f"quantize_to_float8: the FP8 GEMM tiles N and K by 128, inner dim {d} is not a multiple")
    model.quantization = "fp8"
    model.invalidate()
    return model


def quantize_to_float8(model, config=None):
    """the reference's name.  Returns the model with ``model.quantization = "fp8"`` and its packs invalidated: the next call packs
    the six block linears as (bytes, scale, bias) and runs them on ``lkgd_gemm_fp8``.  ``config`` (torchao's QuantConfig) is
    accepted and ignored: dynamic activation casting is the one mode."""
    return quantize(model, "fp8")


def dequantize(model):
    """back to the fp16 linears: the module's fp16 parameters were never touched, the next call packs them again"""
    model.quantization = None
    model.invalidate()
    return model
