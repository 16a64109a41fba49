"""LKGD latent-knowledge fuse, hoisted out of the sampling loop.

Reference: /root/reference/models/unet_spatio_temporal_condition.py:536-595 recomputes this block in every UNet
forward although its inputs (CLIP embedding, domain-ViT logits, flow-ViT logits) are the same for all 25 steps
(SURVEY.md finding 6).  It is ~1.3 M multiply-adds of fp32 work on [B, 1024] vectors (grouped 1x1 conv taps, quaternion
linears, a 256-point real DFT and a 512-sample inverse), so here it runs ONCE per clip (`pipeline.denoise`): one launch of
`lkgd_lk_fuse` (lkgd_amd/csrc/lk_fuse.hip, one workgroup per batch entry, fp32 - the reference's FFT has no half path
either).  Until round 5 this was PyTorch-ROCm tensor ops (rocFFT + hipBLASLt); `unet.forward` callers that pass the same
tensor objects hit a one-entry cache.  The per-step UNet forward never touches it.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import LkgdHipError, check


def hamilton(q) -> torch.Tensor:
    """core_qnn quaternion_linear weight: [in, out] block matrix from r/i/j/k [in/4, out/4]"""
    r, i, j, k = (w.detach().float() for w in (q.r_weight, q.i_weight, q.j_weight, q.k_weight))
    return torch.cat([torch.cat([r, -i, -j, -k], 0), torch.cat([i, r, -k, j], 0),
                      torch.cat([j, k, r, -i], 0), torch.cat([k, -j, i, r], 0)], 1)


def pack_lk(unet):
    """the 18 fp32 operands of lkgd_lk_fuse (include/lkgd_hip.h section 17), matrices as (in, out) row-major; built once per
    weight version (kept on the model's pack)"""
    def dev32(t):
        return t.detach().to(device=unet.device, dtype=torch.float32).contiguous()
    sf = unet.quaternion_lora_fuse_sf
    l0m, l0p = unet.quaternion_lora_fuse_fft_mag0, unet.quaternion_lora_fuse_fft_pha0
    ws = [dev32(unet.quaternion_lora_lconv.weight.reshape(256, 4)), dev32(unet.quaternion_lora_dconv.weight.reshape(256, 4)),
          dev32(unet.quaternion_lora_fconv.weight.reshape(256, 4)), dev32(unet.quaternion_lora_texts.reshape(256)),
          dev32(hamilton(unet.quaternion_lora_fuse)), dev32(unet.quaternion_lora_fuse.bias),
          dev32(unet.quaternion_lora_texts_fft_mag.reshape(129)), dev32(unet.quaternion_lora_texts_fft_pha.reshape(129)),
          dev32(hamilton(unet.quaternion_lora_fuse_fft_mag)), dev32(unet.quaternion_lora_fuse_fft_mag.bias),
          dev32(hamilton(unet.quaternion_lora_fuse_fft_pha)), dev32(unet.quaternion_lora_fuse_fft_pha.bias),
          dev32(torch.cat([l0m.weight.reshape(4), l0m.bias.reshape(1)])), dev32(torch.cat([l0p.weight.reshape(4), l0p.bias.reshape(1)])),
          dev32(sf[0].weight.T), dev32(sf[0].bias), dev32(sf[2].weight.T), dev32(sf[2].bias)]
    shapes = [(256, 4)] * 3 + [(256,), (1024, 512), (512,), (129,), (129,), (512, 256), (256,), (512, 256), (256,), (5,), (5,),
              (1024, 256), (256,), (256, 1024), (1024,)]
    for w, shp in zip(ws, shapes):
        if tuple(w.shape) != shp:
            raise LkgdHipError(f"latent-knowledge fuse: parameter of shape {tuple(w.shape)}, expected {shp}")
    ptrs = (C.c_void_p * 18)(*[w.data_ptr() for w in ws])
    return ws, ptrs


@torch.no_grad()
def lk_fuse(unet, encoder_hidden_states, domain_features, flow_features) -> torch.Tensor:
    dev = unet.device
    if dev.type != "cuda":
        raise LkgdHipError("the latent-knowledge fuse runs on the GPU (lkgd_amd has no CPU path)")
    unet.prepare()
    pk = unet._pk
    if getattr(pk, "lk", None) is None:
        pk.lk = pack_lk(unet)
    e = encoder_hidden_states.to(device=dev, dtype=torch.float32).contiguous()
    d = domain_features.to(device=dev, dtype=torch.float32).contiguous()
    f = flow_features.to(device=dev, dtype=torch.float32).contiguous()
    if e.dim() != 3 or e.shape[1] != 1 or e.shape[2] != 1024:
        raise LkgdHipError("latent-knowledge fuse: encoder_hidden_states must be [batch, 1, 1024]")
    B, Bd = e.shape[0], d.shape[0]
    if tuple(d.shape[1:]) != (1, 1000) or tuple(f.shape) != tuple(d.shape):
        raise LkgdHipError("latent-knowledge fuse: domain / flow features must be [1 or batch, 1, 1000]")
    if Bd != B and Bd != 1:
        raise LkgdHipError(f"latent-knowledge fuse: {Bd} feature rows for a batch of {B} (1 or {B})")
    out = torch.empty(B, 1, 1024, dtype=torch.float16, device=dev)
    check(_lib.lib().lkgd_lk_fuse(e.data_ptr(), d.data_ptr(), f.data_ptr(), B, Bd, pk.lk[1], out.data_ptr(), 1024,
                                  torch.cuda.current_stream(dev).cuda_stream), "lkgd_lk_fuse")
    return out                                                         # REPLACES the CLIP embedding (:595,:613)


def lk_fuse_cached(unet, e, d, f) -> torch.Tensor:
    """one-entry cache for callers that pass the SAME tensor objects every Euler step (`unet.forward` in a caller-owned
    loop).  The entry keeps the three input tensors alive and compares identity + in-place version, so the allocator
    cannot hand a recycled address of a different clip back as a hit; fresh tensors always recompute."""
    c = unet._lk_cache
    ins = (e, d, f)
    if c is not None and all(a is b and a._version == v for a, (b, v) in zip(ins, c[0])):
        return c[1]
    out = lk_fuse(unet, e, d, f)
    unet._lk_cache = (tuple((t, t._version) for t in ins), out)
    return out


# ---- the DiT form: the fuse of the CogVideoX text tokens (include/lkgd_hip_dit_loop.h, lkgd_amd/csrc/lk_fuse.hip) ----------------------
LK_TOKENS_SHAPES = [(256, 16), (256, 4), (256, 4), (256,), (1024, 512), (512,), (129,), (129,), (512, 256), (256,), (512, 256), (256,),
                    (5,), (5,), (1024, 512), (512,), (512, 4096), (4096,)]


def pack_lk_tokens(transformer):
    """the 18 fp32 operands of lkgd_lk_fuse_tokens in the order of ``pack_lk`` with the DiT's shapes (16-tap lconv from 4096
    channels, fuse_sf 1024 -> 512 -> 4096), matrices as (in, out) row-major; built once per weight version (kept on the model's
    pack)"""
    dev = transformer.device

    def dev32(t):
        return t.detach().to(device=dev, dtype=torch.float32).contiguous()
    m = transformer
    sf = m.quaternion_lora_fuse_sf
    l0m, l0p = m.quaternion_lora_fuse_fft_mag0, m.quaternion_lora_fuse_fft_pha0
    ws = [dev32(m.quaternion_lora_lconv.weight.reshape(256, 16)), dev32(m.quaternion_lora_dconv.weight.reshape(256, 4)),
          dev32(m.quaternion_lora_fconv.weight.reshape(256, 4)), dev32(m.quaternion_lora_texts.reshape(256)),
          dev32(hamilton(m.quaternion_lora_fuse)), dev32(m.quaternion_lora_fuse.bias),
          dev32(m.quaternion_lora_texts_fft_mag.reshape(129)), dev32(m.quaternion_lora_texts_fft_pha.reshape(129)),
          dev32(hamilton(m.quaternion_lora_fuse_fft_mag)), dev32(m.quaternion_lora_fuse_fft_mag.bias),
          dev32(hamilton(m.quaternion_lora_fuse_fft_pha)), dev32(m.quaternion_lora_fuse_fft_pha.bias),
          dev32(torch.cat([l0m.weight.reshape(4), l0m.bias.reshape(1)])), dev32(torch.cat([l0p.weight.reshape(4), l0p.bias.reshape(1)])),
          dev32(sf[0].weight.T), dev32(sf[0].bias), dev32(sf[2].weight.T), dev32(sf[2].bias)]
    for w, shp in zip(ws, LK_TOKENS_SHAPES):
        if tuple(w.shape) != shp:
            raise LkgdHipError(f"latent-knowledge fuse of the text tokens: parameter of shape {tuple(w.shape)}, expected {shp}")
    ptrs = (C.c_void_p * 18)(*[w.data_ptr() for w in ws])
    return ws, ptrs


@torch.no_grad()
def lk_fuse_tokens(pack, encoder_hidden_states, domain_features, flow_features, out=None) -> torch.Tensor:
    """one launch of lkgd_lk_fuse_tokens: ``encoder_hidden_states`` [B, L, 4096], ``domain_features`` / ``flow_features``
    [1 or B, 1, 1000] -> fp16 [B, L, 4096].  ``pack`` = ``pack_lk_tokens(model)``; everything lives on the pack's device."""
    ws, ptrs = pack
    dev = ws[0].device
    if dev.type != "cuda":
        raise LkgdHipError("the latent-knowledge fuse runs on the GPU (lkgd_amd has no CPU path)")
    e = encoder_hidden_states.to(device=dev, dtype=torch.float32)
    d = domain_features.to(device=dev, dtype=torch.float32).contiguous()
    f = flow_features.to(device=dev, dtype=torch.float32).contiguous()
    if e.dim() != 3 or e.shape[2] != 4096 or e.shape[0] < 1 or e.shape[1] < 1:
        raise LkgdHipError(f"latent-knowledge fuse: encoder_hidden_states must be [batch, tokens, 4096], got {tuple(e.shape)}")
    if e.stride(2) != 1 or e.stride(0) != e.shape[1] * e.stride(1) or e.stride(1) % 4 or e.data_ptr() % 16:
        e = e.contiguous()
    B, L, Bd = e.shape[0], e.shape[1], d.shape[0]
    if d.dim() != 3 or tuple(d.shape[1:]) != (1, 1000) or tuple(f.shape) != tuple(d.shape):
        raise LkgdHipError("latent-knowledge fuse: domain / flow features must be [1 or batch, 1, 1000]")
    if Bd != B and Bd != 1:
        raise LkgdHipError(f"latent-knowledge fuse: {Bd} feature rows for a batch of {B} (1 or {B})")
    if out is None:
        out = torch.empty(B, L, 4096, dtype=torch.float16, device=dev)
    elif out.dtype != torch.float16 or out.device != dev or tuple(out.shape) != (B, L, 4096) or out.stride(2) != 1 \
            or out.stride(0) != L * out.stride(1):
        raise LkgdHipError(f"latent-knowledge fuse: out must be a GPU fp16 [{B}, {L}, 4096] tensor with one row stride")
    check(_lib.lib().lkgd_lk_fuse_tokens(e.data_ptr(), e.stride(1), d.data_ptr(), f.data_ptr(), B, L, Bd, ptrs, out.data_ptr(),
                                         out.stride(1), torch.cuda.current_stream(dev).cuda_stream), "lkgd_lk_fuse_tokens")
    return out
