"""The pre-LN image encoder CLIP (lkgd_amd/clip.py) and the ViT (lkgd_amd/vit.py) both are: class row + patch rows + position
rows, a stack of [LN -> q|k|v -> attention -> out-projection + residual -> LN -> fc1 -> activation -> fc2 + residual] layers, and a
head on the class row.  The two hosts keep their parameter trees, config checks and patch extraction and call these four pieces; what
differs between them - the attention kernel, the activation, eps, a patch bias, the head's bias - is an argument.

* the LayerNorm affine is folded into the consumer Linear (``fold_ln``), so the norm launches run without one;
* exact-erf GELU goes through the GEGLU epilogue with a constant-one "hidden" half (zero weights, bias 1): out = 1 * gelu(fc1 x);
  ``quick_gelu(x) = x sigmoid(1.702 x) = silu(1.702 x) / 1.702`` with both constants folded into fc1 / fc2.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops
from .packing import f32, pack_geglu, pack_linear


def fold_ln(norm: nn.LayerNorm, w: torch.Tensor, b: torch.Tensor):
    """Linear(LN(x)) = (W diag(g)) x_hat + (W beta + b), in fp32"""
    g, be = norm.weight.detach().float(), norm.bias.detach().float()
    w32 = w.detach().float()
    return w32 * g[None, :], w32 @ be + b.detach().float()


def pack_layer(norm1: nn.LayerNorm, wqkv: torch.Tensor, bqkv: torch.Tensor, out_proj: nn.Linear, norm2: nn.LayerNorm,
               fc1: nn.Linear, fc2: nn.Linear, act: str) -> SimpleNamespace:
    """one layer's kernel-layout weights; ``wqkv`` / ``bqkv``: the fused [3D, D] projection (rows q | k | v); ``act``: "gelu" or
    "quick_gelu" """
    wq, bq = fold_ln(norm1, wqkv, bqkv)
    w1, b1 = fold_ln(norm2, fc1.weight, fc1.bias)
    pk = SimpleNamespace(wqkv=pack_linear(wq), bqkv=bq.contiguous(), wo=pack_linear(out_proj.weight), bo=f32(out_proj.bias),
                         b2=f32(fc2.bias), act=act)
    if act == "gelu":
        # GELU(fc1 x) as GEGLU with a constant-one hidden half: hidden = 0 * x + 1, gate = fc1 x
        wg = torch.cat([torch.zeros_like(w1), w1], dim=0)
        bg = torch.cat([torch.ones_like(b1), b1], dim=0)
        pk.w1, pk.b1, pk.half = pack_geglu(wg, bg)
        pk.w2 = pack_linear(fc2.weight)
    else:
        pk.w1, pk.b1, pk.half = pack_linear(w1 * 1.702), (b1 * 1.702).contiguous(), 0
        pk.w2 = pack_linear(fc2.weight.detach().float() / 1.702)
    return pk


def embed_rows(patches: torch.Tensor, wpe: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, N: int, P: int, bias=None):
    """patch rows [N*P, K] -> token rows fp16 [N*(P+1), D]: row 0 of an image is ``cls`` (class embedding + position 0, folded at
    pack time), row 1 + m is patch m through the embedding GEMM + ``pos[m]``"""
    S, (D, K) = P + 1, wpe.shape
    tok = torch.empty(N * S, D, dtype=torch.float16, device=patches.device)
    tok.view(N, S, D)[:, 0] = cls
    for n in range(N):       # one GEMM per image: its patch rows land behind the image's class row, + position row 1 + m
        ops.gemm(patches[n * P:(n + 1) * P], wpe, tok[n * S + 1:(n + 1) * S], M=P, N=D, K=K, bias=bias, rowbias=pos,
                 rowmap=(1, 1, 1, 1 << 30))
    return tok


def run_layers(tok: torch.Tensor, layers, N: int, S: int, heads: int, eps: float, attn) -> torch.Tensor:
    """token rows [N*S, D] through the packed ``layers``; ``attn(q, k, v, out, N, S, heads)`` is the attention launch"""
    (T, D), dev = tok.shape, tok.device
    for p in layers:
        ln = ops.layernorm(tok, None, None, eps)
        qkv = torch.empty(T, 3 * D, dtype=torch.float16, device=dev)
        ops.gemm(ln, p.wqkv, qkv, M=T, N=3 * D, K=D, bias=p.bqkv)
        att = torch.empty(T, D, dtype=torch.float16, device=dev)
        attn(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], att, N, S, heads)
        t1 = torch.empty(T, D, dtype=torch.float16, device=dev)
        ops.gemm(att, p.wo, t1, M=T, N=D, K=D, bias=p.bo, res1=tok)
        ln2 = ops.layernorm(t1, None, None, eps)
        inner = p.w2.shape[1]
        h = torch.empty(T, inner, dtype=torch.float16, device=dev)
        if p.act == "gelu":
            ops.gemm(ln2, p.w1, h, M=T, N=2 * inner, K=D, bias=p.b1, geglu=p.half)
        else:
            ops.gemm(ln2, p.w1, h, M=T, N=inner, K=D, bias=p.b1)
            h = ops.silu(h)
        tok = torch.empty(T, D, dtype=torch.float16, device=dev)
        ops.gemm(h, p.w2, tok, M=T, N=D, K=inner, bias=p.b2, res1=t1)
    return tok


def class_head(tok: torch.Tensor, N: int, S: int, g: torch.Tensor, b: torch.Tensor, eps: float, w: torch.Tensor, bias=None):
    """class row of every image -> LayerNorm(g, b) -> Linear ``w`` [out, D] (+ ``bias``): fp16 [N, out]"""
    D = tok.shape[1]
    cls = ops.layernorm(tok.view(N, S, D)[:, 0].contiguous(), g, b, eps)
    out = torch.empty(N, w.shape[0], dtype=torch.float16, device=tok.device)
    ops.gemm(cls, w, out, M=N, N=w.shape[0], K=D, bias=bias)
    return out
