"""The T5 text encoder in front of the CogVideoX loop, on the MI355X path.

The reference encodes the prompt once per clip with ``self.text_encoder(text_input_ids.to(device))[0]``
(CogVideo-main/finetune/models/cogvideox_i2v/pipeline_cogvideox_image2video.py:262; ``text_encoder`` is transformers'
``T5EncoderModel`` [EXT], for CogVideoX the T5-v1.1-XXL encoder of ``text_encoder/``: 24 layers x 4096 channels, 64 heads of 64,
d_ff 10240, gated tanh-GELU, 226 tokens, NO attention mask - padding is attended).  This module keeps that class's name, its call
(``model(input_ids)[0]`` / ``.last_hidden_state``) and its parameter names - so the sharded ``text_encoder/model-*.safetensors``
loads as it is - and runs the forward on the kernels of include/lkgd_hip_t5.h and the fp16 GEMM.  Per layer, ten launches:

    lkgd_t5_rmsnorm -> lkgd_gemm_f16 (q|k|v) -> lkgd_attn_dense_relbias -> lkgd_gemm_f16 (o) -> lkgd_t5_residual_add
    lkgd_t5_rmsnorm -> lkgd_gemm_f16 (wi_0|wi_1) -> lkgd_t5_gated_gelu -> lkgd_gemm_f16 (wo) -> lkgd_t5_residual_add

in front of them ``lkgd_t5_embed_rows``, behind them the final ``lkgd_t5_rmsnorm``.  T5 has no bias anywhere, does not scale its
scores by 1/sqrt(d_kv), and adds a relative-position bias that depends on key position minus query position only: one fp32
[heads, 2S - 1] table per sequence length, built on the host with transformers' bucket expression and shared by every layer.

Range.  The residual stream is fp32.  T5-XXL is known to overflow fp16 in its feed-forward output (transformers keeps ``wo`` in fp32
and clamps for that reason), so the two closing projections run with the GEMM's accumulator scale ``s_acc = 2^-6`` (applied to the fp32
accumulator before the one rounding to fp16) and their residual add with ``s = 2^6``: a sublayer output up to 65504 * 64 = 4.2e6 stays
finite.  Real XXL activations have not been measured on this path.

Parity: tests/test_t5_gpu.py against transformers' own fp32 forward of the same fp16-rounded random weights (transformers is
third-party and not part of the reference tree; the tests skip where it is absent).  Attention masks, the decoder and bf16 are not
built.
"""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from ._lib import LkgdHipError
from .loading import build_from_transformers, save_transformers
from .module import PackedModule
from .packing import f32, pack_linear

#: the closing projections' accumulator scale and the factor their residual add undoes it with (both powers of two: exact)
S_ACC = 2.0 ** -6
S_RES = 2.0 ** 6

#: what ``forward`` returns: ``out[0]`` and ``out.last_hidden_state``, as transformers' BaseModelOutput gives them
T5EncoderOutput = namedtuple("T5EncoderOutput", ["last_hidden_state"])


@dataclass
class T5Config:
    """the keys of ``text_encoder/config.json`` the encoder reads; defaults: the T5-v1.1-XXL encoder of CogVideoX"""
    vocab_size: int = 32128
    d_model: int = 4096
    d_kv: int = 64
    d_ff: int = 10240
    num_layers: int = 24
    num_heads: int = 64
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "gated-gelu"


def check_t5_config(cfg: T5Config) -> None:
    """what the HIP path builds; everything else raises, naming the key"""
    if cfg.feed_forward_proj != "gated-gelu":
        raise LkgdHipError(f"T5 on the HIP path: feed_forward_proj {cfg.feed_forward_proj!r} (only 'gated-gelu', the activation of "
                           "CogVideoX's text_encoder/, is built)")
    if cfg.d_kv % 8 or not 0 < cfg.d_kv <= 128:
        raise LkgdHipError(f"T5 on the HIP path: d_kv {cfg.d_kv} (a multiple of 8 up to 128: lkgd_attn_dense_relbias)")
    if cfg.d_model > 4096 or cfg.d_model <= 0 or cfg.d_model % 64:
        raise LkgdHipError(f"T5 on the HIP path: d_model {cfg.d_model} (a multiple of 64 up to 4096: lkgd_t5_rmsnorm, lkgd_gemm_f16)")
    if cfg.num_heads <= 0 or (cfg.num_heads * cfg.d_kv) % 64:
        raise LkgdHipError(f"T5 on the HIP path: num_heads * d_kv = {cfg.num_heads * cfg.d_kv} (a multiple of 64: lkgd_gemm_f16)")
    if cfg.d_ff <= 0 or cfg.d_ff % 8:
        raise LkgdHipError(f"T5 on the HIP path: d_ff {cfg.d_ff} (a multiple of 8: lkgd_t5_gated_gelu)")
    if cfg.num_layers <= 0 or cfg.vocab_size <= 0 or cfg.relative_attention_num_buckets < 4:
        raise LkgdHipError(f"T5 on the HIP path: num_layers {cfg.num_layers}, vocab_size {cfg.vocab_size}, "
                           f"relative_attention_num_buckets {cfg.relative_attention_num_buckets}")


def relative_position_bucket(relative_position: torch.Tensor, num_buckets: int, max_distance: int) -> torch.Tensor:
    """transformers' ``T5Attention._relative_position_bucket`` [EXT] for the bidirectional (encoder) case, statement for statement -
    including the fp32 ``log`` and the truncation: another logarithm can land on the other side of a bucket edge"""
    num_buckets //= 2
    relative_buckets = (relative_position > 0).to(torch.long) * num_buckets
    relative_position = torch.abs(relative_position)
    max_exact = num_buckets // 2
    is_small = relative_position < max_exact
    relative_position_if_large = max_exact + (
        torch.log(relative_position.float() / max_exact) / math.log(max_distance / max_exact) * (num_buckets - max_exact)
    ).to(torch.long)
    relative_position_if_large = torch.min(relative_position_if_large, torch.full_like(relative_position_if_large, num_buckets - 1))
    return relative_buckets + torch.where(is_small, relative_position, relative_position_if_large)


def relative_bias_table(weight: torch.Tensor, S: int, num_buckets: int, max_distance: int) -> torch.Tensor:
    """``relative_attention_bias.weight`` [num_buckets, heads] -> fp32 [heads, 2S - 1] on the weight's device: entry d + S - 1 of a
    row is the bias at key position minus query position d, so ``compute_bias(S, S)[0, h, i, j] == table[h, j - i + S - 1]``.  The
    buckets are computed on the host"""
    d = torch.arange(-(S - 1), S, dtype=torch.long)
    bucket = relative_position_bucket(d, num_buckets, max_distance)
    return weight.detach().float()[bucket.to(weight.device)].t().contiguous()


# ---- the parameter holders: transformers' module tree ------------------------------------------------------------------------------
class T5LayerNorm(nn.Module):
    def __init__(self, d: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.variance_epsilon = eps


class T5Attention(nn.Module):
    def __init__(self, cfg: T5Config, has_relative_attention_bias: bool):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        self.q, self.k, self.v = (nn.Linear(cfg.d_model, inner, bias=False) for _ in range(3))
        self.o = nn.Linear(inner, cfg.d_model, bias=False)
        if has_relative_attention_bias:
            self.relative_attention_bias = nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_heads)


class T5LayerSelfAttention(nn.Module):
    def __init__(self, cfg: T5Config, has_relative_attention_bias: bool):
        super().__init__()
        self.SelfAttention = T5Attention(cfg, has_relative_attention_bias)
        self.layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)


class T5DenseGatedActDense(nn.Module):
    def __init__(self, cfg: T5Config):
        super().__init__()
        self.wi_0 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wi_1 = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wo = nn.Linear(cfg.d_ff, cfg.d_model, bias=False)


class T5LayerFF(nn.Module):
    def __init__(self, cfg: T5Config):
        super().__init__()
        self.DenseReluDense = T5DenseGatedActDense(cfg)
        self.layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)


class T5Block(nn.Module):
    def __init__(self, cfg: T5Config, has_relative_attention_bias: bool):
        super().__init__()
        self.layer = nn.ModuleList([T5LayerSelfAttention(cfg, has_relative_attention_bias), T5LayerFF(cfg)])

    def pack(self):
        a, ff = self.layer[0].SelfAttention, self.layer[1].DenseReluDense
        F_ = ff.wi_0.weight.shape[0]
        Fp = (F_ + 63) // 64 * 64          # the GEMM's K is a multiple of 64: zero rows of wi / zero columns of wo up to it
        wi = torch.zeros(2 * Fp, ff.wi_0.weight.shape[1], dtype=torch.float16, device=ff.wi_0.weight.device)
        wi[:F_] = ff.wi_0.weight.detach().to(torch.float16)
        wi[Fp:Fp + F_] = ff.wi_1.weight.detach().to(torch.float16)
        wo = torch.zeros(ff.wo.weight.shape[0], Fp, dtype=torch.float16, device=ff.wo.weight.device)
        wo[:, :F_] = ff.wo.weight.detach().to(torch.float16)
        self._pk = SimpleNamespace(
            g1=f32(self.layer[0].layer_norm.weight), g2=f32(self.layer[1].layer_norm.weight),
            wqkv=pack_linear(torch.cat([a.q.weight, a.k.weight, a.v.weight], dim=0).detach()), wo=pack_linear(a.o.weight.detach()),
            wi=wi, wo2=wo, Fp=Fp)


class T5Stack(nn.Module):
    def __init__(self, cfg: T5Config, embed_tokens: nn.Embedding):
        super().__init__()
        self.embed_tokens = embed_tokens
        self.block = nn.ModuleList([T5Block(cfg, has_relative_attention_bias=(i == 0)) for i in range(cfg.num_layers)])
        self.final_layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)


TIED = ("shared.weight", "encoder.embed_tokens.weight")


class T5EncoderModel(PackedModule):
    """transformers' class of the same name: parameter holder + HIP forward; ``model(input_ids)[0]`` is fp16 [B, S, d_model]"""

    def __init__(self, config: Optional[T5Config] = None, **kw):
        super().__init__()
        cfg = config if config is not None else T5Config(**kw)
        check_t5_config(cfg)
        self.config = cfg
        self.shared = nn.Embedding(cfg.vocab_size, cfg.d_model)
        self.encoder = T5Stack(cfg, self.shared)          # embed_tokens IS shared (transformers ties them): both keys, one tensor
        self._bias_tables = {}

    OFF_GPU = "lkgd_amd T5 runs on MI355X only: move the module to cuda first"

    # ---- loading ------------------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = "text_encoder", torch_dtype=torch.float16, dtype=None,
                        variant: Optional[str] = None, **_ignored):
        """a local ``text_encoder/`` directory: ``config.json`` + ``model[.<variant>].safetensors``, the sharded
        ``model.safetensors.index.json`` form of the released checkpoint, or ``pytorch_model.bin``; every key is checked"""
        return build_from_transformers(cls, T5Config, path, subfolder, torch_dtype, dtype, variant)

    def save_pretrained(self, path: str, **_kw):
        # one tensor per storage: the tied copy is left out, as transformers' own save does
        save_transformers(self, path, {"architectures": ["T5EncoderModel"], "model_type": "t5", "is_gated_act": True,
                                       "dense_act_fn": "gelu_new"}, omit=(TIED[1],))

    def load_state_dict(self, state_dict, *a, **k):
        """``encoder.embed_tokens.weight`` is the tied copy of ``shared.weight``: either may be absent (a safetensors file holds one
        tensor per storage); both present and different is refused"""
        sd = dict(state_dict)
        if TIED[0] in sd and TIED[1] in sd:
            if sd[TIED[0]].shape != sd[TIED[1]].shape or not torch.equal(sd[TIED[0]], sd[TIED[1]]):
                raise LkgdHipError(f"T5EncoderModel.load_state_dict: {TIED[1]} differs from {TIED[0]} (the two are one tied tensor)")
            sd[TIED[1]] = sd[TIED[0]]
        elif TIED[0] in sd or TIED[1] in sd:
            sd[TIED[0]] = sd[TIED[1]] = sd[TIED[0]] if TIED[0] in sd else sd[TIED[1]]
        return super().load_state_dict(sd, *a, **k)

    def _forget(self):
        self._bias_tables = {}          # built from layer 0's relative_attention_bias

    # ---- forward ------------------------------------------------------------------------------------------------------
    def bias_table(self, S: int) -> torch.Tensor:
        """the fp32 [heads, 2S - 1] relative-position table of layer 0, used by every layer; built once per S"""
        t = self._bias_tables.get(S)
        if t is None:
            cfg = self.config
            w = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
            t = self._bias_tables[S] = relative_bias_table(w, S, cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance)
        return t

    def _pack(self):
        for blk in self.encoder.block:
            blk.pack()
        return SimpleNamespace(table=self.shared.weight.detach().to(torch.float16).contiguous(),
                               g_final=f32(self.encoder.final_layer_norm.weight))

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, attention_mask=None, **_kw):
        """input_ids int64 [B, S] -> ``T5EncoderOutput``: ``[0]`` / ``.last_hidden_state`` fp16 [B, S, d_model].  No mask: the
        reference calls the encoder without one, so padding tokens are attended (pipeline_cogvideox_image2video.py:262)"""
        if attention_mask is not None:
            raise LkgdHipError("lkgd_amd T5: attention_mask is not built (the CogVideoX pipeline calls the text encoder without one)")
        cfg = self.config
        if input_ids.dim() != 2 or input_ids.dtype != torch.int64:
            raise ValueError(f"expected input_ids int64 [B, S], got {input_ids.dtype} {tuple(input_ids.shape)}")
        host = input_ids.cpu()
        if host.numel() == 0 or int(host.min()) < 0 or int(host.max()) >= cfg.vocab_size:
            raise ValueError(f"input_ids must be non-empty with every id in [0, {cfg.vocab_size})")
        self.prepare()
        pk, dev = self._pk, self.device
        B, S = input_ids.shape
        T, D, heads, hd, eps = B * S, cfg.d_model, cfg.num_heads, cfg.d_kv, cfg.layer_norm_epsilon
        inner = heads * hd
        bias = self.bias_table(S)
        x = ops.t5_embed_rows(input_ids.to(dev).reshape(T).contiguous(), pk.table)          # the fp32 residual stream
        ln = torch.empty(T, D, dtype=torch.float16, device=dev)
        qkv = torch.empty(T, 3 * inner, dtype=torch.float16, device=dev)
        att = torch.empty(T, inner, dtype=torch.float16, device=dev)
        y = torch.empty(T, D, dtype=torch.float16, device=dev)
        for blk in self.encoder.block:
            p = blk._pk
            ops.t5_rmsnorm(x, p.g1, eps, out=ln)
            ops.gemm(ln, p.wqkv, qkv, M=T, N=3 * inner, K=D)
            ops.attn_dense_relbias(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], att, B, S, heads, hd, bias, scale=1.0)
            ops.gemm(att, p.wo, y, M=T, N=D, K=inner, s_acc=S_ACC)
            ops.t5_residual_add_(x, y, S_RES)
            ops.t5_rmsnorm(x, p.g2, eps, out=ln)
            h = torch.empty(T, 2 * p.Fp, dtype=torch.float16, device=dev)
            ops.gemm(ln, p.wi, h, M=T, N=2 * p.Fp, K=D)
            g = ops.t5_gated_gelu(h)
            ops.gemm(g, p.wo2, y, M=T, N=D, K=p.Fp, s_acc=S_ACC)
            ops.t5_residual_add_(x, y, S_RES)
        out = ops.t5_rmsnorm(x, pk.g_final, eps)
        return T5EncoderOutput(last_hidden_state=out.view(B, S, D))
