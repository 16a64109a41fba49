"""The CogVideoX DiT sampling loop with LKGD's latent-knowledge fuse on the MI355X path (BASELINE.json
configs[4]).

Mirrors /root/reference/CogVideo-main/finetune/models/cogvideox_i2v/cogvideox_transformer_3d.py (``CogVideoXBlock`` :41-160,
``CogVideoXTransformer3DModel`` :163-335, ``init_quaternion_modules`` :337-366, ``forward`` :473-638 with the same positional
``domain_features`` / ``flow_features``) and the loop of ``pipeline_cogvideox_image2video.py:829-885`` (CFG duplication, channel
concat with the image latents, dynamic CFG scale :866-869, scheduler step).  The blocks those files import from diffusers >= 0.32
[EXT] are restated with diffusers' parameter names (a ``transformer/`` checkpoint loads by ``load_state_dict``); oracle/cogvideox.py
is the fp32 twin the tests compare with, and tests/golden/cogvideox.safetensors pins the in-tree wiring on the reference's own
``forward``.

MI355X design - the UNet's kernels, one joint token buffer:
* tokens [B * (L_text + L_video), D] fp16, text rows first in every batch entry (the order of the reference's
  ``torch.cat([encoder_hidden_states, hidden_states], dim=1)`` for attention and feed-forward): the two streams are row
  slices, never concatenated or split;
* adaLN-zero: the 6 x D modulation vectors of all 2 x 30 ``CogVideoXLayerNormZero`` layers come from ONE GEMM per step
  ([sum, 512] weights on silu(emb)); ``norm(x) * (1 + scale) + shift`` is the LayerNorm kernel with per-(batch, stream)
  effective affine vectors gamma (1 + scale), beta (1 + scale) + shift (rows up to 2048 channels); the gated residuals of both
  streams are one pass of ``lkgd_gated_add``;
* attention: three projections (bias), per-head LayerNorm of q and k as the LayerNorm kernel over [tokens * heads, 64] rows in
  place, then the head_dim-64 flash kernel over the joint sequence (S = 226 + 17 550, ragged last tile);
* feed-forward: GEMM + ``lkgd_gelu_tanh`` + GEMM;
* the latent-knowledge fuse acts on the TEXT embeddings and is step-invariant: one launch per clip, fp32
  (``lkgd_lk_fuse_tokens``, include/lkgd_hip_dit_loop.h; lkgd_amd/lk_fuse.py); the 3-D sin-cos position table is added in the
  patch-embedding GEMM's epilogue (row-indexed bias);
* rotary models (CogVideoX-5B-I2V: ``use_rotary_positional_embeddings``, 48 heads, 3072 channels): no sin-cos table; the
  learned joint position table, when the checkpoint has one, rides the same row-indexed bias of BOTH embedding GEMMs (text
  rows included); the per-head q / k norms and the rotation of the video rows are one launch per layer
  (``lkgd_qk_norm_rope``, include/lkgd_hip_dit.h) over tables built once per clip (``rotary_tables``);
* the sampling loop's glue is two launches per step (include/lkgd_hip_dit_loop.h): ``lkgd_dit_patch_rows`` writes the patch rows
  of latents | image latents ONCE for both CFG entries (no duplicated batch, no channel concat), ``forward_rows`` runs the DiT on
  them, ``lkgd_dit_cfg_ddim_step`` takes proj_out's token rows through the CFG combine and the DDIM update into the latents in
  place.  ``forward_tokens`` / ``forward`` keep the [B, F, C, H, W] interface: their patch unfold / un-patchify are torch permutes
  (data movement at the API edge);
* the loop's other scheduler branch (``CogVideoXDPMScheduler``: DPM-Solver++ SDE 2M, what the reference installs for the 5B models;
  DESIGN.md section 15): the same two launches per step with ``lkgd_dit_cfg_dpm_step`` (include/lkgd_hip_dit_dpm.h) as the second -
  CFG combine, x0, the first- or second-order update with the step's noise, the fp32 ``old_pred_original_sample`` state and the
  cast back, 2-D and temporal patches;
* the 1.5 models (``patch_size_t = 2``, rotary, no learned table, with or without ``ofs_embed_dim``): a token
  spans two latent frames, so the patch embedding is a Linear over C p_t p p columns and the grid is (F / p_t, h, w); the loop's
  glue is the ``_t`` pair of include/lkgd_hip_dit_tpatch.h; the ``ofs`` embedding (timestep-embedding kernel + two small GEMMs,
  step-invariant: once per clip) is added to the time embedding before the modulation GEMM; ``rotary_tables`` restates the
  pipeline's ``grid_type="slice"`` branch; ``pad_for_temporal_patches`` / ``drop_temporal_padding`` restate its frame padding;
* the opt-in FP8 mode (``lkgd_amd.fp8.quantize_to_float8`` or LKGD_DIT_FP8=1; DESIGN.md section 14, include/lkgd_hip_fp8.h): the six
  linears of every block run on ``lkgd_gemm_fp8`` over e4m3 weights (one scale per output channel, quantised when the model packs)
  and e4m3 activations (one scale per token row, quantised by the kernel that produces them: ``lkgd_layernorm_quant_fp8`` for the
  two modulated norms, ``lkgd_quant_rows_fp8`` for the attention output, ``lkgd_gelu_tanh_quant_fp8`` for the feed-forward's hidden
  rows).  Residual stream, norms, q/k norm + rope, attention, gates and every other linear stay as they are.
* ``encode_prompt``: the pipeline's method in front of the loop, with the T5 text encoder of ``lkgd_amd/t5.py``
  (include/lkgd_hip_t5.h) and the caller's tokenizer as arguments; its embeddings are what ``denoise`` takes.
* LoRA adapters (the reference's fine-tune, finetune/trainer.py:247-257): the six block linears may sit in
  ``lkgd_amd.lora.Linear`` wrappers (peft's state-dict names).  An adapter that applies to every row is a different WEIGHT: a wrapped
  linear packs the fp16 (or e4m3) form of ``W + sum_a c_a B_a A_a``, folded in fp32 when the model packs, and the sampling loop
  issues the launch list it issues without adapters.  There is no per-step low-rank path.
* text-to-video and video-to-video ([EXT] diffusers' two classes, parity unpinned): the stock transformer has no
  ``quaternion_lora_*`` path, so ``denoise`` without feature tensors takes the prompt embeddings as the text rows, and without image
  latents ``lkgd_dit_patch_rows`` writes the latents' channels alone; ``denoise(start_step=)`` runs the tail of the schedule on a clip
  noised by ``add_noise`` (``get_timesteps``, ``prepare_video_latents``; ``prepare_noise_latents`` for text-to-video).  All of it is
  once-per-clip host glue over existing launches: the step stays ``lkgd_dit_patch_rows[_t]`` -> ``forward_rows`` ->
  ``lkgd_dit_cfg_ddim_step[_t]`` / ``lkgd_dit_cfg_dpm_step[_t]``.
* reference attention (inference/ddim_inversion.py, lkgd_amd/ddim_inversion.py): ``Attention`` holds a marker
  processor (``get_processor`` / ``set_processor``).  While a block's marker has ``reference_attention``, ``forward_rows`` takes the
  batch as [sample, reference] pairs: a pair's keys / values are 2L adjacent rows, so a sample entry's attention is
  ``lkgd_attn_spatial_qk`` with ``nbatch`` 1 (Sq = L, S = 2L) on row windows and its reference's ``lkgd_attn_spatial`` on its own L
  rows - K and V are never copied -, and the head runs for the sample entries only.  With the default marker nothing changes.
"""
from __future__ import annotations

import logging
import math
import re
from collections import namedtuple
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import fp8 as fp8_mode
from . import lora as _lora
from . import ops
from ._lib import LkgdHipError
from .lk_fuse import lk_fuse_tokens, pack_lk_tokens
from .module import PackedModule
from .packing import f32, pack_linear
from .unet import QuaternionLinearAutograd, TimestepEmbedding

_log = logging.getLogger(__name__)


@dataclass
class DiTConfig:
    """constructor keywords of CogVideoXTransformer3DModel (cogvideox_transformer_3d.py:224-255) used by the 2B and the 5B
    1.0 models (5B-I2V: 48 heads, 42 layers, in_channels 32, rotary embeddings + a learned position table) and by the 1.5
    models (``patch_size_t`` 2, ``patch_bias`` False, rotary embeddings without a learned table; I2V: ``ofs_embed_dim`` 512)"""
    num_attention_heads: int = 30
    attention_head_dim: int = 64
    in_channels: int = 16
    out_channels: int = 16
    time_embed_dim: int = 512
    text_embed_dim: int = 4096
    num_layers: int = 30
    sample_width: int = 90
    sample_height: int = 60
    sample_frames: int = 49
    patch_size: int = 2
    temporal_compression_ratio: int = 4
    max_text_seq_length: int = 226
    spatial_interpolation_scale: float = 1.875
    temporal_interpolation_scale: float = 1.0
    norm_eps: float = 1e-5
    attention_bias: bool = True
    use_rotary_positional_embeddings: bool = False
    use_learned_positional_embeddings: bool = False
    patch_size_t: Optional[int] = None
    ofs_embed_dim: Optional[int] = None
    patch_bias: bool = True


def check_temporal_config(patch_size_t, ofs_embed_dim, rotary: bool, learned: bool, where: str) -> None:
    """the one released combination of the 1.5 keys is built: ``patch_size_t == 2`` with rotary embeddings and no learned table,
    with or without ``ofs_embed_dim``; every other use of either key raises, naming the key"""
    if ofs_embed_dim and not patch_size_t:
        raise LkgdHipError(f"{where}: ofs_embed_dim={ofs_embed_dim!r} without patch_size_t; the ofs embedding is built for the "
                           "1.5 image-to-video architecture only (patch_size_t 2)")
    if not patch_size_t:
        return
    if patch_size_t != 2:
        raise LkgdHipError(f"{where}: patch_size_t={patch_size_t!r}; the temporal-patch kernels are built for patch_size_t 2")
    if learned:
        raise LkgdHipError(f"{where}: patch_size_t={patch_size_t!r} together with use_learned_positional_embeddings; the 1.5 "
                           "models have no learned position table, the combination is not built")
    if not rotary:
        raise LkgdHipError(f"{where}: patch_size_t={patch_size_t!r} without use_rotary_positional_embeddings; the 1.5 models "
                           "are rotary, a sin-cos table over temporal patches is not built")


def _sincos_1d(embed_dim: int, pos: np.ndarray) -> np.ndarray:
    omega = 1.0 / 10000 ** (np.arange(embed_dim // 2, dtype=np.float64) / (embed_dim / 2.0))
    out = np.einsum("m,d->md", pos.reshape(-1), omega)
    return np.concatenate([np.sin(out), np.cos(out)], axis=1)


def sincos_pos_embed_3d(embed_dim, width, height, frames, spatial_scale, temporal_scale) -> torch.Tensor:
    """[EXT diffusers embeddings.py get_3d_sincos_pos_embed] -> [frames * height * width, D]: temporal quarter, then the
    (h half | w half) of the spatial three quarters"""
    ds, dt = 3 * embed_dim // 4, embed_dim // 4
    gh = np.arange(height, dtype=np.float32) / spatial_scale
    gw = np.arange(width, dtype=np.float32) / spatial_scale
    grid = np.stack(np.meshgrid(gw, gh), axis=0).reshape([2, 1, height, width])
    spatial = np.concatenate([_sincos_1d(ds // 2, grid[0]), _sincos_1d(ds // 2, grid[1])], axis=1)
    temporal = _sincos_1d(dt, np.arange(frames, dtype=np.float32) / temporal_scale)
    pe = np.concatenate([np.repeat(temporal[:, None], height * width, axis=1), np.repeat(spatial[None], frames, axis=0)], axis=-1)
    return torch.from_numpy(pe).float().flatten(0, 1)


def _rope_1d(dim: int, pos: torch.Tensor, theta: float = 10000.0):
    """[EXT diffusers embeddings.py get_1d_rotary_pos_embed, use_real] -> cos, sin [len(pos), dim], every frequency twice"""
    freqs = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float32)[: dim // 2] / dim))
    ang = torch.outer(pos.to(torch.float32), freqs)
    return ang.cos().repeat_interleave(2, dim=1), ang.sin().repeat_interleave(2, dim=1)


def rope_crop_region(grid_h: int, grid_w: int, base_w: int, base_h: int):
    """[EXT diffusers get_resize_crop_region_for_grid((grid_h, grid_w), base_w, base_h)] -> (top, left), (bottom, right): the grid
    resized into the base grid keeping its aspect ratio, centred"""
    if grid_h / grid_w > base_h / base_w:
        rh, rw = base_h, int(round(base_h / grid_h * grid_w))
    else:
        rw, rh = base_w, int(round(base_w / grid_w * grid_h))
    top, left = int(round((base_h - rh) / 2.0)), int(round((base_w - rw) / 2.0))
    return (top, left), (top + rh, left + rw)


def _rope_3d(d: int, gt, gh, gw, frames: int, h: int, w: int):
    """the 1-D tables of the positions gt / gh / gw (the first h / w rows of the height / width tables) expanded over the
    (frames, h, w) grid -> (cos, sin) [frames * h * w, d]"""
    dt, ds = d // 4, d // 8 * 3
    out = []
    for ct, ch, cw in zip(_rope_1d(dt, gt), _rope_1d(ds, gh), _rope_1d(ds, gw)):
        ch, cw = ch[:h], cw[:w]
        out.append(torch.cat([ct[:, None, None, :].expand(frames, h, w, dt), ch[None, :, None, :].expand(frames, h, w, ds),
                              cw[None, None, :, :].expand(frames, h, w, ds)], dim=-1).reshape(frames * h * w, d).contiguous())
    return out[0], out[1]


def rotary_tables(config, frames: int, h: int, w: int):
    """the pipeline's ``_prepare_rotary_positional_embeddings`` for ``patch_size_t is None``
    (pipeline_cogvideox_image2video.py:544-571) -> (cos, sin) fp32 [frames * h * w, attention_head_dim]; frames / h / w are the
    TOKEN grid (latent frames, latent size // patch_size).  PARITY UNPINNED: restates diffusers' [EXT]
    ``get_resize_crop_region_for_grid`` and ``get_3d_rotary_pos_embed`` (linspace grid over the crop region of the configured
    sample grid, theta 10 000): dim/4 temporal channels, then 3 dim/8 for the height and 3 dim/8 for the width (16 + 24 + 24 of
    64), each frequency repeated for the pair (2i, 2i+1) it rotates.  Tested by its properties only.
    With ``config.patch_size_t`` (the 1.5 models) it is the pipeline's ``grid_type="slice"`` branch (:572-584) instead ([EXT]
    ``get_3d_rotary_pos_embed(grid_type="slice", max_size=(max_h, max_w))``): the integer positions 0 .. max - 1 of the configured
    sample grid, the first h (w) rows of their tables - no crop region, no linspace; ``frames`` is then the token grid's
    (latent frames + p_t - 1) // p_t, as the pipeline passes it."""
    d, p = config.attention_head_dim, config.patch_size
    max_h, max_w = config.sample_height // p, config.sample_width // p
    if getattr(config, "patch_size_t", None):
        if h > max_h or w > max_w:
            raise LkgdHipError(f"rotary_tables: a {h} x {w} token grid exceeds the {max_h} x {max_w} (sample_height // patch_size, "
                               "sample_width // patch_size) the 1.5 tables are sliced from")
        gh, gw = torch.arange(max_h, dtype=torch.float32), torch.arange(max_w, dtype=torch.float32)
    else:
        (top, left), (bottom, right) = rope_crop_region(h, w, max_w, max_h)
        gh = torch.linspace(top, bottom * (h - 1) / h, h, dtype=torch.float32)
        gw = torch.linspace(left, right * (w - 1) / w, w, dtype=torch.float32)
    return _rope_3d(d, torch.arange(frames, dtype=torch.float32), gh, gw, frames, h, w)


def pad_for_temporal_patches(latents, image_latents, p_t: Optional[int]):
    """``prepare_latents`` of pipeline_cogvideox_image2video.py for ``patch_size_t`` -> (latents shape or tensor, image_latents)
    with a frame count the temporal patch divides.  ``latents`` as a SHAPE [B, F, C, h, w] (the noise is drawn afterwards) gets
    :383-384's ``F + F % p_t``, arithmetic as written; ``image_latents`` [B, F, C, h, w] gets :416-418: its first ``F % p_t`` frames
    once more at the FRONT.  A latents TENSOR is padded by the rule of the image latents (the pipeline takes given latents as
    they are, already padded).  ``p_t`` None: both returned as they are."""
    if p_t is None:
        return latents, image_latents
    if torch.is_tensor(latents):
        latents = torch.cat([latents[:, : latents.size(1) % p_t, ...], latents], dim=1)
    else:
        shape = tuple(latents)
        latents = shape[:1] + (shape[1] + shape[1] % p_t,) + shape[2:]
    if image_latents is not None:
        first_frame = image_latents[:, : image_latents.size(1) % p_t, ...]
        image_latents = torch.cat([first_frame, image_latents], dim=1)
    return latents, image_latents


def temporal_padding_frames(latent_frames: int, p_t: Optional[int]) -> int:
    """``additional_frames`` of :781-786: how many latent frames the pipeline adds so that ``p_t`` divides the count"""
    if p_t is not None and latent_frames % p_t != 0:
        return p_t - latent_frames % p_t
    return 0


def drop_temporal_padding(latents: torch.Tensor, additional_frames: int) -> torch.Tensor:
    """:907 - the padding frames leave at the front before the VAE decodes"""
    return latents[:, additional_frames:]


# ------------------------------------------------------------------------------------------------ parameter holders
class CogVideoXLayerNormZero(nn.Module):
    def __init__(self, conditioning_dim, embedding_dim, eps):
        super().__init__()
        self.silu = nn.SiLU()
        self.linear = nn.Linear(conditioning_dim, 6 * embedding_dim)
        self.norm = nn.LayerNorm(embedding_dim, eps=eps)


class AdaLayerNorm(nn.Module):
    def __init__(self, embedding_dim, output_dim, eps):
        super().__init__()
        self.silu = nn.SiLU()
        self.linear = nn.Linear(embedding_dim, output_dim)
        self.norm = nn.LayerNorm(output_dim // 2, eps)


class CogVideoXAttnProcessor2_0:
    """[EXT diffusers attention_processor.py] as a MARKER: the attention itself is ``CogVideoXBlock.run``'s launches, and the processor
    an ``Attention`` holds only selects among them.  ``reference_attention`` False: every batch entry attends itself"""
    reference_attention = False


class Attention(nn.Module):
    def __init__(self, dim, heads, head_dim, bias):
        super().__init__()
        self.processor = CogVideoXAttnProcessor2_0()
        if head_dim != 64:
            raise LkgdHipError("the attention kernel is built for head_dim 64")
        self.heads = heads
        self.to_q = nn.Linear(dim, dim, bias=bias)
        self.to_k = nn.Linear(dim, dim, bias=bias)
        self.to_v = nn.Linear(dim, dim, bias=bias)
        self.norm_q = nn.LayerNorm(head_dim, eps=1e-6)
        self.norm_k = nn.LayerNorm(head_dim, eps=1e-6)
        self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])

    def get_processor(self):
        """[EXT diffusers Attention.get_processor]"""
        return self.processor

    def set_processor(self, processor) -> None:
        """[EXT diffusers Attention.set_processor]; a processor is a marker (``CogVideoXAttnProcessor2_0``) - anything else has no
        launches to select and raises"""
        if not isinstance(processor, CogVideoXAttnProcessor2_0):
            raise LkgdHipError(f"set_processor: {type(processor).__qualname__} is no CogVideoXAttnProcessor2_0 marker; the attention "
                               "runs as HIP launches, a processor's own __call__ is never executed")
        self.processor = processor


class GELU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out)


class FeedForward(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.net = nn.ModuleList([GELU(dim, 4 * dim), nn.Dropout(0.0), nn.Linear(4 * dim, dim), nn.Dropout(0.0)])


def pack_block_linear(m, fp8: bool = False):
    """one of a block's six linears as its GEMM reads it: (fp16 [N, K], bias), or in the FP8 mode (e4m3 bytes [N, K], fp32 scale [N],
    bias).  A linear inside a ``lora.Linear`` wrapper packs its folded weight: fp32 ``W + sum_a c_a B_a A_a`` over the wrapper's
    effective adapters (one sum, on the module's device), rounded ONCE to fp16 - in the FP8 mode that fp32 weight goes to
    ``quantize_weight`` (fold, then quantise: what quantising a fused model computes)"""
    bias = f32(m.bias) if m.bias is not None else None
    w = m.effective_weight(m.effective_adapters()) if isinstance(m, _lora.Linear) else m.weight
    if fp8:
        return fp8_mode.quantize_weight(w) + (bias,)
    return pack_linear(w), bias


class CogVideoXBlock(nn.Module):
    def __init__(self, dim, heads, head_dim, time_embed_dim, attention_bias, eps):
        super().__init__()
        self.norm1 = CogVideoXLayerNormZero(time_embed_dim, dim, eps)
        self.attn1 = Attention(dim, heads, head_dim, attention_bias)
        self.norm2 = CogVideoXLayerNormZero(time_embed_dim, dim, eps)
        self.ff = FeedForward(dim)

    def pack(self, fp8: bool = False):
        """``fp8``: the six linears pack as (e4m3 bytes [N, K], fp32 scale [N], bias) and their fp16 copies are not made
        (``pack_block_linear``)"""
        a, f = self.attn1, self.ff

        def lin(m):
            return pack_block_linear(m, fp8)
        self._pk = SimpleNamespace(q=lin(a.to_q), k=lin(a.to_k), v=lin(a.to_v), o=lin(a.to_out[0]),
                                   nq=(f32(a.norm_q.weight), f32(a.norm_q.bias)), nk=(f32(a.norm_k.weight), f32(a.norm_k.bias)),
                                   f1=lin(f.net[0].proj), f2=lin(f.net[2]))

    def run(self, st, X, eff_g, eff_b, gates):
        """the joint rows X [B * L, D] -> the new X.  ``st``: ``forward_rows``' sizes, rotary tables, shard and row format; eff_g /
        eff_b [B, norm (1, 2), stream, D] and gates [norm, B, stream, D]: this block's modulation"""
        bp, rows, B, L, Tt, heads = self._pk, st.rows, st.B, st.L, st.Tt, st.heads
        T, D = X.shape

        def modnorm(which):     # norm(x) * (1 + scale) + shift of both streams -> the operand of the next linears
            n = rows.empty(T, D, X.device)
            for b in range(B):
                for r0, r1, s in ((b * L, b * L + Tt, 0), (b * L + Tt, (b + 1) * L, 1)):
                    rows.norm(X[r0:r1], eff_g[b, which, s], eff_b[b, which, s], st.eps, [t[r0:r1] for t in n])
            return n

        def empty(width=D):
            return torch.empty(T, width, dtype=torch.float16, device=X.device)
        n = modnorm(0)
        q, k, v = empty(), empty(), empty()
        for dst, lin in ((q, bp.q), (k, bp.k), (v, bp.v)):      # one operand feeds the three
            rows.linear(n, lin, dst)
        if st.rope is not None:    # per-head qk norm + rotation of the video rows, q and k in one launch
            ops.qk_norm_rope(q, k, heads, bp.nq, bp.nk, 1e-6, st.rope, L, Tt)
        else:
            ops.layernorm(q.view(T * heads, 64), bp.nq[0], bp.nq[1], 1e-6, out=q.view(T * heads, 64))     # per-head qk norm
            ops.layernorm(k.view(T * heads, 64), bp.nk[0], bp.nk[1], 1e-6, out=k.view(T * heads, 64))
        a = empty()
        if st.pairs and self.attn1.processor.reference_attention:
            # the batch is [sample, its reference] pairs (``forward_rows``): a pair's keys / values are 2L adjacent rows, so a sample
            # entry's L queries read them in place (Sq = L, S = 2L) and its reference entry attends its own L rows
            for b in range(0, B, 2):
                s0, r0, r1 = b * L, (b + 1) * L, (b + 2) * L
                ops.attn_spatial(q[s0:r0], k[s0:r1], v[s0:r1], a[s0:r0], 1, 2 * L, heads, Sq=L)
                ops.attn_spatial(q[r0:r1], k[r0:r1], v[r0:r1], a[r0:r1], 1, L, heads)
        elif st.shard is None:
            ops.attn_spatial(q, k, v, a, B, L, heads)
        else:                   # keys / values of every frame of this CFG half: text rows (replicated) + gathered video rows
            for full, loc in zip(st.KV, (k, v)):
                full[:Tt].copy_(loc[:Tt])
                full[Tt:].copy_(st.shard.gather(loc[Tt:]))
            ops.attn_spatial(q, st.KV[0], st.KV[1], a, 1, st.KV[0].shape[0], heads, Sq=L)
        o = empty()
        rows.linear(rows.of(a), bp.o, o)
        X = ops.gated_add(o, gates[0].reshape(2 * B, D), X, L, Tt)
        hdn = empty(4 * D)
        rows.linear(modnorm(1), bp.f1, hdn)
        rows.linear(rows.gelu(hdn), bp.f2, o)
        return ops.gated_add(o, gates[1].reshape(2 * B, D), X, L, Tt)


# the five places where the fp16 and the FP8 block differ.  A block linear's operand is a tuple: (fp16 rows,) for ``ops.gemm`` over
# (w, bias), or (e4m3 bytes, a scale per row) from the kernel that produces the rows, for ``ops.gemm_fp8`` over (bytes, scale, bias)
_FP16_ROWS = SimpleNamespace(
    empty=lambda T, D, dev: (torch.empty(T, D, dtype=torch.float16, device=dev),),
    norm=lambda x, gamma, beta, eps, out: ops.layernorm(x, gamma, beta, eps, out=out[0]),
    linear=lambda n, lin, out: ops.gemm(n[0], lin[0], out, M=out.shape[0], N=out.shape[1], K=n[0].shape[1], bias=lin[1]),
    of=lambda a: (a,),
    gelu=lambda hdn: (ops.gelu_tanh_(hdn),))
_FP8_ROWS = SimpleNamespace(
    empty=lambda T, D, dev: (torch.empty(T, D, dtype=torch.uint8, device=dev), torch.empty(T, dtype=torch.float32, device=dev)),
    norm=lambda x, gamma, beta, eps, out: ops.layernorm_quant_fp8(x, gamma, beta, eps, q=out[0], scale=out[1]),
    linear=lambda n, lin, out: ops.gemm_fp8(*n, *lin, out=out),
    of=ops.quant_rows_fp8,
    gelu=ops.gelu_tanh_quant_fp8)       # GELU and Q in one pass over the hidden rows


class CogVideoXPatchEmbed(nn.Module):
    def __init__(self, cfg: DiTConfig, dim: int):
        super().__init__()
        if cfg.patch_size_t is None:
            self.proj = nn.Conv2d(cfg.in_channels, dim, kernel_size=(cfg.patch_size, cfg.patch_size), stride=cfg.patch_size,
                                  bias=cfg.patch_bias)
        else:       # [EXT diffusers CogVideoXPatchEmbed, 1.5]: a Linear over a patch's (c, pt, py, px) columns
            self.proj = nn.Linear(cfg.in_channels * cfg.patch_size * cfg.patch_size * cfg.patch_size_t, dim, bias=cfg.patch_bias)
        self.text_proj = nn.Linear(cfg.text_embed_dim, dim)
        if cfg.use_learned_positional_embeddings:
            # [EXT diffusers CogVideoXPatchEmbed]: a persistent buffer over the JOINT sequence (text rows included), present in
            # the checkpoint; initialised as diffusers does, with the sin-cos table under zero text rows
            f = (cfg.sample_frames - 1) // cfg.temporal_compression_ratio + 1
            h, w = cfg.sample_height // cfg.patch_size, cfg.sample_width // cfg.patch_size
            joint = torch.zeros(1, cfg.max_text_seq_length + f * h * w, dim)
            if joint.device.type != "meta":
                joint[0, cfg.max_text_seq_length:] = sincos_pos_embed_3d(dim, w, h, f, cfg.spatial_interpolation_scale,
                                                                         cfg.temporal_interpolation_scale)
            self.register_buffer("pos_embedding", joint, persistent=True)


@dataclass
class Transformer2DModelOutput:
    sample: torch.Tensor


class CogVideoXTransformer3DModel(PackedModule):
    def __init__(self, config: Optional[DiTConfig] = None, **kw):
        super().__init__()
        cfg = config if config is not None else DiTConfig(**kw)
        self.config = SimpleNamespace(**cfg.__dict__)
        if not cfg.use_rotary_positional_embeddings and cfg.use_learned_positional_embeddings:
            raise ValueError(                                                                   # cogvideox_transformer_3d.py:258-263
                "There are no CogVideoX checkpoints available with disable rotary embeddings and learned positional "
                "embeddings. If you're using a custom model and/or believe this should be supported, please open an "
                "issue at https://github.com/huggingface/diffusers/issues.")
        check_temporal_config(cfg.patch_size_t, cfg.ofs_embed_dim, cfg.use_rotary_positional_embeddings,
                              cfg.use_learned_positional_embeddings, "CogVideoXTransformer3DModel")
        if cfg.ofs_embed_dim and cfg.ofs_embed_dim != cfg.time_embed_dim:
            raise LkgdHipError(f"CogVideoXTransformer3DModel: ofs_embed_dim={cfg.ofs_embed_dim} is added to the time embedding "
                               f"and has to equal time_embed_dim={cfg.time_embed_dim}")
        d = cfg.num_attention_heads * cfg.attention_head_dim
        pt = cfg.patch_size_t or 1
        if d % 64 or (cfg.in_channels * cfg.patch_size ** 2 * pt) % 64 or cfg.time_embed_dim % 64 or cfg.text_embed_dim % 64 \
                or d > 3072 or (cfg.patch_size ** 2 * pt * cfg.out_channels) % 8:
            raise LkgdHipError("DiT on the HIP path: dims multiples of 64 (K granularity), inner dim <= 3072")
        self.inner_dim = d
        self.patch_embed = CogVideoXPatchEmbed(cfg, d)
        self.time_embedding = TimestepEmbedding(d, cfg.time_embed_dim)
        # cogvideox_transformer_3d.py:290-296: the sinusoid of ``ofs`` has ofs_embed_dim channels, the MLP keeps that width
        self.ofs_embedding = TimestepEmbedding(cfg.ofs_embed_dim, cfg.ofs_embed_dim) if cfg.ofs_embed_dim else None
        self.transformer_blocks = nn.ModuleList([
            CogVideoXBlock(d, cfg.num_attention_heads, cfg.attention_head_dim, cfg.time_embed_dim, cfg.attention_bias,
                           cfg.norm_eps) for _ in range(cfg.num_layers)])
        self.norm_final = nn.LayerNorm(d, cfg.norm_eps)
        self.norm_out = AdaLayerNorm(cfg.time_embed_dim, 2 * d, cfg.norm_eps)
        self.proj_out = nn.Linear(d, cfg.patch_size * cfg.patch_size * pt * cfg.out_channels)              # :326-333
        self.init_quaternion_modules()
        #: None, or "fp8" after ``lkgd_amd.fp8.quantize_to_float8`` (the block linears then pack and run as e4m3)
        self.quantization = None
        self._pos = {}

    def init_quaternion_modules(self):
        """cogvideox_transformer_3d.py:337-366 (the reference calls it after construction; here the modules always exist)"""
        self.quaternion_lora_dconv = nn.Conv1d(1024, 256, 1, groups=256, bias=False)
        self.quaternion_lora_lconv = nn.Conv1d(4096, 256, 1, groups=256, bias=False)
        self.quaternion_lora_fconv = nn.Conv1d(1024, 256, 1, groups=256, bias=False)
        self.quaternion_lora_fuse = QuaternionLinearAutograd(1024, 512)
        self.quaternion_lora_fuse_fft_mag = QuaternionLinearAutograd(512, 256)
        self.quaternion_lora_fuse_fft_pha = QuaternionLinearAutograd(512, 256)
        self.quaternion_lora_fuse_fft_mag0 = nn.Linear(4, 1)
        self.quaternion_lora_fuse_fft_pha0 = nn.Linear(4, 1)
        self.quaternion_lora_fuse_sf = nn.Sequential(nn.Linear(1024, 512), nn.LeakyReLU(0.1, inplace=True), nn.Linear(512, 4096))
        self.quaternion_lora_texts = nn.Parameter(torch.zeros(256))
        self.quaternion_lora_texts_fft_mag = nn.Parameter(torch.zeros(129))
        self.quaternion_lora_texts_fft_pha = nn.Parameter(torch.zeros(129))

    # ---- bookkeeping -------------------------------------------------------------------------------------------
    OFF_GPU = "lkgd_amd DiT runs on MI355X only: move the module to cuda first"
    config_class = DiTConfig
    #: lkgd_amd.lora: the modules adapters fold into (``CogVideoXBlock.pack``), and the sentence for every other key
    lora_targetable = (re.compile(r"^transformer_blocks\.\d+\.(attn1\.(to_q|to_k|to_v|to_out\.0)|ff\.net\.(0\.proj|2))$"),
                       "the DiT folds adapters into the six block linears (attn1.to_q / to_k / to_v / to_out.0, ff.net.0.proj, "
                       "ff.net.2 of transformer_blocks.<i>) only")

    # ---- LoRA adapters (lkgd_amd/lora.py).  Module state only: all of it works before ``.to("cuda")`` -------
    def load_lora_adapter(self, state_dict, adapter_name: Optional[str] = None, network_alphas=None):
        """diffusers' ``transformer.load_lora_adapter`` [EXT] for a state dict whose ``transformer.`` prefix is already stripped:
        ``<module>.lora_A.weight`` / ``.lora_B.weight`` pairs become the adapter ``adapter_name`` (default ``default_<n>``) on
        ``lora.Linear`` wrappers - rank per module from ``lora_B.shape[1]``, ``lora_alpha = r`` (scaling 1.0) unless
        ``network_alphas`` names one; the trainer's alpha / rank enters through ``fuse_lora(lora_scale=)`` or ``set_adapters``' weights,
        as the reference's tools pass it.  ``quaternion_lora_*`` keys replace the module's own parameters (shape-checked).  Every key
        is checked before anything changes; a key naming any other module raises and names it.  Returns the ``quaternion_lora_*``
        state-dict names the dict did NOT hold (they stay as they are; logged once per call)."""
        have = _lora.adapter_names(self)
        if adapter_name is None:
            n = 0
            while f"default_{n}" in have:
                n += 1
            adapter_name = f"default_{n}"
        if adapter_name in have:
            raise ValueError(f"Adapter name '{adapter_name}' already in use in the model - please select a new adapter name.")
        own = {k: v for k, v in self.state_dict().items() if k.startswith("quaternion_lora_")}
        lk = {k: v for k, v in state_dict.items() if k.startswith("quaternion_lora_")}
        for k, v in lk.items():
            if k not in own:
                raise LkgdHipError(f"LoRA file key '{k}': the model has no such latent-knowledge parameter")
            if tuple(v.shape) != tuple(own[k].shape):
                raise ValueError(f"LoRA file key '{k}' has shape {tuple(v.shape)}, the model's parameter {tuple(own[k].shape)}")
        rest = {k: v for k, v in state_dict.items() if k not in lk}
        if rest:
            _lora.load_lora_into_model(rest, network_alphas, self, adapter_name, prefix="transformer.")
        elif not lk:
            raise ValueError("empty LoRA state dict")
        with torch.no_grad():
            for k, v in lk.items():
                own[k].copy_(v)         # state_dict() tensors share the parameters' storage
        self.invalidate()
        absent = sorted(k for k in own if k not in lk)
        if absent:
            _log.warning("load_lora_adapter('%s'): %d quaternion_lora_* tensors are not in the file and stay as they are: %s",
                         adapter_name, len(absent), ", ".join(absent))
        return absent

    def set_adapters(self, adapter_names, weights=None):
        """``transformer.set_adapters`` [EXT PeftAdapterMixin]: the named adapters are the active ones, ``weights`` scale them"""
        _lora.set_adapters(self, adapter_names, weights)

    def fuse_lora(self, lora_scale: float = 1.0, adapter_names=None):
        """[EXT] ``fuse_lora``.  The base parameters are never written while adapters are present: the fused adapters are marked, and
        the pack folds ``W + sum_a c_a B_a A_a`` with c_a = set_adapters weight x ``lora_scale`` x lora_alpha_a / r_a.  So
        ``unfuse_lora`` restores the base forward to the bit; peft's fp16 add followed by a subtract does not."""
        _lora.fuse(self, lora_scale, adapter_names)

    def unfuse_lora(self):
        _lora.unfuse(self)

    def enable_lora(self):
        _lora.set_enabled(self, True)

    def disable_lora(self):
        _lora.set_enabled(self, False)

    def unload_lora(self):
        """[EXT] ``unload_lora``: while fused the base weights take the fp16 values of the fold first (fuse-then-unload); otherwise
        they stay as they were.  The state-dict names are the stock ones afterwards"""
        _lora.unload(self)

    def active_adapters(self):
        """the adapters the next pack folds, in order"""
        seen = []
        for _, m in _lora.lora_layers(self):
            if not m.disable_adapters:
                seen += [a for a in m.effective_adapters() if a not in seen]
        return seen

    def lora_coefficients(self):
        """{module name: {adapter: c}} of ``W + sum_a c_a B_a A_a`` as the next pack folds it"""
        return {n: ({} if m.disable_adapters else {a: m.coefficient(a) for a in m.effective_adapters()})
                for n, m in _lora.lora_layers(self)}

    def _forget(self):
        self._pos = {}                  # sin-cos tables in the module's device

    @classmethod
    def _build_options(cls, **_ignored):
        return {"strict": False}        # from_pretrained checks the keys itself

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, subfolder: Optional[str] = None, torch_dtype=None,
                        variant: Optional[str] = None, **kw):
        from .loading import load_config, load_state_dict
        raw = load_config(pretrained_model_name_or_path, subfolder)
        # before any weight is read: of the 1.5 keys only the released combination is built
        check_temporal_config(raw.get("patch_size_t"), raw.get("ofs_embed_dim"), bool(raw.get("use_rotary_positional_embeddings")),
                              bool(raw.get("use_learned_positional_embeddings")), "CogVideoXTransformer3DModel.from_pretrained")
        # stock checkpoints have no quaternion_lora_* modules: those may be missing; anything else missing or unexpected
        # (a truncated shard, renamed parameters) would leave meta-initialised garbage behind a non-strict load
        sd_keys = set(load_state_dict(pretrained_model_name_or_path, subfolder, variant).keys())
        m = super().from_pretrained(pretrained_model_name_or_path, subfolder, torch_dtype, variant, **kw)
        own = set(m.state_dict().keys())
        missing = sorted(k for k in own - sd_keys if not k.startswith("quaternion_lora_"))
        unexpected = sorted(sd_keys - own)
        if missing or unexpected:
            raise RuntimeError(f"CogVideoXTransformer3DModel.from_pretrained({pretrained_model_name_or_path!r}): missing keys "
                               f"{missing[:5]}{'...' if len(missing) > 5 else ''}, unexpected keys {unexpected[:5]}"
                               f"{'...' if len(unexpected) > 5 else ''}")
        return m

    def _saved_config(self):
        return {k: v for k, v in self.config.__dict__.items() if k in DiTConfig.__dataclass_fields__}

    def _check_packable(self):
        if fp8_mode.active(self) and self.inner_dim % 128:
            raise LkgdHipError(f"the FP8 mode (quantize_to_float8 / LKGD_DIT_FP8) tiles N and K by 128: inner dim {self.inner_dim} is "
                               "not a multiple")

    def _pack(self):
        fp8 = fp8_mode.active(self)
        for b in self.transformer_blocks:
            b.pack(fp8)
        self.time_embedding.pack()
        if self.ofs_embedding is not None:
            self.ofs_embedding.pack()
        pk = SimpleNamespace(fp8=fp8)
        # every block's two modulation linears as ONE [blocks * 2 * 6D, Te] GEMM per step (+ norm_out's [2D, Te])
        mods = [m for b in self.transformer_blocks for m in (b.norm1.linear, b.norm2.linear)] + [self.norm_out.linear]
        pk.w_mod = torch.cat([pack_linear(m.weight) for m in mods], dim=0).contiguous()
        pk.b_mod = torch.cat([f32(m.bias) for m in mods]).contiguous()
        nb = len(self.transformer_blocks)
        pk.ln_g = torch.stack([torch.stack([f32(b.norm1.norm.weight), f32(b.norm2.norm.weight)]) for b in self.transformer_blocks])
        pk.ln_b = torch.stack([torch.stack([f32(b.norm1.norm.bias), f32(b.norm2.norm.bias)]) for b in self.transformer_blocks])
        pk.nb = nb
        pk.fin = (f32(self.norm_final.weight), f32(self.norm_final.bias))
        pk.out_g, pk.out_b = f32(self.norm_out.norm.weight), f32(self.norm_out.norm.bias)
        pe = self.patch_embed
        # [D, C*p*p], k = (c, ky, kx); temporal patches: [D, C*p_t*p*p], k = (c, pt, ky, kx) - both the order of the weight itself
        pk.w_pe, pk.b_pe = pack_linear(pe.proj.weight.detach()), (f32(pe.proj.bias) if pe.proj.bias is not None else None)
        pk.w_tx, pk.b_tx = pack_linear(pe.text_proj.weight), f32(pe.text_proj.bias)
        pk.w_po, pk.b_po = pack_linear(self.proj_out.weight), f32(self.proj_out.bias)
        pk.learned = pe.pos_embedding[0].detach().to(torch.float16).contiguous() if self.config.use_learned_positional_embeddings else None
        return pk

    def _learned_table(self, Tt: int, f: int, h: int, w: int) -> torch.Tensor:
        """the learned joint table [max_text_seq_length + T h w, D] fp16; it has rows for the configured grid only, so any
        other clip raises (diffusers raises for another resolution and silently falls back to the sin-cos table for another
        frame count; here both are refused)"""
        c = self.config
        want = (c.max_text_seq_length, (c.sample_frames - 1) // c.temporal_compression_ratio + 1, c.sample_height // c.patch_size,
                c.sample_width // c.patch_size)
        if (Tt, f, h, w) != want:
            raise ValueError(f"learned positional embeddings cover (text, frames, h, w) tokens = {want} only, got {(Tt, f, h, w)}: "
                             "it is not possible to run a clip of another size with this checkpoint")
        return self._pk.learned

    def _pos_table(self, f: int, h: int, w: int) -> torch.Tensor:
        key = (f, h, w)
        t = self._pos.get(key)
        if t is None:
            c = self.config
            t = sincos_pos_embed_3d(self.inner_dim, w, h, f, c.spatial_interpolation_scale, c.temporal_interpolation_scale)
            t = self._pos[key] = t.to(device=self.device, dtype=torch.float16).contiguous()
        return t

    # ---- latent-knowledge fuse on the text embeddings (:519-582), once per clip -----------------------------------
    @torch.no_grad()
    def fused_text(self, encoder_hidden_states, domain_features, flow_features) -> torch.Tensor:
        """[B, L, 4096] prompt embeddings, [1 or B, 1, 1000] domain / flow logits -> fp16 [B, L, 4096]: one launch of
        ``lkgd_lk_fuse_tokens`` over operands packed once per weight version"""
        if self.device.type != "cuda":
            raise LkgdHipError("the latent-knowledge fuse runs on the GPU (lkgd_amd has no CPU path)")
        if self.config.text_embed_dim != 4096:
            raise LkgdHipError(f"the latent-knowledge fuse is built for text_embed_dim 4096, got {self.config.text_embed_dim}")
        if encoder_hidden_states.dim() != 3 or encoder_hidden_states.shape[2] != 4096:
            raise LkgdHipError(f"fused_text: encoder_hidden_states must be [batch, tokens, 4096], got "
                               f"{tuple(encoder_hidden_states.shape)}")
        self.prepare()
        pk = self._pk
        if getattr(pk, "lk_tokens", None) is None:
            pk.lk_tokens = pack_lk_tokens(self)
        return lk_fuse_tokens(pk.lk_tokens, encoder_hidden_states, domain_features, flow_features)

    # ---- the per-step forward ------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_tokens(self, hidden_states: torch.Tensor, fused_text: torch.Tensor, timestep, shard=None,
                       image_rotary_emb=None, ofs=None) -> torch.Tensor:
        """hidden_states [B, F, C, h, w]; fused_text [B, L, 4096] fp16 (``fused_text`` of the prompt embeddings) ->
        [B, F, out_channels, h, w] fp16: patch unfold, ``forward_rows``, un-patchify (two torch permutes at the API edge).
        ``ofs``: a scalar or a [1] / [B] tensor, exactly when the model has an ``ofs_embedding``."""
        B, Fr, C_, H, W = hidden_states.shape
        p, pt = self.config.patch_size, self.config.patch_size_t or 1
        h, w = H // p, W // p
        if (self.ofs_embedding is None) != (ofs is None):
            raise LkgdHipError("ofs is given exactly when the model has an ofs_embedding (config ofs_embed_dim)")
        if Fr % pt:
            raise LkgdHipError(f"patch_size_t {pt} does not divide the {Fr} latent frames: pad_for_temporal_patches first")
        extra = dict(ofs_emb=self.embed_ofs(ofs, B)) if ofs is not None else {}
        xh = hidden_states.to(device=self.device, dtype=torch.float16)
        pair = None
        if any(b.attn1.processor.reference_attention for b in self.transformer_blocks):
            # the script's batch [samples | references] (ddim_inversion.py:212-215) -> ``forward_rows``' pairs, and back: host indexing
            if B % 2:
                raise LkgdHipError(f"reference attention (CogVideoXAttnProcessor2_0ForDDIMInversion): the batch is [sample | reference] "
                                   f"entries and has to be even, got {B}")
            pair = torch.arange(B, device=self.device).reshape(2, B // 2).t().reshape(-1)
            xh, fused_text = xh[pair], fused_text.to(self.device)[pair]
            if torch.is_tensor(timestep) and timestep.numel() == B:
                timestep = timestep.to(self.device).reshape(-1)[pair]
            extra["reference_rows"] = True
        # [EXT diffusers CogVideoXPatchEmbed, 1.5] (column (c, pt, py, px)), and cogvideox_transformer_3d.py:626-630; with pt = 1
        # bit for bit the 2-D unfold (column (c, py, px)) and un-patchify of :624-625
        patches = xh.permute(0, 1, 3, 4, 2).reshape(B, Fr // pt, pt, h, p, w, p, C_).permute(0, 1, 3, 5, 7, 2, 4, 6) \
            .flatten(4, 7).flatten(1, 3).reshape(B * (Fr // pt) * h * w, C_ * pt * p * p).contiguous()
        out_tok = self.forward_rows(patches, (Fr // pt, h, w), fused_text, timestep, shard=shard, image_rotary_emb=image_rotary_emb,
                                    **extra)
        out = out_tok.reshape(B, Fr // pt, h, w, -1, pt, p, p).permute(0, 1, 5, 4, 2, 6, 3, 7).flatten(6, 7).flatten(4, 5).flatten(1, 2)
        if pair is not None:
            out = out[torch.argsort(pair)]
        return out.contiguous()

    @torch.no_grad()
    def embed_ofs(self, ofs, batch: int) -> torch.Tensor:
        """cogvideox_transformer_3d.py:513-516: ``ofs`` (a scalar or a [1] / [batch] tensor) -> ofs_embedding(ofs_proj(ofs)) fp16
        [batch, ofs_embed_dim]; the sinusoid leaves the timestep-embedding kernel in fp16 (the cast of :515), the MLP is the two
        small GEMMs of the time embedding.  Step-invariant: ``denoise`` calls it once per clip."""
        if self.ofs_embedding is None:
            raise LkgdHipError("ofs: this model has no ofs_embedding (config ofs_embed_dim)")
        self.prepare()
        o = ofs if torch.is_tensor(ofs) else torch.tensor([float(ofs)])
        o = o.to(device=self.device, dtype=torch.float32).reshape(-1)
        if o.numel() not in (1, batch):
            raise LkgdHipError(f"ofs must be a scalar or have 1 or {batch} entries, got {o.numel()}")
        return self.ofs_embedding.run(ops.timestep_embedding(o.expand(batch).contiguous(), self.config.ofs_embed_dim))

    @torch.no_grad()
    def forward_rows(self, patch_rows: torch.Tensor, grid, fused_text: torch.Tensor, timestep, shard=None,
                     image_rotary_emb=None, ofs_emb=None, reference_rows: bool = False) -> torch.Tensor:
        """the row-level core.  ``patch_rows`` fp16 [Bv * Tv, in_channels * p * p] (``ops.dit_patch_rows``; column (c, py, px)),
        ``grid`` = (F, h, w) tokens, Tv = F h w; fused_text [B, L, 4096] fp16.  Bv divides B: batch entry b embeds the rows of
        entry b % Bv, so ONE copy of the rows (Bv = 1) serves both CFG entries, as ``torch.cat([latents] * 2)`` did.  Returns
        proj_out's token rows [B * Tv, out_channels * p * p] fp16 (before the un-patchify).
        ``image_rotary_emb`` = (cos, sin) fp32 [F h w tokens, 64] (``rotary_tables``) exactly when the model is rotary.
        ``shard`` (lkgd_amd.dist_run.ShardInfo): this rank holds ONE batch entry (its CFG half) and the latent frames [f0, f0 + F)
        of the clip; everything is row-local except the attention, whose local queries (the replicated text rows + the rank's video
        rows) attend to the keys / values of ALL frames, all-gathered over the frame group every layer (``CogVideoXBlock.run``).
        A ``patch_size_t`` model: ``patch_rows`` [Bv * Tv, in_channels * p_t * p * p] (``ops.dit_patch_rows(p_t=)``; column
        (c, pt, py, px)), ``grid`` = (F / p_t, h, w), the result [B * Tv, out_channels * p_t * p * p]; ``ofs_emb`` fp16
        [B, time_embed_dim] (``embed_ofs``) exactly when the model has an ``ofs_embedding``: added to the time embedding in fp16
        (:517) before the modulation GEMM.
        Reference attention (``lkgd_amd.ddim_inversion.OverrideAttnProcessors``): while a block's ``attn1`` holds
        a processor with ``reference_attention``, the batch is PAIRS - entry 2i a sample, entry 2i + 1 its reference
        (``[u, ref_u, c, ref_c]`` under guidance; ``patch_rows`` with Bv = 2: ``[sample rows | reference rows]``, text
        ``[neg, neg, pos, pos]``).  In such a block a sample entry's queries attend its own L rows followed by its reference's L rows -
        adjacent rows of k and v, read in place - and a reference entry attends itself; everything else is row-local.  The result holds
        the SAMPLE entries' rows only, [(B / 2) * Tv, ...] contiguous (what the step kernel takes), or with ``reference_rows`` every
        entry's, in the pair order.  An odd batch, a non-rotary model, a ``patch_size_t`` model, a frame shard and the FP8 mode raise."""
        st = self._check_rows(patch_rows, grid, fused_text, shard, image_rotary_emb, ofs_emb)
        eff_g, eff_b, gates, fin = self._modulation(timestep, st.B, ofs_emb)
        X = self._embed_rows(st, patch_rows, fused_text)
        for i, block in enumerate(self.transformer_blocks):
            X = block.run(st, X, eff_g[:, i], eff_b[:, i], gates[i])
        # under reference attention the loop reads the sample entries' prediction only (ddim_inversion.py:416-417)
        return self._head(st, X, fin, range(0, st.B, 2) if st.pairs and not reference_rows else range(st.B))

    def _check_rows(self, patch_rows, grid, fused_text, shard, image_rotary_emb, ofs_emb):
        """``forward_rows``' argument checks -> the call's sizes, shard window, rotary tables and row format"""
        if shard is not None and fp8_mode.active(self):
            raise LkgdHipError("frame sharding together with the FP8 mode (quantize_to_float8 / LKGD_DIT_FP8) is not built")
        self.prepare()
        pk, cfg, dev = self._pk, self.config, self.device
        B = fused_text.shape[0]
        Fr, h, w = grid
        if shard is not None and cfg.patch_size_t is not None:
            raise LkgdHipError("frame sharding of a patch_size_t (CogVideoX 1.5) model is not built")
        if (self.ofs_embedding is None) != (ofs_emb is None):
            raise LkgdHipError("ofs_emb (embed_ofs) is given exactly when the model has an ofs_embedding (config ofs_embed_dim)")
        if shard is not None and B != 1:
            raise LkgdHipError("frame sharding of the DiT supports one batch entry per rank")
        Tt, Tv = fused_text.shape[1], Fr * h * w
        Kp = pk.w_pe.shape[1]
        pairs = any(b.attn1.processor.reference_attention for b in self.transformer_blocks)
        if pairs:
            what = "reference attention (CogVideoXAttnProcessor2_0ForDDIMInversion)"
            if not cfg.use_rotary_positional_embeddings:
                raise NotImplementedError("This script supports CogVideoX 5B model only.")               # ddim_inversion.py:477-478
            if cfg.patch_size_t is not None:
                raise LkgdHipError(f"{what} of a patch_size_t (CogVideoX 1.5) model is not built")
            if shard is not None:
                raise LkgdHipError(f"{what} together with frame sharding is not built")
            if pk.fp8:
                raise LkgdHipError(f"{what} together with the FP8 mode (quantize_to_float8 / LKGD_DIT_FP8) is not built")
            if B % 2:
                raise LkgdHipError(f"{what}: the batch is [sample | reference] entries and has to be even, got {B}")
        if patch_rows.dim() != 2 or patch_rows.dtype != torch.float16 or patch_rows.device != dev or patch_rows.shape[1] != Kp \
                or patch_rows.shape[0] % Tv or patch_rows.shape[0] == 0 or B % (patch_rows.shape[0] // Tv) \
                or patch_rows.stride(1) != 1:
            raise LkgdHipError(f"forward_rows: patch_rows must be GPU fp16 [Bv * {Tv}, {Kp}] with Bv a divisor of the batch {B}, got "
                               f"{tuple(patch_rows.shape)} {patch_rows.dtype}")
        rotary = cfg.use_rotary_positional_embeddings
        if rotary != (image_rotary_emb is not None):
            raise LkgdHipError("image_rotary_emb is given exactly when the model has use_rotary_positional_embeddings "
                               "(rotary_tables builds it)")
        rope = None
        F_all = Fr if shard is None else shard.F_total          # latent frames of the whole clip
        v0 = 0 if shard is None else shard.f0 * h * w            # the rank's first video row in the clip
        if rotary:
            # to the device once per call; every layer reads the same two tables.  A frame-sharded rank is handed the tables of
            # the WHOLE clip and rotates its local q and k (before the K gather) with the rows of its frames
            rope = tuple(t.to(device=dev, dtype=torch.float32) for t in image_rotary_emb)
            if any(tuple(t.shape) != (F_all * h * w, 64) for t in rope):
                raise LkgdHipError(f"image_rotary_emb: (cos, sin) must each be [{F_all * h * w}, 64], got "
                                   f"{[tuple(t.shape) for t in rope]}")
            rope = tuple(t[v0:v0 + Tv].contiguous() for t in rope)
        KV = [] if shard is None else [torch.empty(Tt + F_all * h * w, self.inner_dim, dtype=torch.float16, device=dev) for _ in range(2)]
        return SimpleNamespace(B=B, Bv=patch_rows.shape[0] // Tv, Tt=Tt, Tv=Tv, L=Tt + Tv, grid=(F_all, h, w), v0=v0, rope=rope, KV=KV,
                               shard=shard, pairs=pairs, heads=cfg.num_attention_heads, eps=cfg.norm_eps, rows=_FP8_ROWS if pk.fp8 else _FP16_ROWS)

    def _modulation(self, timestep, B: int, ofs_emb):
        """time embedding (+ ``ofs_emb``) -> the step's modulation (one GEMM), fp32: the effective affine of norm(x) * (1 + scale) +
        shift, eff_g / eff_b [B, nb, 2, stream (0 text, 1 video), D]; gates [nb, 2, B, stream, D]; norm_out's (shift, scale) [B, 2, D]"""
        pk, dev, D = self._pk, self.device, self.inner_dim
        t = timestep if torch.is_tensor(timestep) else torch.tensor([timestep])
        t = t.to(device=dev, dtype=torch.float32).reshape(-1).expand(B).contiguous()
        emb = self.time_embedding.run(ops.timestep_embedding(t, D))
        if ofs_emb is not None:
            if ofs_emb.dtype != torch.float16 or tuple(ofs_emb.shape) != tuple(emb.shape) or not ofs_emb.is_contiguous():
                raise LkgdHipError(f"ofs_emb must be contiguous fp16 {tuple(emb.shape)} (embed_ofs), got {tuple(ofs_emb.shape)} "
                                   f"{ofs_emb.dtype}")
            emb = ops.add(emb, ofs_emb)
        semb = ops.silu(emb)
        mod = torch.empty(B, pk.w_mod.shape[0], dtype=torch.float16, device=dev)
        ops.gemm(semb, pk.w_mod, mod, M=B, N=pk.w_mod.shape[0], K=pk.w_mod.shape[1], bias=pk.b_mod)
        mod = mod.float()
        nb = pk.nb
        blk = mod[:, :nb * 12 * D].reshape(B, nb, 2, 6, D)            # (shift, scale, gate, enc_shift, enc_scale, enc_gate)
        g, be = pk.ln_g[None], pk.ln_b[None]                          # [1, nb, 2, D]
        eff_g = torch.stack([g * (1 + blk[:, :, :, 4]), g * (1 + blk[:, :, :, 1])], dim=3).contiguous()
        eff_b = torch.stack([be * (1 + blk[:, :, :, 4]) + blk[:, :, :, 3], be * (1 + blk[:, :, :, 1]) + blk[:, :, :, 0]], dim=3).contiguous()
        gates = torch.stack([blk[:, :, :, 5], blk[:, :, :, 2]], dim=3).permute(1, 2, 0, 3, 4).contiguous()
        return eff_g, eff_b, gates, mod[:, nb * 12 * D:].reshape(B, 2, D)

    def _embed_rows(self, st, patch_rows, fused_text):
        """the two embedding GEMMs into the joint buffer [B * L, D]: text rows, then video rows (+ position table in the epilogue)"""
        pk, cfg, dev, D = self._pk, self.config, self.device, self.inner_dim
        B, Bv, Tt, Tv, L, v0 = st.B, st.Bv, st.Tt, st.Tv, st.L, st.v0
        X = torch.empty(B * L, D, dtype=torch.float16, device=dev)
        txt = fused_text.to(device=dev, dtype=torch.float16).reshape(B * Tt, -1).contiguous()
        pos_txt = pos = None
        if not cfg.use_rotary_positional_embeddings:
            pos = self._pos_table(*st.grid)[v0:v0 + Tv]
        elif cfg.use_learned_positional_embeddings:     # the learned joint table covers the text rows as well
            tab = self._learned_table(Tt, *st.grid)
            pos_txt, pos = tab[:Tt], tab[Tt + v0:Tt + v0 + Tv]
        rb_t, rb_v = (dict(rowbias=t, rowmap=(1, 1, 1, 1 << 30)) if t is not None else {} for t in (pos_txt, pos))
        for b in range(B):
            ops.gemm(txt[b * Tt:(b + 1) * Tt], pk.w_tx, X[b * L:b * L + Tt], M=Tt, N=D, K=txt.shape[1], bias=pk.b_tx, **rb_t)
            ops.gemm(patch_rows[(b % Bv) * Tv:(b % Bv + 1) * Tv], pk.w_pe, X[b * L + Tt:(b + 1) * L], M=Tv, N=D, K=pk.w_pe.shape[1],
                     bias=pk.b_pe, **rb_v)
        return X

    def _head(self, st, X, fin, entries):
        """norm_final on the video stream, norm_out (adaLN), proj_out of the batch ``entries`` -> [len(entries) * Tv, out_channels * p * p]"""
        pk, L, Tt, Tv = self._pk, st.L, st.Tt, st.Tv
        po = pk.w_po.shape[0]
        B = len(entries)
        out_tok = torch.empty(B, Tv, po, dtype=torch.float16, device=X.device)
        for o, b in enumerate(entries):
            vid = X[b * L + Tt:(b + 1) * L]
            y = ops.layernorm(vid, pk.fin[0], pk.fin[1], st.eps)
            gg = (pk.out_g * (1 + fin[b, 1])).contiguous()
            bb = (pk.out_b * (1 + fin[b, 1]) + fin[b, 0]).contiguous()
            y = ops.layernorm(y, gg, bb, st.eps)
            ops.gemm(y, pk.w_po, out_tok[o], M=Tv, N=po, K=self.inner_dim, bias=pk.b_po)
        return out_tok.view(B * Tv, po)

    @torch.no_grad()
    def forward(self, hidden_states, encoder_hidden_states, timestep, domain_features, flow_features, timestep_cond=None,
                ofs=None, image_rotary_emb=None, attention_kwargs=None, return_dict: bool = True):
        """cogvideox_transformer_3d.py:473-486 - ``domain_features`` / ``flow_features`` are positional"""
        if timestep_cond is not None:
            raise LkgdHipError("timestep_cond belongs to none of the released CogVideoX models: not built")
        if ofs is not None and self.ofs_embedding is None:
            raise LkgdHipError("ofs belongs to the CogVideoX 1.5 image-to-video models: this model has no ofs_embedding "
                               "(config ofs_embed_dim)")
        if ofs is None and self.ofs_embedding is not None:
            raise LkgdHipError("this model has an ofs_embedding (config ofs_embed_dim): forward needs ofs (the pipeline passes 2.0)")
        text = self.fused_text(encoder_hidden_states, domain_features, flow_features)
        out = self.forward_tokens(hidden_states, text, timestep, image_rotary_emb=image_rotary_emb, ofs=ofs)
        if not return_dict:
            return (out,)
        return Transformer2DModelOutput(sample=out)


# ------------------------------------------------------------------------------------------------ scheduler + loop
class SchedulerConfig(dict):
    """[EXT diffusers FrozenDict]: a scheduler's config, its keys readable as attributes as well"""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class _CogVideoXSchedule:
    """what the two CogVideoX schedulers share, [EXT diffusers scheduling_ddim_cogvideox.py / scheduling_dpm_cogvideox.py] with
    CogVideoX's scheduler_config.json (scaled-linear betas 0.00085..0.012, snr_shift_scale 3.0 for the 2B and 1.0 for the 5B models,
    zero-terminal-SNR rescale, trailing spacing, v-prediction, set_alpha_to_one): the host tables in fp64 and the timesteps"""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, snr_shift_scale=3.0, **_ignored):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float64) ** 2
        ac = torch.cumprod(1.0 - betas, dim=0)
        ac = ac / (snr_shift_scale + (1 - snr_shift_scale) * ac)
        s = ac.sqrt()
        s0, sT = s[0].clone(), s[-1].clone()
        self.alphas_cumprod = ((s - sT) * (s0 / (s0 - sT))) ** 2
        self.final_alpha_cumprod = torch.tensor(1.0, dtype=torch.float64)
        # the keys of scheduler_config.json with the values built here: a mapping, so that ``Scheduler(**other.config)`` works as it
        # does with diffusers' FrozenDict (ddim_inversion.py:489)
        self.config = SchedulerConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule="scaled_linear", clip_sample=False, set_alpha_to_one=True,
                                      rescale_betas_zero_snr=True, prediction_type="v_prediction", timestep_spacing="trailing",
                                      snr_shift_scale=snr_shift_scale, _class_name=type(self).__name__)
        self.timesteps = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        self.num_inference_steps = num_inference_steps
        n = self.config.num_train_timesteps
        self.timesteps = torch.from_numpy(np.round(np.arange(n, 0, -n / num_inference_steps)).astype(np.int64) - 1)

    def scale_model_input(self, sample, timestep=None):
        return sample

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps) -> torch.Tensor:
        """[EXT diffusers ``add_noise`` of both schedulers], parity unpinned: ``alphas_cumprod`` cast to the samples' dtype,
        ``a = alphas_cumprod[timesteps] ** 0.5``, ``s = (1 - alphas_cumprod[timesteps]) ** 0.5`` shaped [B, 1, ...], and
        ``a * original_samples + s * noise`` with both products and the sum rounded in that dtype.  Plain tensor arithmetic, once per
        clip (the video-to-video pipeline's start of the loop)"""
        ac = self.alphas_cumprod.to(device=original_samples.device, dtype=original_samples.dtype)
        timesteps = torch.as_tensor(timesteps, dtype=torch.int64).reshape(-1).to(original_samples.device)
        shape = (-1,) + (1,) * (original_samples.dim() - 1)
        a = (ac[timesteps] ** 0.5).reshape(shape)
        s = ((1 - ac[timesteps]) ** 0.5).reshape(shape)
        return a * original_samples + s * noise

    def _alpha_pair(self, t: int):
        """(alphas_cumprod[t], alphas_cumprod of the step's target, the target's timestep), fp64 0-dim tensors"""
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        return self.alphas_cumprod[t], (self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod), prev_t


class CogVideoXDDIMScheduler(_CogVideoXSchedule):
    """[EXT diffusers scheduling_ddim_cogvideox.py] (the reference's cli_demo.py recommends it for CogVideoX-2B); host tables in
    fp64, the update itself runs on the device"""
    step_kind = "ddim"

    def coefficients(self, t: int):
        at, ap, _ = self._alpha_pair(t)
        a = ((1 - ap) / (1 - at)) ** 0.5
        b = ap ** 0.5 - at ** 0.5 * a
        return float(a), float(b), float(at ** 0.5), float((1 - at) ** 0.5)

    def step(self, model_output, timestep, sample, **_):
        a, b, sa, sb = self.coefficients(int(timestep))
        x0 = sa * sample - sb * model_output
        return (a * sample + b * x0,)


#: ``CogVideoXDPMScheduler.coefficients``: x0 = sqrt_alpha x - sqrt_beta n; order 1: x' = m1 x - m2 x0 + mn eps; order 2: the same
#: with m3 x0 - m4 x0_old in the place of x0
DPMCoefficients = namedtuple("DPMCoefficients", "sqrt_alpha sqrt_beta m1 m2 m3 m4 mn order")


class CogVideoXDPMScheduler(_CogVideoXSchedule):
    """[EXT diffusers scheduling_dpm_cogvideox.py], PARITY UNPINNED: DPM-Solver++ (SDE, 2M) on the tables of
    the DDIM class - the scheduler the reference's pipeline keeps ``old_pred_original_sample`` for
    (pipeline_cogvideox_image2video.py:832-883) and its cli_demo.py installs for CogVideoX-5B / 5B-I2V.  ``coefficients`` in fp64 on
    the host; ``step`` is the out-of-place ATen form, ``denoise`` runs the same statements as one launch (``ops.dit_cfg_dpm_step``)"""
    step_kind = "dpm"

    def coefficients(self, t: int, t_back: Optional[int] = None) -> DPMCoefficients:
        """``t_back``: the previous timestep of the loop, None on its first step.  At t = 999 alphas_cumprod is 0 (zero terminal SNR):
        lam = -inf, h = +inf, and the multipliers are their finite limits (m1 = 0, m2 = -sqrt(ap)); on the step after it r = inf gives
        m3 = 1, m4 = 0; a last step onto final_alpha_cumprod = 1 has lam_next = +inf and (m1, m2, mn) = (0, -1, 0) - all of it by
        IEEE arithmetic on fp64 0-dim tensors, as written"""
        at, ap, prev_t = self._alpha_pair(int(t))
        lam = torch.log((at / (1 - at)) ** 0.5)
        lam_next = torch.log((ap / (1 - ap)) ** 0.5)
        h = lam_next - lam
        m1 = ((1 - ap) / (1 - at)) ** 0.5 * torch.exp(-h)
        m2 = torch.expm1(-2 * h) * ap ** 0.5
        mn = (1 - ap) ** 0.5 * (1 - torch.exp(-2 * h)) ** 0.5
        m3, m4, order = 1.0, 0.0, 1
        if t_back is not None and prev_t >= 0:
            ab = self.alphas_cumprod[int(t_back)]
            r = (lam - torch.log((ab / (1 - ab)) ** 0.5)) / h
            m3, m4, order = 1 + 1 / (2 * r), 1 / (2 * r), 2
        return DPMCoefficients(float(at ** 0.5), float((1 - at) ** 0.5), float(m1), float(m2), float(m3), float(m4), float(mn), order)

    def step(self, model_output, old_pred_original_sample, timestep, timestep_back, sample, eta: float = 0.0, generator=None,
             return_dict: bool = False):
        """the reference's argument order -> (prev_sample, pred_original_sample), both fp32 (the pipeline casts the first back).
        The noise is ``randn`` of the sample's shape in the sample's dtype from ``generator`` (a generator of another device draws
        on that device and the tensor is moved; lkgd_amd/scheduler.py); a second-order step draws twice and uses the second draw"""
        if eta != 0.0:
            raise LkgdHipError(f"CogVideoXDPMScheduler.step: eta={eta!r} is not built (eta 0.0 only)")
        if return_dict:
            raise LkgdHipError("CogVideoXDPMScheduler.step: return_dict=True is not built (the pipeline passes False)")
        second = old_pred_original_sample is not None and timestep_back is not None
        k = self.coefficients(int(timestep), int(timestep_back) if second else None)
        eps = dpm_noise(sample.shape, sample.dtype, sample.device, generator, k.order)
        x = sample.float()
        x0 = k.sqrt_alpha * x - k.sqrt_beta * model_output.float()
        d = x0 if k.order == 1 else k.m3 * x0 - k.m4 * old_pred_original_sample.float()
        prev = k.m1 * x - k.m2 * d
        if k.mn != 0.0:
            prev = prev + k.mn * eps.float()
        return prev, x0


def dpm_noise(shape, dtype, device, generator, order: int) -> torch.Tensor:
    """the draws of one DPM step: ``order`` calls of randn, the last one kept ([EXT] scheduling_dpm_cogvideox.py: a second-order step
    draws twice and uses the second draw - with a caller's generator the discarded draw is observable in its state).  A list of
    generators, one per batch entry, draws every entry from its own ([EXT] diffusers ``randn_tensor``)"""
    if isinstance(generator, (list, tuple)):
        if len(generator) != shape[0]:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {shape[0]}. Make sure the batch size matches the length of the generators.")
        one = (1,) + tuple(shape[1:])
        for _ in range(order):
            eps = torch.cat([torch.randn(one, generator=g, device=g.device, dtype=dtype) for g in generator])
        return eps.to(device)
    gdev = generator.device if generator is not None else device
    for _ in range(order):
        eps = torch.randn(tuple(shape), generator=generator, device=gdev, dtype=dtype)
    return eps.to(device)


_SCHEDULERS = {c.__name__: c for c in (CogVideoXDDIMScheduler, CogVideoXDPMScheduler)}


def scheduler_from_config(path_or_dict):
    """a checkpoint directory (its ``scheduler/scheduler_config.json``, read as lkgd_amd/loading.py reads the other configs) or that
    file's contents as a dict -> the scheduler its ``_class_name`` names.  Every value that is not the one implemented raises,
    naming the key"""
    raw, where = path_or_dict, "scheduler_from_config"
    if not isinstance(raw, dict):
        from .loading import load_config
        raw = load_config(str(path_or_dict), "scheduler", name="scheduler_config.json")
        where = f"scheduler_from_config({str(path_or_dict)!r})"
    name = raw.get("_class_name")
    if name not in _SCHEDULERS:
        raise LkgdHipError(f"{where}: _class_name={name!r}; built: {sorted(_SCHEDULERS)}")
    built = dict(prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True, set_alpha_to_one=True,
                 beta_schedule="scaled_linear")
    # a key the file leaves out has the constructor default of [EXT] diffusers' two CogVideoX schedulers - for three of the five not
    # the value the released checkpoints set, so a config without them is refused like one that sets them otherwise
    absent = dict(prediction_type="epsilon", timestep_spacing="leading", rescale_betas_zero_snr=False, set_alpha_to_one=True,
                  beta_schedule="scaled_linear")
    for key, want in built.items():
        got = raw.get(key, absent[key])
        if got != want:
            raise LkgdHipError(f"{where}: {key}={got!r}{'' if key in raw else ' (the default of an absent key)'}; only "
                               f"{key}={want!r} is built")
    kw = {k: raw[k] for k in ("num_train_timesteps", "beta_start", "beta_end", "snr_shift_scale") if k in raw}
    return _SCHEDULERS[name](**kw)


def dynamic_guidance(guidance_scale: float, num_inference_steps: int, t: int) -> float:
    """pipeline_cogvideox_image2video.py:866-869"""
    return 1 + guidance_scale * ((1 - math.cos(math.pi * ((num_inference_steps - t) / num_inference_steps) ** 5.0)) / 2)


class LoopPlacement:
    """What ``denoise`` asks about the batch it embeds and the process it runs in.  The default: this process holds every entry and
    frame, and there are no reference entries.  A rank of a sharded run (lkgd_amd/dist_run.py) answers for its CFG half and frame
    slice, reference-guided sampling (lkgd_amd/ddim_inversion.py) for its [sample | reference] pairs."""
    shard = None          # handed to ``forward_rows``: the rows are then those of the shard's ``plan.f_local`` frames
    after_step = None     # f(i, t, latents) after step i: the loop's own latents, updated in place - no clone

    def rows(self, i: int, latents, img, out, p: int, **glue) -> torch.Tensor:
        """the patch rows step i's forward embeds; ``out``: what the previous step's call returned (None on the first)"""
        return ops.dit_patch_rows(latents, img, p, out=out, **glue)

    def text(self, text: torch.Tensor) -> torch.Tensor:
        """the text rows of the entries ``forward_rows`` runs, of the [cfg * B, L, 4096] of the whole batch"""
        return text

    def noise(self, noise_rows: torch.Tensor) -> torch.Tensor:
        """``forward_rows``' result -> the [cfg * B * Tv, C p p] rows of the whole batch, which the step kernel takes"""
        return noise_rows


@torch.no_grad()
def denoise(transformer: CogVideoXTransformer3DModel, scheduler, latents, image_latents, prompt_embeds,
            domain_features, flow_features, num_inference_steps: int = 50, guidance_scale: float = 6.0,
            use_dynamic_cfg: bool = True, callback=None, image_rotary_emb=None, ofs=None, generator=None,
            start_step: int = 0, _placement: Optional[LoopPlacement] = None) -> torch.Tensor:
    """the loop of pipeline_cogvideox_image2video.py:829-885 (the rotary tables are built once per clip when the config asks for
    them and none are given, :819-823).  latents / image_latents [B, F, C, h, w]; prompt_embeds
    [2B, L, 4096] (negative first) when guidance_scale > 1.  The update runs in fp32 (``noise_pred.float()`` :863) and the
    latents are cast back to the prompt dtype, fp16, after every step (:881 - reproduced).  Per step: ``lkgd_dit_patch_rows`` ->
    ``forward_rows`` -> ``lkgd_dit_cfg_ddim_step`` (include/lkgd_hip_dit_loop.h); ``scheduler`` supplies ``coefficients(t)``.
    A ``patch_size_t`` model takes tensors prepared by ``pad_for_temporal_patches`` (F % p_t == 0, or it raises), runs the ``_t``
    glue pair (include/lkgd_hip_dit_tpatch.h) on the (F / p_t, h, w) grid, and embeds ``ofs`` (default 2.0 when the config has
    ``ofs_embed_dim``, :826) once per clip.
    ``scheduler`` declares its step in a class attribute ``step_kind``.  ``"ddim"`` (``CogVideoXDDIMScheduler``, the steps above;
    ``lkgd_amd.ddim_inversion.DDIMInverseScheduler``, whose ``coefficients`` have the same four-tuple form), or ``"dpm"``
    (``CogVideoXDPMScheduler``, :874-883): the step is then
    ``lkgd_dit_cfg_dpm_step`` (include/lkgd_hip_dit_dpm.h) on ``coefficients(t, previous t)``, with ``old_pred_original_sample`` kept
    in one fp32 tensor per clip and the step's noise drawn from ``generator`` in the latents' dtype (``dpm_noise``: twice on a
    second-order step).  Anything else raises: there is no step to fall back to.
    ``domain_features`` and ``flow_features`` both None (the stock text-to-video / video-to-video transformer, which has no
    ``quaternion_lora_*`` path): the text rows are ``prompt_embeds`` in fp16, ``fused_text`` is not called; exactly one of them None
    raises, naming it.
    ``start_step`` ([EXT] diffusers' video-to-video ``__call__``, parity unpinned): the loop runs ``scheduler.timesteps[start_step:]``.
    Its first executed step has no previous timestep - a first-order DPM step with one draw; the callback's index counts executed
    steps; and ``dynamic_guidance`` is given ``num_inference_steps - start_step`` as its step count, because diffusers' class
    overwrites ``num_inference_steps`` with the truncated count before its loop (a quirk, reproduced: the ramp is not the one of the
    untruncated schedule).
    ``_placement`` (private, ``LoopPlacement``): the one loop also serves the ranks of ``DistDiTDenoiser`` and the pairs of
    ``ddim_inversion.sample``; without it the launches are the ones listed above."""
    kind = getattr(type(scheduler), "step_kind", None)
    dpm = kind == "dpm"
    if kind not in ("ddim", "dpm"):
        raise LkgdHipError(f"denoise: scheduler is a {type(scheduler).__module__}.{type(scheduler).__qualname__}; the loop's step is "
                           "built for CogVideoXDDIMScheduler and CogVideoXDPMScheduler")
    dev = transformer.device
    if transformer.config.patch_size_t is not None and latents.shape[1] % transformer.config.patch_size_t:
        raise LkgdHipError(f"denoise: patch_size_t {transformer.config.patch_size_t} does not divide the {latents.shape[1]} latent "
                           "frames: pad_for_temporal_patches first")
    if ofs is not None and transformer.ofs_embedding is None:
        raise LkgdHipError("denoise: ofs given, but the model has no ofs_embedding (config ofs_embed_dim)")
    if not 0 <= start_step < num_inference_steps:
        raise ValueError(f"denoise: start_step={start_step} lies outside [0, num_inference_steps={num_inference_steps})")
    scheduler.set_timesteps(num_inference_steps)
    cfg = guidance_scale > 1.0
    if domain_features is None and flow_features is None:         # no latent-knowledge fuse: the prompt embeddings are the text rows
        text = prompt_embeds.to(device=dev, dtype=torch.float16).contiguous()
    elif domain_features is None or flow_features is None:
        raise LkgdHipError(f"denoise: `{'domain_features' if domain_features is None else 'flow_features'}` is None and the other "
                           "is given; the latent-knowledge fuse takes both, the stock transformer neither")
    else:
        text = transformer.fused_text(prompt_embeds, domain_features, flow_features)      # step-invariant: once per clip
    place = _placement if _placement is not None else LoopPlacement()
    text = place.text(text)
    # the loop's own copy: the step kernel updates it in place
    latents = latents.to(device=dev, dtype=torch.float16).clone(memory_format=torch.contiguous_format)
    # text-to-video (no image latents): the rows hold the latents' channels alone
    img = image_latents.to(device=dev, dtype=torch.float16).contiguous() if image_latents is not None else None
    tc = transformer.config
    p, pt = tc.patch_size, tc.patch_size_t
    grid = (latents.shape[1] // (pt or 1), latents.shape[3] // p, latents.shape[4] // p)       # of the whole clip
    local_grid = grid if place.shard is None else (place.shard.plan.f_local,) + grid[1:]
    extra = {} if place.shard is None else {"shard": place.shard}
    if transformer.ofs_embedding is not None:         # step-invariant: once per clip
        extra["ofs_emb"] = transformer.embed_ofs(2.0 if ofs is None else ofs, text.shape[0])
    glue = {} if pt is None else {"p_t": pt}
    if tc.use_rotary_positional_embeddings:
        if image_rotary_emb is None:
            image_rotary_emb = rotary_tables(tc, *grid)
        image_rotary_emb = tuple(t.to(device=dev, dtype=torch.float32).contiguous() for t in image_rotary_emb)
    rows = None
    # DPM: old_pred_original_sample, fp32; step i reads step i - 1's x0 (second order only) and leaves its own
    x0_state = torch.empty(latents.shape, dtype=torch.float32, device=dev) if dpm else None
    t_back = None
    guidance_steps = num_inference_steps - start_step
    for i, t in enumerate(scheduler.timesteps[start_step:].tolist()):
        # torch.cat([latents] * 2), the channel concat and the patch unfold: ONE set of rows, embedded for every CFG entry
        rows = place.rows(i, latents, img, rows, p, **glue)
        noise_rows = place.noise(transformer.forward_rows(rows, local_grid, text, float(t), image_rotary_emb=image_rotary_emb, **extra))
        g = dynamic_guidance(guidance_scale, guidance_steps, t) if use_dynamic_cfg else guidance_scale
        # noise_pred.float(), the CFG combine, scheduler.step and the cast back: one launch, in place
        if dpm:
            k = scheduler.coefficients(int(t), t_back)
            eps = dpm_noise(latents.shape, latents.dtype, dev, generator, k.order)
            ops.dit_cfg_dpm_step(noise_rows, latents, x0_state, eps, p, 2 if cfg else 1, k.order, g, k, **glue)
            t_back = int(t)
        else:
            ops.dit_cfg_ddim_step(noise_rows, latents, p, 2 if cfg else 1, g, *scheduler.coefficients(int(t)), **glue)
        if place.after_step is not None:
            place.after_step(i, t, latents)
        if callback is not None:
            callback(i, t, latents.clone())         # a tensor of the callback's own, as the out-of-place loop handed out
    return latents


# ---- the prompt in front of the loop ------------------------------------------------------------------------------------------------
def _get_t5_prompt_embeds(text_encoder, tokenizer, prompt, num_videos_per_prompt: int = 1, max_sequence_length: int = 226,
                          device=None, dtype=None) -> torch.Tensor:
    """pipeline_cogvideox_image2video.py:230-270 with ``self.text_encoder`` / ``self.tokenizer`` as arguments.  ``prompt``: a string,
    a list of strings, or the token ids themselves as an int64 [B, S] tensor (no tokenizer needed).  The tokenizer is called as the
    reference calls it; its second, untruncated call only feeds a warning about cut-off text and is not made."""
    device = device or text_encoder.device
    dtype = dtype or text_encoder.dtype
    if isinstance(prompt, torch.Tensor):
        if prompt.dim() != 2 or prompt.dtype != torch.int64:
            raise ValueError(f"a prompt given as token ids must be an int64 [B, S] tensor, got {prompt.dtype} {tuple(prompt.shape)}")
        text_input_ids, batch_size = prompt, prompt.shape[0]
    else:
        prompt = [prompt] if isinstance(prompt, str) else prompt
        batch_size = len(prompt)
        if tokenizer is None:
            raise LkgdHipError("encode_prompt: a text prompt needs a tokenizer (the T5 sentencepiece vocabulary is the caller's: "
                               "transformers' T5Tokenizer of the checkpoint's tokenizer/ directory); token ids need none")
        text_inputs = tokenizer(prompt, padding="max_length", max_length=max_sequence_length, truncation=True,
                                add_special_tokens=True, return_tensors="pt")
        text_input_ids = text_inputs.input_ids
    prompt_embeds = text_encoder(text_input_ids.to(device))[0]
    prompt_embeds = prompt_embeds.to(dtype=dtype, device=device)
    # duplicate text embeddings for each generation per prompt (:265-268)
    _, seq_len, _ = prompt_embeds.shape
    prompt_embeds = prompt_embeds.repeat(1, num_videos_per_prompt, 1)
    return prompt_embeds.view(batch_size * num_videos_per_prompt, seq_len, -1)


def encode_prompt(text_encoder, tokenizer, prompt, negative_prompt=None, do_classifier_free_guidance: bool = True,
                  num_videos_per_prompt: int = 1, prompt_embeds: Optional[torch.Tensor] = None,
                  negative_prompt_embeds: Optional[torch.Tensor] = None, max_sequence_length: int = 226, device=None, dtype=None):
    """the reference's ``encode_prompt`` (pipeline_cogvideox_image2video.py:273-352): same parameters, defaults and errors, with
    ``text_encoder`` (``lkgd_amd.t5.T5EncoderModel``) and ``tokenizer`` in place of ``self``.  Returns ``(prompt_embeds,
    negative_prompt_embeds)``, each [B * num_videos_per_prompt, max_sequence_length, d_model] in the encoder's dtype (the second None
    without guidance).  For :func:`denoise` under guidance the pipeline concatenates them negative first (:772):
    ``torch.cat([negative_prompt_embeds, prompt_embeds])``.  Prompts may also be int64 id tensors [B, S]."""
    device = device or text_encoder.device
    prompt = [prompt] if isinstance(prompt, str) else prompt
    if prompt is not None:
        batch_size = len(prompt)
    else:
        batch_size = prompt_embeds.shape[0]

    if prompt_embeds is None:
        prompt_embeds = _get_t5_prompt_embeds(text_encoder, tokenizer, prompt, num_videos_per_prompt, max_sequence_length, device, dtype)

    if do_classifier_free_guidance and negative_prompt_embeds is None:
        if not isinstance(negative_prompt, torch.Tensor):
            negative_prompt = negative_prompt or ""
        negative_prompt = batch_size * [negative_prompt] if isinstance(negative_prompt, str) else negative_prompt
        ids = isinstance(prompt, torch.Tensor) or isinstance(negative_prompt, torch.Tensor)      # id tensors mix with the "" default

        if prompt is not None and not ids and type(prompt) is not type(negative_prompt):
            raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                            f" {type(prompt)}.")
        elif batch_size != len(negative_prompt):
            raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                             f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                             " the batch size of `prompt`.")

        negative_prompt_embeds = _get_t5_prompt_embeds(text_encoder, tokenizer, negative_prompt, num_videos_per_prompt,
                                                       max_sequence_length, device, dtype)

    return prompt_embeds, negative_prompt_embeds


# ---- the image in front of the loop -------------------------------------------------------------------------------------------------
def retrieve_latents(encoder_output, generator=None, sample_mode: str = "sample"):
    """pipeline_cogvideox_image2video.py:153-163"""
    if hasattr(encoder_output, "latent_dist") and sample_mode == "sample":
        return encoder_output.latent_dist.sample(generator)
    elif hasattr(encoder_output, "latent_dist") and sample_mode == "argmax":
        return encoder_output.latent_dist.mode()
    elif hasattr(encoder_output, "latents"):
        return encoder_output.latents
    else:
        raise AttributeError("Could not access latents of provided encoder_output")


def _scaled_sample(encoder_output, generator, scale: float):
    """``scale * retrieve_latents(encoder_output, generator)``; a posterior of lkgd_amd's VAE folds the scale into the launch that
    samples (``lkgd_cogvae_posterior``)"""
    from .cogvideox_vae import DiagonalGaussianDistribution
    dist = getattr(encoder_output, "latent_dist", None)
    if isinstance(dist, DiagonalGaussianDistribution):
        return dist.sample(generator, scale=scale)
    return scale * retrieve_latents(encoder_output, generator)


@torch.no_grad()
def prepare_latents(vae, scheduler, transformer_config, image: torch.Tensor, batch_size: int = 1, num_channels_latents: int = 16,
                    num_frames: int = 13, height: int = 60, width: int = 90, dtype=None, device=None, generator=None, latents=None):
    """the reference's ``prepare_latents`` (pipeline_cogvideox_image2video.py:354-427) with ``self.vae`` / ``self.scheduler`` /
    ``self.transformer.config`` as arguments: every image [C, H, W] of ``image`` [B, C, H, W] is encoded on its own
    (``vae.encode(img[None, :, None])``) and sampled with its generator, scaled by ``scaling_factor`` (its inverse under
    ``invert_scale_latents``), followed by ``num_frames - 1`` zero latent frames and, under ``patch_size_t``, padded at the front
    (``pad_for_temporal_patches``); the noise is drawn with the (padded) latent shape - or ``latents`` taken as given - and
    multiplied by ``scheduler.init_noise_sigma``.  Returns ``(latents, image_latents)``, both [B, F, C, h, w]: what :func:`denoise`
    takes."""
    _check_generators(generator, batch_size)
    vc = vae.config
    scale_t, scale_s = vc.temporal_compression_ratio, 2 ** (len(vc.block_out_channels) - 1)
    device = device if device is not None else vae.device
    dtype = dtype if dtype is not None else vae.dtype
    p_t = transformer_config.patch_size_t

    num_frames = (num_frames - 1) // scale_t + 1
    shape = (batch_size, num_frames, num_channels_latents, height // scale_s, width // scale_s)
    shape, _ = pad_for_temporal_patches(shape, None, p_t)                               # :383-384

    image = image.unsqueeze(2)                                                          # [B, C, F, H, W]
    factor = vc.scaling_factor if not vc.invert_scale_latents else 1 / vc.scaling_factor          # :397-402
    if isinstance(generator, list):
        image_latents = [_scaled_sample(vae.encode(image[i].unsqueeze(0)), generator[i], factor) for i in range(batch_size)]
    else:
        image_latents = [_scaled_sample(vae.encode(img.unsqueeze(0)), generator, factor) for img in image]
    image_latents = torch.cat(image_latents, dim=0).to(device=device, dtype=dtype).permute(0, 2, 1, 3, 4)      # [B, F, C, h, w]

    padding_shape = (batch_size, num_frames - 1, num_channels_latents, height // scale_s, width // scale_s)
    latent_padding = torch.zeros(padding_shape, device=device, dtype=dtype)
    image_latents = torch.cat([image_latents, latent_padding], dim=1)
    _, image_latents = pad_for_temporal_patches(shape, image_latents, p_t)              # :416-418 (the shape is padded already)

    latents = initial_noise(shape, dtype, device, generator) if latents is None else latents.to(device)
    latents = latents * scheduler.init_noise_sigma
    return latents, image_latents


def _check_generators(generator, batch_size: int) -> None:
    if isinstance(generator, list) and len(generator) != batch_size:
        raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                         f" size of {batch_size}. Make sure the batch size matches the length of the generators.")


def initial_noise(shape, dtype, device, generator) -> torch.Tensor:
    """the clip's initial noise ([EXT] diffusers ``randn_tensor``): drawn on the generator's device and moved; a list of generators
    draws every batch entry from its own"""
    shape = tuple(shape)
    if isinstance(generator, list):
        gdev = generator[0].device
        return torch.cat([torch.randn((1,) + shape[1:], generator=g, device=gdev, dtype=dtype) for g in generator]).to(device)
    gdev = generator.device if generator is not None else device
    return torch.randn(shape, generator=generator, device=gdev, dtype=dtype).to(device)


# ---- text-to-video and video-to-video in front of the loop ([EXT] diffusers pipeline_cogvideox.py / pipeline_cogvideox_video2video.py,
# ---- parity unpinned: the reference imports the two classes and does not vendor them) ------------------------------------------------
def get_timesteps(scheduler, num_inference_steps: int, strength: float):
    """[EXT] the video-to-video class's ``get_timesteps``, called after ``set_timesteps`` -> (the timesteps the loop runs, their count,
    ``t_start``: ``denoise``'s ``start_step``).  ``strength`` 1.0 runs the whole schedule, 0.8 of 50 steps its last 40.  A strength that
    leaves no step raises here (diffusers fails later, on the empty ``timesteps[:1]``)"""
    init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
    t_start = max(num_inference_steps - init_timestep, 0)
    if init_timestep <= 0:
        raise ValueError(f"`strength`={strength} with `num_inference_steps`={num_inference_steps} leaves no denoising step "
                         f"(int(num_inference_steps * strength) = {init_timestep})")
    return scheduler.timesteps[t_start:], num_inference_steps - t_start, t_start


def prepare_noise_latents(scheduler, transformer_config, vae_config, batch_size: int = 1, num_channels_latents: int = 16,
                          num_frames: int = 13, height: int = 60, width: int = 90, dtype=None, device=None, generator=None,
                          latents=None) -> torch.Tensor:
    """[EXT] the text-to-video class's ``prepare_latents``: noise [B, (num_frames - 1) // temporal ratio + 1, C, height // 8,
    width // 8] drawn as ``prepare_latents`` draws it (``initial_noise``) - or ``latents`` as given - times
    ``scheduler.init_noise_sigma``.  For a ``patch_size_t`` model the caller passes the padded pixel frame count
    (``pipeline_cogvideox.additional_latent_frames``); ``transformer_config`` takes no part in the shape"""
    _check_generators(generator, batch_size)
    scale_t, scale_s = vae_config.temporal_compression_ratio, 2 ** (len(vae_config.block_out_channels) - 1)
    shape = (batch_size, (num_frames - 1) // scale_t + 1, num_channels_latents, height // scale_s, width // scale_s)
    latents = initial_noise(shape, dtype, device, generator) if latents is None else latents.to(device)
    return latents * scheduler.init_noise_sigma


@torch.no_grad()
def prepare_video_latents(vae, scheduler, video: Optional[torch.Tensor] = None, batch_size: int = 1, num_channels_latents: int = 16,
                          height: int = 60, width: int = 90, dtype=None, device=None, generator=None, latents=None,
                          timestep=None) -> torch.Tensor:
    """[EXT] the video-to-video class's ``prepare_latents``: every clip [3, T, H, W] of ``video`` [B, 3, T, H, W] is encoded on its own
    and sampled with its generator (or the shared one), ``scaling_factor`` folded into the sampling launch (``_scaled_sample``); the
    samples, concatenated and permuted to [B, F, C, h, w], are noised to ``timestep`` [B] - ``scheduler.add_noise(init, noise,
    timestep)`` with noise of their shape - and multiplied by ``init_noise_sigma``.  The generator is consumed in that order: all
    posterior samples, then the noise.  Given ``latents`` are taken as they are (times ``init_noise_sigma``); the video is not encoded"""
    _check_generators(generator, batch_size)
    vc = vae.config
    scale_t, scale_s = vc.temporal_compression_ratio, 2 ** (len(vc.block_out_channels) - 1)
    device = device if device is not None else vae.device
    dtype = dtype if dtype is not None else vae.dtype
    if latents is not None:
        return latents.to(device) * scheduler.init_noise_sigma
    if video is None or video.dim() != 5 or video.shape[0] != batch_size:
        raise ValueError(f"prepare_video_latents: `video` must be [{batch_size}, C, T, H, W], got "
                         f"{None if video is None else tuple(video.shape)}")
    T = video.shape[2]
    frames = (T - 1) // scale_t + 1
    shape = (batch_size, frames, num_channels_latents, height // scale_s, width // scale_s)
    gens = generator if isinstance(generator, list) else [generator] * batch_size
    init = [_scaled_sample(vae.encode(video[i].unsqueeze(0)), gens[i], vc.scaling_factor) for i in range(batch_size)]
    init = torch.cat(init, dim=0).to(device=device, dtype=dtype).permute(0, 2, 1, 3, 4)      # [B, F, C, h, w]
    if tuple(init.shape) != shape:
        raise LkgdHipError(f"prepare_video_latents: the encoder returned latents {tuple(init.shape)} for T = {T} pixel frames at "
                           f"{height} x {width}; the loop takes {shape} ((T - 1) // {scale_t} + 1 latent frames)")
    noise = initial_noise(shape, dtype, device, generator)
    return scheduler.add_noise(init, noise, timestep) * scheduler.init_noise_sigma
