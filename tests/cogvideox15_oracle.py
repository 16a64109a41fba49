"""fp32 twin of the CogVideoX 1.5 DiT (``patch_size_t = 2``, rotary embeddings without a learned table, ``ofs_embed_dim``) - TEST
INFRASTRUCTURE ONLY, composed from tests/cogvideox_rope_oracle.py and oracle/cogvideox.py.

In-tree reference: CogVideo-main/finetune/models/cogvideox_i2v/cogvideox_transformer_3d.py (config :233-296, ``proj_out`` :326-331,
``ofs`` :513-517, the un-patchify :619-630) and pipeline_cogvideox_image2video.py (:572-584 the slice rotary grid, :826 ``ofs``).

**[EXT] - PARITY UNPINNED**, restated from the published diffusers >= 0.32 source: ``CogVideoXPatchEmbed`` with ``patch_size_t`` (a
Linear over a patch's (c, pt, py, px) columns) and ``get_3d_rotary_pos_embed(grid_type="slice")``.
tests/golden/cogvideox15.safetensors executes the reference's in-tree model OVER these restatements, so it pins the wiring - ``ofs``,
``proj_out``'s width, the un-patchify - not these interiors.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional

import torch
import torch.nn as nn

import cogvideox_rope_oracle as ro
from oracle import blocks as ob
from oracle import cogvideox as oc


@dataclass
class V15DiTConfig(ro.RopeDiTConfig):
    use_learned_positional_embeddings: bool = False
    patch_size_t: Optional[int] = 2
    ofs_embed_dim: Optional[int] = None
    patch_bias: bool = False


#: TINY_DIT with temporal patches: in_channels 32 -> K = 32 * 2 * 2 * 2 = 256 patch columns (K % 64), 4 latent frames (sample_frames
#: 13) on the 8 x 12 latent grid = 2 x 4 x 6 tokens; ofs_embed_dim = time_embed_dim (the two embeddings are added)
TINY_V15_DIT = V15DiTConfig(**{**oc.TINY_DIT.__dict__, "sample_frames": 13}, ofs_embed_dim=64)
#: config.json of THUDM/CogVideoX1.5-5B-I2V's transformer (the fields the constructor reads)
COGVIDEOX_15_5B_I2V = V15DiTConfig(num_attention_heads=48, num_layers=42, in_channels=32, ofs_embed_dim=512, sample_height=300,
                                   sample_width=300, sample_frames=81, max_text_seq_length=224)
OFS = 2.0               # pipeline_cogvideox_image2video.py:826
OFS_GAIN = 1.0          # gain on every ofs_embedding weight of the fixture: none needed, ``ofs`` matters as initialised (see the generator)


# ------------------------------------------------------------------------------------------------ [EXT] embeddings.py
def get_3d_rotary_pos_embed_slice(embed_dim, grid_size, temporal_size, max_size, theta=10000.0):
    """``get_3d_rotary_pos_embed(crops_coords=None, grid_type="slice", max_size=(max_h, max_w))`` -> cos, sin [T * H * W, embed_dim]:
    integer positions 0 .. max - 1, the tables sliced to the grid"""
    gh_n, gw_n = grid_size
    max_h, max_w = max_size
    grid_h = torch.arange(max_h, dtype=torch.float32)
    grid_w = torch.arange(max_w, dtype=torch.float32)
    grid_t = torch.arange(temporal_size, dtype=torch.float32)
    dim_t, dim_h, dim_w = embed_dim // 4, embed_dim // 8 * 3, embed_dim // 8 * 3
    ft, fh, fw = (ro.get_1d_rotary_pos_embed(d, g, theta) for d, g in ((dim_t, grid_t), (dim_h, grid_h), (dim_w, grid_w)))

    def combine(t, h, w):
        t = t[:temporal_size, None, None, :].expand(-1, gh_n, gw_n, -1)
        h = h[None, :gh_n, None, :].expand(temporal_size, -1, gw_n, -1)
        w = w[None, None, :gw_n, :].expand(temporal_size, gh_n, -1, -1)
        return torch.cat([t, h, w], dim=-1).reshape(temporal_size * gh_n * gw_n, -1)
    return combine(ft[0], fh[0], fw[0]), combine(ft[1], fh[1], fw[1])


def rotary_tables(cfg, latent_frames, h, w):
    """pipeline_cogvideox_image2video.py:572-584; ``latent_frames`` as the pipeline passes them (``latents.size(1)``), h / w tokens"""
    p, p_t = cfg.patch_size, cfg.patch_size_t
    return get_3d_rotary_pos_embed_slice(cfg.attention_head_dim, (h, w), (latent_frames + p_t - 1) // p_t,
                                         (cfg.sample_height // p, cfg.sample_width // p))


class CogVideoXPatchEmbed(ro.CogVideoXPatchEmbed):
    def __init__(self, patch_size=2, patch_size_t=None, in_channels=16, embed_dim=1920, bias=True, **kw):
        super().__init__(patch_size=patch_size, patch_size_t=None, in_channels=in_channels, embed_dim=embed_dim, bias=bias, **kw)
        self.patch_size_t = patch_size_t
        if patch_size_t is not None:
            self.proj = nn.Linear(in_channels * patch_size * patch_size * patch_size_t, embed_dim, bias=bias)

    def forward(self, text_embeds, image_embeds):
        if self.patch_size_t is None:
            return super().forward(text_embeds, image_embeds)
        assert not (self.use_positional_embeddings or self.use_learned_positional_embeddings), "the 1.5 models are rotary"
        text_embeds = self.text_proj(text_embeds)
        b, f, c, h, w = image_embeds.shape
        p, p_t = self.patch_size, self.patch_size_t
        x = image_embeds.permute(0, 1, 3, 4, 2)
        x = x.reshape(b, f // p_t, p_t, h // p, p, w // p, p, c)
        x = x.permute(0, 1, 3, 5, 7, 2, 4, 6).flatten(4, 7).flatten(1, 3)
        x = self.proj(x)
        return torch.cat([text_embeds, x], dim=1).contiguous()


# ------------------------------------------------------------------------------------------------ the model
class CogVideoXTransformer3DModel(ro.CogVideoXTransformer3DModel):
    def __init__(self, cfg: V15DiTConfig = TINY_V15_DIT):
        # the parents build (and discard) a sin-cos table of the sample grid: keep that one small - the 1.5 models have no table,
        # and their 300 x 300 x 81 sample grid would cost gigabytes for nothing
        super().__init__(replace(cfg, sample_height=cfg.patch_size, sample_width=cfg.patch_size, sample_frames=1))
        self.config.sample_height, self.config.sample_width, self.config.sample_frames = cfg.sample_height, cfg.sample_width, \
            cfg.sample_frames
        self.config.patch_size_t, self.config.ofs_embed_dim, self.config.patch_bias = cfg.patch_size_t, cfg.ofs_embed_dim, cfg.patch_bias
        d = cfg.num_attention_heads * cfg.attention_head_dim
        self.patch_embed = CogVideoXPatchEmbed(
            patch_size=cfg.patch_size, patch_size_t=cfg.patch_size_t, in_channels=cfg.in_channels, embed_dim=d,
            text_embed_dim=cfg.text_embed_dim, bias=cfg.patch_bias, sample_width=cfg.sample_width, sample_height=cfg.sample_height,
            sample_frames=cfg.sample_frames, temporal_compression_ratio=cfg.temporal_compression_ratio,
            max_text_seq_length=cfg.max_text_seq_length, spatial_interpolation_scale=cfg.spatial_interpolation_scale,
            temporal_interpolation_scale=cfg.temporal_interpolation_scale,
            use_positional_embeddings=not cfg.use_rotary_positional_embeddings,
            use_learned_positional_embeddings=cfg.use_learned_positional_embeddings)
        self.ofs_proj = self.ofs_embedding = None
        if cfg.ofs_embed_dim:                                                                            # :290-296
            self.ofs_proj = ob.Timesteps(cfg.ofs_embed_dim, True, 0)
            self.ofs_embedding = ob.TimestepEmbedding(cfg.ofs_embed_dim, cfg.ofs_embed_dim)
        if cfg.patch_size_t is not None:                                                                 # :326-333
            self.proj_out = nn.Linear(d, cfg.patch_size * cfg.patch_size * cfg.patch_size_t * cfg.out_channels)

    def forward(self, hidden_states, encoder_hidden_states, timestep, domain_features, flow_features, ofs=None,
                image_rotary_emb=None, return_dict=False):
        b, f, c, h, w = hidden_states.shape
        emb = self.time_embedding(self.time_proj(timestep).to(hidden_states.dtype))
        if self.ofs_embedding is not None:                                                               # :513-517
            emb = emb + self.ofs_embedding(self.ofs_proj(ofs).to(hidden_states.dtype))
        encoder_hidden_states = self.lk_fuse(encoder_hidden_states, domain_features, flow_features)
        x = self.patch_embed(encoder_hidden_states, hidden_states)
        tl = encoder_hidden_states.shape[1]
        enc, hid = x[:, :tl], x[:, tl:]
        for blk in self.transformer_blocks:
            hid, enc = blk(hid, enc, emb, image_rotary_emb=image_rotary_emb)
        hid = self.norm_final(hid)
        hid = self.proj_out(self.norm_out(hid, temb=emb))
        p, p_t = self.config.patch_size, self.config.patch_size_t
        if p_t is None:
            out = hid.reshape(b, f, h // p, w // p, -1, p, p).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4)
        else:                                                                                            # :626-630
            out = hid.reshape(b, (f + p_t - 1) // p_t, h // p, w // p, -1, p_t, p, p)
            out = out.permute(0, 1, 5, 4, 2, 6, 3, 7).flatten(6, 7).flatten(4, 5).flatten(1, 2)
        return (out,)


# ------------------------------------------------------------------------------------------------ seeded weights
def scale_ofs_embedding_(m, gain: float):
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.startswith("ofs_embedding.") and n.endswith(".weight"):
                p.mul_(gain)
    return m


def seeded_model(cfg, seed: int, qk_gain: float = ro.NORM_QK_GAIN, ofs_gain: float = OFS_GAIN):
    """``init_weights_`` + every norm_q / norm_k weight x ``qk_gain`` + every ofs_embedding weight x ``ofs_gain`` + fp16-representable
    values: the weights of tests/golden/cogvideox15.safetensors"""
    m = oc.init_weights_(CogVideoXTransformer3DModel(cfg), seed)
    ro.scale_qk_norm_(m, qk_gain)
    scale_ofs_embedding_(m, ofs_gain)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    return m


def swap_frames_in_patches(x: torch.Tensor, p_t: int = 2) -> torch.Tensor:
    """[B, F, ...] with the two frames of every temporal patch exchanged (the fixture's second decoy input)"""
    b, f = x.shape[:2]
    return x.reshape(b, f // p_t, p_t, *x.shape[2:]).flip(2).reshape(x.shape).contiguous()
