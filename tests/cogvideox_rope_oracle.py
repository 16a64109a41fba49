"""fp32 twin of the rotary CogVideoX DiT (CogVideoX-5B-I2V: ``use_rotary_positional_embeddings`` + a learned joint position
table) - TEST INFRASTRUCTURE ONLY, composed from oracle/cogvideox.py's blocks.

In-tree reference: CogVideo-main/finetune/models/cogvideox_i2v/cogvideox_transformer_3d.py (``image_rotary_emb`` handed from
``forward`` :482 through every block :126-143 to the attention processor; ``use_positional_embeddings=not use_rotary...`` :280) and
pipeline_cogvideox_image2video.py:544-571 (``_prepare_rotary_positional_embeddings``, ``patch_size_t is None``).

**[EXT] - PARITY UNPINNED**, restated from the published diffusers >= 0.32 source: ``CogVideoXAttnProcessor2_0`` with
``apply_rotary_emb(use_real_unbind_dim=-1)`` on the video rows of the queries and keys after their per-head LayerNorm,
``CogVideoXPatchEmbed`` without / with learned positions (a persistent buffer over the joint sequence, added to the text rows
too; another resolution raises), ``get_resize_crop_region_for_grid``, ``get_1d_rotary_pos_embed`` / ``get_3d_rotary_pos_embed``.
tests/golden/cogvideox_rope.safetensors executes the reference's in-tree model OVER these restatements, so it pins the wiring,
not these interiors.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import cogvideox as oc


@dataclass
class RopeDiTConfig(oc.DiTConfig):
    use_rotary_positional_embeddings: bool = True
    use_learned_positional_embeddings: bool = True


TINY_ROPE_DIT = RopeDiTConfig(**oc.TINY_DIT.__dict__)
#: config.json of THUDM/CogVideoX-5b-I2V's transformer (the fields the constructor reads)
COGVIDEOX_5B_I2V = RopeDiTConfig(num_attention_heads=48, num_layers=42, in_channels=32)
NORM_QK_GAIN = 4.0      # the fixture scales every norm_q / norm_k weight by this so that the rotation matters (see the generator)


# ------------------------------------------------------------------------------------------------ [EXT] embeddings.py
def get_resize_crop_region_for_grid(src, tgt_width, tgt_height):
    h, w = src
    if h / w > tgt_height / tgt_width:
        resize_height, resize_width = tgt_height, int(round(tgt_height / h * w))
    else:
        resize_width, resize_height = tgt_width, int(round(tgt_width / w * h))
    top, left = int(round((tgt_height - resize_height) / 2.0)), int(round((tgt_width - resize_width) / 2.0))
    return (top, left), (top + resize_height, left + resize_width)


def get_1d_rotary_pos_embed(dim, pos, theta=10000.0):
    freqs = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float32)[: dim // 2] / dim))
    freqs = torch.outer(pos.float(), freqs)
    return freqs.cos().repeat_interleave(2, dim=1).float(), freqs.sin().repeat_interleave(2, dim=1).float()


def get_3d_rotary_pos_embed(embed_dim, crops_coords, grid_size, temporal_size, theta=10000.0):
    """-> cos, sin [T * H * W, embed_dim]: (t | h | w) channel blocks of embed_dim / 4, 3/8, 3/8; linspace grid"""
    start, stop = crops_coords
    gh_n, gw_n = grid_size
    grid_h = torch.linspace(start[0], stop[0] * (gh_n - 1) / gh_n, gh_n, dtype=torch.float32)
    grid_w = torch.linspace(start[1], stop[1] * (gw_n - 1) / gw_n, gw_n, dtype=torch.float32)
    grid_t = torch.arange(temporal_size, dtype=torch.float32)
    dim_t, dim_h, dim_w = embed_dim // 4, embed_dim // 8 * 3, embed_dim // 8 * 3
    ft, fh, fw = (get_1d_rotary_pos_embed(d, g, theta) for d, g in ((dim_t, grid_t), (dim_h, grid_h), (dim_w, grid_w)))

    def combine(t, h, w):
        t = t[:, None, None, :].expand(-1, gh_n, gw_n, -1)
        h = h[None, :, None, :].expand(temporal_size, -1, gw_n, -1)
        w = w[None, None, :, :].expand(temporal_size, gh_n, -1, -1)
        return torch.cat([t, h, w], dim=-1).reshape(temporal_size * gh_n * gw_n, -1)
    return combine(ft[0], fh[0], fw[0]), combine(ft[1], fh[1], fw[1])


def rotary_tables(cfg, frames, h, w):
    """pipeline_cogvideox_image2video.py:544-571 on the token grid"""
    p = cfg.patch_size
    crops = get_resize_crop_region_for_grid((h, w), cfg.sample_width // p, cfg.sample_height // p)
    return get_3d_rotary_pos_embed(cfg.attention_head_dim, crops, (h, w), frames)


def apply_rotary_emb(x, freqs_cis):
    """use_real=True, use_real_unbind_dim=-1; x [B, H, S, D]"""
    cos, sin = freqs_cis
    cos, sin = cos[None, None].to(x.device), sin[None, None].to(x.device)
    x_real, x_imag = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
    x_rotated = torch.stack([-x_imag, x_real], dim=-1).flatten(3)
    return (x.float() * cos + x_rotated.float() * sin).to(x.dtype)


class CogVideoXAttnProcessor2_0:
    """joint attention over [text | video] tokens; per-head LayerNorm on q and k, then the rotation of their video rows"""

    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask=None, image_rotary_emb=None):
        tl = encoder_hidden_states.size(1)
        x = torch.cat([encoder_hidden_states, hidden_states], dim=1)
        b = x.shape[0]
        hd = attn.inner_dim // attn.heads
        q, k, v = (m(x).view(b, -1, attn.heads, hd).transpose(1, 2) for m in (attn.to_q, attn.to_k, attn.to_v))
        if attn.norm_q is not None:
            q = attn.norm_q(q)
        if attn.norm_k is not None:
            k = attn.norm_k(k)
        if image_rotary_emb is not None:
            q = torch.cat([q[:, :, :tl], apply_rotary_emb(q[:, :, tl:], image_rotary_emb)], dim=2)
            k = torch.cat([k[:, :, :tl], apply_rotary_emb(k[:, :, tl:], image_rotary_emb)], dim=2)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=attention_mask, dropout_p=0.0, is_causal=False)
        o = o.transpose(1, 2).reshape(b, -1, attn.heads * hd)
        o = attn.to_out[1](attn.to_out[0](o))
        enc, hid = o.split([tl, o.size(1) - tl], dim=1)
        return hid, enc


class CogVideoXPatchEmbed(nn.Module):
    def __init__(self, patch_size=2, patch_size_t=None, in_channels=16, embed_dim=1920, text_embed_dim=4096, bias=True,
                 sample_width=90, sample_height=60, sample_frames=49, temporal_compression_ratio=4,
                 max_text_seq_length=226, spatial_interpolation_scale=1.875, temporal_interpolation_scale=1.0,
                 use_positional_embeddings=True, use_learned_positional_embeddings=False):
        super().__init__()
        assert patch_size_t is None
        self.patch_size, self.embed_dim = patch_size, embed_dim
        self.sample_height, self.sample_width, self.sample_frames = sample_height, sample_width, sample_frames
        self.temporal_compression_ratio, self.max_text_seq_length = temporal_compression_ratio, max_text_seq_length
        self.spatial_interpolation_scale, self.temporal_interpolation_scale = spatial_interpolation_scale, temporal_interpolation_scale
        self.use_positional_embeddings = use_positional_embeddings
        self.use_learned_positional_embeddings = use_learned_positional_embeddings
        self.proj = nn.Conv2d(in_channels, embed_dim, kernel_size=(patch_size, patch_size), stride=patch_size, bias=bias)
        self.text_proj = nn.Linear(text_embed_dim, embed_dim)
        if use_positional_embeddings or use_learned_positional_embeddings:
            self.register_buffer("pos_embedding", self._get_positional_embeddings(sample_height, sample_width, sample_frames),
                                 persistent=use_learned_positional_embeddings)

    def _get_positional_embeddings(self, sample_height, sample_width, sample_frames):
        h, w = sample_height // self.patch_size, sample_width // self.patch_size
        t = (sample_frames - 1) // self.temporal_compression_ratio + 1
        pe = torch.from_numpy(oc.get_3d_sincos_pos_embed(self.embed_dim, (w, h), t, self.spatial_interpolation_scale,
                                                         self.temporal_interpolation_scale)).float().flatten(0, 1)
        joint = torch.zeros(1, self.max_text_seq_length + t * h * w, self.embed_dim)
        if joint.device.type != "meta":
            joint[:, self.max_text_seq_length:] = pe
        return joint

    def forward(self, text_embeds, image_embeds):
        text_embeds = self.text_proj(text_embeds)
        b, f, c, h, w = image_embeds.shape
        x = self.proj(image_embeds.reshape(-1, c, h, w))
        x = x.view(b, f, *x.shape[1:]).flatten(3).transpose(2, 3).flatten(1, 2)
        embeds = torch.cat([text_embeds, x], dim=1).contiguous()
        if self.use_positional_embeddings or self.use_learned_positional_embeddings:
            if self.use_learned_positional_embeddings and (self.sample_width != w or self.sample_height != h):
                raise ValueError("It is currently not possible to generate videos at a different resolution that the defaults.")
            pre = (f - 1) * self.temporal_compression_ratio + 1
            if self.sample_height != h or self.sample_width != w or self.sample_frames != pre:
                pos = self._get_positional_embeddings(h, w, pre).to(embeds.device)
            else:
                pos = self.pos_embedding
            embeds = embeds + pos.to(embeds.dtype)
        return embeds


# ------------------------------------------------------------------------------------------------ the model
class CogVideoXBlock(oc.CogVideoXBlock):
    """cogvideox_transformer_3d.py:121-160 with ``image_rotary_emb`` handed to the attention"""

    def forward(self, hidden_states, encoder_hidden_states, temb, image_rotary_emb=None):
        tl = encoder_hidden_states.size(1)
        n, ne, g, eg = self.norm1(hidden_states, encoder_hidden_states, temb)
        a, ea = self.attn1(hidden_states=n, encoder_hidden_states=ne, image_rotary_emb=image_rotary_emb)
        hidden_states = hidden_states + g * a
        encoder_hidden_states = encoder_hidden_states + eg * ea
        n, ne, g, eg = self.norm2(hidden_states, encoder_hidden_states, temb)
        ff = self.ff(torch.cat([ne, n], dim=1))
        return hidden_states + g * ff[:, tl:], encoder_hidden_states + eg * ff[:, :tl]


class CogVideoXTransformer3DModel(oc.CogVideoXTransformer3DModel):
    def __init__(self, cfg: RopeDiTConfig = TINY_ROPE_DIT):
        if not cfg.use_rotary_positional_embeddings and cfg.use_learned_positional_embeddings:
            raise ValueError("There are no CogVideoX checkpoints available with disable rotary embeddings and learned positional "
                             "embeddings.")
        base = {k: v for k, v in cfg.__dict__.items() if k in oc.DiTConfig.__dataclass_fields__}
        super().__init__(oc.DiTConfig(**base))
        self.config.use_rotary_positional_embeddings = cfg.use_rotary_positional_embeddings
        self.config.use_learned_positional_embeddings = cfg.use_learned_positional_embeddings
        d = cfg.num_attention_heads * cfg.attention_head_dim
        self.patch_embed = CogVideoXPatchEmbed(
            patch_size=cfg.patch_size, in_channels=cfg.in_channels, embed_dim=d, text_embed_dim=cfg.text_embed_dim,
            sample_width=cfg.sample_width, sample_height=cfg.sample_height, sample_frames=cfg.sample_frames,
            temporal_compression_ratio=cfg.temporal_compression_ratio, max_text_seq_length=cfg.max_text_seq_length,
            spatial_interpolation_scale=cfg.spatial_interpolation_scale,
            temporal_interpolation_scale=cfg.temporal_interpolation_scale,
            use_positional_embeddings=not cfg.use_rotary_positional_embeddings,
            use_learned_positional_embeddings=cfg.use_learned_positional_embeddings)
        self.transformer_blocks = nn.ModuleList([
            CogVideoXBlock(d, cfg.num_attention_heads, cfg.attention_head_dim, cfg.time_embed_dim, cfg.attention_bias,
                           cfg.norm_eps) for _ in range(cfg.num_layers)])
        for blk in self.transformer_blocks:
            blk.attn1.processor = CogVideoXAttnProcessor2_0()

    def forward(self, hidden_states, encoder_hidden_states, timestep, domain_features, flow_features, image_rotary_emb=None,
                return_dict=False):
        b, f, c, h, w = hidden_states.shape
        emb = self.time_embedding(self.time_proj(timestep).to(hidden_states.dtype))
        encoder_hidden_states = self.lk_fuse(encoder_hidden_states, domain_features, flow_features)
        x = self.patch_embed(encoder_hidden_states, hidden_states)
        tl = encoder_hidden_states.shape[1]
        enc, hid = x[:, :tl], x[:, tl:]
        for blk in self.transformer_blocks:
            hid, enc = blk(hid, enc, emb, image_rotary_emb=image_rotary_emb)
        hid = self.norm_final(hid)
        hid = self.proj_out(self.norm_out(hid, temb=emb))
        p = self.config.patch_size
        out = hid.reshape(b, f, h // p, w // p, -1, p, p).permute(0, 1, 4, 2, 5, 3, 6).flatten(5, 6).flatten(3, 4)
        return (out,)


# ------------------------------------------------------------------------------------------------ seeded weights
def seed_pos_embedding_(m, seed: int):
    """the learned table of a seeded model: every row random, the text rows included (a stock init leaves them zero)"""
    g = torch.Generator().manual_seed(seed)
    pe = m.patch_embed.pos_embedding
    with torch.no_grad():
        pe.copy_((0.5 * torch.randn(pe.shape, generator=g)).half().float())
    return m


def seeded_model(cfg, seed: int, gain: float = NORM_QK_GAIN):
    """``init_weights_`` + every norm_q / norm_k weight x ``gain`` + fp16-representable values + the seeded learned table"""
    m = oc.init_weights_(CogVideoXTransformer3DModel(cfg), seed)
    scale_qk_norm_(m, gain)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.half().float())
    if cfg.use_learned_positional_embeddings:
        seed_pos_embedding_(m, seed + 2)
    return m


def scale_qk_norm_(m, gain: float):
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith(("attn1.norm_q.weight", "attn1.norm_k.weight")):
                p.mul_(gain)
    return m
