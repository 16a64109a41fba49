"""fp32 torch restatement of the decoder of diffusers' ``AutoencoderKLCogVideoX`` ([EXT] autoencoder_kl_cogvideox.py, PARITY UNPINNED:
diffusers is not installed and the reference tree only imports the class) as an ``nn.Module`` tree with diffusers' attribute names - the
reference of tests/test_cogvideox_vae_*.py and, in fp16 on the GPU, the ATen baseline of tools/cogvideox_vae_bench.py.

Three switches turn it into a DECOY (a plausible misreading the HIP path must stay away from):
    ``zero_time_pad``   zero padding in time instead of replicating the chunk's first frame
    ``no_split``        the spatial norm resizes zq in one piece (no first-frame split for odd frame counts)
    ``drop_cache``      the conv caches are dropped between chunks (every chunk starts from its own first frame)
and ``decode(z, whole=True)`` is the fourth: the whole clip in one pass instead of chunks of two latent frames."""
from dataclasses import dataclass, field
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F


@dataclass
class CogVAEConfig:
    block_out_channels: Tuple[int, ...] = (128, 256, 256, 512)
    latent_channels: int = 16
    layers_per_block: int = 3
    norm_eps: float = 1e-6
    norm_num_groups: int = 32
    temporal_compression_ratio: int = 4
    scaling_factor: float = 1.15258426
    out_channels: int = 3
    act_fn: str = "silu"
    use_quant_conv: bool = False
    use_post_quant_conv: bool = False
    invert_scale_latents: bool = False


TINY = CogVAEConfig(block_out_channels=(64, 64, 128, 128), layers_per_block=1)


@dataclass
class Switches:
    zero_time_pad: bool = False
    no_split: bool = False
    drop_cache: bool = False


def chunk_bounds(T: int):
    """latent-frame ranges ``decode`` runs one after the other: chunks of two, the remainder in the first"""
    n, rem = max(T // 2, 1), T % 2
    return [(2 * i + (0 if i == 0 else rem), min(2 * (i + 1) + rem, T)) for i in range(n)]


class CausalConv3d(nn.Module):
    def __init__(self, cin, cout, k, sw: Switches):
        super().__init__()
        self.k, self.sw = k, sw
        self.conv = nn.Conv3d(cin, cout, k, padding=(0, k // 2, k // 2))
        self.cache = None

    def forward(self, x):
        if self.k == 1:
            return self.conv(x)
        if self.cache is not None:
            ctx = self.cache
        elif self.sw.zero_time_pad:
            ctx = torch.zeros_like(x[:, :, :1]).repeat(1, 1, self.k - 1, 1, 1)
        else:
            ctx = x[:, :, :1].repeat(1, 1, self.k - 1, 1, 1)
        x = torch.cat([ctx, x], dim=2)
        self.cache = x[:, :, -(self.k - 1):].clone()
        return self.conv(x)


def resize_zq(zq, f, no_split=False):
    """zq resized to f's (T, H, W) by nearest interpolation, the first frame apart when f has an odd number (> 1) of frames"""
    T = f.shape[2]
    if T > 1 and T % 2 == 1 and not no_split:
        first = F.interpolate(zq[:, :, :1], size=(1,) + tuple(f.shape[-2:]))
        rest = F.interpolate(zq[:, :, 1:], size=(T - 1,) + tuple(f.shape[-2:]))
        return torch.cat([first, rest], dim=2)
    return F.interpolate(zq, size=tuple(f.shape[-3:]))


class SpatialNorm3D(nn.Module):
    def __init__(self, c, zq_c, groups, eps, sw):
        super().__init__()
        self.sw = sw
        self.norm_layer = nn.GroupNorm(groups, c, eps=eps, affine=True)
        self.conv_y = CausalConv3d(zq_c, c, 1, sw)
        self.conv_b = CausalConv3d(zq_c, c, 1, sw)

    def forward(self, f, zq):
        z = resize_zq(zq, f, self.sw.no_split)
        return self.norm_layer(f) * self.conv_y(z) + self.conv_b(z)


class ResnetBlock3D(nn.Module):
    def __init__(self, cin, cout, cfg, sw):
        super().__init__()
        self.norm1 = SpatialNorm3D(cin, cfg.latent_channels, cfg.norm_num_groups, cfg.norm_eps, sw)
        self.conv1 = CausalConv3d(cin, cout, 3, sw)
        self.norm2 = SpatialNorm3D(cout, cfg.latent_channels, cfg.norm_num_groups, cfg.norm_eps, sw)
        self.conv2 = CausalConv3d(cout, cout, 3, sw)
        self.conv_shortcut = nn.Conv3d(cin, cout, 1) if cin != cout else None

    def forward(self, x, zq):
        h = self.conv1(F.silu(self.norm1(x, zq)))
        h = self.conv2(F.silu(self.norm2(h, zq)))
        return h + (self.conv_shortcut(x) if self.conv_shortcut is not None else x)


class Upsample3D(nn.Module):
    def __init__(self, c, compress_time):
        super().__init__()
        self.compress_time = compress_time
        self.conv = nn.Conv2d(c, c, 3, padding=1)

    def forward(self, x):
        T = x.shape[2]
        if self.compress_time and T > 1 and T % 2 == 1:
            first = F.interpolate(x[:, :, 0], scale_factor=2.0)
            rest = F.interpolate(x[:, :, 1:], scale_factor=2.0)
            x = torch.cat([first[:, :, None], rest], dim=2)
        elif self.compress_time and T > 1:
            x = F.interpolate(x, scale_factor=2.0)
        else:
            B, C, _, H, W = x.shape
            x = F.interpolate(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W), scale_factor=2.0)
            x = x.reshape(B, T, C, 2 * H, 2 * W).permute(0, 2, 1, 3, 4)
        B, C, T, H, W = x.shape
        x = self.conv(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W))
        return x.reshape(B, T, C, H, W).permute(0, 2, 1, 3, 4)


class MidBlock3D(nn.Module):
    def __init__(self, c, cfg, sw):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock3D(c, c, cfg, sw) for _ in range(2)])


class UpBlock3D(nn.Module):
    def __init__(self, cin, cout, layers, add_upsample, compress_time, cfg, sw):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock3D(cin if i == 0 else cout, cout, cfg, sw) for i in range(layers)])
        self.upsamplers = nn.ModuleList([Upsample3D(cout, compress_time)]) if add_upsample else None


class Decoder3D(nn.Module):
    def __init__(self, cfg, sw):
        super().__init__()
        r = list(reversed(cfg.block_out_channels))
        self.conv_in = CausalConv3d(cfg.latent_channels, r[0], 3, sw)
        self.mid_block = MidBlock3D(r[0], cfg, sw)
        nt = cfg.temporal_compression_ratio.bit_length() - 1          # log2
        self.up_blocks = nn.ModuleList()
        c = r[0]
        for i, co in enumerate(r):
            self.up_blocks.append(UpBlock3D(c, co, cfg.layers_per_block + 1, i != len(r) - 1, i < nt, cfg, sw))
            c = co
        self.norm_out = SpatialNorm3D(r[-1], cfg.latent_channels, cfg.norm_num_groups, cfg.norm_eps, sw)
        self.conv_out = CausalConv3d(r[-1], cfg.out_channels, 3, sw)

    def forward(self, z):
        h = self.conv_in(z)
        for r in self.mid_block.resnets:
            h = r(h, z)
        for blk in self.up_blocks:
            for r in blk.resnets:
                h = r(h, z)
            if blk.upsamplers is not None:
                h = blk.upsamplers[0](h)
        return self.conv_out(F.silu(self.norm_out(h, z)))


class AutoencoderKLCogVideoX(nn.Module):
    def __init__(self, cfg: CogVAEConfig = TINY, sw: Switches = None):
        super().__init__()
        self.cfg, self.sw = cfg, sw if sw is not None else Switches()
        self.decoder = Decoder3D(cfg, self.sw)

    def clear_cache(self):
        for m in self.modules():
            if isinstance(m, CausalConv3d):
                m.cache = None

    @torch.no_grad()
    def decode(self, z, whole=False):
        """[B, 16, T, h, w] -> [B, 3, T', 8h, 8w]"""
        self.clear_cache()
        outs = []
        for a, b in ([(0, z.shape[2])] if whole else chunk_bounds(z.shape[2])):
            if self.sw.drop_cache:
                self.clear_cache()
            outs.append(self.decoder(z[:, :, a:b]))
        self.clear_cache()
        return torch.cat(outs, dim=2)


def decode_latents(vae, latents):
    """pipeline_cogvideox_image2video.py:430-435"""
    return vae.decode(latents.permute(0, 2, 1, 3, 4) * (1.0 / vae.cfg.scaling_factor))


def tiny_pair_weights(seed=1, cfg=TINY):
    """the test recipe: default torch init from ``seed``, 1.0 added to every conv_y bias, weights rounded to fp16 values"""
    torch.manual_seed(seed)
    o = AutoencoderKLCogVideoX(cfg)
    with torch.no_grad():
        for n, p in o.named_parameters():
            if n.endswith("conv_y.conv.bias"):
                p.add_(1.0)
            p.copy_(p.half().float())
    return o


def with_switches(o, **sw):
    """a copy of ``o`` (same weights) with decoy switches set"""
    d = AutoencoderKLCogVideoX(o.cfg, Switches(**sw))
    d.load_state_dict(o.state_dict())
    return d.to(next(o.parameters()).device, next(o.parameters()).dtype)


def tiny_latents(T, B=1, seed=2):
    """z [B, 16, T, 6, 10], latent frame t scaled by 1 + 2t, fp16 values"""
    g = torch.Generator().manual_seed(seed + T)
    z = torch.randn(B, 16, T, 6, 10, generator=g)
    z = z * (1.0 + 2.0 * torch.arange(T, dtype=torch.float32))[None, None, :, None, None]
    return z.half().float()
