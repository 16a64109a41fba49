"""fp32 torch restatement of the ENCODER of diffusers' ``AutoencoderKLCogVideoX`` ([EXT] autoencoder_kl_cogvideox.py, PARITY UNPINNED:
diffusers is not installed and the reference tree only imports the class) with diffusers' attribute names, next to the decoder of
tests/cogvideox_vae_oracle.py - the reference of tests/test_cogvideox_vae_encoder_*.py and, in fp16 on the GPU, the ATen baseline of
tools/cogvideox_vae_encode_bench.py.

Five switches turn it into a DECOY (a plausible misreading the HIP path must stay away from):
    ``zero_time_pad``    zeros, not the first frame, in front of the first frame batch
    ``pad_symmetric``    the downsampler's convolution padded 1 on all sides instead of F.pad(0,1,0,1)
    ``pool_split_last``  odd frame counts pooled with the LAST frame apart instead of the first
    ``drop_cache``       the conv caches dropped between frame batches
    ``remainder_last``   the remainder of the frame count in the last batch (17 -> 8|9) instead of the first (9|8)
and ``moments(x, whole=True)`` is the sixth: the whole clip in one pass instead of frame batches of eight."""
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

import cogvideox_vae_oracle as oc
from cogvideox_vae_oracle import TINY, CogVAEConfig  # noqa: F401  (re-exported: the tests take them from here)

FRAME_BATCH = 8
IN_CHANNELS = 3


@dataclass
class Switches:
    zero_time_pad: bool = False
    pad_symmetric: bool = False
    pool_split_last: bool = False
    drop_cache: bool = False
    remainder_last: bool = False


def frame_batch_bounds(T: int, remainder_last: bool = False):
    """frame ranges ``encode`` runs one after the other: batches of eight, the remainder in the first (``_encode``)"""
    n, rem = max(T // FRAME_BATCH, 1), T % FRAME_BATCH
    if remainder_last:
        return [(FRAME_BATCH * i, min(FRAME_BATCH * (i + 1) + (rem if i == n - 1 else 0), T)) for i in range(n)]
    return [(FRAME_BATCH * i + (0 if i == 0 else rem), min(FRAME_BATCH * (i + 1) + rem, T)) for i in range(n)]


def time_pool(x, split_last=False):
    """the ``compress_time`` half of CogVideoXDownsample3D.forward as diffusers writes it: [B, C, T, H, W] -> [B, C, T', H, W]"""
    B, C, T, H, W = x.shape
    x = x.permute(0, 3, 4, 1, 2).reshape(B * H * W, C, T)
    if T % 2 == 1:
        if split_last:
            rest, last = x[..., :-1], x[..., -1]
            if rest.shape[-1] > 0:
                rest = F.avg_pool1d(rest, kernel_size=2, stride=2)
            x = torch.cat([rest, last[..., None]], dim=-1)
        else:
            first, rest = x[..., 0], x[..., 1:]
            if rest.shape[-1] > 0:
                rest = F.avg_pool1d(rest, kernel_size=2, stride=2)
            x = torch.cat([first[..., None], rest], dim=-1)
    else:
        x = F.avg_pool1d(x, kernel_size=2, stride=2)
    return x.reshape(B, H, W, C, x.shape[-1]).permute(0, 3, 4, 1, 2)


class EncResnetBlock3D(nn.Module):
    def __init__(self, cin, cout, cfg, sw):
        super().__init__()
        self.norm1 = nn.GroupNorm(cfg.norm_num_groups, cin, eps=cfg.norm_eps)
        self.conv1 = oc.CausalConv3d(cin, cout, 3, sw)
        self.norm2 = nn.GroupNorm(cfg.norm_num_groups, cout, eps=cfg.norm_eps)
        self.conv2 = oc.CausalConv3d(cout, cout, 3, sw)
        self.conv_shortcut = nn.Conv3d(cin, cout, 1) if cin != cout else None

    def forward(self, x):
        h = self.conv1(F.silu(self.norm1(x)))
        h = self.conv2(F.silu(self.norm2(h)))
        return h + (self.conv_shortcut(x) if self.conv_shortcut is not None else x)


class Downsample3D(nn.Module):
    def __init__(self, c, compress_time, sw):
        super().__init__()
        self.compress_time, self.sw = compress_time, sw
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)

    def forward(self, x):
        if self.compress_time:
            x = time_pool(x, self.sw.pool_split_last)
        x = F.pad(x, (1, 1, 1, 1) if self.sw.pad_symmetric else (0, 1, 0, 1))
        B, C, T, H, W = x.shape
        x = self.conv(x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W))
        return x.reshape(B, T, C, x.shape[-2], x.shape[-1]).permute(0, 2, 1, 3, 4)


class EncMidBlock3D(nn.Module):
    def __init__(self, c, cfg, sw):
        super().__init__()
        self.resnets = nn.ModuleList([EncResnetBlock3D(c, c, cfg, sw) for _ in range(2)])


class DownBlock3D(nn.Module):
    def __init__(self, cin, cout, layers, add_downsample, compress_time, cfg, sw):
        super().__init__()
        self.resnets = nn.ModuleList([EncResnetBlock3D(cin if i == 0 else cout, cout, cfg, sw) for i in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample3D(cout, compress_time, sw)]) if add_downsample else None


class Encoder3D(nn.Module):
    def __init__(self, cfg, sw):
        super().__init__()
        ch = list(cfg.block_out_channels)
        self.conv_in = oc.CausalConv3d(IN_CHANNELS, ch[0], 3, sw)
        nt = cfg.temporal_compression_ratio.bit_length() - 1          # log2
        self.down_blocks = nn.ModuleList()
        c = ch[0]
        for i, co in enumerate(ch):
            self.down_blocks.append(DownBlock3D(c, co, cfg.layers_per_block, i != len(ch) - 1, i < nt, cfg, sw))
            c = co
        self.mid_block = EncMidBlock3D(ch[-1], cfg, sw)
        self.norm_out = nn.GroupNorm(cfg.norm_num_groups, ch[-1], eps=1e-6)
        self.conv_out = oc.CausalConv3d(ch[-1], 2 * cfg.latent_channels, 3, sw)

    def forward(self, x):
        h = self.conv_in(x)
        for blk in self.down_blocks:
            for r in blk.resnets:
                h = r(h)
            if blk.downsamplers is not None:
                h = blk.downsamplers[0](h)
        for r in self.mid_block.resnets:
            h = r(h)
        return self.conv_out(F.silu(self.norm_out(h)))


class AutoencoderKLCogVideoX(nn.Module):
    """encoder + decoder: the state dict a checkpoint's ``vae/`` holds (without the optional quant convolutions)"""

    def __init__(self, cfg: CogVAEConfig = TINY, sw: Switches = None):
        super().__init__()
        self.cfg, self.sw = cfg, sw if sw is not None else Switches()
        self.encoder = Encoder3D(cfg, self.sw)
        self.decoder = oc.Decoder3D(cfg, oc.Switches())

    def clear_cache(self):
        for m in self.modules():
            if isinstance(m, oc.CausalConv3d):
                m.cache = None

    @torch.no_grad()
    def moments(self, x, whole=False):
        """[B, 3, T, H, W] -> [B, 2*16, T', H/8, W/8]: mean | log-variance as conv_out leaves them"""
        self.clear_cache()
        outs = []
        for a, b in ([(0, x.shape[2])] if whole else frame_batch_bounds(x.shape[2], self.sw.remainder_last)):
            if self.sw.drop_cache:
                self.clear_cache()
            outs.append(self.encoder(x[:, :, a:b]))
        self.clear_cache()
        return torch.cat(outs, dim=2)

    def posterior(self, x):
        """(mean, clamped logvar, std) of ``moments(x)`` - DiagonalGaussianDistribution"""
        mean, logvar = self.moments(x).chunk(2, dim=1)
        logvar = torch.clamp(logvar, -30.0, 20.0)
        return mean, logvar, torch.exp(0.5 * logvar)


def tiny_weights(seed=1, cfg=TINY):
    """the test recipe: default torch init from ``seed``, weights rounded to fp16 values"""
    torch.manual_seed(seed)
    o = AutoencoderKLCogVideoX(cfg)
    with torch.no_grad():
        for p in o.parameters():
            p.copy_(p.half().float())
    return o


def with_switches(o, **sw):
    """a copy of ``o`` (same weights) with decoy switches set"""
    d = AutoencoderKLCogVideoX(o.cfg, Switches(**sw))
    d.load_state_dict(o.state_dict())
    return d


def tiny_clip(T, B=1, seed=3):
    """x [B, 3, T, 48, 80]: 0.5 randn + sin(0.9 t), clamped to [-1, 1], fp16 values"""
    g = torch.Generator().manual_seed(seed + T)
    x = 0.5 * torch.randn(B, 3, T, 48, 80, generator=g)
    x = x + torch.sin(0.9 * torch.arange(T, dtype=torch.float32))[None, None, :, None, None]
    return x.clamp(-1.0, 1.0).half().float()


#: decoy -> the frame counts at which it differs from the truth (relative L2 of the moments, measured on the CPU with this recipe;
#: see tests/test_cogvideox_vae_encoder_gpu.py) and those at which it is the truth itself
DECOYS = {
    "zero_time_pad": dict(differs=(1, 2, 5, 9, 16, 17), equal=()),
    "pad_symmetric": dict(differs=(1, 2, 5, 9, 16, 17), equal=()),
    "pool_split_last": dict(differs=(5, 9, 17, 25), equal=(1, 2)),
    "drop_cache": dict(differs=(16, 17), equal=(1, 2, 5)),
    "remainder_last": dict(differs=(17,), equal=(1, 5, 16)),
    "whole": dict(differs=(16, 17), equal=(1, 2, 5)),
}


def decoy_moments(o, name, x):
    if name == "whole":
        return o.moments(x, whole=True)
    return with_switches(o, **{name: True}).moments(x)
