"""The CogVideoX 3-D causal VAE (``AutoencoderKLCogVideoX``) on the MI355X path: the decoder (denoised latents -> frames, the last
boundary stage of the CogVideoX pipeline) and, built on request (``encoder=True``), the encoder (image or clip -> the posterior
whose sample conditions every step of the image-to-video loop).

Call sites in the reference: CogVideo-main/finetune/models/cogvideox_i2v/pipeline_cogvideox_image2video.py:430-435 (``decode_latents``:
permute, ``1 / scaling_factor``, ``vae.decode(latents).sample``), called at :908; ``inference/cli_vae_demo.py`` (``model.decode``).
The class itself is diffusers' ``autoencoder_kl_cogvideox.py`` - [EXT], PARITY UNPINNED: diffusers is not vendored and the reference
tree only imports the class, so module tree, parameter names and arithmetic restate the published source
(tests/cogvideox_vae_oracle.py carries the same restatement in fp32 torch).  A real ``vae/`` checkpoint loads with
``from_pretrained`` / ``load_state_dict``: its ``quant_conv.*`` keys are accepted and DROPPED, and so are its ``encoder.*`` keys when
the module was constructed without its encoder (the default: ``encode`` then raises); with ``encoder=True`` the ``encoder.*`` keys
load strictly.  Any other missing or unexpected key raises.

MI355X design: channels-last fp16 token matrices [B*T*H*W, C], rows (b, t, y, x) -
* every causal 3x3x3 convolution is ONE implicit-GEMM launch (``LKGD_A_CCONV3``: 27 taps, fp32 accumulation) over a buffer that
  holds two context frames in front of the chunk's frames per batch entry: the chunk's first frame twice, or the conv cache = the
  last two frames of the previous chunk's buffer.  The producer of the convolution's input - the spatial norm - writes straight
  into that buffer behind the context frames;
* ``CogVideoXSpatialNorm3D`` is ``lkgd_spatial_norm3d``: GroupNorm apply, modulation by conv_y(zq) / conv_b(zq) and SiLU in one
  pass.  The two 1x1x1 convolutions commute with the nearest resize of zq, so they run once per chunk and norm on the LATENT grid
  (one plain GEMM, K 16 -> 64 padded, N = 2C) and the kernel gathers their rows through a frame table and a shift;
* ``CogVideoXUpsample3D``: the per-frame 3x3 convolution with the nearest 2x folded into its gather (``LKGD_A_CONV3X3``, ups = 1);
  the doubling in time commutes with it - T frames are convolved once and each result placed twice (a strided device copy).
Activations are fp16 with fp32 accumulation whatever dtype the parameters are kept in.  Chunks of two latent frames, as diffusers.

The encoder (call sites pipeline_cogvideox_image2video.py:386-393 ``prepare_latents`` and
inference/cli_vae_demo.py:63) runs frame batches of eight, the remainder in the first, on the same token matrices -
* ``conv_in`` (3 pixel channels) is ``lkgd_cogvae_pixel_taps`` + ONE plain GEMM with K = 128: the taps are gathered from the clip
  itself, whose earlier frames are the conv cache, so neither a cache nor a context-prefixed buffer exists for it;
* the resnets' plain GroupNorm + SiLU is ``lkgd_groupnorm_apply`` writing behind the two context frames of the buffer the causal
  convolution reads (statistics over the batch's frames, from the producing GEMM's column sums where the tile form allows);
* ``CogVideoXDownsample3D``: ``lkgd_cogvae_time_pool`` (where ``compress_time``) in front of the stride-2 ``LKGD_A_CONV3X3`` with
  ``pad_off = 1`` (F.pad(0,1,0,1) + padding 0), one image per frame;
* ``lkgd_cogvae_posterior`` turns ``conv_out``'s moment rows into the mean and the scaled sample, [B, 16, T, h, w].

Tiling and slicing (every entry point of the reference calls ``vae.enable_slicing()`` and
``vae.enable_tiling()``: inference/cli_demo.py:151-152, finetune/trainer.py:156-159).  With ``use_tiling`` an input larger than one tile
(half the configured sample size: 240 x 360 pixels, 30 x 45 latents) is cut into overlapping tiles, every tile runs through the paths
above ALONE - its own GroupNorm statistics, its own zero padding - and the seams are cross-faded, so a tiled result is another function
of the input than an untiled one (``decode_tile_geometry`` / ``encode_tile_geometry`` hold diffusers' arithmetic).  Tiles run one at a
time (``LKGD_COGVAE_TILE_BATCH=1``: tiles of equal shape as the entries of one batch - within the gate, but not the same bits, see
``tile_batch``), and the seams and the placement of a tile are ONE launch per tile, ``lkgd_cogvae_tile_blend_planar`` on the decoded
frames and ``lkgd_cogvae_tile_blend_rows`` on the encoder's moment rows (include/lkgd_hip_cogvae_tile.h).  With ``use_slicing`` a batch
decodes entry by entry (``encode`` always does).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from types import SimpleNamespace
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from ._lib import LkgdHipError
from .module import PackedModule
from .packing import f32, pack_cconv3, pack_conv3x3, pack_linear
from .vae import DecoderOutput, _new, _pad_cout

#: frames per batch of ``encode`` (diffusers' num_sample_frames_batch_size)
ENCODE_FRAME_BATCH = 8


@dataclass
class CogVAEConfig:
    """constructor keywords of AutoencoderKLCogVideoX [EXT] the decoder and the encoder read (CogVideoX ``vae/config.json``)"""
    block_out_channels: Tuple[int, ...] = (128, 256, 256, 512)
    latent_channels: int = 16
    layers_per_block: int = 3
    norm_eps: float = 1e-6
    norm_num_groups: int = 32
    temporal_compression_ratio: int = 4
    scaling_factor: float = 1.15258426          # 2B; 0.7 for 5B
    out_channels: int = 3
    in_channels: int = 3
    act_fn: str = "silu"
    use_quant_conv: bool = False
    use_post_quant_conv: bool = False
    invert_scale_latents: bool = False
    sample_height: int = 480                    # 768 / 1360 in the 1.5 checkpoints; half of each is the default tile
    sample_width: int = 720


def _spatial_factor(cfg) -> int:
    """pixels per latent in height and width: every block but the last halves (the encoder) or doubles (the decoder) them"""
    return 2 ** (len(cfg.block_out_channels) - 1)


def _time_levels(cfg) -> int:
    """how many blocks, counted from the encoder's first / the decoder's first, also halve / double the frames"""
    return cfg.temporal_compression_ratio.bit_length() - 1


@dataclass
class TileGeometry:
    """how one tiled pass cuts its input and assembles its output.  ``rows`` / ``cols``: (origin, size) of every tile row / column in
    INPUT units (latents for the decode, pixels for the encode); ``step``: the distance of two origins, input units; ``extent``: the
    rows / columns that are cross-faded with the neighbour, ``crop``: what a tile contributes, ``out_rows`` / ``out_cols``: (origin,
    size) of every tile's crop in the output - all three in OUTPUT units (pixels for the decode, latents for the encode)"""
    step: Tuple[int, int]
    extent: Tuple[int, int]
    crop: Tuple[int, int]
    rows: List[Tuple[int, int]]
    cols: List[Tuple[int, int]]
    out_rows: List[Tuple[int, int]]
    out_cols: List[Tuple[int, int]]


def _tile_axis(n: int, size: int, step: int) -> List[Tuple[int, int]]:
    return [(o, min(size, n - o)) for o in range(0, n, step)]


def _crop_axis(tiles: List[int], crop: int, total: int, what: str) -> List[Tuple[int, int]]:
    """(origin, size) of the tiles' crops laid side by side; they must add up to ``total`` (diffusers returns a tensor of another
    size when they do not)"""
    out, o = [], 0
    for t in tiles:
        out.append((o, min(crop, t)))
        o += out[-1][1]
    if o != total:
        raise LkgdHipError(f"AutoencoderKLCogVideoX: the tiles do not add up - {what}: the cropped tiles cover {o}, the output has "
                           f"{total}")
    return out


def _tile_geometry(n_h: int, n_w: int, in_tile, out_tile, f, to_out, unit: int, what: str) -> TileGeometry:
    """diffusers' tile arithmetic over an n_h x n_w input: tiles of ``in_tile`` (h, w) input units every int(in_tile * (1 - f)),
    int(out_tile * f) output units cross-faded, out_tile - int(out_tile * f) kept of every tile (f: the overlap factors).  The
    Python float expressions are diffusers'.  ``to_out``: input units -> output units; a tile must be a multiple of ``unit`` input
    units; ``what`` names the setting in a refusal, with {} for the two steps and the two crops."""
    step = (int(in_tile[0] * (1 - f[0])), int(in_tile[1] * (1 - f[1])))
    extent = (int(out_tile[0] * f[0]), int(out_tile[1] * f[1]))
    crop = (out_tile[0] - extent[0], out_tile[1] - extent[1])
    what = what.format(*step, *crop)
    if min(step) <= 0 or min(crop) <= 0:
        raise LkgdHipError(f"AutoencoderKLCogVideoX: the tiles do not add up - {what}")
    rows, cols = _tile_axis(n_h, in_tile[0], step[0]), _tile_axis(n_w, in_tile[1], step[1])
    for _, s in rows + cols:
        if s % unit:
            raise LkgdHipError(f"AutoencoderKLCogVideoX: the tiles do not add up - {what}: a tile of {s} pixels is no multiple of {unit}")
    return TileGeometry(step, extent, crop, rows, cols,
                        _crop_axis([to_out(s) for _, s in rows], crop[0], to_out(n_h), what + ", height"),
                        _crop_axis([to_out(s) for _, s in cols], crop[1], to_out(n_w), what + ", width"))


#: a tiling setting as a refusal names it: sample tile, latent tile, overlap factors, (input units, output units), input size and unit
_TILING = ("tile_sample_min {} x {}, tile_latent_min {} x {}, overlap factors {:.4g} / {:.4g} (step {{}} / {{}} {}, crop {{}} / {{}} {}) "
           "over {} x {} {}")


def decode_tile_geometry(h: int, w: int, S_h: int, S_w: int, L_h: int, L_w: int, f_h: float, f_w: float, up: int = 8) -> TileGeometry:
    """``tiled_decode`` of diffusers over an h x w latent grid: tiles of L_h x L_w latents (the minimal latent tile), pixels
    cross-faded and kept (S: the minimal sample tile)"""
    return _tile_geometry(h, w, (L_h, L_w), (S_h, S_w), (f_h, f_w), lambda s: up * s, 1,
                          _TILING.format(S_h, S_w, L_h, L_w, f_h, f_w, "latents", "pixels", h, w, "latents"))


def encode_tile_geometry(H: int, W: int, S_h: int, S_w: int, L_h: int, L_w: int, f_h: float, f_w: float, down: int = 8) -> TileGeometry:
    """``tiled_encode`` of diffusers over H x W pixels: tiles of S_h x S_w pixels, each a multiple of ``down`` pixels, latents
    cross-faded and kept"""
    return _tile_geometry(H, W, (S_h, S_w), (L_h, L_w), (f_h, f_w), lambda s: s // down, down,
                          _TILING.format(S_h, S_w, L_h, L_w, f_h, f_w, "pixels", "latents", H, W, "pixels"))


def _tile_groups(g: TileGeometry, batch: bool) -> List[List[Tuple[int, int]]]:
    """the tiles (i, j) in the runs they are computed in: tiles of equal shape together (480 x 720: 4 + 2 + 2 + 1), or one by one"""
    by_shape = {}
    for i, (_, sy) in enumerate(g.rows):
        for j, (_, sx) in enumerate(g.cols):
            by_shape.setdefault((sy, sx), []).append((i, j))
    runs = list(by_shape.values())
    return runs if batch else [[ij] for run in runs for ij in run]


def tile_batch() -> bool:
    """``LKGD_COGVAE_TILE_BATCH=1``: tiles of equal shape run as the entries of one batch; the default (``0``) is one tile at a time.
    A/B switch, read at every call.  The default is the form whose every tile is bit for bit what the untiled path gives for that
    tile alone: the GEMM planner picks its program by the row count, so an entry of a batch is NOT bit-identical to a single run
    (measured on the tiny decode: about a third of the elements differ in the last bits; both forms are 6e-4 - 1.2e-3 from the
    oracle), and profiles/cogvideox_vae_tiling_bench.json records what batching would buy."""
    return os.environ.get("LKGD_COGVAE_TILE_BATCH", "0") == "1"


def _group_bounds(T: int, size: int) -> List[Tuple[int, int]]:
    """the frame ranges a clip runs in, one after the other: groups of ``size``, the remainder in the FIRST; fewer than ``size``
    frames are one group"""
    n, rem = max(T // size, 1), T % size
    return [(size * i + (0 if i == 0 else rem), min(size * (i + 1) + rem, T)) for i in range(n)]


def chunk_bounds(T: int) -> List[Tuple[int, int]]:
    """the latent-frame ranges ``decode`` runs one after the other: chunks of two (13 -> 3|2|2|2|2|2)"""
    return _group_bounds(T, 2)


def frame_batch_bounds(T: int) -> List[Tuple[int, int]]:
    """the frame ranges ``encode`` runs one after the other: batches of eight (49 -> 9|8|8|8|8|8; AutoencoderKLCogVideoX._encode)"""
    return _group_bounds(T, ENCODE_FRAME_BATCH)


def _run_clip(step, clip: torch.Tensor, bounds, out: torch.Tensor) -> None:
    """one clip through its frame groups: ``step(clip, a, b, out, t_out, caches)`` runs frames [a, b), writes its output frames
    into ``out`` from ``t_out`` on and returns their count.  ``caches`` - {causal convolution: the last two frames of its previous
    group's buffer} - belongs to this clip alone and is gone when the loop returns or raises: a tile, a batch entry and a slice
    each start without context."""
    caches, t_out = {}, 0
    for a, b in bounds:
        t_out += step(clip, a, b, out, t_out, caches)


def _run_tiles(g: TileGeometry, cut, run, blend, new_out) -> torch.Tensor:
    """one tiled pass.  The tiles are computed in the runs of ``_tile_groups`` (one at a time, or under ``tile_batch()`` tiles of
    equal shape as one batch): ``cut(ys, xs)`` is that window of the input, ``run`` turns the concatenated windows into their
    results, first dimension the tile.  Then in row-major order ONE ``blend`` launch per tile: the cross-fade with its upper and
    left neighbours' blended tiles, and its crop into the output.  ``new_out()`` is asked for the output only then - the decoded
    frames do not exist while the tiles run."""
    tiles = {}
    for grp in _tile_groups(g, tile_batch()):
        sy, sx = g.rows[grp[0][0]][1], g.cols[grp[0][1]][1]
        res = run(torch.cat([cut(slice(g.rows[i][0], g.rows[i][0] + sy), slice(g.cols[j][0], g.cols[j][0] + sx))
                             for i, j in grp]).contiguous())
        for k, ij in enumerate(grp):
            tiles[ij] = res[k]
    out = new_out()
    for i, (y0, _) in enumerate(g.out_rows):
        for j, (x0, _) in enumerate(g.out_cols):
            blend(tiles[i, j], tiles.get((i - 1, j)), tiles.get((i, j - 1)), out, y0, x0, g.extent[0], g.extent[1], g.crop[0], g.crop[1])
    return out


def spatial_norm_tmap(Tz: int, T: int) -> List[int]:
    """latent frame of every one of f's T frames: nearest resize of Tz frames to T, the first frame apart when T is odd and above one
    (CogVideoXSpatialNorm3D.forward)"""
    if T > 1 and T % 2 == 1:
        if Tz < 2:
            raise LkgdHipError("spatial norm: an odd chunk of more than one frame needs at least two latent frames")
        return [0] + [1 + (i * (Tz - 1)) // (T - 1) for i in range(T - 1)]
    return [(t * Tz) // T for t in range(T)]


def upsample_frame_map(T: int, compress_time: bool) -> List[int]:
    """source frame of every output frame of CogVideoXUpsample3D: with ``compress_time`` frames are doubled - all of an even count,
    all but the first of an odd count above one; a single frame stays single"""
    if not compress_time or T == 1:
        return list(range(T))
    if T % 2 == 1:
        return [0] + [1 + i // 2 for i in range(2 * (T - 1))]
    return [i // 2 for i in range(2 * T)]


class _Chunk:
    """what the blocks of one chunk share: geometry, the padded latent rows, the per-(Tz, T) frame tables and the clip's conv
    caches (``_run_clip``)"""

    def __init__(self, B, Tz, h, w, zq64, caches):
        self.B, self.Tz, self.h, self.w, self.zq64, self.caches = B, Tz, h, w, zq64, caches
        self.T, self.H, self.W, self.sh = Tz, h, w, 0
        self._tmaps = {}

    def tmap(self):
        t = self._tmaps.get(self.T)
        if t is None:
            t = self._tmaps[self.T] = torch.tensor(spatial_norm_tmap(self.Tz, self.T), dtype=torch.int32).to(self.zq64.device)
        return t


def _prefixed(c: _Chunk, C_: int, dev) -> torch.Tensor:
    """[B, T + 2, H*W, C]: two context frames, then the chunk's frames"""
    return torch.empty(c.B, c.T + 2, c.H * c.W, C_, dtype=torch.float16, device=dev)


# ------------------------------------------------------------------------------------------------ parameter holders
class CogVideoXCausalConv3d(nn.Module):
    """CogVideoXCausalConv3d(cin, cout, k) [EXT]: zero padding k//2 in height / width, k - 1 context frames in time"""

    def __init__(self, cin: int, cout: int, k: int):
        super().__init__()
        self.cin, self.cout, self.k = cin, cout, k
        self.conv = nn.Conv3d(cin, cout, k, padding=(0, k // 2, k // 2))

    def pack(self, pad_cin: int = 0, pad_cout: int = 0):
        w, b = self.conv.weight.detach().float(), self.conv.bias.detach().float()
        if pad_cin and w.shape[1] < pad_cin:
            w = torch.nn.functional.pad(w, (0, 0, 0, 0, 0, 0, 0, pad_cin - w.shape[1]))
        if pad_cout:
            w, b = _pad_cout(w, b, pad_cout)
        self._cin, self._n = w.shape[1], w.shape[0]
        self._w, self._b = pack_cconv3(w), b.contiguous()

    def run(self, P: torch.Tensor, c: _Chunk, res1=None, colstats: int = 0):
        """``P`` = [B, T + 2, H*W, Cin] with the chunk's frames in place behind two free frames: puts the context there, leaves the
        buffer's last two frames in ``c.caches`` as the next chunk's context, convolves"""
        if self not in c.caches:
            P[:, 0] = P[:, 2]
            P[:, 1] = P[:, 2]
        else:
            P[:, :2] = c.caches[self]
        c.caches[self] = P[:, -2:].clone()
        M = c.B * c.T * c.H * c.W
        out = _new(M, self._n, P.device)
        ops.gemm(P.view(-1, self._cin), self._w, out, M=M, N=self._n, K=27 * self._cin, bias=self._b, mode=ops.A_CCONV3,
                 Cin=self._cin, cconv=(c.T, c.H, c.W), res1=res1, colstats=colstats)
        return out


class CogVideoXSpatialNorm3D(nn.Module):
    """CogVideoXSpatialNorm3D(C, zq_channels) [EXT]: norm_layer(f) * conv_y(zq') + conv_b(zq')"""

    def __init__(self, c: int, zq: int, groups: int, eps: float):
        super().__init__()
        self.c, self.eps = c, eps
        self.norm_layer = nn.GroupNorm(groups, c, eps=eps, affine=True)
        self.conv_y = CogVideoXCausalConv3d(zq, c, 1)
        self.conv_b = CogVideoXCausalConv3d(zq, c, 1)

    def pack(self):
        self._g, self._bt = f32(self.norm_layer.weight), f32(self.norm_layer.bias)
        wy, wb = pack_linear(self.conv_y.conv.weight.detach()), pack_linear(self.conv_b.conv.weight.detach())
        w = torch.cat([wy, wb])                                       # [2C, zq]: the 1x1x1 pair as one GEMM on the latent grid
        self._wyb = torch.nn.functional.pad(w, (0, 64 - w.shape[1])).contiguous()
        self._byb = torch.cat([f32(self.conv_y.conv.bias), f32(self.conv_b.conv.bias)]).contiguous()

    def run(self, x: torch.Tensor, c: _Chunk, silu: bool = True):
        """norm (+ SiLU) of the chunk's rows ``x`` into a fresh [B, T + 2, H*W, C] buffer behind its two context frames"""
        P = _prefixed(c, self.c, x.device)
        Mz = c.B * c.Tz * c.h * c.w
        yb = _new(Mz, 2 * self.c, x.device)
        ops.gemm(c.zq64, self._wyb, yb, M=Mz, N=2 * self.c, K=64, bias=self._byb)
        stats = ops.groupnorm_stats(x, None, c.B, c.T * c.H * c.W, self.eps)
        hw = c.H * c.W
        ops.spatial_norm3d(x, stats, self._g, self._bt, yb, c.tmap(), P.view(-1, self.c)[2 * hw:], c.B, c.T, c.H, c.W, c.Tz, c.sh,
                           silu, out_batch_rows=(c.T + 2) * hw)
        return P


class CogVideoXGroupNorm(nn.GroupNorm):
    """the plain GroupNorm of the encoder (its resnets' norm1 / norm2, norm_out) with the call shape of ``CogVideoXSpatialNorm3D``;
    an ``nn.GroupNorm`` itself, so its state-dict keys are diffusers' ``...norm1.weight`` / ``...norm1.bias``"""

    def pack(self):
        self._g, self._bt = f32(self.weight), f32(self.bias)

    def run(self, x: torch.Tensor, c: _Chunk, silu: bool = True):
        """GroupNorm (+ SiLU) of the batch's rows ``x`` into a fresh [B, T + 2, H*W, C] buffer behind its two context frames: the
        statistics span the batch's frames (from the producing GEMM's column sums where it left them), then one
        ``lkgd_groupnorm_apply`` per batch entry - ``out`` behind that entry's context frames, ``stats`` offset to the entry"""
        rows, C_ = c.T * c.H * c.W, x.shape[1]
        stats = ops.groupnorm_stats(x, None, c.B, rows, self.eps)
        P = _prefixed(c, C_, x.device)
        for b in range(c.B):
            ops.groupnorm_apply(x[b * rows:(b + 1) * rows], None, 1, rows, stats[b], self._g, self._bt, silu, P[b, 2:].view(rows, C_))
        return P


def _norm(c: int, cfg: CogVAEConfig, spatial_norm: bool) -> nn.Module:
    if spatial_norm:
        return CogVideoXSpatialNorm3D(c, cfg.latent_channels, cfg.norm_num_groups, cfg.norm_eps)
    return CogVideoXGroupNorm(cfg.norm_num_groups, c, eps=cfg.norm_eps)


class CogVideoXResnetBlock3D(nn.Module):
    """CogVideoXResnetBlock3D [EXT]: the decoder's with a spatial norm dimension (``spatial_norm``), the encoder's without one"""

    def __init__(self, cin: int, cout: int, cfg: CogVAEConfig, spatial_norm: bool):
        super().__init__()
        self.cin, self.cout = cin, cout
        self.norm1 = _norm(cin, cfg, spatial_norm)
        self.conv1 = CogVideoXCausalConv3d(cin, cout, 3)
        self.norm2 = _norm(cout, cfg, spatial_norm)
        self.conv2 = CogVideoXCausalConv3d(cout, cout, 3)
        self.conv_shortcut = nn.Conv3d(cin, cout, 1) if cin != cout else None

    def pack(self):
        self.norm1.pack(); self.norm2.pack(); self.conv1.pack(); self.conv2.pack()
        if self.conv_shortcut is not None:
            self._ws, self._bs = pack_linear(self.conv_shortcut.weight.detach()), f32(self.conv_shortcut.bias)

    def run(self, x: torch.Tensor, c: _Chunk):
        """launches: [the norm - spatial: plain GEMM (conv_y | conv_b), GroupNorm statistics unless the producing GEMM left column
        sums, spatial norm; plain: the statistics likewise, GroupNorm apply per batch entry - then the causal conv] x 2, + the 1x1x1
        shortcut GEMM where the channel count changes; the residual is conv2's epilogue"""
        rows = c.T * c.H * c.W
        h = self.conv1.run(self.norm1.run(x, c), c, colstats=rows)
        P2 = self.norm2.run(h, c)
        del h
        sc = x
        if self.conv_shortcut is not None:
            sc = _new(x.shape[0], self.cout, x.device)
            ops.gemm(x, self._ws, sc, M=x.shape[0], N=self.cout, K=self.cin, bias=self._bs)
        return self.conv2.run(P2, c, res1=sc, colstats=rows)


class CogVideoXUpsample3D(nn.Module):
    def __init__(self, c: int, compress_time: bool):
        super().__init__()
        self.c, self.compress_time = c, compress_time
        self.conv = nn.Conv2d(c, c, 3, padding=1)

    def pack(self):
        self._w, self._b = pack_conv3x3(self.conv.weight.detach()), f32(self.conv.bias)

    def run(self, x: torch.Tensor, c: _Chunk):
        """conv(dup(x)) = dup(conv(x)): the T frames are convolved once (nearest 2x in height / width inside the gather), then each
        result frame is placed as often as the time doubling repeats it"""
        N, Ho, Wo = c.B * c.T, 2 * c.H, 2 * c.W
        fmap = upsample_frame_map(c.T, self.compress_time)
        To = len(fmap)
        out = _new(N * Ho * Wo, self.c, x.device)
        ops.gemm(x, self._w, out, M=N * Ho * Wo, N=self.c, K=9 * self.c, bias=self._b, mode=ops.A_CONV3X3, Cin=self.c,
                 conv=(Ho, Wo, c.H, c.W, 1, 1), colstats=(c.T * Ho * Wo if To == c.T else 0))
        if To != c.T:
            idx = torch.tensor(fmap, dtype=torch.int64).to(x.device)
            out = out.view(c.B, c.T, Ho * Wo * self.c).index_select(1, idx).view(-1, self.c)      # the strided device copy
        c.T, c.H, c.W, c.sh = To, Ho, Wo, c.sh + 1
        return out


class CogVideoXMidBlock3D(nn.Module):
    def __init__(self, c: int, cfg: CogVAEConfig, spatial_norm: bool):
        super().__init__()
        self.resnets = nn.ModuleList([CogVideoXResnetBlock3D(c, c, cfg, spatial_norm) for _ in range(2)])


class CogVideoXUpBlock3D(nn.Module):
    def __init__(self, cin, cout, layers, add_upsample, compress_time, cfg):
        super().__init__()
        self.resnets = nn.ModuleList([CogVideoXResnetBlock3D(cin if i == 0 else cout, cout, cfg, True) for i in range(layers)])
        self.upsamplers = nn.ModuleList([CogVideoXUpsample3D(cout, compress_time)]) if add_upsample else None


class CogVideoXDecoder3D(nn.Module):
    def __init__(self, cfg: CogVAEConfig):
        super().__init__()
        r = list(reversed(cfg.block_out_channels))
        self.conv_in = CogVideoXCausalConv3d(cfg.latent_channels, r[0], 3)
        self.mid_block = CogVideoXMidBlock3D(r[0], cfg, True)
        self.up_blocks = nn.ModuleList()
        c = r[0]
        for i, co in enumerate(r):
            self.up_blocks.append(CogVideoXUpBlock3D(c, co, cfg.layers_per_block + 1, i != len(r) - 1, i < _time_levels(cfg), cfg))
            c = co
        self.norm_out = _norm(r[-1], cfg, True)
        self.conv_act = nn.SiLU()
        self.conv_out = CogVideoXCausalConv3d(r[-1], cfg.out_channels, 3)


# ------------------------------------------------------------------------------------------------ the encoder's holders
class CogVideoXDownsample3D(nn.Module):
    """CogVideoXDownsample3D(c, c, padding=0, compress_time) [EXT]: avg_pool1d(2, 2) along the frames (the first frame apart when the
    count is odd), then F.pad(0,1,0,1) and a 3x3 stride-2 convolution per frame"""

    def __init__(self, c: int, compress_time: bool):
        super().__init__()
        self.c, self.compress_time = c, compress_time
        self.conv = nn.Conv2d(c, c, 3, stride=2, padding=0)

    def pack(self):
        self._w, self._b = pack_conv3x3(self.conv.weight.detach()), f32(self.conv.bias)

    def run(self, x: torch.Tensor, c: _Chunk):
        """the pool runs first, as diffusers does: the convolution then has half the rows"""
        if self.compress_time:
            x = ops.cogvae_time_pool(x, c.B, c.T, c.H * c.W)
            c.T = ops.pooled_frames(c.T)
        Ho, Wo = (c.H - 2) // 2 + 1, (c.W - 2) // 2 + 1
        M = c.B * c.T * Ho * Wo
        out = _new(M, self.c, x.device)
        ops.gemm(x, self._w, out, M=M, N=self.c, K=9 * self.c, bias=self._b, mode=ops.A_CONV3X3, Cin=self.c,
                 conv=(Ho, Wo, c.H, c.W, 2, 0, 1), colstats=c.T * Ho * Wo)
        c.H, c.W = Ho, Wo
        return out


class CogVideoXDownBlock3D(nn.Module):
    def __init__(self, cin, cout, layers, add_downsample, compress_time, cfg):
        super().__init__()
        self.resnets = nn.ModuleList([CogVideoXResnetBlock3D(cin if i == 0 else cout, cout, cfg, False) for i in range(layers)])
        self.downsamplers = nn.ModuleList([CogVideoXDownsample3D(cout, compress_time)]) if add_downsample else None


class CogVideoXEncoder3D(nn.Module):
    def __init__(self, cfg: CogVAEConfig):
        super().__init__()
        ch = list(cfg.block_out_channels)
        self.conv_in = CogVideoXCausalConv3d(cfg.in_channels, ch[0], 3)
        self.down_blocks = nn.ModuleList()
        c = ch[0]
        for i, co in enumerate(ch):
            self.down_blocks.append(CogVideoXDownBlock3D(c, co, cfg.layers_per_block, i != len(ch) - 1, i < _time_levels(cfg), cfg))
            c = co
        self.mid_block = CogVideoXMidBlock3D(ch[-1], cfg, False)
        self.norm_out = CogVideoXGroupNorm(cfg.norm_num_groups, ch[-1], eps=1e-6)
        self.conv_act = nn.SiLU()
        self.conv_out = CogVideoXCausalConv3d(ch[-1], 2 * cfg.latent_channels, 3)

    def pack(self):
        """conv_in's weight in the k order of ``lkgd_cogvae_pixel_taps`` - k = ((kt*3 + ky)*3 + kx)*Cin + c, zeros up to K = 128"""
        w = self.conv_in.conv.weight.detach().float()                                  # [c0, Cin, 3, 3, 3]
        wk = w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1)
        self._w_in = torch.nn.functional.pad(wk, (0, 128 - wk.shape[1])).to(torch.float16).contiguous()
        self._b_in = f32(self.conv_in.conv.bias)
        self.norm_out.pack()
        self.conv_out.pack()


class DiagonalGaussianDistribution:
    """the posterior ``encode`` returns ([EXT] diffusers DiagonalGaussianDistribution) over the moment rows ``conv_out`` left:
    ``mean`` [B, lc, T, h, w] and ``sample`` come from ``lkgd_cogvae_posterior``; ``logvar`` (clamped to [-30, 20]) and ``std`` are
    accessors computed on first use.  Tensors are handed out in ``dtype`` (the parameters')."""

    def __init__(self, moments: torch.Tensor, B: int, lc: int, T: int, h: int, w: int, dtype):
        self._mom, self._geo, self._dtype = moments, (B, lc, T, h, w), dtype
        self.mean = ops.cogvae_posterior(moments, B, lc, T, h, w)[0].to(dtype)
        self._logvar = None

    @property
    def logvar(self) -> torch.Tensor:
        if self._logvar is None:
            B, lc, T, h, w = self._geo
            lv = self._mom[:, lc:2 * lc].reshape(B, T, h, w, lc).permute(0, 4, 1, 2, 3)
            self._logvar = torch.clamp(lv.float(), -30.0, 20.0).to(self._dtype).contiguous()
        return self._logvar

    @property
    def std(self) -> torch.Tensor:
        return torch.exp(0.5 * self.logvar.float()).to(self._dtype)

    def mode(self) -> torch.Tensor:
        return self.mean

    def sample(self, generator=None, scale: float = 1.0) -> torch.Tensor:
        """``scale * (mean + std * noise)`` in one launch; the noise is drawn as ``dpm_noise`` draws: on the generator's device, in
        the parameters' dtype, with the shape of the mean.  ``scale`` (1.0: diffusers' ``sample``) folds a caller's scaling factor."""
        dev = self._mom.device
        gdev = generator.device if generator is not None else dev
        noise = torch.randn(tuple(self.mean.shape), generator=generator, device=gdev, dtype=self._dtype)
        noise = noise.to(device=dev, dtype=torch.float16).contiguous()
        return ops.cogvae_posterior(self._mom, *self._geo, noise=noise, scale=scale)[1].to(self._dtype)


class AutoencoderKLOutput:
    """what ``encode`` returns: ``.latent_dist``, also as item 0 (inference/cli_vae_demo.py indexes it)"""

    def __init__(self, latent_dist: DiagonalGaussianDistribution):
        self.latent_dist = latent_dist

    def __getitem__(self, i):
        return (self.latent_dist,)[i]


def _check_encoder_config(cfg: CogVAEConfig) -> None:
    if not 0 < cfg.in_channels <= 4:
        raise LkgdHipError(f"AutoencoderKLCogVideoX: in_channels = {cfg.in_channels}: the tap rows of conv_in hold at most 4")
    if cfg.use_quant_conv:
        raise LkgdHipError("AutoencoderKLCogVideoX: use_quant_conv = True is not built (no CogVideoX checkpoint sets it)")


def _check_config(cfg: CogVAEConfig) -> None:
    if cfg.use_post_quant_conv:
        raise LkgdHipError("AutoencoderKLCogVideoX: use_post_quant_conv = True is not built (no CogVideoX checkpoint sets it)")
    if cfg.norm_num_groups != 32:
        raise LkgdHipError(f"AutoencoderKLCogVideoX: norm_num_groups = {cfg.norm_num_groups}: the norm kernels have 32 groups")
    for ch in cfg.block_out_channels:
        if ch % 64:
            raise LkgdHipError(f"AutoencoderKLCogVideoX: block_out_channels entry {ch} is not a multiple of 64 "
                               "(implicit-GEMM K granularity)")
    if not 0 < cfg.latent_channels <= 64 or cfg.latent_channels % 8:
        raise LkgdHipError(f"AutoencoderKLCogVideoX: latent_channels = {cfg.latent_channels}: a multiple of 8 up to 64")
    if not 0 < cfg.out_channels <= 4:
        raise LkgdHipError(f"AutoencoderKLCogVideoX: out_channels = {cfg.out_channels}: at most 4")
    if cfg.act_fn != "silu":
        raise LkgdHipError(f"AutoencoderKLCogVideoX: act_fn = {cfg.act_fn!r}: only 'silu' is built")
    t = cfg.temporal_compression_ratio
    if t < 1 or t & (t - 1) or (t.bit_length() - 1) >= len(cfg.block_out_channels):
        raise LkgdHipError(f"AutoencoderKLCogVideoX: temporal_compression_ratio = {t}: a power of two below 2^len(block_out_channels)")


class AutoencoderKLCogVideoX(PackedModule):
    """diffusers' AutoencoderKLCogVideoX [EXT], PARITY UNPINNED: the decoder, and with ``encoder=True`` the encoder.  State-dict
    names are diffusers' (``decoder.conv_in.conv.weight``, ``encoder.down_blocks.0.resnets.0.norm1.weight`` ...).  ``quant_conv.*``
    keys of a checkpoint are accepted and dropped; so are ``encoder.*`` keys when the module has no encoder - with one they load
    strictly.  Any other missing or unexpected key raises."""

    OFF_GPU = "lkgd_amd CogVideoX VAE runs on MI355X only: move the module to cuda first"
    config_class = CogVAEConfig
    DROPPED_PREFIXES = ("encoder.", "quant_conv.")

    def __init__(self, config: Optional[CogVAEConfig] = None, encoder: bool = False, **kw):
        super().__init__()
        cfg = config if config is not None else CogVAEConfig(**kw)
        cfg.block_out_channels = tuple(cfg.block_out_channels)
        _check_config(cfg)
        self.config = SimpleNamespace(**cfg.__dict__)
        self.decoder = CogVideoXDecoder3D(cfg)
        if encoder:
            _check_encoder_config(cfg)
            self.encoder = CogVideoXEncoder3D(cfg)
        # diffusers' tiling / slicing state: off until enable_*; a tile is half the configured sample size
        self.use_tiling = False
        self.use_slicing = False
        self.tile_sample_min_height = cfg.sample_height // 2
        self.tile_sample_min_width = cfg.sample_width // 2
        self.tile_overlap_factor_height = 1 / 6
        self.tile_overlap_factor_width = 1 / 5
        self._set_tile_latent_min()

    def _set_tile_latent_min(self):
        down = _spatial_factor(self.config)
        self.tile_latent_min_height = int(self.tile_sample_min_height / down)
        self.tile_latent_min_width = int(self.tile_sample_min_width / down)

    @property
    def has_encoder(self) -> bool:
        return "encoder" in self._modules

    def _dropped_prefixes(self):
        return ("quant_conv.",) if self.has_encoder else self.DROPPED_PREFIXES

    # ---- reference API surface ---------------------------------------------------------------------------------
    @classmethod
    def _build_options(cls, encoder: Optional[bool] = None, **_ignored):
        """``from_pretrained(..., encoder=None)``: the encoder is built iff the checkpoint holds an ``encoder.`` key (a saved
        decoder-only module comes back decoder-only); True / False: as the constructor"""
        def ctor(sd):
            return {"encoder": any(k.startswith("encoder.") for k in sd) if encoder is None else bool(encoder)}

        return {"ctor_from_state": ctor}

    def load_state_dict(self, state_dict, strict: bool = True, **k):
        """``quant_conv.*`` keys are dropped, ``encoder.*`` keys too when the module has no encoder; every other missing or unexpected
        key raises (whatever ``strict``)"""
        sd = {n: v for n, v in state_dict.items() if not n.startswith(self._dropped_prefixes())}
        r = super().load_state_dict(sd, strict=False, **k)
        if r.missing_keys or r.unexpected_keys:
            raise RuntimeError(f"AutoencoderKLCogVideoX.load_state_dict: missing keys {list(r.missing_keys)[:5]}, "
                               f"unexpected keys {list(r.unexpected_keys)[:5]}")
        return r

    def _require_gpu(self, what: str):
        if self.device.type != "cuda":
            raise LkgdHipError(f"AutoencoderKLCogVideoX.{what}: this module is not on the GPU - move it to cuda first, then call "
                               f"{what} (the reference's order: pipe.to('cuda'), then vae.{what}())")

    def enable_tiling(self, tile_sample_min_height: Optional[int] = None, tile_sample_min_width: Optional[int] = None,
                      tile_overlap_factor_height: Optional[float] = None, tile_overlap_factor_width: Optional[float] = None) -> None:
        """diffusers' ``enable_tiling``: ``decode`` / ``encode`` of an input larger than one tile run tile by tile with cross-faded
        seams.  Given values replace the current ones (the defaults: half the configured sample size, overlap 1/6 and 1/5); the
        latent minima follow.  Refuses a module that is not on the GPU, as ``decode`` and ``encode`` do: move the module first - the
        reference's order, ``pipe.to("cuda")`` and then ``pipe.vae.enable_tiling()``, works."""
        self._require_gpu("enable_tiling")
        self.use_tiling = True
        self.tile_sample_min_height = tile_sample_min_height or self.tile_sample_min_height
        self.tile_sample_min_width = tile_sample_min_width or self.tile_sample_min_width
        self.tile_overlap_factor_height = tile_overlap_factor_height or self.tile_overlap_factor_height
        self.tile_overlap_factor_width = tile_overlap_factor_width or self.tile_overlap_factor_width
        self._set_tile_latent_min()

    def disable_tiling(self) -> None:
        self.use_tiling = False

    def enable_slicing(self) -> None:
        """diffusers' ``enable_slicing``: a batch decodes entry by entry (same bits, a lower peak); ``encode`` runs its entries one
        after the other whatever the switch.  Refuses a module that is not on the GPU: move the module first, as for
        ``enable_tiling``."""
        self._require_gpu("enable_slicing")
        self.use_slicing = True

    def disable_slicing(self) -> None:
        self.use_slicing = False

    def _tiling_args(self):
        return (self.tile_sample_min_height, self.tile_sample_min_width, self.tile_latent_min_height, self.tile_latent_min_width,
                self.tile_overlap_factor_height, self.tile_overlap_factor_width, _spatial_factor(self.config))

    def _tiles(self, h: int, w: int, min_h: int, min_w: int) -> bool:
        """tile by tile iff tiling is on and the input (latents for the decode, pixels for the encode) exceeds one tile"""
        return self.use_tiling and (w > min_w or h > min_h)

    def _frames_out(self, bounds, level) -> int:
        """output frames of a clip run in the groups ``bounds``; ``level``: frames in -> frames out of one temporal level"""
        total = 0
        for a, b in bounds:
            n = b - a
            for _ in range(_time_levels(self.config)):
                n = level(n)
            total += n
        return total

    # ---- packing -----------------------------------------------------------------------------------------------
    def _pack(self):
        d = self.decoder
        for m in self.modules():
            if isinstance(m, (CogVideoXResnetBlock3D, CogVideoXUpsample3D, CogVideoXDownsample3D)):
                m.pack()
        d.conv_in.pack(pad_cin=64)                  # the latent rows are padded to 64 channels with zeros
        d.norm_out.pack()
        d.conv_out.pack(pad_cout=4)                 # GEMM output granularity
        if self.has_encoder:
            self.encoder.pack()
        return True                 # the packed weights live on the submodules

    # ---- encode ------------------------------------------------------------------------------------------------
    def _encode_batch(self, xh: torch.Tensor, a: int, b: int, mom: torch.Tensor, t_out: int, caches) -> int:
        """frames [a, b) of the clip ``xh`` [B, Cin, T, H, W] (fp16) through the encoder; the moment rows of its latent frames go to
        mom[:, t_out:]"""
        e, dev = self.encoder, xh.device
        B, _, _, H, W = xh.shape
        c = _Chunk(B, b - a, H, W, None, caches)
        c0 = self.config.block_out_channels[0]
        M = B * c.T * H * W
        taps = ops.cogvae_pixel_taps(xh, a, b - a)           # the clip's own frames a - 2, a - 1 are conv_in's cache
        x = _new(M, c0, dev)
        ops.gemm(taps, e._w_in, x, M=M, N=c0, K=128, bias=e._b_in, colstats=c.T * H * W)
        del taps
        for blk in e.down_blocks:
            for r in blk.resnets:
                x = r.run(x, c)
            if blk.downsamplers is not None:
                x = blk.downsamplers[0].run(x, c)
        for r in e.mid_block.resnets:
            x = r.run(x, c)
        P = e.norm_out.run(x, c)
        del x
        m = e.conv_out.run(P, c)                                                # [B*T'*h*w, 2 lc]
        mom[:, t_out:t_out + c.T] = m.view(B, c.T, c.H * c.W, m.shape[1])
        return c.T

    def _encode_clip(self, xc: torch.Tensor, mom: torch.Tensor, bounds) -> None:
        """the contiguous clip ``xc`` [n, Cin, T, H, W] through its frame batches, the conv caches carried from batch to batch; the
        moment rows go to ``mom`` [n, T', h*w, 2 lc]"""
        _run_clip(self._encode_batch, xc, bounds, mom)

    def _tiled_encode(self, x1: torch.Tensor, mom: torch.Tensor, bounds) -> None:
        """``tiled_encode`` of diffusers for one batch entry ``x1`` [1, Cin, T, H, W]: every pixel tile through ``_encode_clip``, the
        seams by ``lkgd_cogvae_tile_blend_rows`` on the tiles' moment rows into ``mom`` [1, T', h*w, 2 lc] (``_run_tiles``)"""
        H, W = x1.shape[3:]
        g = encode_tile_geometry(H, W, *self._tiling_args())
        down = _spatial_factor(self.config)
        Tl, C2 = mom.shape[1], mom.shape[3]

        def run(xt):
            n, sy, sx = xt.shape[0], xt.shape[3] // down, xt.shape[4] // down
            mt = torch.empty(n, Tl, sy * sx, C2, dtype=torch.float16, device=xt.device)
            self._encode_clip(xt, mt, bounds)
            return mt.view(n, Tl, sy, sx, C2)

        _run_tiles(g, lambda ys, xs: x1[:, :, :, ys, xs], run, ops.cogvae_tile_blend_rows,
                   lambda: mom[0].view(Tl, H // down, W // down, C2))

    def _encode_f16(self, x1: torch.Tensor, mom: torch.Tensor, bounds) -> None:
        """one batch entry ``x1`` [1, Cin, T, H, W] fp16 -> its moment rows ``mom`` [1, T', h*w, 2 lc]: tile by tile iff ``_tiles``"""
        if self._tiles(x1.shape[3], x1.shape[4], self.tile_sample_min_height, self.tile_sample_min_width):
            return self._tiled_encode(x1, mom, bounds)
        return self._encode_clip(x1, mom, bounds)

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True):
        """[B, 3, T, H, W] in [-1, 1] -> an output with ``.latent_dist`` (also its item 0): the posterior over [B, 16, T', H/8, W/8],
        T' = 1 + (T - 1)/4 for T = 4k + 1.  Frame batches of eight with the remainder in the first (49 -> 9|8|8|8|8|8), the conv caches
        carried from batch to batch; GroupNorm statistics span one batch's frames.  The batch entries are encoded one after the
        other (the I2V pipeline encodes one image at a time): an entry's result does not depend on its neighbours - which is all
        ``use_slicing`` asks for.  With ``use_tiling`` a clip larger than ``tile_sample_min_height`` x ``tile_sample_min_width`` pixels
        encodes tile by tile (``_tiled_encode``): the posterior is built from the blended moment rows."""
        if not self.has_encoder:
            raise LkgdHipError("AutoencoderKLCogVideoX.encode: this module was built without its encoder - construct it with "
                               "encoder=True (from_pretrained builds it when the checkpoint holds encoder.* keys, or with encoder=True)")
        ic, lc = self.config.in_channels, self.config.latent_channels
        if x.dim() != 5 or x.shape[1] != ic:
            raise ValueError(f"expected [B, {ic}, T, H, W]")
        B, _, T, H, W = x.shape
        down = _spatial_factor(self.config)
        if H % down or W % down:
            raise ValueError(f"height and width must be multiples of {down}, got {H} x {W}")
        if x.dtype == torch.bfloat16 or self.dtype == torch.bfloat16:
            raise LkgdHipError("AutoencoderKLCogVideoX.encode: bf16 is not built - activations are fp16 (keep the module in fp16 or fp32)")
        self.prepare()
        dev = self.device
        xh = x.to(device=dev, dtype=torch.float16).contiguous()
        bounds = frame_batch_bounds(T)
        Tl, h, w = self._frames_out(bounds, ops.pooled_frames), H // down, W // down
        mom = torch.empty(B, Tl, h * w, 2 * lc, dtype=torch.float16, device=dev)
        for i in range(B):
            self._encode_f16(xh[i:i + 1], mom[i:i + 1], bounds)
        dist = DiagonalGaussianDistribution(mom.view(-1, 2 * lc), B, lc, Tl, h, w, self.dtype)
        if not return_dict:
            return (dist,)
        return AutoencoderKLOutput(dist)

    # ---- decode ------------------------------------------------------------------------------------------------
    def _decode_chunk(self, zh: torch.Tensor, a: int, b: int, out: torch.Tensor, t_out: int, caches) -> int:
        """latent frames [a, b) of ``zh`` [B, T, h, w, 16] (fp16), one chunk, through the decoder; its frames go to out[:, :, t_out:]"""
        d, dev = self.decoder, zh.device
        zc = zh[:, a:b]
        B, Tz, h, w, lc = zc.shape
        P0 = torch.zeros(B, Tz + 2, h * w, 64, dtype=torch.float16, device=dev)
        P0[:, 2:, :, :lc] = zc.reshape(B, Tz, h * w, lc)
        zq64 = P0[:, 2:].reshape(B * Tz * h * w, 64).contiguous()
        c = _Chunk(B, Tz, h, w, zq64, caches)
        x = d.conv_in.run(P0, c, colstats=Tz * h * w)
        del P0
        for r in d.mid_block.resnets:
            x = r.run(x, c)
        for blk in d.up_blocks:
            for r in blk.resnets:
                x = r.run(x, c)
            if blk.upsamplers is not None:
                x = blk.upsamplers[0].run(x, c)
        P = d.norm_out.run(x, c)
        del x
        rgb = d.conv_out.run(P, c)                                              # [B*T*H*W, 4]
        oc = self.config.out_channels
        frames = ops.tokens_to_nchw(rgb, B * c.T, oc, c.H, c.W)                 # [B*T, 3, H, W]
        out[:, :, t_out:t_out + c.T] = frames.view(B, c.T, oc, c.H, c.W).permute(0, 2, 1, 3, 4)
        return c.T

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = True):
        """[B, 16, T, h, w] -> sample [B, 3, T', 8h, 8w] in z's dtype (T' = 1 + 4 (T - 1) for odd T, 4 T for even T): chunks of two
        latent frames, the conv caches carried from chunk to chunk.  With ``use_tiling`` a grid larger than ``tile_latent_min_height`` x
        ``tile_latent_min_width`` decodes tile by tile (``_tiled_decode``); with ``use_slicing`` a batch decodes entry by entry.  With
        both off the launches are what they were before the switches existed."""
        self.prepare()
        lc = self.config.latent_channels
        if z.dim() != 5 or z.shape[1] != lc:
            raise ValueError(f"expected [B, {lc}, T, h, w]")
        B = z.shape[0]
        zh = z.to(device=self.device, dtype=torch.float16).permute(0, 2, 3, 4, 1).contiguous()   # [B, T, h, w, 16]
        out_dtype = z.dtype if z.dtype in (torch.float16, torch.float32) else torch.float32
        if self.use_slicing and B > 1:
            out = torch.cat([self._decode_f16(zh[i:i + 1]) for i in range(B)])
        else:
            out = self._decode_f16(zh)
        out = out.to(out_dtype)
        if not return_dict:
            return (out,)
        return DecoderOutput(sample=out)

    def _decode_f16(self, zh: torch.Tensor) -> torch.Tensor:
        """``zh`` [B, T, h, w, 16] fp16 -> frames [B, 3, T', 8h, 8w] fp16: tile by tile iff ``_tiles``"""
        if self._tiles(zh.shape[2], zh.shape[3], self.tile_latent_min_height, self.tile_latent_min_width):
            return self._tiled_decode(zh)
        return self._decode_whole(zh)

    def _new_frames(self, B: int, T: int, h: int, w: int, dev) -> torch.Tensor:
        """the frames [B, 3, T', 8h, 8w] that T latent frames of h x w decode to, uninitialised"""
        Tout = self._frames_out(chunk_bounds(T), lambda n: len(upsample_frame_map(n, True)))
        up = _spatial_factor(self.config)
        return torch.empty(B, self.config.out_channels, Tout, up * h, up * w, dtype=torch.float16, device=dev)

    def _decode_whole(self, zh: torch.Tensor) -> torch.Tensor:
        """the chunk loop over the whole latent grid of ``zh`` [B, T, h, w, 16] (a chunk's activations are gone when it returns)"""
        B, T, h, w, _ = zh.shape
        out = self._new_frames(B, T, h, w, zh.device)
        _run_clip(self._decode_chunk, zh, chunk_bounds(T), out)
        return out

    def _tiled_decode(self, zh: torch.Tensor) -> torch.Tensor:
        """``tiled_decode`` of diffusers: every latent tile through ``_decode_whole`` - all B entries of a tile together - and the
        seams by ``lkgd_cogvae_tile_blend_planar`` on the decoded tiles (``_run_tiles``)"""
        B, T, h, w, _ = zh.shape
        g = decode_tile_geometry(h, w, *self._tiling_args())
        return _run_tiles(g, lambda ys, xs: zh[:, :, ys, xs], lambda zt: self._decode_whole(zt).unflatten(0, (-1, B)),
                          ops.cogvae_tile_blend_planar, lambda: self._new_frames(B, T, h, w, zh.device))

    def forward(self, z):
        return self.decode(z)


def decode_latents(vae: AutoencoderKLCogVideoX, latents: torch.Tensor) -> torch.Tensor:
    """``CogVideoXImageToVideoPipeline.decode_latents`` (pipeline_cogvideox_image2video.py:430-435): [B, T, 16, h, w] latents ->
    [B, 3, T', 8h, 8w] frames"""
    latents = latents.permute(0, 2, 1, 3, 4)
    latents = 1 / vae.config.scaling_factor * latents
    return vae.decode(latents).sample
