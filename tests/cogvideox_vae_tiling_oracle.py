"""torch restatement of ``tiled_decode`` / ``tiled_encode`` / ``blend_v`` / ``blend_h`` of diffusers' ``AutoencoderKLCogVideoX`` ([EXT]
autoencoder_kl_cogvideox.py, PARITY UNPINNED: diffusers is not installed and the reference tree only imports the class) around the two
existing oracles: every tile goes through ``cogvideox_vae_oracle.AutoencoderKLCogVideoX.decode`` (or the encoder oracle's ``moments``)
alone, the seams are blended by the literal per-row / per-column loops, the crops are concatenated.  The reference of
tests/test_cogvideox_vae_tiling_*.py and, in fp16 on the GPU, the ATen baseline of tools/cogvideox_vae_tiling_bench.py.

Two assembly variants are DECOYS (plausible misreadings the seam kernel must stay away from):
    ``raw``      a tile is blended with its neighbours' UNBLENDED tiles (diffusers blends in place, so the neighbour a tile sees has
                 already been blended with its own neighbours)
    ``hfirst``   the horizontal blend before the vertical one (the two do not commute in the corner)"""
from dataclasses import dataclass

import torch

VARIANTS = ("true", "raw", "hfirst")


@dataclass
class Tiling:
    """diffusers' tiling attributes: the minimal sample tile, the overlap factors, the spatial compression"""
    S_h: int = 240
    S_w: int = 360
    f_h: float = 1 / 6
    f_w: float = 1 / 5
    down: int = 8

    @property
    def L_h(self):
        return int(self.S_h / self.down)

    @property
    def L_w(self):
        return int(self.S_w / self.down)


#: the geometry of the tests: 48 x 80 pixel tiles, 6 x 10 latents - one tile is the tiny oracle's usual input
TEST_TILING = Tiling(48, 80)


def blend_v(a, b, e):
    e = min(a.shape[-2], b.shape[-2], e)
    for y in range(e):
        b[..., y, :] = a[..., -e + y, :] * (1 - y / e) + b[..., y, :] * (y / e)
    return b


def blend_h(a, b, e):
    e = min(a.shape[-1], b.shape[-1], e)
    for x in range(e):
        b[..., :, x] = a[..., :, -e + x] * (1 - x / e) + b[..., :, x] * (x / e)
    return b


def assemble(rows, extent, crop, variant="true"):
    """``rows[i][j]``: the tiles [..., H_t, W_t], computed alone -> (the assembled output, the tiles as they were blended).  The tiles
    given are left as they are; the blends work on copies, in place, as diffusers' do on the tiles themselves."""
    assert variant in VARIANTS
    raw = rows
    rows = [[t.clone() for t in row] for row in rows]
    nb = raw if variant == "raw" else rows
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if variant == "hfirst":
                if j > 0:
                    tile = blend_h(nb[i][j - 1], tile, extent[1])
                if i > 0:
                    tile = blend_v(nb[i - 1][j], tile, extent[0])
            else:
                if i > 0:
                    tile = blend_v(nb[i - 1][j], tile, extent[0])
                if j > 0:
                    tile = blend_h(nb[i][j - 1], tile, extent[1])
            result_row.append(tile[..., :crop[0], :crop[1]])
        result_rows.append(torch.cat(result_row, dim=-1))
    return torch.cat(result_rows, dim=-2), rows


def decode_geometry(t: Tiling):
    """(step in latents, blend extent in pixels, crop in pixels) of ``tiled_decode``"""
    step = (int(t.L_h * (1 - t.f_h)), int(t.L_w * (1 - t.f_w)))
    extent = (int(t.S_h * t.f_h), int(t.S_w * t.f_w))
    return step, extent, (t.S_h - extent[0], t.S_w - extent[1])


def encode_geometry(t: Tiling):
    """(step in pixels, blend extent in latents, crop in latents) of ``tiled_encode``"""
    step = (int(t.S_h * (1 - t.f_h)), int(t.S_w * (1 - t.f_w)))
    extent = (int(t.L_h * t.f_h), int(t.L_w * t.f_w))
    return step, extent, (t.L_h - extent[0], t.L_w - extent[1])


@torch.no_grad()
def tiled_decode(o, z, t: Tiling = TEST_TILING, variant="true"):
    """``o``: a decoder oracle (``cogvideox_vae_oracle.AutoencoderKLCogVideoX``); z [B, 16, T, h, w] -> [B, 3, T', 8h, 8w]"""
    step, extent, crop = decode_geometry(t)
    h, w = z.shape[3:]
    rows = [[o.decode(z[:, :, :, i:i + t.L_h, j:j + t.L_w]) for j in range(0, w, step[1])] for i in range(0, h, step[0])]
    return assemble(rows, extent, crop, variant)[0]


@torch.no_grad()
def tiled_moments(o, x, t: Tiling = TEST_TILING, variant="true"):
    """``o``: an encoder oracle (``cogvideox_vae_encoder_oracle.AutoencoderKLCogVideoX``); x [B, 3, T, H, W] -> the blended moments
    [B, 32, T', H/8, W/8]"""
    step, extent, crop = encode_geometry(t)
    H, W = x.shape[3:]
    rows = [[o.moments(x[:, :, :, i:i + t.S_h, j:j + t.S_w]) for j in range(0, W, step[1])] for i in range(0, H, step[0])]
    return assemble(rows, extent, crop, variant)[0]


def decode(o, z, t: Tiling = TEST_TILING, use_tiling=True):
    """diffusers' ``decode`` dispatch: tiled iff the latent grid exceeds one tile"""
    if use_tiling and (z.shape[-1] > t.L_w or z.shape[-2] > t.L_h):
        return tiled_decode(o, z, t)
    return o.decode(z)


def moments(o, x, t: Tiling = TEST_TILING, use_tiling=True):
    if use_tiling and (x.shape[-1] > t.S_w or x.shape[-2] > t.S_h):
        return tiled_moments(o, x, t)
    return o.moments(x)


def grid_latents(T, h, w, B=1, seed=2):
    """z [B, 16, T, h, w] built like ``cogvideox_vae_oracle.tiny_latents``: latent frame t scaled by 1 + 2t, fp16 values"""
    g = torch.Generator().manual_seed(seed + T + 31 * h + 7 * w)
    z = torch.randn(B, 16, T, h, w, generator=g)
    z = z * (1.0 + 2.0 * torch.arange(T, dtype=torch.float32))[None, None, :, None, None]
    return z.half().float()


def grid_clip(T, H, W, B=1, seed=3):
    """x [B, 3, T, H, W] built like ``cogvideox_vae_encoder_oracle.tiny_clip``: 0.5 randn + sin(0.9 t), clamped to [-1, 1]"""
    g = torch.Generator().manual_seed(seed + T + 31 * H + 7 * W)
    x = 0.5 * torch.randn(B, 3, T, H, W, generator=g)
    x = x + torch.sin(0.9 * torch.arange(T, dtype=torch.float32))[None, None, :, None, None]
    return x.clamp(-1.0, 1.0).half().float()


def random_tiles(tile_rows, tile_cols, lead, seed=0, device="cpu"):
    """a grid of random fp16 tiles [*lead, Y_i, X_j] for the kernel tests"""
    g = torch.Generator().manual_seed(seed + 13 * sum(tile_rows) + sum(tile_cols))
    return [[(2.0 * torch.randn(*lead, y, x, generator=g)).half().to(device) for x in tile_cols] for y in tile_rows]
