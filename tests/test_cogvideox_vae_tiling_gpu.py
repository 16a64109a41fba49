"""The tiled / sliced CogVideoX VAE on the GPU: the seam kernel in both layouts against torch's own fp16 ``blend_v`` / ``blend_h`` loops
on the same GPU, bit for bit (tests/cogvideox_vae_tiling_oracle.py; the ``raw`` and ``hfirst`` assemblies must differ), on windowed
operands, and the tiny tiled decode / encode against the tiled fp32 oracle with the untiled oracle as the decoy (measured 0.36 - 0.74
away on the CPU: tests/test_cogvideox_vae_tiling_cpu.py), the A/B switch, slicing, and ``prepare_latents`` through a tiling VAE.

The gate is the module's 1e-2 (fp16 activations, fp32 accumulation; the untiled paths measure 6e-4 - 1.3e-3 against it); the tiled
paths measure what the README's status paragraph records."""
from types import SimpleNamespace

import pytest
import torch

import cogvideox_vae_encoder_oracle as eo
import cogvideox_vae_oracle as oc
import cogvideox_vae_tiling_oracle as to
import test_cogvideox_vae_tiling_cpu as host
from cogvideox_support import DEV, rel
from footprint import run_case

pytestmark = pytest.mark.gpu

GATE = 1e-2
DECOY_MIN = 10 * GATE

#: every name in lkgd_amd._lib.COGVAE_TILE_SYMBOLS -> its footprint tests in this module
FOOTPRINT = {
    "lkgd_cogvae_tile_blend_planar": ["test_footprint_planar"],
    "lkgd_cogvae_tile_blend_rows": ["test_footprint_rows"],
}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _origins(tiles, crop):
    o, out = 0, []
    for t in tiles:
        out.append(o)
        o += min(crop, t)
    return out, o


# ------------------------------------------------------------------------------------------------------ the kernel, planar
#: (tile rows, tile columns, extents, crops)
PLANAR_CASES = [
    ((48, 48, 16), (80, 80, 32), (8, 16), (40, 64)),
    ((48, 48, 8), (80, 80, 8), (8, 16), (40, 64)),           # the last column's extent clamps to min(80, 8, 16) = 8
    ((48, 48, 8), (80, 72, 8), (8, 16), (40, 64)),           # 11 x 17 latents as the geometry cuts them
    ((10, 10, 3), (21, 21, 5), (3, 5), (7, 16)),             # nothing a multiple of 8: the 2-byte paths
    ((16, 16), (24, 20), (4, 12), (12, 12)),                 # Xt % 8 == 0 with an extent and a crop that are not
]
LEAD = (2, 3, 2)


def _assemble_planar(tiles, extent, crop, lead=LEAD):
    """the kernel over a grid of tiles (copies), row-major: (output, blended tiles)"""
    from lkgd_amd import ops
    ys, Y = _origins([r[0].shape[-2] for r in tiles], crop[0])
    xs, X = _origins([t.shape[-1] for t in tiles[0]], crop[1])
    mine = [[t.clone() for t in row] for row in tiles]
    out = torch.full((*lead, Y, X), float("nan"), dtype=torch.float16, device=DEV)
    for i, row in enumerate(mine):
        for j, t in enumerate(row):
            ops.cogvae_tile_blend_planar(t, mine[i - 1][j] if i else None, row[j - 1] if j else None, out, ys[i], xs[j], extent[0],
                                         extent[1], crop[0], crop[1])
    return out, mine


@pytest.mark.parametrize("case", PLANAR_CASES)
def test_planar_kernel_equals_the_torch_loops_bitwise(case):
    rows, cols, extent, crop = case
    tiles = to.random_tiles(rows, cols, LEAD, device=DEV)
    want, want_tiles = to.assemble(tiles, extent, crop)
    got, got_tiles = _assemble_planar(tiles, extent, crop)
    assert tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got.float()).all())
    assert torch.equal(_bits(got), _bits(want))
    for i in range(len(rows)):
        for j in range(len(cols)):
            assert torch.equal(_bits(got_tiles[i][j]), _bits(want_tiles[i][j])), (i, j)
    for v in ("raw", "hfirst"):
        assert not torch.equal(_bits(got), _bits(to.assemble(tiles, extent, crop, v)[0])), v


# -------------------------------------------------------------------------------------------------------- the kernel, rows
ROWS_CASES = [((6, 6, 2), (10, 10, 4), (1, 2), (5, 8), 0), ((12, 12, 4), (20, 20, 8), (2, 4), (10, 16), 0),
              ((6, 6, 2), (10, 10, 4), (1, 2), (5, 8), 8)]
C = 32
P_ROWS = 3


def _assemble_rows(tiles, extent, crop, pad):
    """the kernel over channels-last copies of the planar tiles [P, C, Y, X] (row stride C + pad): (output, blended tiles), planar"""
    from lkgd_amd import ops
    ys, Y = _origins([r[0].shape[-2] for r in tiles], crop[0])
    xs, X = _origins([t.shape[-1] for t in tiles[0]], crop[1])

    def rows_of(t):
        wide = torch.full((*t.permute(0, 2, 3, 1).shape[:3], C + pad), float("nan"), dtype=torch.float16, device=DEV)
        wide[..., :C] = t.permute(0, 2, 3, 1)
        return wide[..., :C]

    mine = [[rows_of(t) for t in row] for row in tiles]
    wide = torch.full((P_ROWS, Y, X, C + pad), 7.0, dtype=torch.float16, device=DEV)
    out = wide[..., :C]
    for i, row in enumerate(mine):
        for j, t in enumerate(row):
            ops.cogvae_tile_blend_rows(t, mine[i - 1][j] if i else None, row[j - 1] if j else None, out, ys[i], xs[j], extent[0],
                                       extent[1], crop[0], crop[1])
    assert bool((wide[..., C:] == 7.0).all())
    return out.permute(0, 3, 1, 2), [[t.permute(0, 3, 1, 2) for t in row] for row in mine]


@pytest.mark.parametrize("case", ROWS_CASES)
def test_rows_kernel_equals_the_torch_loops_bitwise(case):
    rows, cols, extent, crop, pad = case
    tiles = to.random_tiles(rows, cols, (P_ROWS, C), seed=5, device=DEV)
    want, want_tiles = to.assemble(tiles, extent, crop)
    got, got_tiles = _assemble_rows(tiles, extent, crop, pad)
    assert tuple(got.shape) == tuple(want.shape)
    assert torch.equal(_bits(got), _bits(want))
    for i in range(len(rows)):
        for j in range(len(cols)):
            assert torch.equal(_bits(got_tiles[i][j]), _bits(want_tiles[i][j])), (i, j)
    for v in ("raw", "hfirst"):
        assert not torch.equal(_bits(got), _bits(to.assemble(tiles, extent, crop, v)[0])), v


# -------------------------------------------------------------------------------------------------------------- footprint
def test_refusals_of_both_entry_points():
    assert host.planar_refusals() and host.rows_refusals()


def _exact(got, ref, what):
    assert torch.equal(_bits(got), _bits(ref)), what


def _one_tile_ref(tile, up, left, extent, crop):
    """the torch loops for ONE tile with given (already blended) neighbours: (blended tile, its crop)"""
    b = tile.clone()
    if up is not None:
        b = to.blend_v(up, b, extent[0])
    if left is not None:
        b = to.blend_h(left, b, extent[1])
    return b, b[..., :crop[0], :crop[1]]


def test_footprint_planar():
    from lkgd_amd import ops
    for (Yt, Xt, Yu, Xl), extent, crop, (Y, X, y0, x0) in (((16, 32, 12, 24), (8, 16), (12, 24), (20, 40, 8, 16)),
                                                           ((9, 13, 4, 6), (3, 5), (7, 10), (11, 15, 3, 4))):
        P = 4
        g = torch.Generator().manual_seed(Yt + Xt)
        tile, up, left = (torch.randn(P, a, b, generator=g).half() for a, b in ((Yt, Xt), (Yu, Xt), (Yt, Xl)))
        wb, wc = _one_tile_ref(tile.to(DEV), up.to(DEV), left.to(DEV), extent, crop)
        want_out = torch.full((P, Y, X), 7.0, dtype=torch.float16)
        want_out[:, y0:y0 + crop[0], x0:x0 + crop[1]] = wc.cpu()

        def case(Wn):
            # planes are contiguous by contract: [P*Y, X] windows without gaps, guard rows around them
            t = Wn.inout(tile.reshape(-1, Xt), pad=0, gap=False, name="tile")
            u = Wn.inp(up.reshape(-1, Xt), pad=0, gap=False, name="up")
            l = Wn.inp(left.reshape(-1, Xl), pad=0, gap=False, name="left")
            o = Wn.out(P * Y, X, pad=0, gap=False, name="out")
            o.fill_(7.0)                                              # the part of out outside the crop window must stay
            ops.cogvae_tile_blend_planar(t.view(P, Yt, Xt), u.view(P, Yu, Xt), l.view(P, Yt, Xl), o.view(P, Y, X), y0, x0, extent[0],
                                         extent[1], crop[0], crop[1])
            return {"tile": t, "out": o}

        refs = {"tile": wb.reshape(-1, Xt), "out": want_out.reshape(-1, X)}
        run_case(case, DEV, lambda: refs, _exact, True, sync=torch.cuda.synchronize)


def test_footprint_rows():
    from lkgd_amd import ops
    for (Yt, Xt, Yu, Xl), extent, crop, (Y, X, y0, x0) in (((6, 10, 4, 8), (2, 4), (5, 8), (9, 14, 3, 5)),):
        P = 3
        g = torch.Generator().manual_seed(Yt + Xt)
        tile, up, left = (torch.randn(P, C, a, b, generator=g).half() for a, b in ((Yt, Xt), (Yu, Xt), (Yt, Xl)))
        wb, wc = _one_tile_ref(tile.to(DEV), up.to(DEV), left.to(DEV), extent, crop)
        want_out = torch.full((P, C, Y, X), 7.0, dtype=torch.float16)
        want_out[:, :, y0:y0 + crop[0], x0:x0 + crop[1]] = wc.cpu()

        def cl(t):                                                    # planar [P, C, Y, X] -> rows [P*Y*X, C]
            return t.permute(0, 2, 3, 1).reshape(-1, C)

        def case(Wn):
            t = Wn.inout(cl(tile), name="tile")
            u = Wn.inp(cl(up), name="up")
            l = Wn.inp(cl(left), pad=16, name="left")
            o = Wn.out(P * Y * X, C, pad=24, name="out")
            o.fill_(7.0)
            ops.cogvae_tile_blend_rows(t.view(P, Yt, Xt, C), u.view(P, Yu, Xt, C), l.view(P, Yt, Xl, C), o.view(P, Y, X, C), y0, x0,
                                       extent[0], extent[1], crop[0], crop[1])
            return {"tile": t, "out": o}

        refs = {"tile": cl(wb), "out": cl(want_out)}
        run_case(case, DEV, lambda: refs, _exact, True, sync=torch.cuda.synchronize)


# ----------------------------------------------------------------------------------------------------------------- decode
DECODE_CASES = [(1, 14, 22), (3, 14, 22), (5, 14, 22), (3, 12, 20)]          # T = 5 crosses a chunk boundary inside every tile
DECOY_AT = {(1, 14, 22)}                                                     # measured >= 10 gates on the CPU at exactly this input


@pytest.fixture(scope="module")
def dec():
    """(fp32 decoder oracle, HIP twin on the GPU with tiling at 48 x 80 pixels = 6 x 10 latents)"""
    from lkgd_amd import cogvideox_vae as pv
    o = oc.tiny_pair_weights()
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**oc.TINY.__dict__))
    m.load_state_dict(o.state_dict())
    m = m.half().to(DEV)
    m.enable_tiling(48, 80)
    assert m.use_tiling and (m.tile_latent_min_height, m.tile_latent_min_width) == (6, 10)
    return o, m


@pytest.mark.parametrize("T,h,w", DECODE_CASES)
def test_tiled_decode_against_the_tiled_oracle(dec, T, h, w):
    o, m = dec
    z = to.grid_latents(T, h, w)
    want = to.tiled_decode(o, z)
    got = m.decode(z.half().to(DEV)).sample
    assert tuple(got.shape) == tuple(want.shape) == (1, 3, 1 + 4 * (T - 1), 8 * h, 8 * w)
    assert got.dtype == torch.float16 and bool(torch.isfinite(got.float()).all())
    r = rel(got, want)
    print(f"tiled decode T={T} {h}x{w}: HIP vs tiled oracle rel L2 {r:.3e}")
    assert r <= GATE, r
    if (T, h, w) in DECOY_AT:
        d = rel(got, o.decode(z))
        print(f"  decoy untiled: HIP result {d:.3f} away")
        assert d >= DECOY_MIN, d


def test_decode_latents_picks_tiling_up_through_the_module(dec):
    from lkgd_amd import cogvideox_vae as pv
    o, m = dec
    z = to.grid_latents(1, 12, 20)
    lat = (z * m.config.scaling_factor).permute(0, 2, 1, 3, 4).half().to(DEV)
    got = pv.decode_latents(m, lat)
    assert tuple(got.shape) == (1, 3, 1, 96, 160)
    assert rel(got, to.tiled_decode(o, z)) <= GATE


def test_decode_tile_batch_switch(dec, monkeypatch):
    """``LKGD_COGVAE_TILE_BATCH=0`` is the default, to the bit.  ``=1`` (equal-shaped tiles as one batch) is NOT the same bits: the
    GEMM planner picks its program by the row count, so a batch entry differs from a single run in the last bits (measured here:
    228 - 246 k of 532 224 elements, at most 0.02 absolute; an untiled batch of four differs from four single decodes the same way).  It
    is held to the oracle by the same gate instead."""
    o, m = dec
    zf = to.grid_latents(3, 14, 22)
    z = zf.half().to(DEV)
    monkeypatch.delenv("LKGD_COGVAE_TILE_BATCH", raising=False)
    a = m.decode(z).sample
    monkeypatch.setenv("LKGD_COGVAE_TILE_BATCH", "0")
    b = m.decode(z).sample
    assert torch.equal(a, b)
    monkeypatch.setenv("LKGD_COGVAE_TILE_BATCH", "1")
    c = m.decode(z).sample
    r = rel(c, to.tiled_decode(o, zf))
    print(f"batched tiles: {int((c != a).sum())} of {a.numel()} elements differ from one tile at a time; vs the oracle {r:.3e}")
    assert tuple(c.shape) == tuple(a.shape) and r <= GATE, r


def test_decode_slicing_is_bit_identical(dec):
    _, m = dec
    z = torch.cat([to.grid_latents(1, 12, 20), to.grid_latents(1, 12, 20, seed=9)]).half().to(DEV)
    off = m.decode(z).sample
    m.enable_slicing()
    try:
        on = m.decode(z).sample
    finally:
        m.disable_slicing()
    assert tuple(on.shape) == (2, 3, 1, 96, 160) and torch.equal(on, off)
    for i in range(2):
        assert torch.equal(m.decode(z[i:i + 1]).sample, off[i:i + 1]), i
    assert rel(off[0], off[1]) > DECOY_MIN


def test_one_tile_and_disable_tiling_are_the_untiled_path(dec):
    o, m = dec
    small = oc.tiny_latents(3).half().to(DEV)                          # 6 x 10 latents: one tile
    big = to.grid_latents(1, 12, 20).half().to(DEV)
    on_small, on_big = m.decode(small).sample, m.decode(big).sample
    m.disable_tiling()
    try:
        off_small, off_big = m.decode(small).sample, m.decode(big).sample
    finally:
        m.enable_tiling(48, 80)
    assert torch.equal(on_small, off_small)
    assert rel(off_big, o.decode(big.float().cpu())) <= GATE           # back to the untiled result ...
    assert rel(on_big, off_big) >= DECOY_MIN                           # ... which is another function
    assert torch.equal(m.decode(big).sample, on_big)


# ----------------------------------------------------------------------------------------------------------------- encode
ENCODE_T = (1, 9, 17)
H_ENC, W_ENC = 112, 176


@pytest.fixture(scope="module")
def enc():
    from lkgd_amd import cogvideox_vae as pv
    o = eo.tiny_weights()
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**eo.TINY.__dict__), encoder=True)
    m.load_state_dict(o.state_dict())
    m = m.half().to(DEV)
    m.enable_slicing()
    m.enable_tiling(48, 80)
    return o, m


def _moments_of(dist):
    return torch.cat([dist.mean.float().cpu(), dist.logvar.float().cpu()], dim=1)


@pytest.mark.parametrize("T", ENCODE_T)
def test_tiled_encode_against_the_tiled_oracle(enc, T):
    o, m = enc
    x = to.grid_clip(T, H_ENC, W_ENC)
    want = to.tiled_moments(o, x)
    dist = m.encode(x.half().to(DEV)).latent_dist
    got = _moments_of(dist)
    Tl = {1: 1, 9: 3, 17: 5}[T]
    assert tuple(got.shape) == tuple(want.shape) == (1, 32, Tl, 14, 22) and bool(torch.isfinite(got).all())
    assert -30.0 < want[:, 16:].min().item() and want[:, 16:].max().item() < 20.0          # the clamp is not exercised
    r = rel(got, want)
    print(f"tiled encode T={T}: HIP vs tiled oracle rel L2 of the moments {r:.3e}")
    assert r <= GATE, r
    if T == 1:
        d = rel(got, o.moments(x))
        print(f"  decoy untiled: HIP result {d:.3f} away")
        assert d >= DECOY_MIN, d


def test_encode_tile_batch_switch_and_sample(enc, monkeypatch):
    """the sample of a tiled posterior is reproducible; ``LKGD_COGVAE_TILE_BATCH=0`` is the default to the bit, ``=1`` is held to the
    oracle by the gate (see ``test_decode_tile_batch_switch``)"""
    o, m = enc
    xf = to.grid_clip(9, H_ENC, W_ENC)
    x = xf.half().to(DEV)
    monkeypatch.delenv("LKGD_COGVAE_TILE_BATCH", raising=False)
    a = m.encode(x).latent_dist
    s1, s2 = a.sample(torch.Generator().manual_seed(21)), a.sample(torch.Generator().manual_seed(21))
    assert torch.equal(s1, s2) and not torch.equal(s1, a.sample(torch.Generator().manual_seed(22)))
    assert tuple(s1.shape) == (1, 16, 3, 14, 22) and rel(s1, a.mean) > DECOY_MIN
    monkeypatch.setenv("LKGD_COGVAE_TILE_BATCH", "0")
    b = m.encode(x).latent_dist
    assert torch.equal(a.mean, b.mean) and torch.equal(a.logvar, b.logvar)
    assert torch.equal(b.sample(torch.Generator().manual_seed(21)), s1)
    monkeypatch.setenv("LKGD_COGVAE_TILE_BATCH", "1")
    c = _moments_of(m.encode(x).latent_dist)
    r = rel(c, to.tiled_moments(o, xf))
    print(f"batched tiles: {int((c != _moments_of(a)).sum())} of {c.numel()} moments differ from one tile at a time; vs the oracle {r:.3e}")
    assert r <= GATE, r


def test_prepare_latents_through_a_tiling_vae(enc):
    from lkgd_amd import cogvideox as pc
    o, m = enc
    x = to.grid_clip(1, H_ENC, W_ENC)
    image = x[:, :, 0].half().to(DEV)                                   # [1, 3, 112, 176]
    g = torch.Generator().manual_seed(77)
    lat, img = pc.prepare_latents(m, SimpleNamespace(init_noise_sigma=1.0), SimpleNamespace(patch_size_t=None), image, batch_size=1,
                                  num_channels_latents=16, num_frames=9, height=H_ENC, width=W_ENC, dtype=torch.float16, device=DEV,
                                  generator=g)
    assert tuple(lat.shape) == tuple(img.shape) == (1, 3, 16, 14, 22)
    assert lat.dtype == img.dtype == torch.float16 and bool((img[:, 1:] == 0).all())
    mom = to.tiled_moments(o, x)
    mean, std = mom[:, :16], torch.exp(0.5 * mom[:, 16:].clamp(-30.0, 20.0))
    noise = torch.randn((1, 16, 1, 14, 22), generator=torch.Generator().manual_seed(77), dtype=torch.float16).float()
    assert rel(img[:, 0], m.config.scaling_factor * (mean + std * noise)[:, :, 0]) <= GATE
