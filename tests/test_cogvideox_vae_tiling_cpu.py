"""Host side of the tiled / sliced CogVideoX VAE without a GPU: diffusers' tile geometry (the table of DESIGN.md section 19) through
``decode_tile_geometry`` / ``encode_tile_geometry`` and through the oracle's own expressions, when ``decode`` / ``encode`` tile, the
switches, the refusals, the two seam entry points' error codes, and the distances between the
oracle's own forms that tests/test_cogvideox_vae_tiling_gpu.py relies on for its decoys.

Distances measured here (fp32 oracle, tiny configuration, tile 48 x 80 pixels = 6 x 10 latents; relative L2 from the tiled truth):
    decode  z [1, 16, T, h, w]        untiled        raw           hfirst
      T = 1, 12 x 20                  0.408          0.060         0.016
      T = 1, 14 x 22                  0.378          0.038         0.012
      T = 1, 11 x 17                  0.362          0.051         0.017
      (T = 3, 12 x 20: 0.137 / 0.033 / 0.009 - later frames are scaled up and dilute the seams; not asserted, six seconds here)
    encode  x [1, 3, T, H, W]         untiled
      T = 1,  96 x 160                0.727
      T = 1, 112 x 176                0.740
The untiled forms lie further than 10 gates (0.1) from the tiled ones and serve as decoys of the GPU parity tests; the two assembly
decoys lie below that at the decode level and are caught by the bit-exact kernel tests instead."""
import pytest
import torch

import cogvideox_vae_encoder_oracle as eo
import cogvideox_vae_oracle as oc
import cogvideox_vae_tiling_oracle as to
from c_interface import ALIGN, NULL, SHAPE, Host, entry
from cogvideox_support import rel

GATE = 1e-2
DECOY_MIN = 10 * GATE
F_H, F_W = 1 / 6, 1 / 5


def _module(cfg=eo.TINY, **kw):
    from lkgd_amd import cogvideox_vae as pv
    return pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**cfg.__dict__), **kw)


# ------------------------------------------------------------------------------------------------------------- geometry
#: sample tile, latent tile -> decode (step, extent, crop), encode (step, extent, crop)
TABLE = [
    ((240, 360), (30, 45), ((25, 36), (40, 72), (200, 288)), ((200, 288), (5, 9), (25, 36))),
    ((384, 680), (48, 85), ((40, 68), (64, 136), (320, 544)), ((320, 544), (8, 17), (40, 68))),
    ((48, 80), (6, 10), ((5, 8), (8, 16), (40, 64)), ((40, 64), (1, 2), (5, 8))),
]


@pytest.mark.parametrize("S,L,dec,enc", TABLE)
def test_geometry_table(S, L, dec, enc):
    from lkgd_amd import cogvideox_vae as pv
    t = to.Tiling(S[0], S[1])
    assert (t.L_h, t.L_w) == L
    assert to.decode_geometry(t) == dec and to.encode_geometry(t) == enc
    g = pv.decode_tile_geometry(2 * L[0], 2 * L[1], S[0], S[1], L[0], L[1], F_H, F_W)
    assert (g.step, g.extent, g.crop) == dec
    g = pv.encode_tile_geometry(2 * S[0], 2 * S[1], S[0], S[1], L[0], L[1], F_H, F_W)
    assert (g.step, g.extent, g.crop) == enc


def test_module_attributes_follow_the_configured_sample_size():
    from lkgd_amd import cogvideox_vae as pv
    m = _module()
    assert m.config.sample_height == 480 and m.config.sample_width == 720
    assert (m.tile_sample_min_height, m.tile_sample_min_width, m.tile_latent_min_height, m.tile_latent_min_width) == (240, 360, 30, 45)
    assert m.tile_overlap_factor_height == 1 / 6 and m.tile_overlap_factor_width == 1 / 5
    assert m.use_tiling is False and m.use_slicing is False
    m15 = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(block_out_channels=(64, 64, 128, 128), layers_per_block=1, sample_height=768,
                                                    sample_width=1360))
    assert (m15.tile_sample_min_height, m15.tile_sample_min_width, m15.tile_latent_min_height, m15.tile_latent_min_width) == (384, 680,
                                                                                                                              48, 85)


def test_tile_origins_of_the_real_grids():
    from lkgd_amd import cogvideox_vae as pv
    g = pv.decode_tile_geometry(60, 90, 240, 360, 30, 45, F_H, F_W)
    assert [o for o, _ in g.rows] == [0, 25, 50] and [o for o, _ in g.cols] == [0, 36, 72]
    assert [s for _, s in g.rows] == [30, 30, 10] and [s for _, s in g.cols] == [45, 45, 18]
    assert g.out_rows == [(0, 200), (200, 200), (400, 80)] and g.out_cols == [(0, 288), (288, 288), (576, 144)]
    g = pv.decode_tile_geometry(96, 170, 384, 680, 48, 85, F_H, F_W)
    assert [o for o, _ in g.rows] == [0, 40, 80] and [o for o, _ in g.cols] == [0, 68, 136]
    assert g.out_rows[-1] == (640, 128) and g.out_cols[-1] == (1088, 272)
    # the nine tiles of 480 x 720 are 4 + 2 + 2 + 1 by shape; one at a time they are nine runs
    g = pv.decode_tile_geometry(60, 90, 240, 360, 30, 45, F_H, F_W)
    assert sorted(len(r) for r in pv._tile_groups(g, True)) == [1, 2, 2, 4]
    assert [len(r) for r in pv._tile_groups(g, False)] == [1] * 9
    assert sorted(ij for r in pv._tile_groups(g, True) for ij in r) == [(i, j) for i in range(3) for j in range(3)]
    e = pv.encode_tile_geometry(480, 720, 240, 360, 30, 45, F_H, F_W)
    assert [o for o, _ in e.rows] == [0, 200, 400] and [o for o, _ in e.cols] == [0, 288, 576]
    assert e.out_rows == [(0, 25), (25, 25), (50, 10)] and e.out_cols == [(0, 36), (36, 36), (72, 18)]


@pytest.mark.parametrize("h,w,rows,cols", [(12, 20, [6, 6, 2], [10, 10, 4]), (14, 22, [6, 6, 4], [10, 10, 6]),
                                           (11, 17, [6, 6, 1], [10, 9, 1])])
def test_output_shapes_at_the_test_tile(h, w, rows, cols):
    from lkgd_amd import cogvideox_vae as pv
    g = pv.decode_tile_geometry(h, w, 48, 80, 6, 10, F_H, F_W)
    assert [s for _, s in g.rows] == rows and [s for _, s in g.cols] == cols
    assert sum(s for _, s in g.out_rows) == 8 * h and sum(s for _, s in g.out_cols) == 8 * w
    assert g.out_rows[1][0] == 40 and g.out_cols[1][0] == 64
    # the restatement assembles the same size from tiles of those shapes
    tiles = [[torch.zeros(1, 8 * y, 8 * x) for x in cols] for y in rows]
    out, _ = to.assemble(tiles, g.extent, g.crop)
    assert tuple(out.shape) == (1, 8 * h, 8 * w)


def test_a_geometry_that_does_not_add_up_raises():
    from lkgd_amd import LkgdHipError
    from lkgd_amd import cogvideox_vae as pv
    # tile_sample_min_height = 32: crops of 27 + 24 rows for 48 (diffusers returns a 51-row tensor)
    with pytest.raises(LkgdHipError, match=r"tile_sample_min 32 x 80.*covers? 51.*48"):
        pv.decode_tile_geometry(6, 20, 32, 80, 4, 10, F_H, F_W)
    tiles = [[torch.zeros(1, 32, 80)] * 3, [torch.zeros(1, 24, 80)] * 3]
    assert to.assemble(tiles, (5, 16), (27, 64))[0].shape[-2] == 51
    with pytest.raises(LkgdHipError, match="do not add up"):
        pv.decode_tile_geometry(12, 20, 8, 80, 1, 10, F_H, F_W)              # a step of int(1 * 5/6) = 0 latents
    with pytest.raises(LkgdHipError, match="do not add up.*multiple of 8"):
        pv.encode_tile_geometry(100, 160, 50, 80, 6, 10, F_H, F_W)


# -------------------------------------------------------------------------------------------------------------- switches
@pytest.fixture
def on_gpu(monkeypatch):
    """the module believes it is on the GPU: the switches and the dispatch are host code"""
    from lkgd_amd import cogvideox_vae as pv
    monkeypatch.setattr(pv.AutoencoderKLCogVideoX, "device", property(lambda self: torch.device("cuda", 0)))


def test_switches_toggle_the_attributes(on_gpu):
    m = _module()
    m.enable_tiling()
    assert m.use_tiling and (m.tile_sample_min_height, m.tile_latent_min_height) == (240, 30)
    m.enable_tiling(48, 80)
    assert (m.tile_sample_min_height, m.tile_sample_min_width, m.tile_latent_min_height, m.tile_latent_min_width) == (48, 80, 6, 10)
    assert m.tile_overlap_factor_height == 1 / 6 and m.tile_overlap_factor_width == 1 / 5
    m.enable_tiling(tile_overlap_factor_height=0.25, tile_overlap_factor_width=0.5)
    assert (m.tile_sample_min_height, m.tile_overlap_factor_height, m.tile_overlap_factor_width) == (48, 0.25, 0.5)
    m.disable_tiling()
    assert not m.use_tiling and m.tile_sample_min_height == 48          # the values stay, as in diffusers
    m.enable_slicing()
    assert m.use_slicing
    m.disable_slicing()
    assert not m.use_slicing


def test_enable_on_a_cpu_module_names_itself_and_says_to_move_first():
    from lkgd_amd import LkgdHipError
    m = _module(encoder=True)
    with pytest.raises(LkgdHipError, match=r"enable_tiling.*not on the GPU.*move it to cuda first"):
        m.enable_tiling()
    with pytest.raises(LkgdHipError, match=r"enable_slicing.*not on the GPU.*move it to cuda first"):
        m.enable_slicing()
    assert not m.use_tiling and not m.use_slicing
    m.disable_tiling(); m.disable_slicing()                               # switching off needs no GPU


def test_decode_tiles_iff_the_grid_exceeds_one_tile(on_gpu, monkeypatch):
    """the decode over four latent grids, and the encode over the same four sizes x 8 pixels"""
    m = _module()
    calls = []
    monkeypatch.setattr(m, "_decode_whole", lambda zh: calls.append("whole") or zh)
    monkeypatch.setattr(m, "_tiled_decode", lambda zh: calls.append("tiled") or zh)
    monkeypatch.setattr(m, "_encode_clip", lambda x1, mom, bounds: calls.append("whole"))
    monkeypatch.setattr(m, "_tiled_encode", lambda x1, mom, bounds: calls.append("tiled"))
    sizes = ((6, 10), (7, 10), (6, 11), (12, 20))
    z = {hw: torch.zeros(1, 1, hw[0], hw[1], 16) for hw in sizes}
    x = {hw: torch.zeros(1, 3, 1, 8 * hw[0], 8 * hw[1]) for hw in sizes}
    for run, inp in ((m._decode_f16, z), (lambda x1: m._encode_f16(x1, None, None), x)):
        del calls[:]
        m.disable_tiling()
        for hw in sizes:
            run(inp[hw])
        assert calls == ["whole"] * 4                                     # off: never
        del calls[:]
        m.enable_tiling(48, 80)
        for hw in sizes:
            run(inp[hw])
        assert calls == ["whole", "tiled", "tiled", "tiled"]
        del calls[:]
        m.disable_tiling()
        run(inp[12, 20])
        assert calls == ["whole"]


def test_tiled_equals_untiled_when_the_input_fits_one_tile():
    """the restatement's dispatch, and a single-tile assembly: no neighbour, nothing blended, the crop is the tile"""
    o = oc.tiny_pair_weights()
    z = oc.tiny_latents(1)
    assert torch.equal(to.decode(o, z), o.decode(z))
    one = o.decode(z)
    out, blended = to.assemble([[one]], (8, 16), (48, 80))
    assert torch.equal(out, one) and torch.equal(blended[0][0], one)
    e = eo.tiny_weights()
    x = eo.tiny_clip(1)
    assert torch.equal(to.moments(e, x), e.moments(x))


def test_config_round_trip_carries_the_sample_size(tmp_path):
    from lkgd_amd import cogvideox_vae as pv
    m = pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(block_out_channels=(64, 64, 128, 128), layers_per_block=1, sample_height=768,
                                                  sample_width=1360))
    m.save_pretrained(str(tmp_path / "vae"))
    r = pv.AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "vae"))
    assert (r.config.sample_height, r.config.sample_width) == (768, 1360)
    assert (r.tile_sample_min_height, r.tile_latent_min_width) == (384, 85)


# -------------------------------------------------------------------------------------------------------------- refusals
def planar_refusals():
    """every refusal include/lkgd_hip_cogvae_tile.h lists for the planar entry point; host pointers: a refused call launches nothing"""
    h = Host()
    tile_bytes = 2 * 2 * 8 * 16
    call = entry("lkgd_cogvae_tile_blend_planar", tile=h.p, up=h.p + 1024, left=h.p + 2048, out=h.p + 3072, P=2, Yt=8, Xt=16, Yu=8, Xl=16,
                 Y=8, X=16, y0=0, x0=0, e_y=2, e_x=8, c_y=8, c_x=16)

    for k in ("tile", "out"):
        assert call(**{k: None}) == NULL, k
    for kw in (dict(P=0), dict(Yt=0), dict(Xt=0), dict(Y=0), dict(X=0), dict(Yu=0), dict(Xl=0), dict(e_y=-1), dict(e_x=-1), dict(c_y=-1),
               dict(c_x=-1), dict(y0=-1), dict(x0=-1),
               dict(y0=1), dict(x0=8), dict(Y=7), dict(X=15), dict(y0=4, c_y=5), dict(x0=8, c_x=9),          # the crop leaves out
               dict(up=h.p), dict(up=h.p + tile_bytes - 2), dict(left=h.p + 2), dict(out=h.p + tile_bytes - 2),      # tile overlaps
               dict(out=h.p - 2 * 2 * 8 * 16 + 2), dict(P=1 << 30, Yt=1 << 10)):
        assert call(**kw) == SHAPE, kw
    for k in ("tile", "up", "left", "out"):
        assert call(**{k: h.p + {"tile": 0, "up": 1024, "left": 2048, "out": 3072}[k] + 1}) == ALIGN, k
    return True


def rows_refusals():
    """the same for the channels-last entry point"""
    h = Host()
    tile_bytes = 2 * 1 * 2 * 4 * 32          # P = 1, 2 x 4 rows of 32 channels
    call = entry("lkgd_cogvae_tile_blend_rows", tile=h.p, ldt=32, up=h.p + 1024, ldu=32, left=h.p + 2048, ldl=32, out=h.p + 3072, ldo=32,
                 P=1, C=32, Yt=2, Xt=4, Yu=2, Xl=4, Y=2, X=4, y0=0, x0=0, e_y=1, e_x=2, c_y=2, c_x=4)

    for k in ("tile", "out"):
        assert call(**{k: None}) == NULL, k
    for kw in (dict(P=0), dict(C=0), dict(C=12), dict(Yt=0), dict(Xt=0), dict(Y=0), dict(X=0), dict(Yu=0), dict(Xl=0), dict(ldt=24),
               dict(ldu=24), dict(ldl=24), dict(ldo=24), dict(e_y=-1), dict(e_x=-1), dict(c_y=-1), dict(c_x=-1), dict(y0=-1), dict(x0=-1),
               dict(y0=1), dict(x0=1), dict(Y=1), dict(X=3),
               dict(up=h.p + 16), dict(left=h.p + tile_bytes - 16), dict(out=h.p + 256), dict(P=1 << 30, Yt=1 << 10)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(tile=h.p + 8), dict(up=h.p + 1024 + 8), dict(left=h.p + 2048 + 8), dict(out=h.p + 3072 + 8), dict(ldt=36), dict(ldu=36),
               dict(ldl=36), dict(ldo=36)):
        assert call(**kw) == ALIGN, kw
    return True


def test_planar_refuses_before_launching():
    assert planar_refusals()


def test_rows_refuses_before_launching():
    assert rows_refusals()


# ------------------------------------------------------------------------------------------------- the oracle's own forms
@pytest.fixture(scope="module")
def dec_oracle():
    return oc.tiny_pair_weights()


@pytest.mark.parametrize("T,h,w", [(1, 12, 20), (1, 14, 22), (1, 11, 17)])
def test_decode_forms_differ_as_the_docstring_says(dec_oracle, T, h, w):
    z = to.grid_latents(T, h, w)
    truth = to.tiled_decode(dec_oracle, z)
    assert tuple(truth.shape) == (1, 3, 1 + 4 * (T - 1), 8 * h, 8 * w)
    d = {"untiled": rel(dec_oracle.decode(z), truth)}
    for v in ("raw", "hfirst"):
        d[v] = rel(to.tiled_decode(dec_oracle, z, variant=v), truth)
    print(f"decode T={T} {h}x{w}: " + ", ".join(f"{k} {x:.3f}" for k, x in d.items()))
    assert d["untiled"] >= DECOY_MIN, d                                   # a decoy of the GPU parity test
    assert 0.0 < d["hfirst"] < d["raw"] < DECOY_MIN, d                    # too close for a parity gate: the kernel tests catch them


@pytest.mark.parametrize("T,H,W", [(1, 96, 160), (1, 112, 176)])
def test_encode_forms_differ_as_the_docstring_says(T, H, W):
    e = eo.tiny_weights()
    x = to.grid_clip(T, H, W)
    truth = to.tiled_moments(e, x)
    assert tuple(truth.shape) == (1, 32, 1, H // 8, W // 8)
    d = rel(e.moments(x), truth)
    print(f"encode T={T} {H}x{W}: untiled {d:.3f}")
    assert d >= DECOY_MIN, d
