"""Host side of the rotary CogVideoX DiT (CogVideoX-5B-I2V) without a GPU: the fp32 twin (tests/cogvideox_rope_oracle.py) against
tests/golden/cogvideox_rope.safetensors = the reference's own in-tree ``CogVideoXTransformer3DModel`` with
``use_rotary_positional_embeddings=True, use_learned_positional_embeddings=True`` run over the twin's restated diffusers pieces (PARITY
UNPINNED for those interiors; make_goldens_cogvideox_rope.py); ``rotary_tables`` by its properties; configuration, parameter names and
the save / load round trip."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

import cogvideox_rope_oracle as ro
from cogvideox_support import DIT_SEED, REPO, dit_inputs as _inputs, hip_twin, rel as _rel


@pytest.fixture(scope="module")
def golden():
    return load_file(os.path.join(REPO, "tests", "golden", "cogvideox_rope.safetensors"))


def test_twin_vs_reference_golden(golden):
    """the bound of test_oracle_dit_vs_reference_golden; and the rotation matters in this fixture: identity tables move the
    reference's own output by >= 0.1 relative L2 (with init_weights_ defaults it was 0.03, under a 1e-2 parity bound's radar -
    hence the x 4 on the norm_q / norm_k gains, recorded in the fixture)"""
    cfg = ro.TINY_ROPE_DIT
    assert golden["norm_qk_gain"].item() == ro.NORM_QK_GAIN == 4.0
    o = ro.seeded_model(cfg, DIT_SEED)
    ck = float(sum(p.detach().double().abs().sum() for p in o.parameters()))
    assert abs(ck - golden["checksum"].item()) <= 1e-9 * ck
    assert torch.equal(o.patch_embed.pos_embedding, golden["pos_embedding"])
    assert golden["pos_embedding"][0, :cfg.max_text_seq_length].abs().min() > 0          # text rows of the learned table act
    cos, sin = ro.rotary_tables(cfg, 3, 4, 6)
    assert torch.equal(cos, golden["cos"]) and torch.equal(sin, golden["sin"])
    i = _inputs(cfg)
    with torch.no_grad():
        y = o(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], image_rotary_emb=(cos, sin))[0]
        y0 = o(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], image_rotary_emb=(torch.ones_like(cos), torch.zeros_like(sin)))[0]
    assert y.shape == golden["out"].shape == (2, 3, 16, 8, 12)
    assert _rel(y, golden["out"]) < 1e-5 and _rel(y0, golden["out_no_rope"]) < 1e-5
    gap = _rel(golden["out_no_rope"], golden["out"])
    print(f"\nrotating q / k moves the reference's output by rel L2 {gap:.3f}")
    assert gap >= 0.1


# --------------------------------------------------------------------------------------------------------- rotary_tables
def _rot(x, cos, sin):
    """apply_rotary_emb on one 64-vector per table row, fp64"""
    xr = torch.stack([-x[..., 1::2], x[..., 0::2]], dim=-1).flatten(-2)
    return x * cos + xr * sin


def test_rotary_tables_properties():
    from lkgd_amd import cogvideox as pc
    cfg = pc.DiTConfig(num_attention_heads=2, sample_width=12, sample_height=8, sample_frames=9, use_rotary_positional_embeddings=True)
    T, h, w = 3, 4, 6
    cos, sin = pc.rotary_tables(cfg, T, h, w)
    assert cos.shape == sin.shape == (T * h * w, 64) and cos.dtype == sin.dtype == torch.float32
    assert (cos.double() ** 2 + sin.double() ** 2 - 1).abs().max() < 1e-6
    assert torch.equal(cos[:, 0::2], cos[:, 1::2]) and torch.equal(sin[:, 0::2], sin[:, 1::2])     # repeat_interleave(2)
    for tab in (cos.view(T, h, w, 64), sin.view(T, h, w, 64)):
        # row (t, y, x) depends on t only in channels 0-15, on y only in 16-39, on x only in 40-63
        assert torch.equal(tab[:, :, :, :16], tab[:, :1, :1, :16].expand(T, h, w, 16))
        assert torch.equal(tab[:, :, :, 16:40], tab[:1, :, :1, 16:40].expand(T, h, w, 24))
        assert torch.equal(tab[:, :, :, 40:], tab[:1, :1, :, 40:].expand(T, h, w, 24))
        assert not torch.equal(tab[0, 0, 0, :16], tab[1, 0, 0, :16]) and not torch.equal(tab[0, 0, 0, 16:40], tab[0, 1, 0, 16:40]) \
            and not torch.equal(tab[0, 0, 0, 40:], tab[0, 0, 1, 40:])
    assert torch.equal(cos[0], torch.ones(64)) and torch.equal(sin[0], torch.zeros(64))             # the grid starts at 0
    # the two restatements (product code, twin) agree
    oc_, os_ = ro.rotary_tables(ro.TINY_ROPE_DIT, T, h, w)
    assert torch.equal(cos, oc_) and torch.equal(sin, os_)
    # relative positions: <rot_p(a), rot_q(b)> == <rot_{p+d}(a), rot_{q+d}(b)> for shifts d along each axis.  The products are formed
    # in fp64 from the fp32 tables: an entry carries the rounding of its angle (positions <= 5, frequencies <= 1: 5 * 2^-24 = 3e-7)
    # and its own (6e-8), and a rotated inner product is a sum of 64 terms a_i b_j c c' of size ~1 with four such factors each:
    # |difference| <~ 2 * 64 * 4 * 4e-7 = 2e-4.  1e-3 leaves a factor of five; a wrong channel block or frequency moves it by O(1)
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    c4, s4 = cos.double().view(T, h, w, 64), sin.double().view(T, h, w, 64)

    def dot(p, q):
        return float((_rot(a, c4[p], s4[p]) * _rot(b, c4[q], s4[q])).sum())
    for p, q, d in (((0, 1, 2), (1, 0, 4), (1, 0, 0)), ((0, 1, 2), (1, 0, 4), (0, 2, 0)), ((0, 1, 2), (1, 0, 4), (0, 0, 1)),
                    ((1, 0, 0), (0, 2, 3), (1, 1, 2))):
        ps, qs = tuple(x + y for x, y in zip(p, d)), tuple(x + y for x, y in zip(q, d))
        assert abs(dot(p, q) - dot(ps, qs)) < 1e-3, (p, q, d)
    assert abs(dot((0, 1, 2), (1, 0, 4)) - dot((0, 1, 2), (1, 0, 5))) > 1e-2                        # and positions do matter


def test_rotary_tables_5b_i2v_grid_uses_the_whole_crop_region():
    """13 x 30 x 45 tokens of a 480 x 720 clip under the configured 60 x 90 sample: the crop region is the whole base grid, so
    the grid is arange(h), arange(w): position (y, x) turns channel pair i of its block by y (or x) * theta^(-2i/24)"""
    from lkgd_amd import cogvideox as pc
    cfg = pc.DiTConfig(num_attention_heads=48, num_layers=42, in_channels=32, use_rotary_positional_embeddings=True,
                       use_learned_positional_embeddings=True)
    assert pc.rope_crop_region(30, 45, 45, 30) == ((0, 0), (30, 45)) == ro.get_resize_crop_region_for_grid((30, 45), 45, 30)
    cos, sin = pc.rotary_tables(cfg, 13, 30, 45)
    assert cos.shape == (13 * 30 * 45, 64)
    c4 = cos.view(13, 30, 45, 64)
    f24 = 1.0 / (10000.0 ** (torch.arange(0, 24, 2, dtype=torch.float32) / 24))
    f16 = 1.0 / (10000.0 ** (torch.arange(0, 16, 2, dtype=torch.float32) / 16))
    assert torch.allclose(c4[0, 29, 0, 16:40:2], torch.cos(29 * f24), atol=1e-5)
    assert torch.allclose(c4[0, 0, 44, 40::2], torch.cos(44 * f24), atol=1e-5)
    assert torch.allclose(c4[12, 0, 0, 0:16:2], torch.cos(12 * f16), atol=1e-5)
    # a narrower clip is centred in the base grid
    assert pc.rope_crop_region(30, 30, 45, 30) == ro.get_resize_crop_region_for_grid((30, 30), 45, 30) == ((0, 8), (30, 38))


# ------------------------------------------------------------------------------------------------------------- configuration
KW_5B_I2V = dict(num_attention_heads=48, attention_head_dim=64, in_channels=32, out_channels=16, time_embed_dim=512,
                 text_embed_dim=4096, num_layers=42, sample_width=90, sample_height=60, sample_frames=49, patch_size=2,
                 temporal_compression_ratio=4, max_text_seq_length=226, spatial_interpolation_scale=1.875,
                 temporal_interpolation_scale=1.0, norm_eps=1e-5, attention_bias=True, use_rotary_positional_embeddings=True,
                 use_learned_positional_embeddings=True)


def test_5b_i2v_config_constructs_with_the_twins_names():
    from lkgd_amd import cogvideox as pc
    with torch.device("meta"):
        m = pc.CogVideoXTransformer3DModel(**KW_5B_I2V)
        o = ro.CogVideoXTransformer3DModel(ro.RopeDiTConfig(**KW_5B_I2V))
    assert m.inner_dim == 3072 and len(m.transformer_blocks) == 42
    assert m.config.use_rotary_positional_embeddings is True and m.config.use_learned_positional_embeddings is True
    assert m.config.patch_size_t is None and m.config.ofs_embed_dim is None
    sm, so = ({k: tuple(v.shape) for k, v in x.state_dict().items()} for x in (m, o))
    assert sm == so
    assert sm["patch_embed.pos_embedding"] == (1, 226 + 13 * 30 * 45, 3072)
    assert {k for k, _ in m.named_buffers()} == {k for k, _ in o.named_buffers()} == {"patch_embed.pos_embedding"}
    # rotary without a learned table: no position table at all
    with torch.device("meta"):
        r = pc.CogVideoXTransformer3DModel(**{**KW_5B_I2V, "num_layers": 1, "use_learned_positional_embeddings": False})
    assert "patch_embed.pos_embedding" not in r.state_dict() and not list(r.named_buffers())
    # the 2B models are what they were
    with torch.device("meta"):
        b = pc.CogVideoXTransformer3DModel(pc.DiTConfig(in_channels=32, num_layers=1))
    assert b.config.use_rotary_positional_embeddings is False and not list(b.named_buffers())


def test_config_refusals():
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    with pytest.raises(ValueError, match="rotary"):
        with torch.device("meta"):
            pc.CogVideoXTransformer3DModel(pc.DiTConfig(num_layers=1, use_learned_positional_embeddings=True))
    with pytest.raises(LkgdHipError):
        with torch.device("meta"):
            pc.CogVideoXTransformer3DModel(pc.DiTConfig(num_layers=1, num_attention_heads=49))       # 3136 channels


def _tiny_rotary(learned=True):
    cfg = ro.RopeDiTConfig(**{**ro.TINY_ROPE_DIT.__dict__, "use_learned_positional_embeddings": learned})
    return hip_twin(ro.seeded_model(cfg, DIT_SEED), cfg)


@pytest.mark.parametrize("learned", [True, False])
def test_save_and_from_pretrained_round_trip(tmp_path, learned):
    from lkgd_amd import cogvideox as pc
    m = _tiny_rotary(learned)
    d = str(tmp_path / "transformer")
    m.save_pretrained(d)
    raw = json.load(open(os.path.join(d, "config.json")))
    assert raw["use_rotary_positional_embeddings"] is True and raw["use_learned_positional_embeddings"] is learned
    r = pc.CogVideoXTransformer3DModel.from_pretrained(d)
    assert r.config.use_rotary_positional_embeddings is True and r.config.use_learned_positional_embeddings is learned
    a, b = m.state_dict(), r.state_dict()
    assert set(a) == set(b) and ("patch_embed.pos_embedding" in a) == learned
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_from_pretrained_stays_strict_and_refuses_the_1_5_models(tmp_path):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    from safetensors.torch import save_file
    m = _tiny_rotary(True)
    d = str(tmp_path / "t")
    m.save_pretrained(d)
    cfg_path, w_path = os.path.join(d, "config.json"), os.path.join(d, "diffusion_pytorch_model.safetensors")
    raw = json.load(open(cfg_path))
    for key, val in (("patch_size_t", 2), ("ofs_embed_dim", 512)):
        json.dump({**raw, key: val}, open(cfg_path, "w"))
        with pytest.raises(LkgdHipError, match=key):
            pc.CogVideoXTransformer3DModel.from_pretrained(d)
    json.dump(raw, open(cfg_path, "w"))
    sd = load_file(w_path)
    save_file({k: v for k, v in sd.items() if k != "patch_embed.pos_embedding"}, w_path)       # a checkpoint without the table
    with pytest.raises(RuntimeError, match="pos_embedding"):
        pc.CogVideoXTransformer3DModel.from_pretrained(d)
    save_file({**sd, "patch_embed.extra": torch.zeros(1)}, w_path)
    with pytest.raises(RuntimeError, match="unexpected"):
        pc.CogVideoXTransformer3DModel.from_pretrained(d)


def test_forward_refusals_need_no_gpu():
    """ofs / timestep_cond keep raising before anything touches a device"""
    from lkgd_amd._lib import LkgdHipError
    m = _tiny_rotary(True)
    i = _inputs(ro.TINY_ROPE_DIT)
    for kw in (dict(ofs=torch.zeros(2)), dict(timestep_cond=torch.zeros(2, 4))):
        with pytest.raises(LkgdHipError):
            m(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], **kw)
