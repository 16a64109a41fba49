"""Host side of the CogVideoX 1.5 path without a GPU: the refusals of its two entry points; the 1.5 configurations (I2V with
``ofs_embed_dim``, T2V without) with the twin's names and shapes; the save / load round trip; every refused combination of the 1.5
keys; the slice rotary tables by their properties; the frame padding against the pipeline's statements; the fp32 twin
(tests/cogvideox15_oracle.py) against tests/golden/cogvideox15.safetensors = the reference's own in-tree forward
(make_goldens_cogvideox15.py)."""
import json
import os

import pytest
import torch
from safetensors import safe_open
from safetensors.torch import load_file

import cogvideox15_oracle as vo
from c_interface import ALIGN, NULL, SHAPE, Host, entry
from cogvideox_support import DIT_SEED, REPO, dit_inputs as _inputs, hip_twin, rel as _rel

KW_15_I2V = dict(num_attention_heads=48, attention_head_dim=64, in_channels=32, out_channels=16, time_embed_dim=512,
                 text_embed_dim=4096, num_layers=42, sample_width=300, sample_height=300, sample_frames=81, patch_size=2,
                 temporal_compression_ratio=4, max_text_seq_length=224, norm_eps=1e-5, attention_bias=True,
                 use_rotary_positional_embeddings=True, use_learned_positional_embeddings=False, patch_size_t=2, ofs_embed_dim=512,
                 patch_bias=False)


# ------------------------------------------------------------------------------------------------------------ the C interface
def test_dit_tpatch_refusals():
    """the errors of lkgd_dit_patch_rows / lkgd_dit_cfg_ddim_step, plus LKGD_E_SHAPE unless p_t == 2 and F % p_t == 0; host memory
    stands in for device pointers: a refused call never launches, so nothing dereferences them"""
    hp = Host().p
    patch = entry("lkgd_dit_patch_rows_t", latents=hp, latents_is_f32=0, image_latents=hp, B=1, F=4, C=16, H=8, W=12, p=2, p_t=2,
                  rows_out=hp, ldp=256)
    step = entry("lkgd_dit_cfg_ddim_step_t", noise_rows=hp, ldn=128, latents=hp, latents_is_f32=1, B=1, F=4, C=16, H=8, W=12, p=2, p_t=2,
                 cfg=2, guidance=3.0, a=0.9, b=0.1, sqrt_alpha=0.8, sqrt_beta=0.6)
    assert patch(latents=None) == NULL and patch(rows_out=None) == NULL
    assert step(noise_rows=None) == NULL and step(latents=None) == NULL
    for name, fn, ld in (("patch", patch, "ldp"), ("step", step, "ldn")):
        for kw in (dict(p=1), dict(p=4), dict(W=13), dict(H=7), dict(B=0), dict(F=0), dict(C=0), dict(C=3), {ld: 120},
                   {ld: 260},                         # p = 1, odd W, odd H, empty, C * 4 % 8, short ld, ld % 8
                   dict(p_t=1), dict(p_t=0), dict(p_t=4), dict(p_t=3, F=3), dict(F=3), dict(F=5)):      # p_t != 2, F % p_t
            assert fn(**kw) == SHAPE, (name, kw)
    assert patch(ldp=128) == SHAPE                     # 2C channels with image latents: 256 columns
    assert patch(image_latents=None, ldp=120) == SHAPE     # C channels without them: 128
    assert step(cfg=0) == SHAPE and step(cfg=3) == SHAPE
    assert patch(rows_out=hp + 8) == ALIGN and step(noise_rows=hp + 2) == ALIGN
    assert patch(latents=None, p_t=3) == NULL          # NULL comes first


# ------------------------------------------------------------------------------------------------------------- configuration
def test_15_i2v_config_constructs_with_the_twins_names():
    from lkgd_amd import cogvideox as pc
    with torch.device("meta"):
        m = pc.CogVideoXTransformer3DModel(**KW_15_I2V)
        o = vo.CogVideoXTransformer3DModel(vo.V15DiTConfig(**KW_15_I2V))
    assert m.inner_dim == 3072 and len(m.transformer_blocks) == 42
    assert m.config.patch_size_t == 2 and m.config.ofs_embed_dim == 512 and m.config.patch_bias is False
    sm, so = ({k: tuple(v.shape) for k, v in x.state_dict().items()} for x in (m, o))
    assert sm == so
    assert sm["patch_embed.proj.weight"] == (3072, 256) and "patch_embed.proj.bias" not in sm
    assert sm["proj_out.weight"] == (128, 3072) and sm["proj_out.bias"] == (128,)
    assert {k: v for k, v in sm.items() if k.startswith("ofs_embedding.")} == {
        "ofs_embedding.linear_1.weight": (512, 512), "ofs_embedding.linear_1.bias": (512,),
        "ofs_embedding.linear_2.weight": (512, 512), "ofs_embedding.linear_2.bias": (512,)}
    assert "patch_embed.pos_embedding" not in sm and not list(m.named_buffers())
    assert vo.COGVIDEOX_15_5B_I2V == vo.V15DiTConfig(**KW_15_I2V)
    # the text-to-video form: 16 input channels, no ofs embedding
    kw = {**KW_15_I2V, "in_channels": 16, "ofs_embed_dim": None, "num_layers": 1}
    with torch.device("meta"):
        t = pc.CogVideoXTransformer3DModel(**kw)
        ot = vo.CogVideoXTransformer3DModel(vo.V15DiTConfig(**kw))
    st = {k: tuple(v.shape) for k, v in t.state_dict().items()}
    assert st == {k: tuple(v.shape) for k, v in ot.state_dict().items()}
    assert st["patch_embed.proj.weight"] == (3072, 128) and not any(k.startswith("ofs_embedding") for k in st)
    assert t.ofs_embedding is None and t.config.ofs_embed_dim is None
    # the 1.0 models are what they were
    with torch.device("meta"):
        b = pc.CogVideoXTransformer3DModel(pc.DiTConfig(in_channels=32, num_layers=1))
    assert b.config.patch_size_t is None and b.config.ofs_embed_dim is None and b.ofs_embedding is None
    assert tuple(b.patch_embed.proj.weight.shape) == (1920, 32, 2, 2) and b.patch_embed.proj.bias is not None


def _tiny(ofs=True):
    cfg = vo.TINY_V15_DIT if ofs else vo.V15DiTConfig(**{**vo.TINY_V15_DIT.__dict__, "ofs_embed_dim": None})
    return hip_twin(vo.seeded_model(cfg, DIT_SEED), cfg)


@pytest.mark.parametrize("ofs", [True, False])
def test_save_and_from_pretrained_round_trip(tmp_path, ofs):
    from lkgd_amd import cogvideox as pc
    m = _tiny(ofs)
    d = str(tmp_path / "transformer")
    m.save_pretrained(d)
    raw = json.load(open(os.path.join(d, "config.json")))
    assert raw["patch_size_t"] == 2 and raw["ofs_embed_dim"] == (64 if ofs else None) and raw["patch_bias"] is False
    r = pc.CogVideoXTransformer3DModel.from_pretrained(d)
    assert r.config.patch_size_t == 2 and r.config.ofs_embed_dim == (64 if ofs else None) and r.config.patch_bias is False
    assert (r.ofs_embedding is not None) == ofs and isinstance(r.patch_embed.proj, torch.nn.Linear)
    a, b = m.state_dict(), r.state_dict()
    assert set(a) == set(b) and ("ofs_embedding.linear_1.weight" in a) == ofs and "patch_embed.proj.bias" not in a
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # still strict: a checkpoint that lacks the ofs MLP, or has one it should not have, is refused
    if ofs:
        from safetensors.torch import save_file
        w_path = os.path.join(d, "diffusion_pytorch_model.safetensors")
        sd = load_file(w_path)
        save_file({k: v for k, v in sd.items() if k != "ofs_embedding.linear_2.bias"}, w_path)
        with pytest.raises(RuntimeError, match="ofs_embedding"):
            pc.CogVideoXTransformer3DModel.from_pretrained(d)


def test_refused_combinations_name_their_key(tmp_path):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    base = dict(num_attention_heads=2, in_channels=32, time_embed_dim=64, num_layers=1, sample_width=12, sample_height=8,
                sample_frames=13, max_text_seq_length=16)
    cases = [
        (dict(patch_size_t=2, use_rotary_positional_embeddings=True, use_learned_positional_embeddings=True), "patch_size_t"),
        (dict(patch_size_t=2), "patch_size_t"),                                                          # without rotary
        (dict(ofs_embed_dim=64, use_rotary_positional_embeddings=True), "ofs_embed_dim"),                 # without patch_size_t
        (dict(ofs_embed_dim=64), "ofs_embed_dim"),
        (dict(patch_size_t=1, use_rotary_positional_embeddings=True), "patch_size_t"),
        (dict(patch_size_t=4, use_rotary_positional_embeddings=True), "patch_size_t"),
        (dict(patch_size_t=2, ofs_embed_dim=128, use_rotary_positional_embeddings=True), "ofs_embed_dim"),   # != time_embed_dim
    ]
    m = _tiny(True)
    d = str(tmp_path / "t")
    m.save_pretrained(d)
    cfg_path = os.path.join(d, "config.json")
    raw = json.load(open(cfg_path))
    for kw, key in cases:
        with pytest.raises(LkgdHipError, match=key):
            with torch.device("meta"):
                pc.CogVideoXTransformer3DModel(pc.DiTConfig(**{**base, **kw}))
        # from_pretrained applies the same rule to the directory's config.json before any weight is read
        blank = dict(patch_size_t=None, ofs_embed_dim=None, use_rotary_positional_embeddings=False,
                     use_learned_positional_embeddings=False)
        json.dump({**raw, **blank, **kw}, open(cfg_path, "w"))
        with pytest.raises(LkgdHipError, match=key):
            pc.CogVideoXTransformer3DModel.from_pretrained(d)
    # K granularity on the new widths: 4 input channels -> 32 patch columns
    with pytest.raises(LkgdHipError, match="multiples of 64"):
        with torch.device("meta"):
            pc.CogVideoXTransformer3DModel(pc.DiTConfig(**{**base, "in_channels": 4, "patch_size_t": 2,
                                                           "use_rotary_positional_embeddings": True}))


def test_forward_and_loop_refusals_need_no_gpu():
    """ofs on a model without the embedding, no ofs on a model with it, timestep_cond; an odd frame count; sharding - all before
    anything touches a device"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    from lkgd_amd.dist_run import DistDiTDenoiser
    i = _inputs(vo.TINY_V15_DIT)
    with_ofs, without = _tiny(True), _tiny(False)
    with pytest.raises(LkgdHipError, match="ofs"):
        with_ofs(i["hidden"], i["text"], i["t"], i["domain"], i["flow"])
    with pytest.raises(LkgdHipError, match="ofs"):
        without(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], ofs=torch.full((1,), 2.0))
    with pytest.raises(LkgdHipError, match="timestep_cond"):
        with_ofs(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], ofs=2.0, timestep_cond=torch.zeros(2, 4))
    with pytest.raises(LkgdHipError, match="patch_size_t"):
        pc.denoise(without, pc.CogVideoXDDIMScheduler(), torch.zeros(1, 3, 16, 8, 12), torch.zeros(1, 3, 16, 8, 12), i["text"],
                   i["domain"], i["flow"], 2)
    with pytest.raises(LkgdHipError, match="patch_size_t"):
        DistDiTDenoiser(with_ofs, pc.CogVideoXDDIMScheduler(), 2, 0, 4)
    with pytest.raises(LkgdHipError, match="patch_size_t"):
        without.forward_tokens(torch.zeros(1, 3, 32, 8, 12), torch.zeros(1, 16, 4096), 1.0)


# --------------------------------------------------------------------------------------------------------- rotary_tables
def test_slice_rotary_tables_properties():
    from lkgd_amd import cogvideox as pc
    from lkgd_amd._lib import LkgdHipError
    cfg = pc.DiTConfig(num_attention_heads=2, in_channels=32, sample_width=20, sample_height=16, sample_frames=13,
                       use_rotary_positional_embeddings=True, patch_size_t=2)
    T, h, w = 2, 4, 6                                   # tokens: 4 latent frames / p_t, an 8 x 12 latent clip in a 16 x 20 sample
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
    assert torch.equal(cos[0], torch.ones(64)) and torch.equal(sin[0], torch.zeros(64))
    # the 1-D tables at INTEGER positions 0 .. n - 1 on every axis (no crop region, no linspace): bit for bit
    c4, s4 = cos.view(T, h, w, 64), sin.view(T, h, w, 64)
    for n, lo, hi, pick in ((T, 0, 16, lambda t, i: t[i, 0, 0]), (h, 16, 40, lambda t, i: t[0, i, 0]), (w, 40, 64, lambda t, i: t[0, 0, i])):
        c1, s1 = pc._rope_1d(hi - lo, torch.arange(n))
        for i in range(n):
            assert torch.equal(pick(c4, i)[lo:hi], c1[i]) and torch.equal(pick(s4, i)[lo:hi], s1[i]), (lo, i)
    f24 = 1.0 / (10000.0 ** (torch.arange(0, 24, 2, dtype=torch.float32) / 24))
    assert torch.allclose(c4[0, 3, 0, 16:40:2], torch.cos(3 * f24), atol=1e-6) and torch.allclose(s4[0, 0, 5, 40::2], torch.sin(5 * f24), atol=1e-6)
    # the clip's own size does not move the positions (the 1.0 tables stretch a linspace over the crop region instead)
    c2, _ = pc.rotary_tables(cfg, T, 3, 5)
    assert torch.equal(c2.view(T, 3, 5, 64), c4[:, :3, :5])
    # the two restatements (product code, twin) agree; the twin takes latent frames, as the pipeline passes them
    tcfg = vo.V15DiTConfig(**{**vo.TINY_V15_DIT.__dict__, "sample_width": 20, "sample_height": 16})
    for lf in (3, 4):
        oc_, os_ = vo.rotary_tables(tcfg, lf, h, w)
        assert torch.equal(cos, oc_) and torch.equal(sin, os_)
    # max_size = (sample_height // p, sample_width // p) = (8, 10): the slice cannot be longer than what it is taken from
    pc.rotary_tables(cfg, T, 8, 10)
    for hh, ww in ((9, 10), (8, 11)):
        with pytest.raises(LkgdHipError, match="exceeds"):
            pc.rotary_tables(cfg, T, hh, ww)
    # the 1.0 tables are what they were
    cfg10 = pc.DiTConfig(num_attention_heads=2, sample_width=20, sample_height=16, use_rotary_positional_embeddings=True)
    assert not torch.equal(pc.rotary_tables(cfg10, T, h, w)[0], cos)


# ---------------------------------------------------------------------------------------------------------- frame padding
@pytest.mark.parametrize("F_", [3, 4, 21])
def test_temporal_padding_restates_the_pipeline(F_):
    """pipeline_cogvideox_image2video.py:383-384, 416-418 (prepare_latents), :781-786 and :907 (__call__), written out"""
    from lkgd_amd import cogvideox as pc
    patch_size_t = 2
    g = torch.Generator().manual_seed(F_)
    shape = (2, F_, 16, 4, 6)
    image_latents = torch.randn(shape, generator=g)
    # :383-384
    want_shape = shape[:1] + (shape[1] + shape[1] % patch_size_t,) + shape[2:]
    # :416-418
    first_frame = image_latents[:, : image_latents.size(1) % patch_size_t, ...]
    want_img = torch.cat([first_frame, image_latents], dim=1)
    got_shape, got_img = pc.pad_for_temporal_patches(shape, image_latents, patch_size_t)
    assert got_shape == want_shape and isinstance(got_shape, tuple) and torch.equal(got_img, want_img)
    assert got_shape[1] % patch_size_t == 0 and got_img.shape == got_shape
    if F_ % 2:
        assert torch.equal(got_img[:, 0], image_latents[:, 0]) and torch.equal(got_img[:, 1:], image_latents)     # at the front
    else:
        assert got_img is not None and torch.equal(got_img, image_latents)
    lat = torch.randn(shape, generator=g)
    got_lat, _ = pc.pad_for_temporal_patches(lat, None, patch_size_t)
    assert tuple(got_lat.shape) == want_shape and torch.equal(got_lat[:, want_shape[1] - F_:], lat)
    assert pc.pad_for_temporal_patches(shape, image_latents, None) == (shape, image_latents)
    # :781-786
    latent_frames, additional_frames = F_, 0
    if patch_size_t is not None and latent_frames % patch_size_t != 0:
        additional_frames = patch_size_t - latent_frames % patch_size_t
    assert pc.temporal_padding_frames(F_, patch_size_t) == additional_frames == want_shape[1] - F_
    assert pc.temporal_padding_frames(F_, None) == 0
    # :907
    latents = torch.randn(want_shape, generator=g)
    assert torch.equal(pc.drop_temporal_padding(latents, additional_frames), latents[:, additional_frames:])
    assert pc.drop_temporal_padding(latents, additional_frames).shape[1] == F_


# ------------------------------------------------------------------------------------------------------- twin vs the golden
def test_twin_vs_reference_golden():
    """the restated [EXT] pieces (3-D patch embedding, slice rotary grid) + the in-tree forward (ofs, proj_out, un-patchify)
    reproduce the reference's own outputs, the two decoys included, and the decoys are as far from ``out`` as the generator
    recorded: at least ten times the forward test's bound"""
    path = os.path.join(REPO, "tests", "golden", "cogvideox15.safetensors")
    assert os.path.getsize(path) < (1 << 20)
    golden = load_file(path)
    with safe_open(path, "pt") as f:
        meta = f.metadata()
    cfg = vo.TINY_V15_DIT
    assert golden["ofs_gain"].item() == vo.OFS_GAIN and golden["ofs"].item() == vo.OFS == 2.0
    o = vo.seeded_model(cfg, DIT_SEED)
    ck = float(sum(p.detach().double().abs().sum() for p in o.parameters()))
    assert abs(ck - golden["checksum"].item()) <= 1e-9 * ck
    cos, sin = vo.rotary_tables(cfg, 4, 4, 6)
    assert torch.equal(cos, golden["cos"]) and torch.equal(sin, golden["sin"]) and cos.shape == (2 * 4 * 6, 64)
    i = _inputs(cfg)
    assert i["hidden"].shape == (2, 4, 32, 8, 12)

    def run(hidden, ofs):
        with torch.no_grad():
            return o(hidden, i["text"], i["t"], i["domain"], i["flow"], ofs=torch.full((1,), ofs), image_rotary_emb=(cos, sin))[0]
    y, y0, ys = run(i["hidden"], 2.0), run(i["hidden"], 0.0), run(vo.swap_frames_in_patches(i["hidden"]), 2.0)
    assert y.shape == golden["out"].shape == (2, 4, 16, 8, 12)
    assert _rel(y, golden["out"]) < 1e-5 and _rel(y0, golden["out_ofs0"]) < 1e-5 and _rel(ys, golden["out_swapped"]) < 1e-5
    d_ofs, d_swap = _rel(golden["out_ofs0"], golden["out"]), _rel(golden["out_swapped"], golden["out"])
    print(f"\nofs = 0 moves the reference's output by rel L2 {d_ofs:.3f}, swapped frames by {d_swap:.3f}")
    assert d_ofs >= 0.1 and d_swap >= 0.1
    assert abs(d_ofs - golden["decoy_distance"][0].item()) < 1e-6 and abs(d_swap - golden["decoy_distance"][1].item()) < 1e-6
    assert abs(float(meta["out_ofs0_rel_l2"]) - d_ofs) < 1e-5 and abs(float(meta["out_swapped_rel_l2"]) - d_swap) < 1e-5
