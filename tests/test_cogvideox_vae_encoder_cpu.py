"""Host side of the CogVideoX 3-D causal VAE encoder without a GPU: the refusals of the three entry points, state-dict names against
the oracle, which checkpoints build an encoder, frame-batch bounds and pooled frame counts, the oracle's own decoys, ``prepare_latents`` / ``retrieve_latents`` on a stub VAE, and the refusals of ``encode``."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import cogvideox_vae_encoder_oracle as eo
from c_interface import ALIGN, NULL, SHAPE, Host, entry
from cogvideox_support import rel


# ------------------------------------------------------------------------------------------------------------- refusals
def test_pixel_taps_refuses_before_launching():
    h = Host()
    call = entry("lkgd_cogvae_pixel_taps", x=h.p, out=h.p + 2048, ldo=128, B=1, Cin=3, T=5, H=6, W=10, t0=0, Tc=5)
    for k in ("x", "out"):
        assert call(**{k: None}) == NULL, k
    for kw in (dict(B=0), dict(T=0), dict(H=0), dict(W=0), dict(Tc=0), dict(Cin=0), dict(Cin=5), dict(t0=-1), dict(t0=1), dict(Tc=6),
               dict(t0=4, Tc=2), dict(ldo=120), dict(B=1 << 12, T=1 << 10, Tc=1 << 10, H=1 << 5, W=1 << 5)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(out=h.p + 8), dict(ldo=132), dict(x=h.p + 1)):
        assert call(**kw) == ALIGN, kw


def test_time_pool_refuses_before_launching():
    h = Host()
    call = entry("lkgd_cogvae_time_pool", in_=h.p, ldi=64, out=h.p + (1 << 20), ldo=64, B=2, T=5, HW=15, C=64)
    for k in ("in_", "out"):
        assert call(**{k: None}) == NULL, k
    for kw in (dict(B=0), dict(T=0), dict(HW=0), dict(C=0), dict(C=60), dict(ldi=56), dict(ldo=56), dict(B=1 << 12, T=1 << 10, HW=1 << 9),
               dict(out=h.p), dict(out=h.p + 64), dict(out=h.p - 128)):           # the last three: in and out overlap
        assert call(**kw) == SHAPE, kw
    for kw in (dict(in_=h.p + 8), dict(out=h.p + (1 << 20) + 8), dict(ldi=68), dict(ldo=68)):
        assert call(**kw) == ALIGN, kw


def test_posterior_refuses_before_launching():
    h = Host()
    call = entry("lkgd_cogvae_posterior", mom=h.p, ldm=32, noise=h.p, mean=h.p, sample=h.p, scale=1.0, B=1, lc=16, T=1, h=6, w=10)
    for k in ("mom", "mean", "sample"):
        assert call(**{k: None}) == NULL, k
    for kw in (dict(B=0), dict(T=0), dict(h=0), dict(w=0), dict(lc=0), dict(lc=12), dict(ldm=24), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(B=1 << 10, T=1 << 7, h=1 << 7, w=1 << 7)):
        assert call(**kw) == SHAPE, kw
    for kw in (dict(mom=h.p + 8), dict(ldm=36), dict(mean=h.p + 1), dict(noise=h.p + 1), dict(sample=h.p + 1)):
        assert call(**kw) == ALIGN, kw


# ----------------------------------------------------------------------------------------------------------- state dict
def _module(cfg=eo.TINY, **kw):
    from lkgd_amd import cogvideox_vae as pv
    return pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**cfg.__dict__), **kw)


def test_state_dict_with_encoder_equals_the_oracles():
    for cfg in (eo.TINY, eo.CogVAEConfig(block_out_channels=(64, 128, 64, 128), layers_per_block=2)):
        o, m = eo.AutoencoderKLCogVideoX(cfg), _module(cfg, encoder=True)
        ko = {k: tuple(v.shape) for k, v in o.state_dict().items()}
        km = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        assert ko == km
        for name in ("encoder.conv_in.conv.weight", "encoder.down_blocks.0.resnets.0.norm1.weight",
                     "encoder.down_blocks.0.resnets.0.conv1.conv.weight", "encoder.down_blocks.0.downsamplers.0.conv.weight",
                     "encoder.mid_block.resnets.1.conv2.conv.bias", "encoder.norm_out.weight", "encoder.conv_out.conv.weight",
                     "decoder.conv_in.conv.weight"):
            assert name in km, name
        assert km["encoder.conv_in.conv.weight"] == (64, 3, 3, 3, 3) and km["encoder.conv_out.conv.weight"][:2] == (32, 128)
        assert not any(k.startswith(f"encoder.down_blocks.{len(cfg.block_out_channels) - 1}.downsamplers") for k in km)
    assert km["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] == (128, 64, 1, 1, 1)      # (64, 128, 64, 128): the width changes
    assert "encoder.down_blocks.1.resnets.1.conv_shortcut.weight" not in km
    # compress_time on the first log2(4) = 2 downsamplers only
    assert [b.downsamplers[0].compress_time for b in m.encoder.down_blocks[:-1]] == [True, True, False]
    # the default stays decoder-only
    assert all(k.startswith("decoder.") for k in _module().state_dict())


def test_encoder_keys_load_strictly_quant_conv_dropped():
    o = eo.tiny_weights()
    m = _module(encoder=True)
    m.load_state_dict({**o.state_dict(), "quant_conv.weight": torch.zeros(3)})
    assert torch.equal(m.encoder.conv_out.conv.bias, o.encoder.conv_out.conv.bias)
    bad = dict(o.state_dict())
    bad["encoder.conv_in.conv.wieght"] = bad.pop("encoder.conv_in.conv.weight")
    with pytest.raises(RuntimeError, match="encoder.conv_in.conv.w"):
        m.load_state_dict(bad)
    missing = {k: v for k, v in o.state_dict().items() if k != "encoder.norm_out.bias"}
    with pytest.raises(RuntimeError, match="encoder.norm_out.bias"):
        m.load_state_dict(missing)
    d = _module()                                                # decoder-only: the same checkpoint loads, the encoder keys are dropped
    d.load_state_dict(o.state_dict())
    assert torch.equal(d.decoder.conv_out.conv.bias, o.decoder.conv_out.conv.bias)


def test_from_pretrained_builds_the_encoder_iff_the_checkpoint_has_one(tmp_path):
    from safetensors.torch import load_file, save_file
    from lkgd_amd import cogvideox_vae as pv
    o = eo.tiny_weights()
    full = _module(encoder=True)
    full.load_state_dict(o.state_dict())
    full.save_pretrained(str(tmp_path / "full" / "vae"))
    dec = _module()
    dec.load_state_dict(o.state_dict())
    dec.save_pretrained(str(tmp_path / "dec" / "vae"))
    a = pv.AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "full"), subfolder="vae", torch_dtype=torch.float16)
    assert a.has_encoder and a.dtype == torch.float16 and a.config.in_channels == 3
    for k, v in full.state_dict().items():
        assert torch.equal(a.state_dict()[k].float(), v.half().float()), k
    b = pv.AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "dec"), subfolder="vae")
    assert not b.has_encoder and set(b.state_dict()) == set(dec.state_dict())
    # explicit choices override the checkpoint's contents, both ways round
    c = pv.AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "full"), subfolder="vae", encoder=False)
    assert not c.has_encoder
    with pytest.raises(RuntimeError, match="encoder.conv_in"):
        pv.AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "dec"), subfolder="vae", encoder=True)
    # a misspelt encoder key is refused
    f = str(tmp_path / "full" / "vae" / "diffusion_pytorch_model.safetensors")
    sd = load_file(f)
    sd["encoder.conv_in.conv.wieght"] = sd.pop("encoder.conv_in.conv.weight")
    save_file(sd, f)
    with pytest.raises(RuntimeError, match="encoder.conv_in.conv.w"):
        pv.AutoencoderKLCogVideoX.from_pretrained(str(tmp_path / "full"), subfolder="vae")


# --------------------------------------------------------------------------------------------------- batches and frames
@pytest.mark.parametrize("T,bounds", [(49, [(0, 9), (9, 17), (17, 25), (25, 33), (33, 41), (41, 49)]), (17, [(0, 9), (9, 17)]),
                                      (5, [(0, 5)]), (1, [(0, 1)]), (16, [(0, 8), (8, 16)])])
def test_frame_batch_bounds(T, bounds):
    from lkgd_amd import cogvideox_vae as pv
    assert pv.frame_batch_bounds(T) == bounds == eo.frame_batch_bounds(T)
    assert eo.frame_batch_bounds(17, remainder_last=True) == [(0, 8), (8, 17)]


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 8, 9])
def test_pooled_frame_counts_against_avg_pool1d(T):
    from lkgd_amd import cogvideox_vae as pv
    from lkgd_amd import ops
    x = torch.arange(T, dtype=torch.float32).reshape(1, 1, T, 1, 1)
    y = eo.time_pool(x)[0, 0, :, 0, 0]
    assert ops.pooled_frames(T) == y.numel()
    if T % 2:                       # as diffusers writes it: the first frame apart, the rest through avg_pool1d
        want = torch.cat([x[0, 0, :1, 0, 0], F.avg_pool1d(x[0, 0, 1:, 0, 0][None, None], 2, 2)[0, 0]]) if T > 1 else x[0, 0, :, 0, 0]
    else:
        want = F.avg_pool1d(x[0, 0, :, 0, 0][None, None], 2, 2)[0, 0]
    assert torch.equal(y, want)
    # 49 frames -> 13 latent frames through the batches
    assert sum(ops.pooled_frames(ops.pooled_frames(b - a)) for a, b in pv.frame_batch_bounds(49)) == 13


# --------------------------------------------------------------------------------------------------------------- oracle
@pytest.fixture(scope="module")
def oracle():
    return eo.tiny_weights()


@pytest.mark.parametrize("T", [1, 2, 5, 9, 16, 17, 25])
def test_oracle_decoys_differ_where_the_table_says(oracle, T):
    """relative L2 of each decoy's moments from the true ones: at least 0.1 where the table says they differ (measured 0.26 - 1.21),
    exactly equal where it says equal"""
    x = eo.tiny_clip(T)
    truth = oracle.moments(x)
    mean, logvar = truth.chunk(2, dim=1)
    assert mean.abs().max().item() < 1.7 and -1.6 < logvar.min().item() and logvar.max().item() < 1.5      # the clamp is not exercised
    for name, where in eo.DECOYS.items():
        if T in where["differs"]:
            d = rel(eo.decoy_moments(oracle, name, x), truth)
            assert d >= 0.1, (name, T, d)
        elif T in where["equal"]:
            assert torch.equal(eo.decoy_moments(oracle, name, x), truth), (name, T)


# ------------------------------------------------------------------------------------------------------ prepare_latents
class _StubDist:
    def __init__(self, mean):
        self.mean, self.calls = mean, []

    def sample(self, generator=None):
        self.calls.append(generator)
        return self.mean + 1.0

    def mode(self):
        return self.mean


class _StubVAE:
    """``encode`` returns a fixed distribution: mean = the image's index + 1 everywhere"""

    def __init__(self, invert=False, scaling_factor=0.7):
        self.config = SimpleNamespace(temporal_compression_ratio=4, block_out_channels=(128, 256, 256, 512),
                                      scaling_factor=scaling_factor, invert_scale_latents=invert)
        self.device, self.dtype = torch.device("cpu"), torch.float32
        self.seen = []

    def encode(self, x):
        assert x.dim() == 5 and x.shape[0] == 1 and x.shape[2] == 1          # one image at a time, [1, C, 1, H, W]
        self.seen.append(x)
        d = _StubDist(torch.full((1, 16, 1, x.shape[3] // 8, x.shape[4] // 8), float(x[0, 0, 0, 0, 0])))
        return SimpleNamespace(latent_dist=d)


def _images(B):
    return (torch.arange(B, dtype=torch.float32) + 1.0)[:, None, None, None].expand(B, 3, 48, 80).contiguous()


def test_prepare_latents_shapes_padding_and_scale():
    from lkgd_amd import cogvideox as pc
    sched = SimpleNamespace(init_noise_sigma=1.0)
    vae = _StubVAE()
    g = torch.Generator().manual_seed(5)
    lat, img = pc.prepare_latents(vae, sched, SimpleNamespace(patch_size_t=None), _images(2), batch_size=2, num_frames=9, height=48,
                                  width=80, dtype=torch.float32, device="cpu", generator=g)
    assert tuple(lat.shape) == tuple(img.shape) == (2, 3, 16, 6, 10)
    assert len(vae.seen) == 2
    for i in range(2):
        assert torch.allclose(img[i, 0], torch.full((16, 6, 10), 0.7 * (i + 1.0 + 1.0)))          # scaling_factor * sample
    assert bool((img[:, 1:] == 0).all())                                                          # the padding frames
    want = torch.randn((2, 3, 16, 6, 10), generator=torch.Generator().manual_seed(5))
    assert torch.equal(lat, want)
    # invert_scale_latents: the inverse factor
    _, img = pc.prepare_latents(_StubVAE(invert=True), sched, SimpleNamespace(patch_size_t=None), _images(1), num_frames=9, height=48,
                                width=80, dtype=torch.float32, device="cpu")
    assert torch.allclose(img[0, 0], torch.full((16, 6, 10), 2.0 / 0.7))
    # given latents are taken as they are, times init_noise_sigma
    given = torch.ones(1, 3, 16, 6, 10)
    lat, _ = pc.prepare_latents(_StubVAE(), SimpleNamespace(init_noise_sigma=2.5), SimpleNamespace(patch_size_t=None), _images(1),
                                num_frames=9, height=48, width=80, dtype=torch.float32, device="cpu", latents=given)
    assert torch.equal(lat, 2.5 * given)


def test_prepare_latents_temporal_patches_and_generator_list():
    from lkgd_amd import cogvideox as pc
    sched = SimpleNamespace(init_noise_sigma=1.0)
    tc = SimpleNamespace(patch_size_t=2)
    lat, img = pc.prepare_latents(_StubVAE(), sched, tc, _images(1), num_frames=9, height=48, width=80, dtype=torch.float32, device="cpu")
    assert tuple(lat.shape) == tuple(img.shape) == (1, 4, 16, 6, 10)          # 3 latent frames + 3 % 2
    assert torch.equal(img[:, 0], img[:, 1]) and bool((img[:, 0] != 0).all()) and bool((img[:, 2:] == 0).all())
    lat, img = pc.prepare_latents(_StubVAE(), sched, tc, _images(1), num_frames=13, height=48, width=80, dtype=torch.float32,
                                  device="cpu")
    assert tuple(lat.shape) == tuple(img.shape) == (1, 4, 16, 6, 10)          # 4 latent frames: nothing added
    assert bool((img[:, 1:] == 0).all())
    gens = [torch.Generator().manual_seed(s) for s in (1, 2)]
    vae = _StubVAE()
    lat, img = pc.prepare_latents(vae, sched, SimpleNamespace(patch_size_t=None), _images(2), batch_size=2, num_frames=5, height=48,
                                  width=80, dtype=torch.float32, device="cpu", generator=gens)
    want = torch.cat([torch.randn((1, 2, 16, 6, 10), generator=torch.Generator().manual_seed(s)) for s in (1, 2)])
    assert torch.equal(lat, want)
    with pytest.raises(ValueError, match="list of generators of length 2"):
        pc.prepare_latents(_StubVAE(), sched, SimpleNamespace(patch_size_t=None), _images(3), batch_size=3, generator=gens)


def test_retrieve_latents():
    from lkgd_amd import cogvideox as pc
    d = _StubDist(torch.zeros(2))
    out = SimpleNamespace(latent_dist=d)
    g = torch.Generator()
    assert torch.equal(pc.retrieve_latents(out, g), torch.ones(2)) and d.calls == [g]
    assert torch.equal(pc.retrieve_latents(out, sample_mode="argmax"), torch.zeros(2))
    assert torch.equal(pc.retrieve_latents(SimpleNamespace(latents=torch.ones(1))), torch.ones(1))
    with pytest.raises(AttributeError, match="Could not access latents"):
        pc.retrieve_latents(SimpleNamespace())


# ------------------------------------------------------------------------------------------------------------- refusals
def test_encode_refusals_name_what_they_refuse():
    from lkgd_amd import LkgdHipError
    from lkgd_amd import cogvideox_vae as pv
    with pytest.raises(LkgdHipError, match="encode.*without its encoder.*encoder=True"):
        _module().encode(torch.zeros(1, 3, 1, 8, 8))
    m = _module(encoder=True)
    with pytest.raises(ValueError, match="multiples of 8"):
        m.encode(torch.zeros(1, 3, 1, 47, 80))                       # odd H
    with pytest.raises(ValueError, match="multiples of 8"):
        m.encode(torch.zeros(1, 3, 1, 48, 84))
    with pytest.raises(ValueError, match=r"\[B, 3, T, H, W\]"):
        m.encode(torch.zeros(1, 4, 1, 48, 80))
    with pytest.raises(LkgdHipError, match="MI355X"):
        m.encode(torch.zeros(1, 3, 1, 48, 80))                       # no CPU path
    with pytest.raises(LkgdHipError, match="use_quant_conv"):
        pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(block_out_channels=(64, 64, 128, 128), use_quant_conv=True), encoder=True)
    with pytest.raises(LkgdHipError, match="in_channels = 5"):
        pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(block_out_channels=(64, 64, 128, 128), in_channels=5), encoder=True)
    with pytest.raises(LkgdHipError, match="enable_tiling"):
        m.enable_tiling()
    with pytest.raises(LkgdHipError, match="enable_slicing"):
        m.enable_slicing()
    with pytest.raises(LkgdHipError, match="bf16"):
        m.to(torch.bfloat16).encode(torch.zeros(1, 3, 1, 48, 80))
