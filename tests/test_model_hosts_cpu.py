"""The host side every model shares, without a GPU: ``PackedModule``'s bookkeeping on each host class (what forgets the pack, the
off-GPU refusal, where ``device`` / ``dtype`` come from), the CLIP / ViT layer pack of ``lkgd_amd/encoder.py`` against the fold written
out longhand, and the transformers-layout ``save_pretrained`` -> ``from_pretrained`` round trip of T5 and CLIP."""
import json
import os
from types import SimpleNamespace

import pytest
import torch

from t5_support import TINY_A

#: hidden 128, 2 heads of 64, intermediate 512: the smallest widths the CLIP config check admits
TINY_CLIP = dict(hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, patch_size=14, image_size=28,
                 projection_dim=64)


def _unet(name):
    def make():
        from lkgd_amd import controlnet, unet as pu
        from oracle import unet as ou
        cls = getattr(controlnet, name) if name == "ControlNetSDVModel" else getattr(pu, name)
        return cls(pu.UNetConfig(**ou.TINY_CONFIG.__dict__))
    return make


def _vae():
    from lkgd_amd import vae as pv
    from oracle import vae as ov
    return pv.AutoencoderKLTemporalDecoder(pv.VAEConfig(**ov.TINY_VAE_CONFIG.__dict__))


def _cogvae():
    import cogvideox_vae_oracle as oc
    from lkgd_amd import cogvideox_vae as pv
    return pv.AutoencoderKLCogVideoX(pv.CogVAEConfig(**oc.TINY.__dict__))


def _dit():
    from cogvideox_support import tiny_cpu_model
    return tiny_cpu_model()


def _t5():
    from lkgd_amd import t5
    return t5.T5EncoderModel(t5.T5Config(**TINY_A))


def _clip(**over):
    from lkgd_amd import clip
    return clip.CLIPVisionModelWithProjection(clip.CLIPVisionConfig(**{**TINY_CLIP, **over}))


def _vit():
    from lkgd_amd import vit as pv
    from oracle import vit as ov
    return pv.VisionTransformer(pv.ViTConfig(**ov.TINY_VIT.__dict__))


#: class -> (constructor at its tiny config, the parameter ``device`` / ``dtype`` were anchored on before ``PackedModule``, the further
#: weight-derived cache ``invalidate()`` empties as (attribute, a filled value, the empty value) or None, the off-GPU sentence)
HOSTS = {
    "UNetSpatioTemporalConditionModel": (_unet("UNetSpatioTemporalConditionModel"), "conv_in.weight", ("_lk_cache", ("key", 1), None),
                                         "lkgd_amd UNet runs on MI355X only: move the module to cuda before forward()"),
    "UNetSpatioTemporalConditionControlNetModel": (_unet("UNetSpatioTemporalConditionControlNetModel"), "conv_in.weight", None,
                                                   "lkgd_amd UNet runs on MI355X only: move the module to cuda before forward()"),
    "ControlNetSDVModel": (_unet("ControlNetSDVModel"), "conv_in.weight", None,
                           "lkgd_amd UNet runs on MI355X only: move the module to cuda before forward()"),
    "AutoencoderKLTemporalDecoder": (_vae, "quant_conv.weight", None, "lkgd_amd VAE runs on MI355X only: move the module to cuda first"),
    "AutoencoderKLCogVideoX": (_cogvae, "decoder.conv_in.conv.weight", None,
                               "lkgd_amd CogVideoX VAE runs on MI355X only: move the module to cuda first"),
    "CogVideoXTransformer3DModel": (_dit, "proj_out.weight", ("_pos", {(1, 2, 3): 0}, {}),
                                    "lkgd_amd DiT runs on MI355X only: move the module to cuda first"),
    "T5EncoderModel": (_t5, "shared.weight", ("_bias_tables", {7: 0}, {}), "lkgd_amd T5 runs on MI355X only: move the module to cuda first"),
    "CLIPVisionModelWithProjection": (_clip, "visual_projection.weight", None,
                                      "lkgd_amd CLIP runs on MI355X only: move the module to cuda first"),
    "VisionTransformer": (_vit, "cls_token", None, "lkgd_amd ViT runs on MI355X only: move the module to cuda first"),
}


@pytest.fixture(scope="module", params=sorted(HOSTS))
def host(request):
    make, anchor, cache, sentence = HOSTS[request.param]
    return SimpleNamespace(name=request.param, m=make(), anchor=anchor, cache=cache, sentence=sentence)


def _fill(h):
    h.m._pk = object()                  # a stand-in for a packed model
    if h.cache is not None:
        setattr(h.m, h.cache[0], h.cache[1])


def _forgotten(h):
    return h.m._pk is None and (h.cache is None or getattr(h.m, h.cache[0]) == h.cache[2])


def test_host_is_a_packed_module(host):
    from lkgd_amd.module import PackedModule
    assert isinstance(host.m, PackedModule) and type(host.m).__name__ == host.name and host.m._pk is None
    for name in ("load_state_dict", "_apply", "invalidate", "prepare", "device", "dtype"):
        owner = next(c for c in type(host.m).__mro__ if name in c.__dict__)
        # the two overrides that add something class-specific (tied embedding; dropped prefixes) end in the base call
        if name == "load_state_dict" and host.name in ("T5EncoderModel", "AutoencoderKLCogVideoX"):
            assert owner is type(host.m)
        else:
            assert owner is PackedModule, (name, owner)


@pytest.mark.parametrize("how", ["invalidate", "load_state_dict", "float", "to_cpu"])
def test_pack_is_forgotten(host, how):
    _fill(host)
    assert not _forgotten(host)
    if how == "invalidate":
        host.m.invalidate()
    elif how == "load_state_dict":
        host.m.load_state_dict(host.m.state_dict())
    elif how == "float":
        host.m.float()
    else:
        host.m.to("cpu")
    assert _forgotten(host), how


def test_prepare_refuses_a_cpu_module(host):
    from lkgd_amd._lib import LkgdHipError
    host.m.invalidate()
    with pytest.raises(LkgdHipError) as e:
        host.m.prepare()
    assert str(e.value) == host.sentence and host.m._pk is None
    host.m._pk = kept = object()        # packed: prepare() returns before the device check
    host.m.prepare()
    assert host.m._pk is kept
    host.m.invalidate()


def test_device_and_dtype_are_the_old_anchor(host):
    m = host.m.float()
    p = m.get_parameter(host.anchor)
    assert m.dtype == p.dtype == torch.float32 and m.device == p.device
    m.half()
    p = m.get_parameter(host.anchor)
    assert m.dtype == p.dtype == torch.float16 and m.device == p.device
    m.float()


def test_init_synthetic_weights_forgets_the_pack_of_every_host(host):
    """it ends in ``invalidate()``: CLIP and the ViT had none, and kept a stale pack"""
    from lkgd_amd.unet import init_synthetic_weights_
    _fill(host)
    init_synthetic_weights_(host.m, 1)
    assert _forgotten(host)


# ---- the CLIP / ViT layer pack ---------------------------------------------------------------------------------------------------
def _randomise(m, seed):
    """non-trivial norms and biases (the default init leaves them at 1 / 0)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
            elif "norm" in n and n.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=g) * 0.6 + 0.7)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[-1] ** -0.5)
    return m


def _longhand(norm1, W, b, out_proj, norm2, fc1, fc2, act):
    """the pack as clip.py / vit.py wrote it before lkgd_amd/encoder.py: W diag(g) and b + W beta in fp32, GELU as GEGLU with a
    constant-one hidden half, quick_gelu as silu(1.702 x) / 1.702"""
    from lkgd_amd.packing import pack_geglu, pack_linear
    g1, be1, g2, be2 = norm1.weight.float(), norm1.bias.float(), norm2.weight.float(), norm2.bias.float()
    W, W1 = W.float(), fc1.weight.float()
    want = dict(wqkv=pack_linear(W * g1[None, :]), bqkv=b.float() + W @ be1, wo=pack_linear(out_proj.weight), bo=out_proj.bias.float(),
                b2=fc2.bias.float(), act=act)
    b1 = fc1.bias.float() + W1 @ be2
    W1 = W1 * g2[None, :]
    if act == "gelu":
        want["w1"], want["b1"], want["half"] = pack_geglu(torch.cat([torch.zeros_like(W1), W1], dim=0),
                                                          torch.cat([torch.ones_like(b1), b1], dim=0))
        want["w2"] = pack_linear(fc2.weight)
    else:
        want["w1"], want["b1"], want["half"] = pack_linear(W1 * 1.702), b1 * 1.702, 0
        want["w2"] = pack_linear(fc2.weight.float() / 1.702)
    return want


def _same_pack(got, want):
    assert set(vars(got)) == set(want) == {"wqkv", "bqkv", "wo", "bo", "w1", "b1", "half", "w2", "b2", "act"}
    for k, w in want.items():
        g = getattr(got, k)
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape and g.is_contiguous() and torch.equal(g, w), k
        else:
            assert g == w and type(g) is type(w), k


@pytest.mark.parametrize("act", ["gelu", "quick_gelu"])
def test_clip_layer_pack_is_the_longhand_fold(act):
    m = _randomise(_clip(hidden_act=act, num_hidden_layers=1), 3)
    layer = m.vision_model.encoder.layers[0]
    a = layer.self_attn
    with torch.no_grad():
        got = layer.pack(act)
        W = torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], dim=0)
        b = torch.cat([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias], dim=0)
        want = _longhand(layer.layer_norm1, W, b, a.out_proj, layer.layer_norm2, layer.mlp.fc1, layer.mlp.fc2, act)
    _same_pack(got, want)
    assert got.wqkv.shape == (384, 128) and got.w2.shape == (128, 512) and got.w1.shape[0] == (1024 if act == "gelu" else 512)
    assert (got.half > 0) == (act == "gelu")


def test_vit_block_pack_is_the_longhand_fold():
    blk = _randomise(_vit(), 4).blocks[1]
    with torch.no_grad():
        got = blk.pack()
        want = _longhand(blk.norm1, blk.attn.qkv.weight, blk.attn.qkv.bias, blk.attn.proj, blk.norm2, blk.mlp.fc1, blk.mlp.fc2, "gelu")
    _same_pack(got, want)
    assert got.wqkv.shape == (384, 128) and got.w1.shape == (1024, 128) and got.w2.shape == (128, 512)


# ---- the transformers directory layout ---------------------------------------------------------------------------------------------
def _round_trip(ours, cls, path, subfolder, header_keys):
    from safetensors.torch import load_file
    ours._pk = object()
    ours.save_pretrained(os.path.join(path, subfolder) if subfolder else path)
    d = os.path.join(path, subfolder) if subfolder else path
    assert sorted(os.listdir(d)) == ["config.json", "model.safetensors"]
    with open(os.path.join(d, "config.json")) as fh:
        cfg = json.load(fh)
    assert list(cfg) == header_keys + list(type(ours.config).__dataclass_fields__)
    assert {k: cfg[k] for k in type(ours.config).__dataclass_fields__} == ours.config.__dict__
    back = cls.from_pretrained(path, subfolder=subfolder, torch_dtype=torch.float32)
    assert back.config == ours.config and back.dtype == torch.float32 and back._pk is None
    assert list(back.state_dict()) == list(ours.state_dict())
    for k, v in ours.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
    assert cls.from_pretrained(path, subfolder=subfolder).dtype == torch.float16                        # the default
    assert cls.from_pretrained(path, subfolder=subfolder, torch_dtype=torch.float16, dtype=torch.float32).dtype == torch.float32
    return cfg, load_file(os.path.join(d, "model.safetensors"))


def test_t5_transformers_layout_round_trip(tmp_path):
    from lkgd_amd import t5
    ours = _randomise(_t5(), 5)
    cfg, on_disk = _round_trip(ours, t5.T5EncoderModel, str(tmp_path), "text_encoder",
                               ["architectures", "model_type", "is_gated_act", "dense_act_fn"])
    assert cfg["architectures"] == ["T5EncoderModel"] and cfg["model_type"] == "t5" and cfg["is_gated_act"] is True \
        and cfg["dense_act_fn"] == "gelu_new"
    # one tensor per storage: the tied copy stays out of the file, and comes back tied
    assert set(on_disk) == set(ours.state_dict()) - {"encoder.embed_tokens.weight"} and "shared.weight" in on_disk
    back = t5.T5EncoderModel.from_pretrained(str(tmp_path))                                             # subfolder "text_encoder"
    assert back.encoder.embed_tokens.weight is back.shared.weight


def test_clip_transformers_layout_round_trip(tmp_path):
    from safetensors.torch import save_file
    from lkgd_amd import clip
    ours = _randomise(_clip(hidden_act="quick_gelu"), 6)
    cfg, on_disk = _round_trip(ours, clip.CLIPVisionModelWithProjection, str(tmp_path), None, ["architectures", "model_type"])
    assert cfg["architectures"] == ["CLIPVisionModelWithProjection"] and cfg["model_type"] == "clip_vision_model"
    assert set(on_disk) == set(ours.state_dict())
    # a persisted ``position_ids`` buffer of older checkpoints is tolerated; any other stray key is not
    on_disk["vision_model.embeddings.position_ids"] = torch.arange(5)[None]
    save_file(on_disk, str(tmp_path / "model.safetensors"))
    back = clip.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), torch_dtype=torch.float32)
    assert all(torch.equal(back.state_dict()[k], v) for k, v in ours.state_dict().items())
    on_disk["vision_model.embeddings.stray"] = torch.zeros(1)
    save_file(on_disk, str(tmp_path / "model.safetensors"))
    with pytest.raises(RuntimeError, match="stray"):
        clip.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path))
