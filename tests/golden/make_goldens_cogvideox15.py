"""Generator of tests/golden/cogvideox15.safetensors: the reference's own in-tree ``CogVideoXTransformer3DModel``
(CogVideo-main/finetune/models/cogvideox_i2v/cogvideox_transformer_3d.py) constructed as a CogVideoX 1.5 image-to-video model -
``patch_size_t=2, ofs_embed_dim, patch_bias=False, use_rotary_positional_embeddings=True, use_learned_positional_embeddings=False``
- at the tiny geometry (4 latent frames) and run with ``ofs = 2.0`` and the slice rotary tables, over the restated diffusers pieces
of tests/cogvideox15_oracle.py (bound by name, as make_goldens_cogvideox_rope.py binds its twin's).  Runs only where the reference
tree is present; the stub machinery is make_goldens.py's, imported.

The fixture has to see the new code, so two DECOYS are stored beside ``out``: ``out_ofs0`` (the same forward with ``ofs = 0.0``) and
``out_swapped`` (the same forward on an input whose two frames of every temporal patch are exchanged: what a (pt, c) or a
frame-in-patch transposition in the patch rows would feed the model).  Each has to differ from ``out`` by at least ``DECOY_MIN`` =
ten times the forward test's relative-L2 bound (1e-2).  With ``init_weights_`` defaults ``ofs = 0`` moves the output by 0.40 and
the swap by 1.26, so no gain on the ofs_embedding weights is needed (``OFS_GAIN`` = 1 is recorded; x 4 would only inflate the
output's scale ninefold); the q / k norms keep the rope fixture's x 4 so that the rotary tables matter as they do there.  The observed
distances are printed, stored as tensors and written into the file's metadata.
"""
from __future__ import annotations

import os
import sys

import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_goldens as mg                    # noqa: E402
import cogvideox_rope_oracle as ro           # noqa: E402
import cogvideox15_oracle as vo              # noqa: E402
from oracle import blocks as ob              # noqa: E402
from oracle import cogvideox as oc           # noqa: E402

FORWARD_BOUND = 1e-2                          # tests/test_cogvideox15_gpu.py: relative L2 of the HIP forward against ``out``
DECOY_MIN = 10 * FORWARD_BOUND


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def main():
    assert os.path.isdir(mg.REF), "runs only where the reference tree is mounted"
    mg.install_stubs()
    sys.path.insert(0, mg.REF)
    du = sys.modules["diffusers.utils"]
    du.USE_PEFT_BACKEND = False
    du.scale_lora_layers = lambda *a, **k: None
    du.unscale_lora_layers = lambda *a, **k: None
    sys.modules["diffusers.utils.torch_utils"].maybe_allow_in_graph = lambda c: c
    at = mg._mod("diffusers.models.attention")
    at.Attention, at.FeedForward = oc.Attention, oc.FeedForward
    ap = sys.modules["diffusers.models.attention_processor"]
    ap.CogVideoXAttnProcessor2_0 = ap.FusedCogVideoXAttnProcessor2_0 = ro.CogVideoXAttnProcessor2_0
    mg._mod("diffusers.models.cache_utils").CacheMixin = type("CacheMixin", (), {})
    sys.modules["diffusers.models.embeddings"].CogVideoXPatchEmbed = vo.CogVideoXPatchEmbed

    class _TE(ob.TimestepEmbedding):          # diffusers' signature (in_channels, time_embed_dim, act_fn, out_dim) / forward(x, cond)
        def __init__(self, in_channels, time_embed_dim, act_fn="silu", out_dim=None):
            assert act_fn == "silu"
            super().__init__(in_channels, time_embed_dim, out_dim)

        def forward(self, sample, condition=None):
            assert condition is None
            return super().forward(sample)
    sys.modules["diffusers.models.embeddings"].TimestepEmbedding = _TE
    mg._mod("diffusers.models.modeling_outputs").Transformer2DModelOutput = type("Transformer2DModelOutput", (), {})
    nm = sys.modules["diffusers.models.normalization"]
    nm.AdaLayerNorm, nm.CogVideoXLayerNormZero = oc.AdaLayerNorm, oc.CogVideoXLayerNormZero
    ref = mg.load_ref("CogVideo-main/finetune/models/cogvideox_i2v/cogvideox_transformer_3d.py", "ref_cogvideox_transformer_3d_v15")
    cfg = vo.TINY_V15_DIT
    with torch.no_grad():
        m = ref.CogVideoXTransformer3DModel(**cfg.__dict__)
        m.init_quaternion_modules()
        o = vo.CogVideoXTransformer3DModel(cfg)
        assert sorted((k, tuple(v.shape)) for k, v in m.named_parameters()) == sorted((k, tuple(v.shape)) for k, v in o.named_parameters())
        sd = m.state_dict()
        assert sorted(sd) == sorted(o.state_dict()) and "patch_embed.pos_embedding" not in sd and "patch_embed.proj.bias" not in sd
        assert tuple(sd["patch_embed.proj.weight"].shape) == (128, 256) and sd["proj_out.weight"].shape[0] == 128
        assert "ofs_embedding.linear_1.weight" in sd
        oc.init_weights_(m, mg.DIT_SEED)
        ro.scale_qk_norm_(m, ro.NORM_QK_GAIN)
        vo.scale_ofs_embedding_(m, vo.OFS_GAIN)
        for p in m.parameters():
            p.copy_(p.half().float())
        inp = mg.dit_inputs(cfg)
        f = inp["hidden"].shape[1]
        assert f == 4
        h, w = cfg.sample_height // cfg.patch_size, cfg.sample_width // cfg.patch_size
        cos, sin = vo.rotary_tables(cfg, f, h, w)

        def run(hidden, ofs):
            return m(hidden, inp["text"], inp["t"], inp["domain"], inp["flow"], ofs=torch.full((1,), ofs),
                     image_rotary_emb=(cos, sin), return_dict=False)[0]
        out = {"checksum": torch.tensor(mg.checksum(m), dtype=torch.float64), "out": run(inp["hidden"], vo.OFS),
               "out_ofs0": run(inp["hidden"], 0.0), "out_swapped": run(vo.swap_frames_in_patches(inp["hidden"]), vo.OFS),
               "cos": cos, "sin": sin, "norm_qk_gain": torch.tensor(ro.NORM_QK_GAIN), "ofs_gain": torch.tensor(vo.OFS_GAIN),
               "ofs": torch.tensor(vo.OFS)}
    d_ofs, d_swap = _rel(out["out_ofs0"], out["out"]), _rel(out["out_swapped"], out["out"])
    out["decoy_distance"] = torch.tensor([d_ofs, d_swap], dtype=torch.float64)
    print("cogvideox15: out %s std %.4f; ofs = 0 moves it by rel L2 %.3f (ofs_embedding gain x %g), swapping the frames of every "
          "temporal patch by %.3f" % (tuple(out["out"].shape), out["out"].std(), d_ofs, vo.OFS_GAIN, d_swap))
    assert d_ofs >= DECOY_MIN, "raise OFS_GAIN (cogvideox15_oracle.py): ofs does not matter enough in this fixture"
    assert d_swap >= DECOY_MIN, "the frame order inside a temporal patch does not matter enough in this fixture"
    meta = {"out_ofs0_rel_l2": "%.6f" % d_ofs, "out_swapped_rel_l2": "%.6f" % d_swap, "ofs_gain": "%g" % vo.OFS_GAIN,
            "norm_qk_gain": "%g" % ro.NORM_QK_GAIN, "decoy_min": "%g" % DECOY_MIN}
    save_file({k: v.contiguous() for k, v in out.items()}, os.path.join(HERE, "cogvideox15.safetensors"), metadata=meta)


if __name__ == "__main__":
    main()
