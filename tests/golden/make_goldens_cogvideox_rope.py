"""Generator of tests/golden/cogvideox_rope.safetensors: the reference's own in-tree ``CogVideoXTransformer3DModel``
(CogVideo-main/finetune/models/cogvideox_i2v/cogvideox_transformer_3d.py) constructed with ``use_rotary_positional_embeddings=True,
use_learned_positional_embeddings=True`` at the tiny geometry and run with ``image_rotary_emb``, over the restated diffusers
pieces of tests/cogvideox_rope_oracle.py (bound by name, as make_goldens.py::gen_cogvideox binds oracle/cogvideox.py's).  Runs
only where the reference tree is present; the stub machinery is make_goldens.py's, imported.

The rotation has to matter in the fixture: with ``init_weights_`` defaults rotating q / k moves the output by ~3 % (relative
L2), which a 1e-2 parity bound cannot tell from noise.  Every norm_q / norm_k weight is therefore scaled by
``NORM_QK_GAIN`` after ``init_weights_``, ``out_no_rope`` (identity tables: cos = 1, sin = 0) is stored next to ``out``, and the
relative L2 between the two is printed and asserted >= 0.1 here and in tests/test_cogvideox_rope_cpu.py.
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
from oracle import blocks as ob              # noqa: E402
from oracle import cogvideox as oc           # noqa: E402


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
    sys.modules["diffusers.models.embeddings"].CogVideoXPatchEmbed = ro.CogVideoXPatchEmbed

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
    ref = mg.load_ref("CogVideo-main/finetune/models/cogvideox_i2v/cogvideox_transformer_3d.py", "ref_cogvideox_transformer_3d_rope")
    cfg = ro.TINY_ROPE_DIT
    with torch.no_grad():
        m = ref.CogVideoXTransformer3DModel(**cfg.__dict__)
        m.init_quaternion_modules()
        o = ro.CogVideoXTransformer3DModel(cfg)
        assert sorted(k for k, _ in m.named_parameters()) == sorted(k for k, _ in o.named_parameters())
        assert sorted(m.state_dict()) == sorted(o.state_dict()) and "patch_embed.pos_embedding" in m.state_dict()
        oc.init_weights_(m, mg.DIT_SEED)
        ro.scale_qk_norm_(m, ro.NORM_QK_GAIN)
        for p in m.parameters():
            p.copy_(p.half().float())
        ro.seed_pos_embedding_(m, mg.DIT_SEED + 2)
        inp = mg.dit_inputs(cfg)
        f = (cfg.sample_frames - 1) // cfg.temporal_compression_ratio + 1
        h, w = cfg.sample_height // cfg.patch_size, cfg.sample_width // cfg.patch_size
        cos, sin = ro.rotary_tables(cfg, f, h, w)

        def run(tables):
            return m(inp["hidden"], inp["text"], inp["t"], inp["domain"], inp["flow"], image_rotary_emb=tables, return_dict=False)[0]
        out = {"checksum": torch.tensor(mg.checksum(m), dtype=torch.float64), "out": run((cos, sin)),
               "out_no_rope": run((torch.ones_like(cos), torch.zeros_like(sin))), "cos": cos, "sin": sin,
               "pos_embedding": m.patch_embed.pos_embedding.clone(), "norm_qk_gain": torch.tensor(ro.NORM_QK_GAIN)}
    gap = ((out["out"] - out["out_no_rope"]).norm() / out["out"].norm()).item()
    print("cogvideox_rope: out %s std %.4f; rotating q / k moves it by rel L2 %.3f (norm_q / norm_k gain x %g)"
          % (tuple(out["out"].shape), out["out"].std(), gap, ro.NORM_QK_GAIN))
    assert gap >= 0.1, "raise NORM_QK_GAIN: the rotation does not matter enough in this fixture"
    assert out["pos_embedding"][0, :cfg.max_text_seq_length].abs().min() > 0
    save_file({k: v.contiguous() for k, v in out.items()}, os.path.join(HERE, "cogvideox_rope.safetensors"))


if __name__ == "__main__":
    main()
