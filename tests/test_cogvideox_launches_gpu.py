"""The launch list of ``CogVideoXTransformer3DModel.forward_rows``: the C-ABI entry points one call issues, in order, written out
here for the four tiny models (sin-cos fp16 and FP8, rotary + learned table, 1.5 temporal patches + ofs) at batch 2.  The kernels'
values are pinned elsewhere; this pins that the host code strings them together as it did - one norm launch per (batch entry, stream),
one quantised operand for q, k and v, the rotary branch, the head per batch entry."""
import pytest
import torch

import cogvideox15_oracle as vo
import cogvideox_rope_oracle as ro
from cogvideox_support import DEV, DIT_SEED, dit_inputs, hip_twin, patchify, tiny_oracle

gpu = pytest.mark.gpu
B = 2


def _expected(layers, fp8=False, rotary=False, ofs=False):
    prologue = ["lkgd_timestep_embedding", "lkgd_gemm_f16", "lkgd_silu", "lkgd_gemm_f16"]          # time embedding
    if ofs:
        prologue += ["lkgd_add"]
    prologue += ["lkgd_silu", "lkgd_gemm_f16"]                                                       # the step's modulation
    prologue += ["lkgd_gemm_f16", "lkgd_gemm_f16"] * B                                               # text, video embedding per entry
    if fp8:
        block = ["lkgd_layernorm_quant_fp8"] * (2 * B) + ["lkgd_gemm_fp8"] * 3 + ["lkgd_layernorm"] * 2 \
            + ["lkgd_attn_spatial", "lkgd_quant_rows_fp8", "lkgd_gemm_fp8", "lkgd_gated_add"] \
            + ["lkgd_layernorm_quant_fp8"] * (2 * B) + ["lkgd_gemm_fp8", "lkgd_gelu_tanh_quant_fp8", "lkgd_gemm_fp8", "lkgd_gated_add"]
    else:
        block = ["lkgd_layernorm"] * (2 * B) + ["lkgd_gemm_f16"] * 3 + (["lkgd_qk_norm_rope"] if rotary else ["lkgd_layernorm"] * 2) \
            + ["lkgd_attn_spatial", "lkgd_gemm_f16", "lkgd_gated_add"] \
            + ["lkgd_layernorm"] * (2 * B) + ["lkgd_gemm_f16", "lkgd_gelu_tanh", "lkgd_gemm_f16", "lkgd_gated_add"]
    head = ["lkgd_layernorm", "lkgd_layernorm", "lkgd_gemm_f16"] * B
    return prologue + block * layers + head


def _recorded(run):
    """one eager warm-up, then a recorded call (tools/gemm_census.py::record_gemms): the entry-point names, in order"""
    from lkgd_amd import replay
    run()
    torch.cuda.synchronize()
    with replay.strict(False):                 # only the launch list is of interest here: nothing is replayed
        with replay.record() as p:
            run()
    torch.cuda.synchronize()
    names = [name for _, _, name, _ in p.calls]
    p.release()
    return names


@gpu
@pytest.mark.parametrize("model", ["sincos", "sincos_fp8", "rotary_learned", "v15_ofs"])
def test_forward_rows_launch_list(model):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import fp8
    from oracle import cogvideox as oc
    if model == "rotary_learned":
        cfg = ro.TINY_ROPE_DIT
        o = ro.seeded_model(cfg, DIT_SEED)
    elif model == "v15_ofs":
        cfg = vo.TINY_V15_DIT
        o = vo.seeded_model(cfg, DIT_SEED)
    else:
        cfg = oc.TINY_DIT
        o = tiny_oracle()
    m = hip_twin(o, cfg, DEV)
    if model == "sincos_fp8":
        fp8.quantize_to_float8(m)
    i = dit_inputs(cfg, batch=B)
    pt = m.config.patch_size_t
    rows = patchify(i["hidden"].half(), pt).to(DEV)
    F_, H, W = i["hidden"].shape[1], i["hidden"].shape[3], i["hidden"].shape[4]
    grid = (F_ // (pt or 1), H // 2, W // 2)
    text = m.fused_text(i["text"].to(DEV), i["domain"].to(DEV), i["flow"].to(DEV))
    extra = {}
    if m.config.use_rotary_positional_embeddings:
        extra["image_rotary_emb"] = pc.rotary_tables(m.config, *grid)
    if m.ofs_embedding is not None:
        extra["ofs_emb"] = m.embed_ofs(2.0, B)
    got = _recorded(lambda: m.forward_rows(rows, grid, text, 721.0, **extra))
    want = _expected(m.config.num_layers, fp8=model == "sincos_fp8", rotary=m.config.use_rotary_positional_embeddings,
                     ofs=m.ofs_embedding is not None)
    assert m._pk.fp8 == (model == "sincos_fp8")
    first = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (model, len(got), len(want), first, got[first:first + 6], want[first:first + 6])
