"""LoRA adapters on the CogVideoX DiT, on the GPU: the adapter is folded into the packed weight (fp32 ``W + sum c B A`` on the device,
one rounding to fp16), and nothing else changes.

* The fold itself: exact where the exact result is an fp16 number; everywhere else inside the bound derived from the number formats
  (tests/cogvideox_lora_support.py::assert_within_fold_bound) - on the tiny model and on single linears of the 5B and 2B widths.
* Two adapters are ONE fp32 sum rounded once (the joint form; not fold, round, fold, round): held to the derived bound of the joint
  sum, and to the sequential form within that form's own three fp16 roundings.
* The adapted model IS a plain model holding the folded weights: ``forward_rows`` (fp16 and FP8), ``denoise`` and the pipeline's
  ``__call__`` equal that twin to the bit, with the launch list of a model without adapters.
* Against the fp32 oracle holding ``W + c B A``: inside the project's forward gate, with four wrong folds outside it."""
import pytest
import torch
import torch.nn as nn

import cogvideox_lora_support as ls
import cogvideox_pipeline_oracle as po
from cogvideox_support import DEV, hip_twin, loop_inputs, rel, tiny_oracle

pytestmark = pytest.mark.gpu

GATE = 1e-2                      # tests/test_cogvideox.py: the tiny DiT's forward gate
PROMPT, NEGATIVE = "a red kite over the dunes", "blurry"


@pytest.fixture(scope="module")
def cfg():
    from oracle import cogvideox as oc
    return oc.TINY_DIT


@pytest.fixture(scope="module")
def oracle():
    return tiny_oracle()


@pytest.fixture(scope="module")
def adapters(cfg):
    return {4: ls.make_adapter(cfg, 904, 4), 128: ls.make_adapter(cfg, 1028, 128), "six": ls.make_adapter(cfg, 906, 4, ls.ALL_SIX)}


def _adapted(o, loads, cfg=None, weights=None):
    """the HIP model of ``o`` with the adapter dicts of ``loads`` = [(name, dict, c)] loaded on the CPU and weighted by c, then fp16 on
    the GPU"""
    m = hip_twin(o, cfg)
    for name, sd, _ in loads:
        m.load_lora_adapter(sd, adapter_name=name)
    m.set_adapters([n for n, _, _ in loads], [c for _, _, c in loads])
    return m.half().to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------ the fold
@pytest.mark.parametrize("rank", [4, 128])
def test_fold_is_exact_where_the_result_is_an_fp16_number(cfg, oracle, rank):
    """W in 2^-6 Z, |W| <= 1/2; A, B in {-1/4, 0, 1/4}; c = 1/2: every partial sum of the fold is a multiple of 2^-6 below 2^3, exact in
    fp32 in any order, and the result is an fp16 number"""
    c = 0.5
    g = torch.Generator().manual_seed(70 + rank)
    names = ls.module_names(cfg.num_layers, ls.ALL_SIX)
    m = hip_twin(oracle)
    sd, want = {}, {}
    with torch.no_grad():
        for n in names:
            n_out, n_in = ls.linear_shape(cfg, n)
            w = torch.randint(-32, 33, (n_out, n_in), generator=g).float() / 64
            a = torch.randint(-1, 2, (rank, n_in), generator=g).float() / 4
            b = torch.randint(-1, 2, (n_out, rank), generator=g).float() / 4
            assert b.abs().max() > 0 and a.abs().max() > 0
            m.get_submodule(n).weight.copy_(w)
            sd[f"{n}.lora_A.weight"], sd[f"{n}.lora_B.weight"] = a, b
            v = w.double() + c * (b.double() @ a.double())
            assert torch.equal(v.half().double(), v) and not torch.equal(v, w.double())          # representable, in fp64
            want[n] = v.half()
    m.load_lora_adapter(sd, adapter_name="a")
    m.set_adapters(["a"], [c])
    m = m.half().to(DEV)
    m.prepare()
    for n in names:
        assert _same_bits(ls.packed_weight(m, n), want[n]), n


@pytest.mark.parametrize("case", ["attn_r128", "six_r4"])
def test_fold_of_the_tiny_model_is_within_the_derived_bound(cfg, oracle, adapters, case):
    sd, r, c, targets = (adapters[128], 128, 0.5, ls.ATTN) if case == "attn_r128" else (adapters["six"], 4, 0.75, ls.ALL_SIX)
    m = _adapted(oracle, [("a", sd, c)])
    m.prepare()
    base = oracle.state_dict()
    off = 0
    for n in ls.module_names(cfg.num_layers, targets):
        packed = ls.packed_weight(m, n)
        assert packed.dtype == torch.float16 and packed.is_cuda
        off += ls.assert_within_fold_bound(packed.cpu(), base[n + ".weight"], sd[f"{n}.lora_A.weight"], sd[f"{n}.lora_B.weight"], c, r)
        assert not torch.equal(packed.cpu(), base[n + ".weight"].half())
    print(f"\n{case}: {off} packed elements are not the fp16 rounding of the exact fold (all inside the bound)")


@pytest.mark.parametrize("width, rank", [(3072, 256), (1920, 128)])
def test_fold_at_the_real_widths_is_within_the_derived_bound(width, rank):
    """one linear of the 5B (3072) and of the 2B (1920) width through the pack's own statement, fp16 and FP8"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import fp8, lora
    c = 0.75
    g = torch.Generator().manual_seed(width + rank)
    w = (0.03 * torch.randn(width, width, generator=g)).half()
    a = (torch.randn(rank, width, generator=g) / width ** 0.5).half()
    b = (0.05 * torch.randn(width, rank, generator=g)).half()
    lin = lora.Linear(nn.Linear(width, width), "a", rank, rank, init_lora_weights=False).half()
    with torch.no_grad():
        lin.base_layer.weight.copy_(w)
        lin.lora_A["a"].weight.copy_(a)
        lin.lora_B["a"].weight.copy_(b)
    lin.scaling["a"] = c * lin.lora_alpha["a"] / lin.r["a"]
    lin = lin.to(DEV)
    packed, bias = pc.pack_block_linear(lin)
    assert tuple(packed.shape) == (width, width) and packed.dtype == torch.float16 and bias.dtype == torch.float32
    off = ls.assert_within_fold_bound(packed, w.to(DEV), a.to(DEV), b.to(DEV), c, rank)
    print(f"\n{width} x {width}, r {rank}: {off} of {packed.numel()} elements are not the fp16 rounding of the exact fold")
    assert not torch.equal(packed, w.to(DEV))
    q, scale, _ = pc.pack_block_linear(lin, fp8=True)                        # fold, then quantise: the folded fp16 values' quantisation
    q2, scale2 = fp8.quantize_weight(packed)
    assert torch.equal(q, q2) and torch.equal(scale, scale2)


def _rd16(x):
    """the error bound of one rounding of x to fp16 (normal or subnormal)"""
    return 2.0 ** -11 * x.abs() + 2.0 ** -25


def test_two_adapters_fold_as_one_sum_rounded_once(cfg, oracle, adapters):
    """the chosen form is JOINT: fp32 (W + c1 B1 A1) + c2 B2 A2, rounded once.  (a) it is inside the bound of that sum: the terms of
    adapter 1 and W pass at most r1 + 3 fp32 roundings, those of adapter 2 at most r2 + 2.  (b) against the SEQUENTIAL form
    (fold 1, round to fp16, take that as the base, fold 2, round), computed by fuse + unload + load: the two agree within the single
    bound applied twice (d1 on the first fold, d2 on the second) plus the fp16 roundings the forms do not share - the sequential
    form's intermediate one and the two final ones"""
    (r1, c1), (r2, c2) = (4, 0.5), (128, 0.75)
    s1, s2 = adapters[r1], adapters[r2]
    joint = _adapted(oracle, [("a", s1, c1), ("b", s2, c2)])
    joint.prepare()
    assert joint.active_adapters() == ["a", "b"]
    seq = _adapted(oracle, [("a", s1, c1)])
    seq.fuse_lora()
    seq.unload_lora()
    seq.load_lora_adapter(s2, adapter_name="b")
    seq.set_adapters(["b"], [c2])
    seq.prepare()
    base = oracle.state_dict()
    differ = 0
    for n in ls.module_names(cfg.num_layers, ls.ATTN):
        w = base[n + ".weight"]
        v1, m1 = ls.fold_terms(w, s1[f"{n}.lora_A.weight"], s1[f"{n}.lora_B.weight"], c1)
        d2, m2 = ls.fold_terms(torch.zeros_like(w), s2[f"{n}.lora_A.weight"], s2[f"{n}.lora_B.weight"], c2)
        pj, ps = ls.packed_weight(joint, n).cpu().double(), ls.packed_weight(seq, n).cpu().double()
        # (a)
        v, big = v1 + d2, ls.gamma(r1 + 3) * m1 + ls.gamma(r2 + 2) * m2
        assert bool(((pj >= ls.h(v - big)) & (pj <= ls.h(v + big))).all()), n
        # (b)
        p1 = seq.get_submodule(n).base_layer.weight.detach().cpu().double()           # h(first fold): the sequential form's base
        delta1 = ls.gamma(r1 + 2) * m1
        assert bool(((p1 >= ls.h(v1 - delta1)) & (p1 <= ls.h(v1 + delta1))).all()), n
        delta2 = ls.gamma(r2 + 2) * (p1.abs() + m2)
        assert bool(((ps >= ls.h(p1 + d2 - delta2)) & (ps <= ls.h(p1 + d2 + delta2))).all()), n
        tol = big + delta1 + _rd16(v1.abs() + delta1) + delta2 + _rd16(v.abs() + big) + _rd16((p1 + d2).abs() + delta2)
        assert bool(((pj - ps).abs() <= tol).all()), (n, float(((pj - ps).abs() - tol).max()))
        differ += int((pj != ps).sum())
    print(f"\njoint vs sequential two-adapter fold: {differ} elements differ (each within the derived tolerance)")


# -------------------------------------------------------------------------------------------------- the model is its twin
@pytest.fixture(scope="module")
def pair(cfg, oracle, adapters):
    """name -> (adapted model, its plain twin), both packed in the fp16 mode"""
    out = {}
    for name, loads in (("attn", [("a", adapters[128], 0.5)]), ("six", [("a", adapters["six"], 0.75)])):
        m = _adapted(oracle, loads)
        m.prepare()
        out[name] = (m, ls.twin_of(m, cfg))
    return out


@pytest.mark.parametrize("which", ["attn", "six"])
def test_forward_rows_equals_the_twin_bitwise_fp16_and_fp8(cfg, oracle, pair, which):
    from lkgd_amd import fp8
    m, twin = pair[which]
    plain = hip_twin(oracle, dev=DEV)
    got, want, stock = ls.rows_call(m, cfg)(), ls.rows_call(twin, cfg)(), ls.rows_call(plain, cfg)()
    assert _same_bits(got, want) and not torch.equal(got, stock) and torch.isfinite(got.float()).all()
    try:
        fp8.quantize_to_float8(m)
        fp8.quantize_to_float8(twin)
        got8, want8 = ls.rows_call(m, cfg)(), ls.rows_call(twin, cfg)()
        assert m._pk.fp8 and twin._pk.fp8
        assert _same_bits(got8, want8) and not torch.equal(got8, got) and torch.isfinite(got8.float()).all()
    finally:
        fp8.dequantize(m)
        fp8.dequantize(twin)
        m.prepare()
        twin.prepare()


@pytest.mark.parametrize("rank, c", [(4, 0.5), (128, 0.5), (128, 1.0)])
def test_forward_against_the_oracle_and_four_wrong_folds(cfg, oracle, adapters, rank, c):
    sd = adapters[rank]
    ref = ls.oracle_forward(ls.folded_oracle(oracle, [(sd, c)]), cfg)
    r = rel(ls.hip_forward(_adapted(oracle, [("a", sd, c)]), cfg), ref)
    decoys = {"base weights (c = 0)": hip_twin(oracle, dev=DEV),
              "c doubled": _adapted(oracle, [("a", sd, 2 * c)]),
              "q and k adapters swapped": _adapted(oracle, [("a", ls.swapped_qk(sd), c)]),
              "A and B of different layers": _adapted(oracle, [("a", ls.crossed_layers(sd), c)])}
    miss = {k: rel(ls.hip_forward(m, cfg), ref) for k, m in decoys.items()}
    print(f"\nrank {rank}, c {c}: adapted HIP forward vs the fp32 oracle with W + c B A: rel L2 {r:.3e}; decoys "
          + ", ".join(f"{k} {v:.3f}" for k, v in miss.items()))
    assert r < GATE
    for k, v in miss.items():
        assert v > GATE, (k, v)


def _recorded(run):
    """one eager warm-up, then a recorded call: the entry-point names, in order"""
    from lkgd_amd import replay
    run()
    torch.cuda.synchronize()
    with replay.strict(False):
        with replay.record() as p:
            run()
    torch.cuda.synchronize()
    names = [name for _, _, name, _ in p.calls]
    p.release()
    return names


def test_launch_list_is_the_one_without_adapters(cfg, oracle, pair):
    from lkgd_amd import lora
    want = _recorded(ls.rows_call(hip_twin(oracle, dev=DEV), cfg))
    # time embedding 2 + modulation 1, text and video embedding per batch entry, six linears per block, the head per batch entry
    assert want.count("lkgd_gemm_f16") == 3 + 2 * 2 + 6 * cfg.num_layers + 2 and "lkgd_gemm_fp8" not in want
    for which, wrapped in (("attn", 4), ("six", 6)):
        m = pair[which][0]
        assert len(lora.lora_layers(m)) == wrapped * cfg.num_layers
        assert _recorded(ls.rows_call(m, cfg)) == want, which


def test_denoise_equals_the_twin_bitwise(oracle, pair):
    """2 DDIM steps under CFG"""
    from lkgd_amd import cogvideox as pc
    lat, img, pe, dom, flow = loop_inputs()

    def run(model):
        return pc.denoise(model, pc.CogVideoXDDIMScheduler(), lat.half().to(DEV), img.to(DEV), pe.to(DEV), dom.to(DEV), flow.to(DEV), 2, 6.0,
                          False)
    m, twin = pair["attn"]
    got = run(m)
    assert _same_bits(got, run(twin)) and torch.isfinite(got.float()).all()
    assert not torch.equal(got, run(hip_twin(oracle, dev=DEV)))


# ------------------------------------------------------------------------------------------------------------- the pipeline
@pytest.fixture(scope="module")
def parts():
    pytest.importorskip("transformers")
    return po.build()


def _pipe_cfg():
    from oracle import cogvideox as oc
    return oc.DiTConfig(**{**oc.TINY_DIT.__dict__, "sample_height": 6, "sample_width": 10})


def _pipe_with(parts, dit):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd.pipeline_cogvideox import CogVideoXImageToVideoPipeline
    return CogVideoXImageToVideoPipeline(parts.tok, parts.te, parts.vae, dit, pc.CogVideoXDDIMScheduler(), parts.dom, parts.flow)


def _call(pipe, output_type="pt"):
    out = pipe(po.pil_image(), PROMPT, NEGATIVE, height=po.H, width=po.W, num_frames=9, num_inference_steps=2, guidance_scale=6.0,
               generator=torch.Generator().manual_seed(5), output_type=output_type, max_sequence_length=po.SEQ)
    return out.frames


def test_pipeline_fused_on_the_cpu_then_moved_equals_the_twin_then_the_stock_pipeline(parts, adapters):
    cfg, o = _pipe_cfg(), parts.dits["sincos"][0]
    pipe = _pipe_with(parts, hip_twin(o, cfg).half())                       # the DiT is still on the CPU
    assert pipe.transformer.device.type == "cpu"
    pipe.load_lora_weights(ls.with_prefix(adapters[128]), adapter_name="test_1")
    pipe.fuse_lora(components=["transformer"], lora_scale=0.5)
    pipe.to("cuda")
    got = _call(pipe)
    assert got.is_cuda and tuple(got.shape) == (1, 9, 3, po.H, po.W) and torch.isfinite(got.float()).all()
    assert pipe.transformer.lora_coefficients()["transformer_blocks.0.attn1.to_q"] == {"test_1": 0.5}
    twin = ls.twin_of(pipe.transformer, cfg)
    assert _same_bits(got, _call(_pipe_with(parts, twin)))
    stock = _call(parts.pipe("sincos", "ddim"))
    assert not torch.equal(got, stock)
    pipe.unfuse_lora(components=["transformer"])
    pipe.unload_lora_weights()
    assert pipe.transformer._pk is None
    assert _same_bits(_call(pipe), stock)


def test_set_adapters_between_two_calls(parts, adapters):
    cfg, o = _pipe_cfg(), parts.dits["sincos"][0]
    pipe = _pipe_with(parts, hip_twin(o, cfg).half())
    pipe.load_lora_weights(adapters[4], adapter_name="kite")
    pipe.to("cuda")
    pipe.set_adapters(["kite"], [0.5])
    first = _call(pipe, "latent")
    pipe.set_adapters(["kite"], [1.0])
    second = _call(pipe, "latent")
    assert not torch.equal(first, second)
    fresh = _adapted(o, [("other", adapters[4], 1.0)], cfg)
    fresh.prepare()
    assert _same_bits(second, _call(_pipe_with(parts, ls.twin_of(fresh, cfg)), "latent"))
    pipe.set_adapters(["kite"], [0.5])
    assert _same_bits(first, _call(pipe, "latent"))
