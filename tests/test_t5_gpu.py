"""The T5 text encoder on the GPU (include/lkgd_hip_t5.h, lkgd_amd/t5.py): the five kernels against their fp32 torch statements, the
forward against transformers' own fp32 forward of the same fp16-rounded weights (two tiny configurations, S in {7, 226}), three decoy
forwards it has to miss, the fp16 range of the closing projections, the launch list, the footprint cases (tests/footprint.py) and
``encode_prompt`` into ``denoise``.  transformers [EXT] is the checker, never on the product path.

The real ``text_encoder/`` weights are not available to these tests: parity with them is unmeasured."""
import functools
import math

import pytest
import torch

transformers = pytest.importorskip("transformers")

from footprint import run_case
from t5_support import BIAS_STD, DEV, GATE, TINY, TINY_A, StubTokenizer, expand_bias_table, hf_model, hip_twin, ids_for, rel

gpu = pytest.mark.gpu

#: every name in lkgd_amd._lib.T5_SYMBOLS -> its footprint tests in this module
FOOTPRINT = {
    "lkgd_t5_embed_rows": ["test_embed_rows_footprint"],
    "lkgd_t5_rmsnorm": ["test_rmsnorm_footprint"],
    "lkgd_attn_dense_relbias": ["test_attn_dense_relbias_footprint"],
    "lkgd_t5_gated_gelu": ["test_gated_gelu_footprint"],
    "lkgd_t5_residual_add": ["test_residual_add_footprint"],
}
ATTN_SHAPES = [(1, 7, 2, 16), (2, 226, 4, 64), (1, 129, 3, 40)]          # (nbatch, S, heads, head_dim)
HALF_ULP = 2.0 ** -11


# ------------------------------------------------------------------------------------------------------- the fp32 statements
def rmsnorm_ref(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def gated_gelu_ref(h):
    F_ = h.shape[1] // 2
    a, b = h[:, :F_].float(), h[:, F_:].float()
    return 0.5 * a * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (a + 0.044715 * a.pow(3)))) * b      # transformers' gelu_new


def attn_ref(q, k, v, table, nb, S, heads, hd, scale):
    """fp32 softmax(scale q k^T + table[h, j - i + S - 1]) v on [nb * S, heads * hd] rows"""
    q, k, v = (t.float().reshape(nb, S, heads, hd).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(scale * (q @ k.transpose(-1, -2)) + expand_bias_table(table.float(), S), dim=-1)
    return (p @ v).transpose(1, 2).reshape(nb * S, heads * hd)


def _close_fp16(got, ref, what, extra=0.0):
    """one rounding to fp16 of an fp32 value that itself differs from the reference's by fp32 rounding and summation order (a few
    2^-24 relative: far below half an fp16 step, but enough to move a value across a rounding boundary): at most one fp16 step,
    2 * HALF_ULP relative, with the subnormal step 2^-24 as the floor; ``extra``: an absolute allowance the caller derives"""
    got, ref = got.float().cpu(), ref.float().cpu()
    bound = 2 * HALF_ULP * ref.abs() + 2.0 ** -24 + extra
    bad = (got - ref).abs() > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float(((got - ref).abs() - bound).max()))


# ----------------------------------------------------------------------------------------------------------------- kernels
@gpu
def test_embed_rows_is_exact():
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(1)
    table = torch.randn(128, 64, generator=g).half()
    ids = torch.randint(0, 128, (227,), generator=g)
    ids[:3] = torch.tensor([0, 127, 127])
    out = ops.t5_embed_rows(ids.to(DEV), table.to(DEV))
    assert out.dtype == torch.float32 and torch.equal(out.cpu(), table.float()[ids])
    # an id outside the table is the caller's error; the kernel clamps it, so the launch stays inside the table
    wild = torch.tensor([-5, 128, 1 << 40], dtype=torch.int64)
    assert torch.equal(ops.t5_embed_rows(wild.to(DEV), table.to(DEV)).cpu(), table.float()[[0, 127, 127]])


@gpu
@pytest.mark.parametrize("T", [1, 227])
@pytest.mark.parametrize("C", [64, 4096])
def test_rmsnorm_is_the_statement(T, C):
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(T + C)
    x = torch.randn(T, C, generator=g) * (0.05 + 20 * torch.rand(T, 1, generator=g))
    x[0] *= 3e4                                          # a row whose squares an fp16 sum could not hold
    w = 0.7 + 0.6 * torch.rand(C, generator=g)
    got = ops.t5_rmsnorm(x.to(DEV), w.to(DEV), 1e-6)
    assert got.dtype == torch.float16 and got.shape == (T, C)
    _close_fp16(got, rmsnorm_ref(x, w, 1e-6), (T, C))


@gpu
@pytest.mark.parametrize("F_", [8, 160])
def test_gated_gelu_is_the_statement(F_):
    """|gate| <= 8.  The kernel's tanh is 1 - 2 / (exp2(c u) + 1): 1 + tanh carries an absolute error of about two fp32 steps at 2
    (2.4e-7), which the statement's 0.5 |gate| |linear| turns into at most 1e-6 |linear| - the allowance on top of the fp16 step"""
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(F_)
    T = 67
    h = torch.cat([(2.5 * torch.randn(T, F_, generator=g)).clamp(-8, 8), 2 * torch.randn(T, F_, generator=g)], dim=1).half()
    h[0, :8] = torch.tensor([0.0, -0.0, 8.0, -8.0, 1e-4, -1e-4, 3.0, -3.0]).half()
    got = ops.t5_gated_gelu(h.to(DEV))
    assert got.dtype == torch.float16 and got.shape == (T, F_)
    _close_fp16(got, gated_gelu_ref(h), F_, extra=1e-6 * h[:, F_:].float().abs())


@gpu
@pytest.mark.parametrize("s", [1.0, 64.0, 0.125])
def test_residual_add_is_exact_for_powers_of_two(s):
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(9)
    x = torch.randn(227, 64, generator=g) * 100
    y = (torch.randn(227, 64, generator=g) * 30).half()
    xd = x.to(DEV)
    assert ops.t5_residual_add_(xd, y.to(DEV), s) is xd
    assert torch.equal(xd.cpu(), x + s * y.float())


def _attn_case(nb, S, heads, hd, seed=0):
    g = torch.Generator().manual_seed(seed + S)
    w = heads * hd
    qkv = torch.randn(nb * S, 3 * w, generator=g).half()
    table = BIAS_STD * torch.randn(heads, 2 * S - 1, generator=g)
    return qkv, table


@gpu
@pytest.mark.parametrize("nb,S,heads,hd", ATTN_SHAPES)
def test_attn_dense_relbias_matches_fp32_softmax(nb, S, heads, hd):
    """test_attn_dense_matches_sdpa's operands, scale and bound (2e-3), with a table of standard deviation 2 on top; then an all-zero
    table: the bits of lkgd_attn_dense.  (T5's scale = 1 is pinned by the forward tests: the decoy with scaled scores.)"""
    from lkgd_amd import ops
    w = heads * hd
    qkv, table = _attn_case(nb, S, heads, hd)
    d = qkv.to(DEV)
    q, k, v = d[:, :w], d[:, w:2 * w], d[:, 2 * w:]
    out = torch.empty(nb * S, w, device=DEV, dtype=torch.float16)
    ops.attn_dense_relbias(q, k, v, out, nb, S, heads, hd, table.to(DEV))
    want = attn_ref(qkv[:, :w], qkv[:, w:2 * w], qkv[:, 2 * w:], table, nb, S, heads, hd, hd ** -0.5)
    err = float((out.float().cpu() - want).abs().max())
    print(f"\nattn_dense_relbias {(nb, S, heads, hd)}: max err {err:.3e}")
    assert err < 2e-3, err
    # the table is read as [h, j - i + S - 1]: the flipped table (i - j) is a different function
    if S > 1:
        flipped = attn_ref(qkv[:, :w], qkv[:, w:2 * w], qkv[:, 2 * w:], table.flip(1), nb, S, heads, hd, hd ** -0.5)
        assert float((flipped - want).abs().max()) > 0.1
    plain, zero = torch.empty_like(out), torch.empty_like(out)
    ops.attn_dense(q, k, v, plain, nb, S, heads, hd)
    ops.attn_dense_relbias(q, k, v, zero, nb, S, heads, hd, torch.zeros(heads, 2 * S - 1, device=DEV))
    assert torch.equal(zero, plain)


# ------------------------------------------------------------------------------------------------------------- the forward
@functools.lru_cache(maxsize=None)
def _pair(name):
    """(transformers fp32 model, HIP twin on the GPU) of a tiny configuration; neither is modified by a test"""
    ref = hf_model(TINY[name])
    return ref, hip_twin(ref, TINY[name], DEV)


@functools.lru_cache(maxsize=None)
def _reference(name, S):
    ids = ids_for(TINY[name], 2, S)
    with torch.no_grad():
        return ids, _pair(name)[0](input_ids=ids)[0]


@gpu
@pytest.mark.parametrize("S", [7, 226])
@pytest.mark.parametrize("name", ["a", "b"])
def test_forward_matches_transformers_fp32(name, S):
    ids, want = _reference(name, S)
    m = _pair(name)[1]
    out = m(ids.to(DEV))
    got = out[0]
    assert out.last_hidden_state is got and got.dtype == torch.float16 and tuple(got.shape) == (2, S, TINY[name]["d_model"])
    assert bool(torch.isfinite(got.float()).all())
    r = rel(got, want)
    print(f"\nT5 tiny {name} S = {S}: rel L2 vs transformers fp32 {r:.3e}")
    assert r < GATE, r
    assert torch.equal(m(ids)[0], got)                   # ids from the host (a tokenizer's output) or the device: the same bits


def _decoys(ref, cfg):
    """the same transformers model with (a) the bias table zeroed, (b) the table indexed by i - j, (c) scores scaled by 1/sqrt(d_kv)"""
    import copy
    a = copy.deepcopy(ref)
    b = copy.deepcopy(ref)
    c = copy.deepcopy(ref)
    with torch.no_grad():
        a.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight.zero_()
        for blk in c.encoder.block:
            blk.layer[0].SelfAttention.q.weight.mul_(cfg["d_kv"] ** -0.5)
    att = b.encoder.block[0].layer[0].SelfAttention
    true_bias = att.compute_bias
    att.compute_bias = lambda *args, **kw: true_bias(*args, **kw).transpose(-1, -2).contiguous()
    return {"zero table": a, "table by i - j": b, "scores / sqrt(d_kv)": c}


@gpu
@pytest.mark.parametrize("S", [7, 226])
def test_forward_misses_the_decoys(S):
    """each decoy is at least five gates from the true fp32 output (asserted here, on the CPU); the HIP output within one gate of the
    true one is then, by the triangle inequality, at least four gates from every decoy"""
    ids, want = _reference("a", S)
    ref, m = _pair("a")
    for what, decoy in _decoys(ref, TINY_A).items():
        with torch.no_grad():
            far = rel(decoy(input_ids=ids)[0], want)
        print(f"\ndecoy '{what}' at S = {S}: {far:.3e} from the true output")
        assert far >= 5 * GATE, (what, far)
    assert rel(m(ids.to(DEV))[0], want) < GATE


@gpu
def test_closing_projection_survives_a_feed_forward_output_beyond_fp16():
    """the last layer's ``wo`` scaled until transformers' fp32 feed-forward output there peaks between 1e5 and 1e6 (fp16 ends at
    65504): the HIP forward is finite and within the gate - its closing GEMMs store acc * 2^-6 and the residual add multiplies by
    2^6.  Without the pair the GEMM's fp16 output is inf"""
    import copy
    ref = copy.deepcopy(_pair("a")[0])
    ids = ids_for(TINY_A, 2, 7)
    ff = ref.encoder.block[-1].layer[1].DenseReluDense
    peaks = []
    hook = ff.register_forward_hook(lambda mod, args, out: peaks.append(float(out.abs().max())))
    with torch.no_grad():
        ref(input_ids=ids)
        ff.wo.weight.mul_(2.0 ** round(math.log2(3e5 / peaks[0])))          # a power of two: the weights stay fp16 values
        assert float(ff.wo.weight.abs().max()) < 65504
        want = ref(input_ids=ids)[0]
    hook.remove()
    print(f"\nfeed-forward output peak: {peaks[0]:.3e} -> {peaks[1]:.3e}")
    assert 1e5 <= peaks[1] <= 1e6, peaks
    got = hip_twin(ref, TINY_A, DEV)(ids.to(DEV))[0]
    assert bool(torch.isfinite(got.float()).all())
    r = rel(got, want)
    print(f"rel L2 vs transformers fp32 {r:.3e}")
    assert r < GATE, r


@gpu
def test_forward_launch_list():
    """one launch for the embedding, the ten of a layer, one for the final norm - and nothing else reaches the library; a second
    call gives the same bits"""
    from lkgd_amd import replay
    ids, _ = _reference("a", 7)
    m = _pair("a")[1]
    d = ids.to(DEV)
    first = m(d)[0].clone()
    torch.cuda.synchronize()
    with replay.strict(False):                 # only the launch list is of interest here: nothing is replayed
        with replay.record() as p:
            second = m(d)[0]
    torch.cuda.synchronize()
    names = [name for _, _, name, _ in p.calls]
    p.release()
    layer = ["lkgd_t5_rmsnorm", "lkgd_gemm_f16", "lkgd_attn_dense_relbias", "lkgd_gemm_f16", "lkgd_t5_residual_add",
             "lkgd_t5_rmsnorm", "lkgd_gemm_f16", "lkgd_t5_gated_gelu", "lkgd_gemm_f16", "lkgd_t5_residual_add"]
    assert names == ["lkgd_t5_embed_rows"] + layer * TINY_A["num_layers"] + ["lkgd_t5_rmsnorm"], names
    assert torch.equal(second, first)


# --------------------------------------------------------------------------------------------------------------- footprint
def _exact(got, ref, what):
    assert torch.equal(got.cpu(), ref.cpu()), what


@gpu
@pytest.mark.parametrize("T", [1, 227])
def test_embed_rows_footprint(T):
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(T)
    table = torch.randn(128, 64, generator=g).half()
    ids = torch.randint(0, 128, (T, 1), generator=g)
    ids[0, 0], ids[-1, 0] = 127, 0                       # the table's last and first rows: the guard rows are their neighbours

    def case(W):
        iv = W.inp(ids, pad=0, name="ids", gap=False)
        tv = W.inp(table, pad=8, col0=8, name="table")
        out = W.out(T, 64, dtype=torch.float32, pad=4, col0=4, name="out")
        ops.t5_embed_rows(iv[:, 0], tv, out=out)
        return {"out": out}
    run_case(case, DEV, refs=lambda: {"out": table.float()[ids[:, 0]]}, close=_exact, sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("T,C", [(1, 4096), (227, 64), (3, 2056)])
def test_rmsnorm_footprint(T, C):
    """C = 2056: 257 eight-channel pieces, one more than the first pass of the 256 threads"""
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(T)
    x = 3 * torch.randn(T, C, generator=g)
    w = 0.7 + 0.6 * torch.rand(1, C, generator=g)

    def case(W):
        xv = W.inp(x, pad=4, col0=4, name="x")
        wv = W.inp(w, pad=0, name="weight", gap=False)
        out = W.out(T, C, pad=8, col0=8, name="out")
        ops.t5_rmsnorm(xv, wv[0], 1e-6, out=out)
        return {"out": out}
    run_case(case, DEV, refs=lambda: {"out": rmsnorm_ref(x, w[0], 1e-6)}, close=_close_fp16, sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("nb,S,heads,hd", [(2, 7, 2, 16), (1, 129, 3, 40)])
def test_attn_dense_relbias_footprint(nb, S, heads, hd):
    """q | k | v are column blocks of one window, as in the encoder; NaN rows before and after the table"""
    from lkgd_amd import ops
    w = heads * hd
    qkv, table = _attn_case(nb, S, heads, hd, seed=3)
    parts = [qkv[:, i * w:(i + 1) * w] for i in range(3)]

    def case(W):
        q, k, v = W.inp_cols(parts, name="qkv")
        tv = W.inp(table, pad=0, name="relbias", gap=False)
        out = W.out(nb * S, w, pad=8, col0=8, name="out")
        ops.attn_dense_relbias(q, k, v, out, nb, S, heads, hd, tv)
        return {"out": out}

    def close(got, ref, what):
        assert float((got.float().cpu() - ref).abs().max()) < 2e-3, what
    run_case(case, DEV, refs=lambda: {"out": attn_ref(*parts, table, nb, S, heads, hd, hd ** -0.5)}, close=close,
             sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("T,F_", [(1, 8), (67, 160)])
def test_gated_gelu_footprint(T, F_):
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(T)
    h = torch.cat([(2.5 * torch.randn(T, F_, generator=g)).clamp(-8, 8), 2 * torch.randn(T, F_, generator=g)], dim=1).half()

    def case(W):
        hv = W.inp(h, pad=8, col0=8, name="h")
        out = W.out(T, F_, pad=8, col0=8, name="out")
        ops.t5_gated_gelu(hv, out=out)
        return {"out": out}
    run_case(case, DEV, refs=lambda: {"out": gated_gelu_ref(h)},
             close=lambda got, ref, what: _close_fp16(got, ref, what, extra=1e-6 * h[:, F_:].float().abs()), sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("T", [1, 227])
def test_residual_add_footprint(T):
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, 64, generator=g) * 100
    y = (torch.randn(T, 64, generator=g) * 30).half()

    def case(W):
        xv = W.inout(x, pad=4, col0=4, name="x")
        yv = W.inp(y, pad=8, col0=8, name="y")
        ops.t5_residual_add_(xv, yv, 64.0)
        return {"x": xv}
    run_case(case, DEV, refs=lambda: {"x": x + 64.0 * y.float()}, close=_exact, sync=torch.cuda.synchronize)


# ----------------------------------------------------------------------------------------------------------- encode_prompt
@gpu
def test_encode_prompt_feeds_denoise():
    """a one-layer encoder of the DiT's text width (4096) behind a stub tokenizer: fp16 [2, 226, 4096] embeddings, equal to the
    encoder's own output on the tokenizer's ids, accepted by ``denoise`` of a tiny DiT with 226 text tokens"""
    from cogvideox_support import hip_twin as dit_twin, loop_inputs, tiny_oracle
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import t5
    from oracle import cogvideox as oc
    cfg = dict(vocab_size=128, d_model=4096, d_kv=64, d_ff=64, num_layers=1, num_heads=2)
    enc = hip_twin(hf_model(cfg, seed=7), cfg, DEV)
    assert isinstance(enc, t5.T5EncoderModel)
    tok = StubTokenizer()
    pe, ne = pc.encode_prompt(enc, tok, ["a red panda eating bamboo"], negative_prompt=None, num_videos_per_prompt=1)
    assert pe.shape == ne.shape == (1, 226, 4096) and pe.dtype == ne.dtype == torch.float16 and pe.device == ne.device == enc.device
    assert [c["prompt"] for c in tok.calls] == [["a red panda eating bamboo"], [""]]
    assert torch.equal(pe, enc(tok.__call__(["a red panda eating bamboo"], padding="max_length", max_length=226, truncation=True,
                                            add_special_tokens=True, return_tensors="pt").input_ids)[0])
    embeds = torch.cat([ne, pe])                                           # negative first, as the pipeline concatenates them
    assert embeds.shape == (2, 226, 4096) and bool(torch.isfinite(embeds.float()).all()) and not torch.equal(pe, ne)
    dcfg = oc.DiTConfig(**{**oc.TINY_DIT.__dict__, "max_text_seq_length": 226})
    m = dit_twin(tiny_oracle(cfg=dcfg), dcfg, DEV)
    lat, img, _, dom, flow = loop_inputs(dcfg)
    out = pc.denoise(m, pc.CogVideoXDDIMScheduler(), lat.half().to(DEV), img.to(DEV), embeds, dom.to(DEV), flow.to(DEV), 2, 6.0, True)
    assert out.dtype == torch.float16 and out.shape == lat.shape and bool(torch.isfinite(out.float()).all())
