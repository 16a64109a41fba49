"""Host side of the FP8 mode without a GPU: the four entry points refuse bad arguments with the documented codes before any launch;
``quantize_weight`` against the independent restatement of tests/fp8_oracle.py; ``quantize_to_float8`` / ``dequantize`` state, the
refusals and LKGD_DIT_FP8; the fake-quant twin against its fp32 original at ``TINY_DIT`` (the distance ``e_q`` the GPU rule is built
on)."""
import pytest
import torch

import fp8_oracle as fo
from c_interface import ALIGN, NULL, SHAPE, Host, entry
from cogvideox_support import dit_inputs as _inputs, tiny_cpu_model as _tiny_cpu_model, \
    tiny_oracle as _oracle

DIT_SEED = 191                                                      # make_goldens.py


def test_fp8_entry_points_refuse_before_launching():
    h = Host()
    quants = {fn: entry(fn, x=h.p, ldx=128, q=h.p, ldq=128, scale=h.p, T=3, K=128) for fn in ("lkgd_quant_rows_fp8", "lkgd_gelu_tanh_quant_fp8")}
    lnq = entry("lkgd_layernorm_quant_fp8", x=h.p, ldx=128, T=3, C=128, gamma=h.p, beta=h.p, eps=1e-5, q=h.p, ldq=128, scale=h.p)
    gemm = entry("lkgd_gemm_fp8", a=h.p, lda=128, a_scale=h.p, w=h.p, ldw=128, w_scale=h.p, bias=h.p, out=h.p, ldc=128, M=5, N=128, K=128)
    for fn, quant in quants.items():
        for k in ("x", "q", "scale"):
            assert quant(**{k: None}) == NULL, (fn, k)
        for kw in (dict(T=0), dict(K=0), dict(K=100), dict(K=12296, ldx=12296, ldq=12304), dict(ldx=120), dict(ldq=112)):
            assert quant(**kw) == SHAPE, (fn, kw)
        for kw in (dict(x=h.p + 2), dict(q=h.p + 8), dict(ldx=132), dict(ldq=136)):
            assert quant(**kw) == ALIGN, (fn, kw)
    for k in ("x", "q", "scale"):
        assert lnq(**{k: None}) == NULL, k
    assert lnq(gamma=None) == NULL and lnq(beta=None) == NULL            # both or neither
    for kw in (dict(T=0), dict(C=0), dict(C=100), dict(C=3080, ldx=3080, ldq=3088), dict(ldx=120), dict(ldq=112)):
        assert lnq(**kw) == SHAPE, kw
    for kw in (dict(x=h.p + 2), dict(q=h.p + 8), dict(ldx=132), dict(ldq=136), dict(gamma=h.p + 4)):
        assert lnq(**kw) == ALIGN, kw
    for k in ("a", "a_scale", "w", "w_scale", "out"):
        assert gemm(**{k: None}) == NULL, k
    for kw in (dict(M=0), dict(N=0), dict(K=0), dict(N=64), dict(N=192, ldc=192), dict(K=64), dict(K=192, lda=192, ldw=192),
               dict(lda=112), dict(ldw=112), dict(ldc=120)):
        assert gemm(**kw) == SHAPE, kw
    for kw in (dict(a=h.p + 8), dict(w=h.p + 8), dict(out=h.p + 8), dict(w_scale=h.p + 4), dict(bias=h.p + 4), dict(lda=136),
               dict(ldw=136), dict(ldc=132)):
        assert gemm(**kw) == ALIGN, kw
    assert gemm(a=None, N=64) == NULL                                     # NULL comes first


# ------------------------------------------------------------------------------------------------------------ quantisation
def test_the_restated_rounding_is_torchs_cast_after_the_clamp():
    """the helper's table search == torch's host cast (round to nearest even: 17 -> 16, 19 -> 20) on every value of the table, every
    midpoint and its two fp32 neighbours, and random values; 465 is NaN for torch WITHOUT the clamp - hence the explicit clamp"""
    assert fo.decode(fo.torch_cast(torch.tensor([17.0, 19.0]))).tolist() == [16.0, 20.0]
    assert torch.tensor([465.0]).to(torch.float8_e4m3fn).view(torch.uint8).item() & 0x7F == 0x7F
    t = fo.TABLE.float()
    mid = ((fo.TABLE[1:] + fo.TABLE[:-1]) / 2).float()
    g = torch.Generator().manual_seed(3)
    v = torch.cat([t, mid, torch.nextafter(mid, torch.tensor(1e9)), torch.nextafter(mid, torch.tensor(-1e9)),
                   448 * (2 * torch.rand(20000, generator=g) - 1), 0.03 * (2 * torch.rand(20000, generator=g) - 1)])
    v = torch.cat([v, -v])
    assert torch.equal(fo.rne_e4m3(v), fo.torch_cast(v))
    assert torch.equal(fo.decode(torch.arange(127, dtype=torch.uint8)), torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).float())


@pytest.mark.parametrize("K", [128, 520, 1920])
def test_quantize_weight_is_the_statement(K):
    """decoded values and scales equal the restatement's on random rows, a zero row, rows with one +-65504, a row of fp16 subnormals;
    every non-zero row reaches |q| = 448; no NaN byte anywhere"""
    from lkgd_amd import fp8
    w = fo.special_rows(K)
    q, s = fp8.quantize_weight(w)
    rq, rs = fo.q_rows(w)
    assert q.dtype == torch.uint8 and s.dtype == torch.float32 and q.shape == w.shape and s.shape == (w.shape[0],)
    assert q.is_contiguous() and s.is_contiguous()
    assert torch.equal(s, rs)
    assert torch.equal(fo.decode(q), fo.decode(rq))                    # -0 == 0
    assert not bool(((q & 0x7F) == 0x7F).any())
    top = fo.decode(q).abs().amax(dim=1)
    zero = w.float().abs().amax(dim=1) == 0
    assert zero.tolist() == [False, False, False, True, False, False, False, False]
    assert torch.equal(top[~zero], torch.full_like(top[~zero], 448.0)) and top[zero].item() == 0.0 and s[zero].item() == 1.0
    # fp32 weights quantise as their fp16 values: what the fp16 path multiplies with
    w32 = w.float() * (1 + 2.0 ** -14)
    finite = torch.isfinite(w32.half().float()).all(dim=1)
    q32, s32 = fp8.quantize_weight(w32[finite])
    rq32, rs32 = fo.q_rows(w32[finite].half())
    assert torch.equal(s32, rs32) and torch.equal(fo.decode(q32), fo.decode(rq32))
    # the error of a row is at most half a step of its largest binade: 2^-4 relative to amax
    err = (fo.decode(q) * s[:, None] - w.float()).abs().amax(dim=1)
    assert bool((err <= w.float().abs().amax(dim=1) * 2.0 ** -4).all())


# ------------------------------------------------------------------------------------------------------- the mode's state
def test_quantize_to_float8_state_and_refusals(monkeypatch):
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import fp8
    from lkgd_amd._lib import LkgdHipError
    monkeypatch.delenv("LKGD_DIT_FP8", raising=False)
    m = _tiny_cpu_model()
    assert m.quantization is None and not fp8.active(m)
    m._pk = object()                                                   # a stand-in for a packed model
    assert fp8.quantize_to_float8(m) is m and m.quantization == "fp8" and m._pk is None and fp8.active(m)
    m._pk = object()
    assert fp8.dequantize(m) is m and m.quantization is None and m._pk is None and not fp8.active(m)
    assert fp8.quantize(m, "fp8") is m and m.quantization == "fp8"
    fp8.dequantize(m)
    for scheme in ("int8", "fp4", ""):
        with pytest.raises(LkgdHipError, match=repr(scheme)):
            fp8.quantize(m, scheme)
        assert m.quantization is None
    with pytest.raises(LkgdHipError, match="CogVideoXTransformer3DModel"):
        fp8.quantize_to_float8(torch.nn.Linear(4, 4))
    odd = _tiny_cpu_model(num_attention_heads=3)                       # D = 192: a multiple of 64, not of 128
    with pytest.raises(LkgdHipError, match="192"):
        fp8.quantize_to_float8(odd)
    assert odd.quantization is None
    # the environment switch is read when a model packs, not at import
    monkeypatch.setenv("LKGD_DIT_FP8", "1")
    assert fp8.env_on() and fp8.active(m) and m.quantization is None
    monkeypatch.setenv("LKGD_DIT_FP8", "0")
    assert not fp8.active(m)
    # prepare() refuses a width the GEMM cannot tile, before it asks for a GPU
    monkeypatch.setenv("LKGD_DIT_FP8", "1")
    with pytest.raises(LkgdHipError, match="192"):
        odd.prepare()
    monkeypatch.setenv("LKGD_DIT_FP8", "0")
    with pytest.raises(LkgdHipError, match="cuda"):
        odd.prepare()


def test_block_pack_in_the_fp8_mode_makes_no_fp16_copies():
    """the six linears pack as (bytes, scale, bias) - the statement on the weight's rows - and nothing else of the block changes"""
    from lkgd_amd import fp8
    m = _tiny_cpu_model()
    blk = m.transformer_blocks[0]
    blk.pack(fp8=True)
    pk = blk._pk
    for name, lin in (("q", blk.attn1.to_q), ("k", blk.attn1.to_k), ("v", blk.attn1.to_v), ("o", blk.attn1.to_out[0]),
                      ("f1", blk.ff.net[0].proj), ("f2", blk.ff.net[2])):
        q, s, b = getattr(pk, name)
        rq, rs = fp8.quantize_weight(lin.weight)
        assert q.dtype == torch.uint8 and tuple(q.shape) == tuple(lin.weight.shape) and torch.equal(q, rq) and torch.equal(s, rs)
        assert b.dtype == torch.float32 and torch.equal(b, lin.bias.detach().float())
    assert pk.nq[0].dtype == torch.float32 and pk.nq[0].shape == (64,)
    blk.pack()
    assert len(blk._pk.q) == 2 and blk._pk.q[0].dtype == torch.float16


def test_sharding_together_with_the_mode_raises(monkeypatch):
    """``shard=`` and the mode: refused before anything is packed or launched, by either switch; without the mode the call goes on
    (to the next refusal a CPU model meets)"""
    from lkgd_amd import fp8
    from lkgd_amd._lib import LkgdHipError
    monkeypatch.delenv("LKGD_DIT_FP8", raising=False)
    m = _tiny_cpu_model()
    args = (torch.zeros(72, 128, dtype=torch.float16), (3, 4, 6), torch.zeros(1, 16, 4096, dtype=torch.float16), 721.0)
    with pytest.raises(LkgdHipError, match="cuda"):
        m.forward_rows(*args, shard=object())
    fp8.quantize_to_float8(m)
    with pytest.raises(LkgdHipError, match="sharding together with the FP8 mode"):
        m.forward_rows(*args, shard=object())
    fp8.dequantize(m)
    monkeypatch.setenv("LKGD_DIT_FP8", "1")
    with pytest.raises(LkgdHipError, match="sharding together with the FP8 mode"):
        m.forward_rows(*args, shard=object())


# ------------------------------------------------------------------------------------------------------- the twin and e_q
@pytest.mark.parametrize("seed", [191, 7, 23])
def test_twin_is_a_measurable_distance_from_its_original(seed):
    """e_q = d(twin, fp32 original) on the weights of seed and the inputs of seed + 1: at least 5e-3, so the GPU rule
    d(FP8 forward, twin) <= d(fp16 forward, fp32) + e_q / 2 can tell an FP8 forward from an fp16 one (which sits e_q away).
    Measured when written: 1.35e-2, 1.30e-2, 9.5e-3."""
    from oracle import cogvideox as oc
    o = _oracle(seed)
    t = fo.twin(o)
    for blk in t.transformer_blocks:
        assert sum(isinstance(x, fo.FakeQuantLinear) for x in blk.modules()) == 6
    assert not any(isinstance(x, fo.FakeQuantLinear) for x in o.modules())         # the original is left as it is
    i = _inputs(oc.TINY_DIT, seed + 1)
    with torch.no_grad():
        ref = o(i["hidden"], i["text"], i["t"], i["domain"], i["flow"])[0]
        got = t(i["hidden"], i["text"], i["t"], i["domain"], i["flow"])[0]
    e_q = fo.rel(got, ref)
    print(f"\nseed {seed}: e_q = d(twin, fp32 oracle) = {e_q:.3e}")
    assert 5e-3 <= e_q <= 5e-2


def test_fake_quant_linear_is_close_to_the_linear():
    g = torch.Generator().manual_seed(11)
    x, w, b = torch.randn(40, 256, generator=g).half(), (0.05 * torch.randn(128, 256, generator=g)).half(), torch.randn(128, generator=g)
    ref = x.float() @ w.float().t() + b
    assert fo.rel(fo.fake_quant_linear(x, w, b), ref) < 5e-2
