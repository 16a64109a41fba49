"""The FP8 mode on the GPU (include/lkgd_hip_fp8.h): the three quantisers against the restatement of tests/fp8_oracle.py, decoded
values and scales equal; the fused forms bit for bit their two-launch spelling; ``lkgd_gemm_fp8`` bit for bit on integer data
(one-hot rows against an asymmetric weight pin the operand lane map, the scale operand and the tails), within the fp16 output
rounding on random e4m3 data; refusals and the footprint cases of the four entry points (tests/footprint.py); the linear, the DiT
forward against the fake-quant twin, ``denoise`` against the loop stepped by hand, and the mode switched off again."""
import pytest
import torch

import footprint
import fp8_oracle as fo
from cogvideox_support import DEV, dit_inputs as _inputs, hip_twin, loop_inputs as _loop_inputs, tiny_oracle as _oracle
from c_interface import ALIGN, NULL, SHAPE, entry
from footprint import run_case

gpu = pytest.mark.gpu
NAN_BYTE = 0x7F

#: every name in lkgd_amd._lib.FP8_SYMBOLS -> its footprint tests in this module
FOOTPRINT = {
    "lkgd_quant_rows_fp8": ["test_quant_rows_fp8_footprint"],
    "lkgd_gelu_tanh_quant_fp8": ["test_gelu_tanh_quant_fp8_footprint"],
    "lkgd_layernorm_quant_fp8": ["test_layernorm_quant_fp8_footprint"],
    "lkgd_gemm_fp8": ["test_gemm_fp8_footprint"],
}

GEMM_M = [1, 15, 16, 17, 127, 128, 129, 176, 300]           # below, at and above the 16-row fragment and the 128-row tile
#: special rows first, so that T = 1 is the zero row and T = 3 adds +65504 and the subnormal row (fo.special_rows' order)
ROW_ORDER = [3, 4, 6, 0, 5, 1, 2, 7]


def _rows(T, K, seed=0):
    """fp16 [T, K]: fo.special_rows in ROW_ORDER, then random rows"""
    sp = fo.special_rows(K)[ROW_ORDER]
    if T <= 8:
        return sp[:T].clone()
    g = torch.Generator().manual_seed(seed + T + K)
    return torch.cat([sp, (torch.randn(T - 8, K, generator=g) * torch.rand(T - 8, 1, generator=g) * 8).half()])


def _same_q(got_q, got_s, ref_q, ref_s, what):
    assert got_q.dtype == torch.uint8 and got_s.dtype == torch.float32
    assert not bool(((got_q & 0x7F) == NAN_BYTE).any()), what
    assert torch.equal(got_s.cpu(), ref_s), (what, (got_s.cpu() - ref_s).abs().max().item())
    d, r = fo.decode(got_q), fo.decode(ref_q)
    assert torch.equal(d, r), (what, int((d != r).sum()))              # -0 == 0


# ------------------------------------------------------------------------------------------------------------- quantisers
#: T in {1, 3, 64, 65} x K in {128, 512, 1920} (one vector per thread), then two, four and six vectors per thread at T = 3
QUANT_SHAPES = [(T, K) for K in (128, 512, 1920) for T in (1, 3, 64, 65)] + [(3, 3072), (3, 7680), (3, 12288)]


@gpu
@pytest.mark.parametrize("T,K", QUANT_SHAPES)
def test_quant_rows_fp8_is_the_statement(T, K):
    from lkgd_amd import ops
    x = _rows(T, K)
    ref_q, ref_s = fo.q_rows(x)
    q, s = ops.quant_rows_fp8(x.to(DEV))
    _same_q(q, s, ref_q, ref_s, (T, K))
    top = fo.decode(q).abs().amax(dim=1)
    zero = x.float().abs().amax(dim=1) == 0
    assert torch.equal(top[~zero], torch.full_like(top[~zero], 448.0)) and bool((top[zero] == 0).all())
    # row strides wider than the row, on both sides
    xw = torch.full((T, K + 24), float("nan"), dtype=torch.float16, device=DEV)
    xw[:, 8:8 + K] = x.to(DEV)
    qw = torch.full((T, K + 48), 0xAA, dtype=torch.uint8, device=DEV)
    q2, s2 = ops.quant_rows_fp8(xw[:, 8:8 + K], q=qw[:, 16:16 + K])
    assert torch.equal(q2, q) and torch.equal(s2, s)
    assert bool((qw[:, :16] == 0xAA).all()) and bool((qw[:, 16 + K:] == 0xAA).all())      # 0xAA is a value too: look at the gaps only


@gpu
@pytest.mark.parametrize("C", [64, 128, 320, 640, 1280, 1920, 3072])   # every (lanes per row, vectors per lane) lkgd_layernorm dispatches
def test_layernorm_quant_fp8_equals_layernorm_then_quant(C):
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(C)
    T = 37
    x = (torch.randn(T, C, generator=g) * 3 + 0.5).half().to(DEV)
    x[5] = 0.0                                                       # a constant row: every normalised value is beta
    x[6] = x[6, 0]
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV), (0.2 * torch.randn(C, generator=g)).to(DEV)
    for gm, bt in ((gamma, beta), (None, None)):
        ref_q, ref_s = ops.quant_rows_fp8(ops.layernorm(x, gm, bt, 1e-5))
        q, s = ops.layernorm_quant_fp8(x, gm, bt, 1e-5)
        assert torch.equal(s, ref_s), (C, gm is None)
        assert torch.equal(q, ref_q), (C, gm is None, int((q != ref_q).sum()))
    # and the pair is the restatement on the fp16 values the norm stores
    y = ops.layernorm(x, gamma, beta, 1e-5)
    q, s = ops.layernorm_quant_fp8(x, gamma, beta, 1e-5)
    _same_q(q, s, *fo.q_rows(y.cpu()), C)


@gpu
@pytest.mark.parametrize("K", [512, 3072, 7680, 12288])
def test_gelu_tanh_quant_fp8_equals_gelu_then_quant(K):
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(K)
    x = (torch.randn(19, K, generator=g) * 3).half()
    x[2] = 0.0
    x[3] = -20.0                                                     # gelu saturates to -0: a zero row after the activation
    x = x.to(DEV)
    x0 = x.clone()
    ref_q, ref_s = ops.quant_rows_fp8(ops.gelu_tanh_(x.clone()))
    q, s = ops.gelu_tanh_quant_fp8(x)
    assert torch.equal(x, x0)                                        # the input is left as it is
    assert torch.equal(s, ref_s) and torch.equal(q, ref_q), (K, int((q != ref_q).sum()))
    assert s[2].item() == 1.0 and s[3].item() == 1.0


# ------------------------------------------------------------------------------------------- rows beyond the grid caps
# quant_rows_kernel runs at most 8192 workgroups of one row each and uses its two LDS slots in turn from one loop iteration to the
# next; layernorm_quant_kernel runs at most 4096 workgroups of 4 rows each (one row per wave at these widths).  The smallest row
# counts at which a workgroup runs its loop body three times - both slots, and the first one a second time - plus a ragged rest:
QUANT_LOOP_ROWS = 3 * 8192 * 1 + 5             # 24 581
LN_LOOP_ROWS = 3 * 4096 * 4 + 5                # 49 157


def _scaled_rows(T, K, seed, shift=0.0):
    """fp16 [T, K]: row r is N(shift, 1) x (0.05 + r % 97), so every row has its own maximum and scale - a value or scale left
    over from another loop iteration of the same workgroup (rows r +- 8192 / 16384) cannot pass; rows 8192, 16384 and T - 1 are
    zero rows between them"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(T, K, generator=g) + shift) * (0.05 + (torch.arange(T) % 97).float())[:, None]
    x[[8192, 16384, T - 1]] = 0.0
    return x.half()


@gpu
def test_quant_rows_fp8_three_loop_iterations():
    from lkgd_amd import ops
    T, K = QUANT_LOOP_ROWS, 128
    x = _scaled_rows(T, K, 11)
    ref_q, ref_s = fo.q_rows(x)
    # the rows a workgroup sees one after the other (8192 apart) have different scales: a stale one shows
    assert (ref_s[:-8192] != ref_s[8192:]).float().mean() > 0.99 and bool((ref_s[[8192, 16384, T - 1]] == 1.0).all())
    q, s = ops.quant_rows_fp8(x.to(DEV))
    _same_q(q, s, ref_q, ref_s, "quant_rows_fp8 past the grid cap")


@gpu
def test_gelu_tanh_quant_fp8_three_loop_iterations():
    """against fo.q_rows of the fp16 values ``ops.gelu_tanh_`` stores (test_gelu_tanh_quant_fp8_footprint's reference)"""
    from lkgd_amd import ops
    T, K = QUANT_LOOP_ROWS, 128
    x = (_scaled_rows(T, K, 12).float() * 0.1).half().to(DEV)            # |x| up to about 40: both tails of the activation
    ref_q, ref_s = fo.q_rows(ops.gelu_tanh_(x.clone()).cpu())
    # the rows a workgroup sees one after the other (8192 apart) have different scales: a stale one shows
    assert (ref_s[:-8192] != ref_s[8192:]).float().mean() > 0.99 and bool((ref_s[[8192, 16384, T - 1]] == 1.0).all())
    q, s = ops.gelu_tanh_quant_fp8(x)
    _same_q(q, s, ref_q, ref_s, "gelu_tanh_quant_fp8 past the grid cap")


@pytest.fixture(scope="module", params=[1920, 3072])
def ln_loop_case(request):
    """(C, x, gamma, beta, y): LN_LOOP_ROWS rows through the four- (C = 1920) and the six-vector (3072) LayerNorm, y = what
    ``ops.layernorm`` stores; computed once, left unchanged"""
    from lkgd_amd import ops
    C = request.param
    x = _scaled_rows(LN_LOOP_ROWS, C, C, shift=0.3).to(DEV)
    g = torch.Generator().manual_seed(C + 1)
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).to(DEV), (0.2 * torch.randn(C, generator=g)).to(DEV)
    return C, x, gamma, beta, ops.layernorm(x, gamma, beta, 1e-5)


@gpu
def test_layernorm_quant_fp8_three_loop_iterations(ln_loop_case):
    """bit for bit ``quant_rows_fp8(layernorm(x))``, and ``fo.q_rows`` of the stored norm.  A zero row normalises to beta: no
    row of the quantiser's input is zero here, the zero rows of x give three EQUAL rows between differing neighbours"""
    from lkgd_amd import ops
    C, x, gamma, beta, y = ln_loop_case
    T = LN_LOOP_ROWS
    ref_q, ref_s = ops.quant_rows_fp8(y)
    q, s = ops.layernorm_quant_fp8(x, gamma, beta, 1e-5)
    assert torch.equal(s, ref_s), (C, int((s != ref_s).sum()))
    assert torch.equal(q, ref_q), (C, int((q != ref_q).sum()))
    assert torch.equal(q[8192], q[16384]) and torch.equal(q[8192], q[T - 1]) and not torch.equal(q[8192], q[8191])
    # the table search of fo.q_rows on every 61st row (coprime with 97 and with both caps: every scale class, every loop
    # iteration) and on the rows around the iteration edges; the two equalities above carry it to all rows
    rows = torch.unique(torch.cat([torch.arange(0, T, 61), torch.tensor([8191, 8192, 16383, 16384, 16385, 32767, 32768, T - 2, T - 1])]))
    _same_q(q[rows.to(DEV)], s[rows.to(DEV)], *fo.q_rows(y[rows.to(DEV)].cpu()), ("layernorm_quant_fp8 past the grid cap", C))
    ref_q, ref_s = ops.quant_rows_fp8(ops.layernorm(x, None, None, 1e-5))          # no affine: the zero rows stay zero rows
    q, s = ops.layernorm_quant_fp8(x, None, None, 1e-5)
    assert torch.equal(s, ref_s) and torch.equal(q, ref_q), (C, int((q != ref_q).sum()))
    assert bool((s[[8192, 16384, T - 1]] == 1.0).all()) and not bool(q[[8192, 16384, T - 1]].any())


@gpu
def test_layernorm_three_loop_iterations(ln_loop_case):
    """``lkgd_layernorm`` itself past its cap of 4096 workgroups, against fp32 ``F.layer_norm`` on the CPU under the tolerance of
    test_layernorm_rows_up_to_3072 (tests/test_cogvideox_rope_gpu.py: 8e-3 with the affine, 4e-3 without), row by row relative to
    nothing: the bound is absolute on normalised values of unit size"""
    import torch.nn.functional as F
    from lkgd_amd import ops
    C, x, gamma, beta, y = ln_loop_case
    xf = x.float().cpu()
    ea = (y.float().cpu() - F.layer_norm(xf, (C,), gamma.cpu(), beta.cpu(), 1e-5)).abs().amax(dim=1)
    ep = (ops.layernorm(x, None, None, 1e-5).float().cpu() - F.layer_norm(xf, (C,), eps=1e-5)).abs().amax(dim=1)
    print(f"\nLayerNorm {LN_LOOP_ROWS} x {C}: max abs error affine {ea.max():.2e} (row {int(ea.argmax())}), plain {ep.max():.2e} "
          f"(row {int(ep.argmax())})")
    assert ea.max() < 8e-3 and ep.max() < 4e-3


# ------------------------------------------------------------------------------------------------------------- GEMM, exact
def _bytes_of(v):
    """integers (|v| <= 16) -> their exact e4m3 bytes"""
    b = fo.rne_e4m3(v.float())
    assert torch.equal(fo.decode(b), v.float())
    return b


def _one_hot(M, N, K):
    a = torch.zeros(M, K)
    a[torch.arange(M), (7 * torch.arange(M) + 3) % K] = 1.0
    k, n = torch.arange(K)[None, :], torch.arange(N)[:, None]
    w = ((5 * k + 3 * n) % 17 - 8).float()                           # asymmetric, period 17 against fragments of 16 / 32 / 128
    return a, w


def _exact(a, w, a_scale=None, w_scale=None, bias=None):
    """run lkgd_gemm_fp8 on integer operands; the fp64 reference must be exactly representable in fp16; result == reference"""
    from lkgd_amd import ops
    M, N = a.shape[0], w.shape[0]
    a_scale = torch.ones(M) if a_scale is None else a_scale
    w_scale = torch.ones(N) if w_scale is None else w_scale
    ref = (a.double() @ w.double().t()) * a_scale.double()[:, None] * w_scale.double()[None, :]
    if bias is not None:
        ref = ref + bias.double()[None, :]
    assert torch.equal(ref.half().double(), ref)                     # the test's own premise
    out = ops.gemm_fp8(_bytes_of(a).to(DEV), a_scale.float().to(DEV), _bytes_of(w).to(DEV), w_scale.float().to(DEV),
                       None if bias is None else bias.float().to(DEV))
    got = out.cpu().double()
    bad = (got != ref).nonzero()
    assert out.dtype == torch.float16 and bad.numel() == 0, (tuple(a.shape), N, bad.shape[0], bad[:4].tolist(),
                                                            [got[i, j].item() for i, j in bad[:4].tolist()],
                                                            [ref[i, j].item() for i, j in bad[:4].tolist()])


@gpu
def test_gemm_fp8_one_hot_smallest():
    """the first thing to run on a GPU: M = 16, N = K = 128, one K-step, one fragment row block.  Row m of A is 1 at k = (7 m + 3) %
    K, so out[m, n] = W[n, (7 m + 3) % K]: a wrong k position inside a fragment, exchanged operands or a block scale that is not
    2^0 each give a different integer"""
    _exact(*_one_hot(16, 128, 128))


@gpu
@pytest.mark.parametrize("N,K", [(128, 128), (128, 256), (128, 640), (384, 128), (384, 256), (384, 640)])
def test_gemm_fp8_exact_on_integers(N, K):
    g = torch.Generator().manual_seed(N + K)
    for M in GEMM_M:
        _exact(*_one_hot(M, N, K))
        a = torch.randint(-1, 2, (M, K), generator=g).float()
        w = torch.randint(-2, 3, (N, K), generator=g).float()
        _exact(a, w)
        _exact(a, w, a_scale=2.0 ** ((torch.arange(M) % 5) - 2).float(), w_scale=2.0 ** ((torch.arange(N) % 3) - 1).float())
        _exact(a, w, bias=((torch.arange(N) % 7) - 3).float())


@gpu
@pytest.mark.parametrize("M,N,K", [(300, 7680, 1920), (300, 1920, 7680)])
def test_gemm_fp8_exact_at_the_real_loop_depths(M, N, K):
    """the smallest shapes with the block linears' real loop depths: 60 K-steps (K = 7680) and 60 tile columns (N = 7680), with an
    M tail across a 128-row edge.  a in {-1, 0, 1}, w in {-2 .. 2}: a sum of 7680 such products has a standard deviation of
    about 100, the largest |sum| of these seeds is 269 / 471 (computed on the CPU) - below 2048, so every sum is an fp16 value,
    and power-of-two scales keep it one as long as the product stays within fp16's exponent range: a_scale in 2^-4 .. 2^0 (never
    above one), w_scale in 2^-1 .. 2^1 give |ref| <= 904 and >= 2^-5.  ``_exact`` asserts the premise itself"""
    g = torch.Generator().manual_seed(N + K)
    a = torch.randint(-1, 2, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    assert (a.double() @ w.double().t()).abs().max() < 2048
    _exact(*_one_hot(M, N, K))
    _exact(a, w, a_scale=2.0 ** (-(torch.arange(M) % 5)).float(), w_scale=2.0 ** ((torch.arange(N) % 3) - 1).float())
    _exact(a, w, bias=((torch.arange(N) % 7) - 3).float())           # (integers again: no scale beside a bias)


# ------------------------------------------------------------------------------------------------- GEMM, random e4m3 data
def _bound_check(out, ref, S, what):
    """|err| <= 2^-11 |ref| + 2^-13 S: the fp16 output rounding, plus an accumulation at least as fine as fp16 over S = a_scale w_scale
    sum |a| |w| (the instruction's internal width is not documented; exactness is pinned by the integer tests)"""
    err = (out.cpu().double() - ref).abs()
    lim = 2.0 ** -11 * ref.abs() + 2.0 ** -13 * S
    worst = (err / lim).max().item()
    print(f"\n{what}: max |err| / bound = {worst:.3f}, max |err| = {err.max().item():.3e}")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0, (what, worst)


@gpu
@pytest.mark.parametrize("M,N,K", [(129, 256, 640), (176, 384, 1920), (1, 128, 128), (300, 128, 256)])
def test_gemm_fp8_random_e4m3(M, N, K):
    from lkgd_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N + K)
    qa = fo.rne_e4m3((torch.randn(M, K, generator=g) * 60).clamp(-448, 448))
    qw = fo.rne_e4m3((torch.randn(N, K, generator=g) * 60).clamp(-448, 448))
    a_s, w_s = torch.rand(M, generator=g) * 0.02 + 1e-3, torch.rand(N, generator=g) * 0.01 + 1e-4
    da, dw = fo.decode(qa).double(), fo.decode(qw).double()
    sc = a_s.double()[:, None] * w_s.double()[None, :]
    out = ops.gemm_fp8(qa.to(DEV), a_s.to(DEV), qw.to(DEV), w_s.to(DEV), None)
    _bound_check(out, (da @ dw.t()) * sc, (da.abs() @ dw.abs().t()) * sc, (M, N, K))


@gpu
@pytest.mark.parametrize("M,N,K", [(176, 128, 128), (176, 512, 128), (176, 128, 512)])
def test_fp8_linear_against_the_fake_quant_linear(M, N, K):
    """``quant_rows_fp8`` + ``gemm_fp8`` on packed weights against the helper's linear from the same fp16 input, same bound"""
    from lkgd_amd import fp8, ops
    g = torch.Generator().manual_seed(M + N + K)
    x = (torch.randn(M, K, generator=g) * 2).half()
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    bias = torch.randn(N, generator=g)
    xd, xs, wd, ws = fo.fake_quant_parts(x, w)
    sc = xs.double()[:, None] * ws.double()[None, :]
    ref = (xd.double() @ wd.double().t()) * sc + bias.double()[None, :]
    S = (xd.double().abs() @ wd.double().abs().t()) * sc + bias.double().abs()[None, :]
    wq, wsc = fp8.quantize_weight(w.to(DEV))
    assert torch.equal(fo.decode(wq), wd) and torch.equal(wsc.cpu(), ws)       # the pack on the device is the statement too
    out = ops.gemm_fp8(*ops.quant_rows_fp8(x.to(DEV)), wq, wsc, bias.to(DEV))
    _bound_check(out, ref, S, ("linear", M, N, K))
    assert fo.rel(out, x.float() @ w.float().t() + bias) < 5e-2               # and it is the linear, to e4m3's precision


# ------------------------------------------------------------------------------------------------ refusals and footprints
@gpu
def test_fp8_refusals_leave_the_output_alone():
    from lkgd_amd import _lib
    lib = _lib.lib()
    a = torch.zeros(8, 256, dtype=torch.uint8, device=DEV)
    w = torch.zeros(256, 256, dtype=torch.uint8, device=DEV)
    sa, sw = torch.ones(8, device=DEV), torch.ones(256, device=DEV)
    out = torch.full((8, 256), 7.0, dtype=torch.float16, device=DEV)
    x = torch.ones(8, 256, dtype=torch.float16, device=DEV)
    q = torch.full((8, 256), 0xAA, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    gemm = entry("lkgd_gemm_fp8", a=a.data_ptr(), lda=256, a_scale=sa.data_ptr(), w=w.data_ptr(), ldw=256, w_scale=sw.data_ptr(), bias=None,
                 out=out.data_ptr(), ldc=256, M=8, N=256, K=256, stream=st)
    assert gemm(a=None) == NULL and gemm(a_scale=None) == NULL and gemm(w=None) == NULL and gemm(w_scale=None) == NULL and gemm(out=None) == NULL
    assert gemm(N=192) == SHAPE and gemm(K=192) == SHAPE and gemm(N=64) == SHAPE and gemm(K=64) == SHAPE and gemm(M=0) == SHAPE
    assert gemm(a=a.data_ptr() + 8) == ALIGN and gemm(w=w.data_ptr() + 4) == ALIGN and gemm(out=out.data_ptr() + 2) == ALIGN
    assert gemm(lda=264) == ALIGN and gemm(ldw=264) == ALIGN and gemm(ldc=260) == ALIGN
    for fn in (lib.lkgd_quant_rows_fp8, lib.lkgd_gelu_tanh_quant_fp8):
        assert fn(None, 256, q.data_ptr(), 256, sa.data_ptr(), 8, 256, st) == NULL
        assert fn(x.data_ptr(), 256, q.data_ptr(), 256, sa.data_ptr(), 8, 100, st) == SHAPE
        assert fn(x.data_ptr() + 2, 256, q.data_ptr(), 256, sa.data_ptr(), 8, 256, st) == ALIGN
        assert fn(x.data_ptr(), 256, q.data_ptr(), 264, sa.data_ptr(), 8, 256, st) == ALIGN
    assert lib.lkgd_layernorm_quant_fp8(x.data_ptr(), 256, 8, 256, None, None, 1e-5, None, 256, sa.data_ptr(), st) == NULL
    assert lib.lkgd_layernorm_quant_fp8(x.data_ptr(), 256, 8, 3080, None, None, 1e-5, q.data_ptr(), 3088, sa.data_ptr(), st) == SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((q == 0xAA).all()) and bool((sa == 1.0).all())


class _Fp8Windows(footprint.Windows):
    """tests/footprint.py as it is, with e4m3 windows: guards, gaps and unwritten outputs of a byte tensor hold the NaN byte 0x7F"""

    def _poison(self, slab):
        if slab.dtype == torch.uint8:
            slab.fill_(NAN_BYTE)
        else:
            super()._poison(slab)


@pytest.fixture
def fp8_windows(monkeypatch):
    monkeypatch.setattr(footprint, "Windows", _Fp8Windows)


def _as_words(q):
    """a byte window handed to the harness as int32 words: its "unwritten" test compares with a 32-bit poison value, which no byte
    can hold (a zero byte would read as one); the NaN-byte test below takes its place"""
    return q.view(torch.int32)


def _same_bytes(got, ref, what):
    got = got.contiguous().view(torch.uint8)
    assert not bool(((got & 0x7F) == NAN_BYTE).any()), f"{what}: unwritten bytes or a leaked guard value"
    assert torch.equal(fo.decode(got), fo.decode(ref)), what


def _quant_case(name, T, K, make_ref):
    """footprint case of a quantiser ``name(x) -> (q, scale)``: x, q are windows with gaps, scale a window with guard rows"""
    from lkgd_amd import ops
    x = _rows(T, K) if name != "gelu_tanh_quant_fp8" else (_rows(T, K).float().clamp(-30, 30) * 0.5).half()

    def case(W):
        xv = W.inp(x, pad=8, col0=8, name="x")
        q = W.out(T, K, dtype=torch.uint8, pad=16, col0=16, name="q")
        s = W.out(T, 1, dtype=torch.float32, pad=0, name="scale", gap=False)
        getattr(ops, name)(xv, q=q, scale=s[:, 0])
        return {"q": _as_words(q), "scale": s}

    def close(got, ref, what):
        if "scale" in what:
            assert torch.equal(got.cpu().reshape(-1), ref.cpu().reshape(-1)), what
        else:
            _same_bytes(got, ref, what)
    run_case(case, DEV, refs=lambda: dict(zip(("q", "scale"), make_ref(x))), close=close, sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("T", [1, 65])
def test_quant_rows_fp8_footprint(fp8_windows, T):
    _quant_case("quant_rows_fp8", T, 512, lambda x: fo.q_rows(x))


@gpu
@pytest.mark.parametrize("T", [1, 65])
def test_gelu_tanh_quant_fp8_footprint(fp8_windows, T):
    from lkgd_amd import ops
    _quant_case("gelu_tanh_quant_fp8", T, 512, lambda x: fo.q_rows(ops.gelu_tanh_(x.to(DEV).clone()).cpu()))


@gpu
@pytest.mark.parametrize("T", [1, 65])
def test_layernorm_quant_fp8_footprint(fp8_windows, T):
    from lkgd_amd import ops
    C = 1920
    g = torch.Generator().manual_seed(T)
    x = (torch.randn(T, C, generator=g) * 2).half()
    gamma, beta = 1 + 0.3 * torch.randn(1, C, generator=g), 0.2 * torch.randn(1, C, generator=g)

    def case(W):
        xv = W.inp(x, pad=8, col0=8, name="x")
        gv, bv = W.inp(gamma, pad=0, name="gamma", gap=False), W.inp(beta, pad=0, name="beta", gap=False)
        q = W.out(T, C, dtype=torch.uint8, pad=16, col0=16, name="q")
        s = W.out(T, 1, dtype=torch.float32, pad=0, name="scale", gap=False)
        ops.layernorm_quant_fp8(xv, gv[0], bv[0], 1e-5, q=q, scale=s[:, 0])
        return {"q": _as_words(q), "scale": s}

    def refs():
        y = ops.layernorm(x.to(DEV), gamma[0].to(DEV), beta[0].to(DEV), 1e-5)
        return dict(zip(("q", "scale"), fo.q_rows(y.cpu())))

    def close(got, ref, what):
        if "scale" in what:
            assert torch.equal(got.cpu().reshape(-1), ref.cpu().reshape(-1)), what
        else:
            _same_bytes(got, ref, what)
    run_case(case, DEV, refs=refs, close=close, sync=torch.cuda.synchronize)


@gpu
@pytest.mark.parametrize("M", [1, 127, 129, 300])
def test_gemm_fp8_footprint(fp8_windows, M):
    """every operand a window: NaN bytes around a and w, NaN around the scales and the bias - a row read past M - 1, a column past
    K or a scale past its vector would reach the result; the pattern around out must survive"""
    from lkgd_amd import ops
    N, K = 256, 384
    g = torch.Generator().manual_seed(M)
    qa = fo.rne_e4m3((torch.randn(M, K, generator=g) * 60).clamp(-448, 448))
    qw = fo.rne_e4m3((torch.randn(N, K, generator=g) * 60).clamp(-448, 448))
    a_s, w_s, bias = torch.rand(M, 1, generator=g) * 0.02 + 1e-3, torch.rand(N, 1, generator=g) * 0.01 + 1e-4, torch.randn(N, 1, generator=g)

    def case(W):
        a = W.inp(qa, pad=16, col0=16, name="a")
        w = W.inp(qw, pad=16, col0=16, name="w")
        sa, sw, b = (W.inp(t, pad=0, name=n, gap=False) for t, n in ((a_s, "a_scale"), (w_s, "w_scale"), (bias, "bias")))
        out = W.out(M, N, pad=8, col0=8, name="out")
        ops.gemm_fp8(a, sa[:, 0], w, sw[:, 0], b[:, 0], out=out)
        return {"out": out}
    da, dw = fo.decode(qa).double(), fo.decode(qw).double()
    sc = a_s.double() * w_s.double().t()
    ref = (da @ dw.t()) * sc + bias.double().t()
    S = (da.abs() @ dw.abs().t()) * sc + bias.double().abs().t()
    run_case(case, DEV, refs=lambda: {"out": ref}, close=lambda got, r, what: _bound_check(got, r, S, what),
             sync=torch.cuda.synchronize)


# ---------------------------------------------------------------------------------------------------------- the DiT forward
def _hip(o, cfg):
    return hip_twin(o, cfg, DEV)


def _forward_rule(what, run_oracle, run_hip, o, m16, m8):
    """d(HIP FP8, twin) <= d(HIP fp16, fp32 oracle) + e_q / 2 and d(HIP FP8, fp32 oracle) <= 3 e_q, with e_q = d(twin, fp32 oracle)
    measured here.  Quantisation is discontinuous - the fp16 rounding points of the HIP path alone move the quantised output by about
    0.3 e_q from the twin - so "the twin within the fp16 bound" is not achievable, while an fp16 forward sits e_q away and fails the
    first rule.  Two FP8 forwards of one input are bitwise equal."""
    with torch.no_grad():
        ref, tw = run_oracle(o), run_oracle(fo.twin(o))
    e_q = fo.rel(tw, ref)
    out16, out8 = run_hip(m16), run_hip(m8)
    d16, d8t, d8o = fo.rel(out16, ref), fo.rel(out8, tw), fo.rel(out8, ref)
    print(f"\n{what}: e_q = {e_q:.3e}; d(HIP fp16, fp32) = {d16:.3e}; d(HIP FP8, twin) = {d8t:.3e} (bound {d16 + e_q / 2:.3e}); "
          f"d(HIP FP8, fp32) = {d8o:.3e} (bound {3 * e_q:.3e}); d(HIP fp16, twin) = {fo.rel(out16, tw):.3e}")
    assert e_q >= 5e-3
    assert out8.dtype == torch.float16 and out8.shape == ref.shape and bool(torch.isfinite(out8).all())
    assert d8t <= d16 + e_q / 2
    assert d8o <= 3 * e_q
    assert torch.equal(run_hip(m8), out8)
    assert not torch.equal(out8, out16)


@gpu
@pytest.mark.parametrize("seed", [191, 7, 23])
def test_fp8_forward_against_the_twin(seed):
    """TINY_DIT: D = 128, T = 2 x 88 rows (one ragged 128-row tile and a 48-row tail)"""
    from lkgd_amd import fp8
    from oracle import cogvideox as oc
    o = _oracle(seed)
    i = _inputs(oc.TINY_DIT, seed + 1)
    m16, m8 = _hip(o, oc.TINY_DIT), fp8.quantize_to_float8(_hip(o, oc.TINY_DIT))
    assert m8.quantization == "fp8" and m16.quantization is None

    def run_hip(m):
        return m(*(i[k].to(DEV) for k in ("hidden", "text", "t", "domain", "flow")), return_dict=False)[0]
    _forward_rule(f"TINY_DIT seed {seed}", lambda o_: o_(i["hidden"], i["text"], i["t"], i["domain"], i["flow"])[0], run_hip, o, m16, m8)
    bp = m8.transformer_blocks[0]._pk
    assert bp.q[0].dtype == torch.uint8 and len(bp.q) == 3 and m16.transformer_blocks[0]._pk.q[0].dtype == torch.float16


@gpu
def test_fp8_forward_of_the_tiny_15_model_against_its_twin():
    """the same rule on the temporal-patch, rotary, ofs model: the mode touches only the six linears"""
    import cogvideox15_oracle as vo
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import fp8
    cfg = vo.TINY_V15_DIT
    o = vo.seeded_model(cfg, 191)
    i = _inputs(cfg, 192)
    m16, m8 = _hip(o, cfg), fp8.quantize_to_float8(_hip(o, cfg))
    rope_o = vo.rotary_tables(cfg, 4, 4, 6)

    def run_oracle(o_):
        return o_(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], ofs=torch.full((1,), 2.0), image_rotary_emb=rope_o)[0]

    def run_hip(m):
        return m(*(i[k].to(DEV) for k in ("hidden", "text", "t", "domain", "flow")), ofs=2.0,
                 image_rotary_emb=pc.rotary_tables(m.config, 2, 4, 6), return_dict=False)[0]
    _forward_rule("TINY_V15_DIT", run_oracle, run_hip, o, m16, m8)


@gpu
def test_fp8_denoise_equals_the_loop_stepped_by_hand(monkeypatch):
    """2 steps at TINY_DIT with the mode on (here through LKGD_DIT_FP8, read when the model packs): every step has the bits of
    ``dit_patch_rows`` -> ``forward_rows`` -> ``dit_cfg_ddim_step`` called by hand, and of the model switched by
    ``quantize_to_float8``; the loop stays near the fp16 loop and is not it"""
    from lkgd_amd import cogvideox as pc
    from lkgd_amd import fp8, ops
    from oracle import cogvideox as oc
    o = _oracle(4242)
    m16 = _hip(o, oc.TINY_DIT)
    monkeypatch.setenv("LKGD_DIT_FP8", "1")
    m8 = _hip(o, oc.TINY_DIT)
    lat, img, pe, dom, flow = (t.to(DEV) for t in _loop_inputs())
    lat, img = lat.half(), img.half()
    steps = []
    new = pc.denoise(m8, pc.CogVideoXDDIMScheduler(), lat, img, pe, dom, flow, 2, 6.0, True, callback=lambda i, t, l: steps.append(l))
    assert m8._pk.fp8 and m8.quantization is None
    monkeypatch.delenv("LKGD_DIT_FP8")
    mq = fp8.quantize_to_float8(_hip(o, oc.TINY_DIT))
    sched = pc.CogVideoXDDIMScheduler()
    sched.set_timesteps(2)
    text = mq.fused_text(pe, dom, flow)
    cur = lat.clone()
    for i, t in enumerate(sched.timesteps.tolist()):
        rows = ops.dit_patch_rows(cur, img, 2)
        noise = mq.forward_rows(rows, (3, 4, 6), text, float(t))
        ops.dit_cfg_ddim_step(noise, cur, 2, 2, pc.dynamic_guidance(6.0, 2, t), *sched.coefficients(int(t)))
        assert torch.equal(cur, steps[i]), (i, (cur.float() - steps[i].float()).abs().max().item())
    assert len(steps) == 2 and torch.equal(new, cur) and new.dtype == torch.float16
    ref16 = pc.denoise(m16, pc.CogVideoXDDIMScheduler(), lat, img, pe, dom, flow, 2, 6.0, True)
    assert not m16._pk.fp8 and not torch.equal(new, ref16) and fo.rel(new, ref16) < 5e-2


@gpu
def test_dequantize_restores_the_fp16_forward_bitwise():
    from lkgd_amd import fp8
    from oracle import cogvideox as oc
    o = _oracle(191)
    i = {k: v.to(DEV) for k, v in _inputs(oc.TINY_DIT, 192).items()}
    m = _hip(o, oc.TINY_DIT)

    def run():
        return m(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], return_dict=False)[0]
    ref = run()
    fp8.quantize_to_float8(m)
    q = run()
    assert m._pk.fp8 and not torch.equal(q, ref)
    fp8.dequantize(m)
    back = run()
    assert not m._pk.fp8 and torch.equal(back, ref)
    assert torch.equal(_hip(o, oc.TINY_DIT)(i["hidden"], i["text"], i["t"], i["domain"], i["flow"], return_dict=False)[0], ref)
