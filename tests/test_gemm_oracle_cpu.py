"""The descriptor oracle (tests/gemm_oracle.py) against fp64 torch.nn.functional, on the CPU: small descriptors built through
the project's own weight packers, every A mode and every epilogue term.  Agreement <= 1e-10 relative: both sides are fp64 and
differ by summation order only."""
import torch
import torch.nn.functional as F

import gemm_oracle as go
from lkgd_amd import packing as pk

TOL = 1e-10


def _agree(got, ref, what):
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert scale > 0.1, f"{what}: degenerate reference"
    assert err <= TOL * scale, f"{what}: {err:.3e} vs scale {scale:.3e}"


def _tokens(x):          # [N, C, H, W] -> [N*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def test_oracle_never_touches_the_product_front_end():
    src = open(go.__file__).read()
    assert "import lkgd_amd" not in src and "from lkgd_amd" not in src


def test_linear_two_source_rowmap_residuals():
    g = _g(1)
    M, N, K, cs = 37, 24, 192, 128
    a0, a1 = _rn(g, M, 136), _rn(g, M, 72)                # leading dimensions wider than the used columns
    w = pk.pack_linear(_rn(g, N, K) / K ** 0.5).double()
    bias, res1, res2 = _rn(g, N), _rn(g, M, 40), _rn(g, M, N)
    rb = _rn(g, 11, 32)
    d = go.desc(M=M, N=N, K=K, lda0=136, lda1=72, csplit=cs, ldrb=32, rb_d1=4, rb_m1=3, rb_d2=5, rb_md=11, rb_c0=2,
                ldr1=40, ldr2=N, ldc=N, s_acc=0.75, r1=0.5, r2=-1.25)
    rows = torch.arange(M)
    got, S = go.gemm_rows(d, dict(a0=a0, a1=a1, w=w, bias=bias, rowbias=rb, res1=res1, res2=res2), rows)
    a = torch.cat([a0[:, :cs], a1[:, :K - cs]], 1)
    idx = ((rows // 4) * 3 + rows % 5 + 2) % 11
    assert len(set(idx.tolist())) > 5                     # the map really moves
    ref = 0.75 * (F.linear(a, w, bias) + rb[idx, :N]) + 0.5 * res1[:, :N] - 1.25 * res2
    _agree(got, ref, "linear")
    _agree(S, a.abs() @ w.abs().T, "S")
    assert (S >= (a @ w.T).abs() - 1e-12).all()
    # a subset of rows in another order gives those rows
    sub = torch.tensor([36, 0, 17])
    _agree(go.gemm_rows(d, dict(a0=a0, a1=a1, w=w, bias=bias, rowbias=rb, res1=res1, res2=res2), sub)[0], ref[sub], "subset")
    # NULL pointers drop their terms
    _agree(go.gemm_rows(go.desc(M=M, N=N, K=128, lda0=136, ldc=N), dict(a0=a0, w=w[:, :128].contiguous()), rows)[0],
           a0[:, :128] @ w[:, :128].T, "bare")


def _conv_case(g, stride, ups, pad_off, two_source):
    n, Cin, Cout, Hi, Wi = 2, 128, 12, 5, 7
    x = _rn(g, n, Cin, Hi, Wi)
    w4 = (_rn(g, Cout, Cin, 3, 3) / (9 * Cin) ** 0.5).half().double()
    bias = _rn(g, Cout)
    xv = F.interpolate(x, scale_factor=2, mode="nearest") if ups else x
    if pad_off:
        ref4 = F.conv2d(F.pad(xv, (0, 1, 0, 1)), w4, bias, stride=stride, padding=0)
    else:
        ref4 = F.conv2d(xv, w4, bias, stride=stride, padding=1)
    Ho, Wo = ref4.shape[2:]
    t = _tokens(x)
    bufs = dict(w=pk.pack_conv3x3(w4).double(), bias=bias)
    kw = {}
    if two_source:
        bufs.update(a0=t[:, :64].contiguous(), a1=torch.cat([t[:, 64:], _rn(g, t.shape[0], 8)], 1))   # lda1 = 72
        kw = dict(lda0=64, lda1=72, csplit=64)
    else:
        bufs.update(a0=t)
        kw = dict(lda0=Cin)
    d = go.desc(M=n * Ho * Wo, N=Cout, K=9 * Cin, mode=go.A_CONV3X3, Cin=Cin, Hout=Ho, Wout=Wo, Hin=Hi, Win=Wi, stride=stride,
                ups=ups, pad_off=pad_off, ldc=Cout, **kw)
    got, S = go.gemm_rows(d, bufs, torch.arange(d.M))
    _agree(got, _tokens(ref4), f"conv3x3 stride {stride} ups {ups} pad_off {pad_off} two_source {two_source}")
    assert S.shape == got.shape and (S > 0).all()


def test_conv3x3_stride_ups_pad_off_and_channel_concat():
    g = _g(2)
    _conv_case(g, 1, 0, 0, False)
    _conv_case(g, 2, 0, 0, False)          # 5x7 -> 3x4: odd sizes, the last tap column is padding
    _conv_case(g, 1, 1, 0, False)          # nearest-2x upsample folded into the gather
    _conv_case(g, 2, 0, 1, False)          # F.pad((0,1,0,1)) + stride-2 conv, padding 0
    _conv_case(g, 1, 0, 0, True)
    _conv_case(g, 2, 0, 0, True)


def test_conv3x3_c8():
    g = _g(3)
    n, Cout, H, W = 2, 20, 4, 6
    x = _rn(g, n, 8, H, W)
    w4 = (_rn(g, Cout, 8, 3, 3) / 72 ** 0.5).half().double()
    bias = _rn(g, Cout)
    d = go.desc(M=n * H * W, N=Cout, K=128, mode=go.A_CONV3X3_C8, Cin=8, lda0=8, Hout=H, Wout=W, Hin=H, Win=W, stride=1, ldc=Cout)
    got, _ = go.gemm_rows(d, dict(a0=_tokens(x), w=pk.pack_conv3x3_c8(w4).double(), bias=bias), torch.arange(d.M))
    _agree(got, _tokens(F.conv2d(x, w4, bias, padding=1)), "conv3x3 c8")


def test_temporal_conv_whole_and_frame_sharded():
    g = _g(4)
    B, Fr, Cin, Cout, H, W = 2, 5, 64, 16, 2, 3
    HW = H * W
    x = _rn(g, B, Cin, Fr, H, W)
    w5 = (_rn(g, Cout, Cin, 3, 1, 1) / (3 * Cin) ** 0.5).half().double()
    bias = _rn(g, Cout)
    ref = F.conv3d(x, w5, bias, padding=(1, 0, 0)).permute(0, 2, 3, 4, 1).reshape(B, Fr, HW, Cout)     # [b, f, s, c]
    t = x.permute(0, 2, 3, 4, 1).reshape(B * Fr * HW, Cin).contiguous()
    bufs = dict(a0=t, w=pk.pack_tconv3(w5).double(), bias=bias)
    d = go.desc(M=B * Fr * HW, N=Cout, K=3 * Cin, mode=go.A_TCONV3, Cin=Cin, lda0=Cin, F=Fr, HW=HW, ldc=Cout)
    _agree(go.gemm_rows(d, bufs, torch.arange(d.M))[0], ref.reshape(-1, Cout), "tconv")
    for Floc, f_off in ((2, 0), (2, 3), (1, 2)):           # a rank's frames: the source holds all F frames
        d = go.desc(M=B * Floc * HW, N=Cout, K=3 * Cin, mode=go.A_TCONV3, Cin=Cin, lda0=Cin, F=Fr, HW=HW, Floc=Floc, f_off=f_off,
                    ldc=Cout)
        _agree(go.gemm_rows(d, bufs, torch.arange(d.M))[0], ref[:, f_off:f_off + Floc].reshape(-1, Cout),
               f"tconv frames {f_off}+{Floc}")


def test_geglu_both_interleave_widths_on_packed_rows():
    g = _g(5)
    for h, inner, K in ((32, 64, 128), (80, 160, 320)):
        M = 9
        a = _rn(g, M, K)
        w, b = _rn(g, 2 * inner, K) / K ** 0.5, _rn(g, 2 * inner)
        wp, bp, half = pk.pack_geglu(w, b, h if h == 32 else None)
        assert half == h
        d = go.desc(M=M, N=2 * inner, K=K, lda0=K, ldc=inner, geglu=h)
        got, S = go.gemm_rows(d, dict(a0=a, w=wp.double(), bias=bp.double()), torch.arange(M))
        perm = pk.geglu_perm(inner, h)
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(perm.numel())
        hidden, gate = F.linear(a, wp.double()[inv], bp.double()[inv]).chunk(2, dim=-1)
        _agree(got, hidden * F.gelu(gate), f"geglu {h}")
        assert S is None and got.shape == (M, inner)


def test_layernorm_fold():
    g = _g(6)
    M, N, K, eps = 23, 16, 192, 1e-5
    x = _rn(g, M, K) * 1.7 + 0.6
    gamma, beta = 1.0 + 0.2 * _rn(g, K), 0.3 * _rn(g, K)
    w, b = _rn(g, N, K) / K ** 0.5, _rn(g, N)
    wf = pk.pack_linear(w * gamma[None, :]).double()          # the Linear that consumes the LayerNorm carries its affine
    bf = (b + w @ beta).float().double()
    res = _rn(g, M, N)
    d = go.desc(M=M, N=N, K=K, lda0=K, ldc=N, ldr1=N, ln_eps=eps)
    got, S = go.gemm_rows(d, dict(a0=x, w=wf, bias=bf, res1=res, ln_colsum=wf.sum(1)), torch.arange(M))
    ref = F.linear(F.layer_norm(x, (K,), None, None, eps), wf, bf) + res
    _agree(got, ref, "layernorm fold")
    assert (S > 0).all()
    # and through gamma / beta themselves, up to the fp16 rounding of the folded weights
    ref2 = F.linear(F.layer_norm(x, (K,), gamma, beta, eps), w, b) + res
    assert (got - ref2).abs().max() < 2e-3 * ref2.abs().max()


def test_column_blocks_and_cols_select_the_same_numbers():
    """the bounded-memory evaluation: any block size gives the unblocked result (one dot product per element either way: fp64
    summation order at most), and ``cols`` returns exactly those columns of it - every epilogue term included, in any order,
    with repeats, across block edges"""
    g = _g(7)
    M, N, K = 19, 203, 128                                # 203 columns: no block size below divides it
    a0 = _rn(g, M, 136)
    w = pk.pack_linear(_rn(g, N, K) / K ** 0.5).double()
    bias, res1, res2, rb = _rn(g, N), _rn(g, M, N + 5), _rn(g, M, N), _rn(g, 7, N + 3)
    d = go.desc(M=M, N=N, K=K, lda0=136, ldrb=N + 3, rb_d1=3, rb_m1=1, rb_d2=1, rb_md=7, ldr1=N + 5, ldr2=N, ldc=N, s_acc=0.5,
                r1=0.25, r2=-2.0)
    bufs = dict(a0=a0, w=w, bias=bias, rowbias=rb, res1=res1, res2=res2)
    rows = torch.tensor([18, 0, 7, 11])
    full, S = go.gemm_rows(d, bufs, rows, block=N)        # one block: the unblocked evaluation
    idx = (rows // 3) % 7
    _agree(full, 0.5 * (F.linear(a0[rows, :K], w, bias) + rb[idx, :N]) + 0.25 * res1[rows, :N] - 2.0 * res2[rows], "unblocked")
    assert go.COL_BLOCK >= N
    for block in (None, 1, 7, 64, 202):
        got, Sb = go.gemm_rows(d, bufs, rows, block=block)
        _agree(got, full, f"block {block}")
        _agree(Sb, S, f"S, block {block}")
    cols = torch.tensor([202, 0, 64, 63, 7, 7, 201, 100])
    for block in (None, 3):
        got, Sc = go.gemm_rows(d, bufs, rows, cols=cols, block=block)
        assert got.shape == Sc.shape == (4, 8)
        _agree(got, full[:, cols], f"cols, block {block}")
        _agree(Sc, S[:, cols], f"S of cols, block {block}")
    # the LayerNorm fold's column sums follow the selection too
    dl = go.desc(M=M, N=N, K=K, lda0=136, ldc=N, ln_eps=1e-5)
    bl = dict(a0=a0, w=w, bias=bias, ln_colsum=w.sum(1))
    fl, Sl = go.gemm_rows(dl, bl, rows, block=N)
    gl, Sg = go.gemm_rows(dl, bl, rows, cols=cols, block=5)
    _agree(gl, fl[:, cols], "fold cols")
    _agree(Sg, Sl[:, cols], "fold S cols")
