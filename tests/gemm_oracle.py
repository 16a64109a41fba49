"""fp64 interpreter of ``lkgd_gemm_desc`` - what include/lkgd_hip.h section 1 says a descriptor computes, written from the header
text alone.  It never calls into lkgd_amd.ops or the library: the census (tests/test_gemm_census_gpu.py) holds every launch of
the real forward against it, and tests/test_gemm_oracle_cpu.py holds IT against fp64 torch.nn.functional.

    out[m, n] = s_acc * ( sum_k A(m,k) * W[n,k] + bias[n] + rowbias[idx(m), n] ) + r1 * res1[m, n] + r2 * res2[m, n]
    idx(m)    = ((m / rb_d1) * rb_m1 + (m % rb_d2) + rb_c0) % rb_md

``d`` is anything with the descriptor's scalar fields as attributes (the ctypes struct, a SimpleNamespace); pointers are not read.
``bufs`` maps a0 / a1 / w / bias / rowbias / res1 / res2 / ln_colsum to 2-D (1-D: bias, ln_colsum) tensors of any dtype and
device whose row stride is the descriptor's leading dimension (row r of the buffer = elements [r*ld, r*ld + ld) behind the
pointer); absent or None = the NULL pointer.  Only the rows a result needs are gathered and converted to fp64, so the buffers may
stay on the device.  W is converted ``COL_BLOCK`` output columns at a time, so the fp64 copy of a weight never exceeds
COL_BLOCK * K * 8 bytes whatever N is, and ``cols`` restricts a result to the named output columns."""
import math
from types import SimpleNamespace

import torch

A_PLAIN, A_CONV3X3, A_TCONV3, A_CONV3X3_C8 = 0, 1, 2, 3

#: the descriptor's scalar fields, in struct order (pointers and workspace_bytes excluded)
SCALARS = ("M", "N", "K", "lda0", "lda1", "csplit", "mode", "Cin", "Hout", "Wout", "Hin", "Win", "stride", "ups", "F", "HW",
           "Floc", "f_off", "ldrb", "rb_d1", "rb_m1", "rb_d2", "rb_md", "rb_c0", "ldr1", "ldr2", "ldc", "s_acc", "r1", "r2",
           "geglu", "pad_off", "ln_eps", "cs_rows")
_DEFAULTS = dict.fromkeys(SCALARS, 0)
_DEFAULTS.update(s_acc=1.0, r1=1.0, r2=1.0)


def desc(**fields):
    """a descriptor from keyword fields (everything else 0; s_acc = r1 = r2 = 1); csplit defaults to K (plain) / Cin"""
    f = dict(_DEFAULTS)
    f.update(fields)
    if "csplit" not in fields:
        f["csplit"] = f["K"] if f["mode"] == A_PLAIN else f["Cin"]
    if f["mode"] == A_TCONV3 and "Floc" not in fields:
        f["Floc"], f["f_off"] = f["F"], 0
    return SimpleNamespace(**f)


#: output columns whose weights are held in fp64 at one time (gemm_rows)
COL_BLOCK = 8192


def _gather(buf, rows, valid=None, cols=None):
    """rows `rows` (int64 [R]) of a 2-D buffer as fp64 on the CPU; rows where `valid` is False read as zeros; `cols` (int64):
    those columns only, selected before the conversion"""
    rows = torch.as_tensor(rows, dtype=torch.int64)
    if valid is not None:
        rows = torch.where(valid, rows, torch.zeros_like(rows))
    x = buf.index_select(0, rows.to(buf.device))
    if cols is not None:
        x = x.index_select(1, cols.to(buf.device))
    x = x.to("cpu", torch.float64)
    if valid is not None:
        x = x * valid.to(torch.float64)[:, None]
    return x


def _channels(d, bufs, src_rows, valid, C):
    """channels [0, C) of source rows: a0[:, c] for c < csplit, else a1[:, c - csplit]"""
    cs = min(int(d.csplit), C)
    x = _gather(bufs["a0"], src_rows, valid)[:, :cs]
    if cs < C:
        x = torch.cat([x, _gather(bufs["a1"], src_rows, valid)[:, :C - cs]], dim=1)
    return x


def a_rows(d, bufs, rows):
    """A(m, 0..K) for the given rows, fp64 [R, K]"""
    m = torch.as_tensor(rows, dtype=torch.int64)
    R, K, mode = m.numel(), int(d.K), int(d.mode)
    if mode == A_PLAIN:
        return _channels(d, bufs, m, None, K)
    A = torch.zeros(R, K, dtype=torch.float64)
    if mode in (A_CONV3X3, A_CONV3X3_C8):
        Ho, Wo, Hi, Wi = int(d.Hout), int(d.Wout), int(d.Hin), int(d.Win)
        stride, ups, off = (1, 0, 0) if mode == A_CONV3X3_C8 else (int(d.stride), int(d.ups), int(d.pad_off))
        Cin = int(d.Cin)
        n, y, x = m // (Ho * Wo), (m % (Ho * Wo)) // Wo, m % Wo
        c = torch.arange(Cin)
        for ky in range(3):
            for kx in range(3):
                # pad 1: tap (ky, kx) of output (y, x) sits at (y*stride + ky - 1, ..) of the (upsampled) source grid;
                # pad_off = 1: no padding at the top / left, i.e. the tap grid starts one pixel further in
                vy, vx = y * stride + ky - 1 + off, x * stride + kx - 1 + off
                valid = (vy >= 0) & (vy < (Hi << ups)) & (vx >= 0) & (vx < (Wi << ups))
                src = (n * Hi + (vy >> ups)) * Wi + (vx >> ups)
                X = _channels(d, bufs, src, valid, Cin)
                if mode == A_CONV3X3_C8:
                    k = (ky * 3 + kx) * 8 + c                    # one 8-channel chunk per tap; k >= 72 is padding: A = 0
                else:
                    k = ((ky * (Cin // 64) + c // 64) * 3 + kx) * 64 + c % 64
                A[:, k] = X
        return A
    if mode == A_TCONV3:
        Fr, HW, Floc, f_off, Cin = int(d.F), int(d.HW), int(d.Floc), int(d.f_off), int(d.Cin)
        b, fl, s = m // (Floc * HW), (m // HW) % Floc, m % HW
        f = f_off + fl
        for kt in range(3):
            sf = f + kt - 1
            valid = (sf >= 0) & (sf < Fr)
            A[:, kt * Cin:(kt + 1) * Cin] = _channels(d, bufs, (b * Fr + sf) * HW + s, valid, Cin)
        return A
    raise ValueError(f"unknown A mode {mode}")


def rowmap_index(d, rows):
    m = torch.as_tensor(rows, dtype=torch.int64)
    return ((m // int(d.rb_d1)) * int(d.rb_m1) + (m % int(d.rb_d2)) + int(d.rb_c0)) % int(d.rb_md)


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _vector(buf, N, cols):
    v = buf[:N] if cols is None else buf.index_select(0, cols.to(buf.device))
    return v.to("cpu", torch.float64)[None, :]


def gemm_rows(d, bufs, rows, cols=None, block=None):
    """rows `rows` of out in fp64: ([R, N] or, GEGLU, [R, N / 2],  S [R, N] = sum_k |A(m,k) * W[n,k]| or None for GEGLU).
    With the LayerNorm fold S is the magnitude that enters the rounded sum: rstd * (sum_k |A W| + |mean * ln_colsum|).
    ``cols`` (int64 [Q], not with GEGLU): output columns `cols` only, [R, Q] - the same numbers the full result has there.
    ``block``: output columns per fp64 piece of W (default COL_BLOCK); every element is one dot product over K whatever the
    block, so the block size moves a result by fp64 summation order at most."""
    m = torch.as_tensor(rows, dtype=torch.int64)
    N, K = int(d.N), int(d.K)
    block = int(block or COL_BLOCK)
    get = lambda k: bufs.get(k)                                                      # noqa: E731
    if cols is not None:
        cols = torch.as_tensor(cols, dtype=torch.int64)
        assert not int(d.geglu), "cols: GEGLU pairs columns, select on the result instead"
        assert cols.numel() and int(cols.min()) >= 0 and int(cols.max()) < N
    Q = N if cols is None else cols.numel()
    A = a_rows(d, bufs, m)
    Aabs = A.abs()
    W = bufs["w"]
    acc = torch.empty(m.numel(), Q, dtype=torch.float64)
    S = torch.empty(m.numel(), Q, dtype=torch.float64)
    for c0 in range(0, Q, block):
        c1 = min(Q, c0 + block)
        Wb = W[c0:c1, :K] if cols is None else W.index_select(0, cols[c0:c1].to(W.device))[:, :K]
        Wb = Wb.to("cpu", torch.float64)
        acc[:, c0:c1] = A @ Wb.T
        S[:, c0:c1] = Aabs @ Wb.abs().T
        del Wb
    if get("ln_colsum") is not None:
        # LayerNorm of the A rows (no affine: folded into W / bias) applied after the product
        assert int(d.mode) == A_PLAIN and not int(d.geglu)
        mean = A.mean(dim=1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((A - mean) ** 2).mean(dim=1, keepdim=True) + float(d.ln_eps))
        cs = _vector(bufs["ln_colsum"], N, cols)
        acc = rstd * (acc - mean * cs)
        S = rstd * (S + (mean * cs).abs())
    v = acc
    if get("bias") is not None:
        v = v + _vector(bufs["bias"], N, cols)
    if int(d.geglu):
        h = int(d.geglu)
        assert h in (32, 80) and N % (2 * h) == 0
        assert get("rowbias") is None and get("res1") is None and get("res2") is None and float(d.s_acc) == 1.0
        v = v.reshape(m.numel(), N // (2 * h), 2, h)                 # packed rows: h hidden | their h gates
        return (v[:, :, 0] * gelu_erf(v[:, :, 1])).reshape(m.numel(), N // 2), None
    sel = (lambda x: x[:, :N]) if cols is None else (lambda x: x)                    # noqa: E731
    if get("rowbias") is not None:
        v = v + sel(_gather(bufs["rowbias"], rowmap_index(d, m), cols=cols))
    v = float(d.s_acc) * v
    if get("res1") is not None:
        v = v + float(d.r1) * sel(_gather(bufs["res1"], m, cols=cols))
    if get("res2") is not None:
        v = v + float(d.r2) * sel(_gather(bufs["res2"], m, cols=cols))
    return v, S
