"""GroupNorm, LayerNorm and the row softmax on the probes of tests/norm_probes.py, per element against fp64 / integer references with
the bounds derived in that module's docstring:

  lkgd_groupnorm_sums            the float32 rounding of the exact integer sums, bit for bit
  lkgd_groupnorm_stats, _silu    (mean, rstd) to 2^-22; the output to 2^-10 |ref| + 2^-20 (|x A| + |mean A| + |beta|) + 2^-24, in the
                                 one-launch and the three-launch form, and which of the two ran (the one-launch kernel never writes
                                 `partial`; the three launches write exactly the planned chunks)
  lkgd_groupnorm_apply, _apply_segments, lkgd_spatial_norm3d   given statistics on which every intermediate is exact: the
                                 reference rounded once
  lkgd_groupnorm_stats_cols, _finalize_parts                   integer tables: exact sums, (mean, rstd) to 2^-22
  lkgd_layernorm                 one-hot and balanced rows at every (L, NV) of the dispatch, full and clamped lane groups
  lkgd_softmax_rows              uniform, weighted and one-hot rows up to 16384 columns

Inputs and outputs sit inside wider matrices of sentinels (row pitches larger than the widths), the sentinels are checked after
every launch, the debug knobs are restored in `finally`.  Every case prints its worst err / bound (`PROBE ...`, visible with -s),
the last test the worst per entry point.  That the probes reject the faults they are meant for is shown in test_norm_probes_cpu.py."""
import pytest
import torch

import norm_probes as npb
from norm_probes import F16, F32, F64, SENTINEL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
NAN = float("nan")
WORST = {}


def _lib():
    from lkgd_amd import _lib
    return _lib.lib()


def _stream():
    from lkgd_amd import ops
    return ops._stream()


def _report(entry, case, r):
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    print(f"PROBE {entry} {case} {r:.4f}")


def _inp(t, pad, col0=0):
    """t inside a wider device matrix of sentinels: the [rows, C] view"""
    whole, _ = npb.padded(t, pad, col0)
    return whole.to(DEV)[:, col0:col0 + t.shape[1]]


class _Out:
    """an output window inside a wider device matrix of sentinels"""

    def __init__(self, rows, C, pad=40, col0=16, dtype=F16):
        self.whole = torch.full((rows, col0 + C + pad), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.whole[:, col0:col0 + C]
        self.col0, self.C = col0, C

    def get(self, what):
        w = self.whole.cpu()
        assert bool((w[:, :self.col0] == SENTINEL).all()) and bool((w[:, self.col0 + self.C:] == SENTINEL).all()), \
            f"{what}: wrote outside its output window"
        return w[:, self.col0:self.col0 + self.C]


def _sources(p):
    """x of a GnProbe as one or two device sources with row pitches of their own: (x0, x1, C-entry arguments)"""
    if p.c1:
        x0, x1 = _inp(p.x[:, :p.c0], 8), _inp(p.x[:, p.c0:], 24, col0=8)
        return x0, x1, (x0.data_ptr(), p.c0, x0.stride(0), x1.data_ptr(), p.c1, x1.stride(0))
    x0 = _inp(p.x, 16)
    return x0, None, (x0.data_ptr(), p.c0, x0.stride(0), None, 0, 0)


def _partial(p):
    """`partial` as a caller sizes it (lkgd_groupnorm_chunks), NaN-filled, with a guard block behind it"""
    L = _lib()
    nch = L.lkgd_groupnorm_chunks(p.rows, p.C)
    assert nch == npb.gn_chunks_bound(p.C, p.rows)
    n = p.ns * nch * 64
    buf = torch.full((n + 64,), NAN, dtype=F32, device=DEV)
    return buf, n


def _chunks_written(buf, n, p, what):
    """the statistics pass wrote exactly the planned chunks of `partial`, inside the caller's size"""
    b = buf.cpu()
    assert bool(torch.isnan(b[n:]).all()), f"{what}: wrote behind the scratch sized by lkgd_groupnorm_chunks"
    wrote = int((~torch.isnan(b)).sum())
    return wrote


# ================================================================================================== GroupNorm
@pytest.mark.parametrize("ns,rows,C,c0,why", npb.GN_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" + (f"-c0_{c[3]}" if c[3] else "") for c in npb.GN_CASES])
def test_groupnorm(ns, rows, C, c0, why):
    from lkgd_amd import ops
    L = _lib()
    p = npb.GnProbe(ns, rows, C, c0)
    case = f"{ns}x{rows}x{C}" + (f",c0={c0}" if c0 else "")
    x0, x1, src = _sources(p)
    planned = ns * npb.gn_chunks(C, rows, ns) * 64
    # ---- sums: bit for bit the exact ones (through ops, and through the C entry with a watched scratch)
    p.check_sums(ops.groupnorm_sums(x0, x1, ns, rows), f"groupnorm_sums {case}")
    buf, n = _partial(p)
    sums = torch.full((ns, 32, 2), NAN, dtype=F32, device=DEV)
    assert L.lkgd_groupnorm_sums(*src, ns, rows, buf.data_ptr(), sums.data_ptr(), _stream()) == 0
    p.check_sums(sums, f"lkgd_groupnorm_sums {case}")
    assert _chunks_written(buf, n, p, "sums") == planned, (case, why)
    _report("lkgd_groupnorm_sums", case, 0.0)
    # ---- statistics
    _report("lkgd_groupnorm_stats", case, p.check_stats(ops.groupnorm_stats(x0, x1, ns, rows, EPS), EPS, f"groupnorm_stats {case}"))
    # ---- the whole GroupNorm, silu = 0: one launch where the rule allows it, and the three launches
    gamma, beta = p.affine()
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ref, bound = p.out_ref(gamma, beta, EPS, False)
    for form in ("rule", "three_launches"):
        out = _Out(ns * rows, C)
        vec = npb.gn_small_vec(p.c0, p.c1, src[2], src[5], out.view.stride(0), ns, rows) if form == "rule" else 0
        buf, n = _partial(p)
        stats = torch.full((ns, 32, 2), NAN, dtype=F32, device=DEV)
        L.lkgd_debug_set_gn_small(1 if form == "rule" else 0)
        try:
            rc = L.lkgd_groupnorm_silu(*src, ns, rows, EPS, buf.data_ptr(), stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), 0,
                                       out.view.data_ptr(), out.view.stride(0), _stream())
        finally:
            L.lkgd_debug_set_gn_small(1)
        assert rc == 0
        wrote = _chunks_written(buf, n, p, form)
        assert wrote == (0 if vec else planned), f"{case} ({why}): planned {'one launch' if vec else 'three launches'}, " \
                                                 f"`partial` got {wrote} floats"
        entry = "lkgd_groupnorm_silu[one launch]" if vec else "lkgd_groupnorm_silu[three launches]"
        _report(entry + " stats", case, p.check_stats(stats, EPS, f"{entry} stats {case}"))
        _report(entry, case, npb.worst(out.get(entry), ref, bound, f"{entry} {case}"))
    # ---- given statistics: the reference rounded once
    st, ga, be = p.given()
    gref, gbound = p.given_ref(st, ga, be)
    out = _Out(ns * rows, C)
    ops.groupnorm_apply(x0, x1, ns, rows, st.to(DEV), ga.to(DEV), be.to(DEV), False, out.view)
    _report("lkgd_groupnorm_apply", case, npb.worst(out.get("apply"), gref, gbound, f"groupnorm_apply (given statistics) {case}"))


@pytest.mark.parametrize("form", ["one_launch", "three_launches"])
@pytest.mark.parametrize("ns,rows,C,c0", npb.GN_SILU_CASES)
def test_groupnorm_silu(ns, rows, C, c0, form):
    L = _lib()
    p = npb.GnProbe(ns, rows, C, c0)
    x0, x1, src = _sources(p)
    gamma, beta = p.affine()
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ref, bound = p.out_ref(gamma, beta, EPS, True)
    out = _Out(ns * rows, C)
    buf, n = _partial(p)
    stats = torch.full((ns, 32, 2), NAN, dtype=F32, device=DEV)
    vec = npb.gn_small_vec(p.c0, p.c1, src[2], src[5], out.view.stride(0), ns, rows, on=form == "one_launch")
    assert bool(vec) == (form == "one_launch")
    L.lkgd_debug_set_gn_small(1 if form == "one_launch" else 0)
    try:
        assert L.lkgd_groupnorm_silu(*src, ns, rows, EPS, buf.data_ptr(), stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), 1,
                                     out.view.data_ptr(), out.view.stride(0), _stream()) == 0
    finally:
        L.lkgd_debug_set_gn_small(1)
    assert (_chunks_written(buf, n, p, form) == 0) == (form == "one_launch")
    _report(f"lkgd_groupnorm_silu[{form.replace('_', ' ')}] silu", f"{ns}x{rows}x{C}", npb.worst(out.get(form), ref, bound, f"silu {form}"))
    if form == "three_launches":                    # SiLU behind given statistics: the pre-activation is exact
        from lkgd_amd import ops
        st, ga, be = p.given()
        sref, sbound = npb.silu_of_exact(p.given_ref(st, ga, be)[0])
        out = _Out(ns * rows, C)
        ops.groupnorm_apply(x0, x1, ns, rows, st.to(DEV), ga.to(DEV), be.to(DEV), True, out.view)
        _report("lkgd_groupnorm_apply silu", f"{ns}x{rows}x{C}", npb.worst(out.get("apply"), sref, sbound, "groupnorm_apply silu"))


def test_groupnorm_one_launch_limits():
    """the size rule sends a tensor over the byte limit to the three launches, lkgd_debug_set_gn_small_limits moves it"""
    L = _lib()
    p = npb.GnProbe(3, 77, 320)
    x0, x1, src = _sources(p)
    gamma, beta = p.affine()
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ref, bound = p.out_ref(gamma, beta, EPS, False)
    nbytes = p.ns * p.rows * p.C * 2
    try:
        for limit in (nbytes, nbytes - 1):
            out = _Out(p.ns * p.rows, p.C)
            buf, n = _partial(p)
            stats = torch.empty(p.ns, 32, 2, dtype=F32, device=DEV)
            L.lkgd_debug_set_gn_small_limits(limit)
            assert L.lkgd_groupnorm_silu(*src, p.ns, p.rows, EPS, buf.data_ptr(), stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), 0,
                                         out.view.data_ptr(), out.view.stride(0), _stream()) == 0
            vec = npb.gn_small_vec(p.c0, 0, src[2], 0, out.view.stride(0), p.ns, p.rows, max_bytes=limit)
            assert bool(vec) == (limit == nbytes) and (_chunks_written(buf, n, p, "limits") == 0) == bool(vec)
            npb.worst(out.get("limits"), ref, bound, f"limit {limit}")
    finally:
        L.lkgd_debug_set_gn_small_limits(npb.GN_SMALL_MAX_BYTES)


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("C,segs", npb.GN_SEGMENTS, ids=[f"C{c}" for c, _ in npb.GN_SEGMENTS])
def test_groupnorm_apply_segments(C, segs, silu):
    """segments of unequal length (one shorter than an apply chunk, one of several chunks), sample != segment index"""
    from lkgd_amd import ops
    ns, rmax = 1 + max(s for _, s in segs), max(r for r, _ in segs)
    assert min(r for r, _ in segs) < npb.gn_apply_rows(C, rmax, len(segs)) < rmax
    p = npb.GnProbe(ns, rmax, C)
    st, ga, be = p.given()
    gref, gbound = p.given_ref(st, ga, be)
    if silu:
        gref, gbound = npb.silu_of_exact(gref)
    x = _inp(p.x, 24, col0=8)
    out = _Out(ns * rmax, C, pad=24, col0=8)
    table, live = [], torch.zeros(ns * rmax, dtype=torch.bool)
    for k, (rows, sample) in enumerate(segs):
        r0 = sample * rmax + (k % 2)               # the segment's rows inside its sample (their reference rows are r0 .. r0 + rows)
        rows = min(rows, rmax - (k % 2))
        assert not bool(live[r0:r0 + rows].any())
        live[r0:r0 + rows] = True
        table.append((x[r0:r0 + rows], out.view[r0:r0 + rows], sample))
    ops.groupnorm_apply_segments(table, st.to(DEV), ga.to(DEV), be.to(DEV), silu=silu)
    got = out.get("segments")
    assert bool((got[~live] == SENTINEL).all()), "rows outside the segments were written"
    _report("lkgd_groupnorm_apply_segments" + (" silu" if silu else ""), f"C={C}", npb.worst(got[live], gref[live], gbound[live], f"apply_segments C={C}"))


@pytest.mark.parametrize("case", npb.COLS_CASES, ids=str)
@pytest.mark.parametrize("as_sums", [1, 0])
def test_groupnorm_stats_cols(case, as_sums):
    L = _lib()
    cp = npb.ColsProbe(*case)
    S, Q = cp.group_sums()
    t0 = cp.tab[0].to(DEV)
    t1 = cp.tab[1].to(DEV) if cp.c1 else None
    out = torch.full((cp.ns + 1, 32, 2), NAN, dtype=F32, device=DEV)
    assert L.lkgd_groupnorm_stats_cols(t0.data_ptr(), cp.blk[0], cp.ld[0], cp.c0, t1.data_ptr() if cp.c1 else None, cp.blk[1], cp.ld[1],
                                       cp.c1, cp.ns, cp.rows, EPS, as_sums, out.data_ptr(), _stream()) == 0
    got = out.cpu()
    assert bool(torch.isnan(got[cp.ns:]).all())
    if as_sums:
        assert torch.equal(got[:cp.ns], torch.stack([S, Q], -1).to(F64).to(F32)), f"column sums {case}: not the exact sums"
        _report("lkgd_groupnorm_stats_cols[sums]", str(case), 0.0)
    else:
        _report("lkgd_groupnorm_stats_cols", str(case), npb.check_finalized(got[:cp.ns], S, Q, cp.rows * cp.gs, EPS, f"stats_cols {case}"))


@pytest.mark.parametrize("nparts,ns,part_pad,sample_pad", [(1, 1, 0, 0), (3, 2, 40, 16), (8, 5, 2, 6)])
def test_groupnorm_finalize_parts(nparts, ns, part_pad, sample_pad):
    from lkgd_amd import ops
    parts, ps, ss, S, Q, count = npb.parts_probe(nparts, ns, part_pad, sample_pad)
    got = ops.groupnorm_finalize_parts(parts.to(DEV), nparts, ps, ns, ss, count, EPS)
    _report("lkgd_groupnorm_finalize_parts", f"{nparts}x{ns}", npb.check_finalized(got, S, Q, count, EPS, "finalize_parts"))


# ================================================================================================== spatial norm
@pytest.mark.parametrize("C,sh,Tz,T", npb.SPATIAL_CASES)
def test_spatial_norm3d(C, sh, Tz, T):
    from lkgd_amd import ops
    from lkgd_amd.cogvideox_vae import spatial_norm_tmap
    sp = npb.SpatialProbe(C, sh, Tz, T)
    assert spatial_norm_tmap(Tz, T) == sp.tmap
    B, H, W = sp.B, sp.H, sp.W
    hw = H * W
    ref, bound = sp.ref()
    f, yb = _inp(sp.gn.x, 8, col0=8), _inp(sp.yb, 16)
    out = _Out(B * (T + 2) * hw, C, pad=8, col0=8)                  # behind two context frames per batch entry
    ops.spatial_norm3d(f, sp.stats.to(DEV), sp.gamma.to(DEV), sp.beta.to(DEV), yb, torch.tensor(sp.tmap, dtype=torch.int32).to(DEV),
                       out.view[2 * hw:], B, T, H, W, Tz, sh, False, out_batch_rows=(T + 2) * hw)
    got = out.get("spatial norm").reshape(B, T + 2, hw, C)
    assert bool((got[:, :2] == SENTINEL).all()), "the context frames were written"
    _report("lkgd_spatial_norm3d", f"C={C},sh={sh},({Tz},{T})", npb.worst(got[:, 2:].reshape(-1, C), ref, bound, "spatial_norm3d"))
    if (Tz, T) == (3, 5):                           # with SiLU, into a compact output
        sref, sbound = npb.silu_of_exact(ref)
        out = _Out(B * T * hw, C)
        ops.spatial_norm3d(f, sp.stats.to(DEV), sp.gamma.to(DEV), sp.beta.to(DEV), yb, torch.tensor(sp.tmap, dtype=torch.int32).to(DEV),
                           out.view, B, T, H, W, Tz, sh, True)
        _report("lkgd_spatial_norm3d silu", f"C={C},sh={sh},({Tz},{T})", npb.worst(out.get("spatial silu"), sref, sbound, "spatial silu"))


# ================================================================================================== LayerNorm
def _ln_run(p, x=None, **kw):
    from lkgd_amd import ops
    xd = _inp(p.x if x is None else x, 24, col0=8)
    out = _Out(p.T, p.C)
    ops.layernorm(xd, p.gamma.to(DEV) if p.gamma is not None else None, p.beta.to(DEV) if p.beta is not None else None, EPS,
                  out=out.view, **kw)
    return out.get("layernorm")


@pytest.mark.parametrize("C", npb.LN_CS)
def test_layernorm(C):
    from lkgd_amd import ops
    L_, NV = npb.ln_plan(C)
    w = 0.0
    probes = [npb.LnProbe("onehot", C, C, affine=True), npb.LnProbe("onehot", min(C, 4 * (64 // L_) + 1), C, affine=False)]
    probes += [npb.LnProbe("balanced", T, C, affine=a) for T in npb.ln_rows(C) for a in (True, False)]
    for p in probes:
        ref, bound = p.ref(EPS)
        w = max(w, npb.worst(_ln_run(p), ref, bound, f"layernorm {p.kind} T={p.T} C={C} affine={p.gamma is not None}"))
    # in place, with a row pitch larger than the width
    p = probes[0]
    ref, bound = p.ref(EPS)
    io = _Out(p.T, C)
    io.view.copy_(p.x.to(DEV))
    ops.layernorm(io.view, p.gamma.to(DEV), p.beta.to(DEV), EPS, out=io.view)
    w = max(w, npb.worst(io.get("in place"), ref, bound, f"layernorm in place C={C}"))
    # the row-bias table: (row // div) % mod, the biased row is the probe row
    p = npb.LnProbe("balanced", 4 * (64 // L_) + 1 + 20, C)
    ref, bound = p.ref(EPS)
    xp, table, _ = p.rowbias(5, 3)
    w = max(w, npb.worst(_ln_run(p, xp, rowbias=_inp(table, 8), rowmap=ops.rowmap_div_mod(5, 3)), ref, bound, f"layernorm row bias C={C}"))
    _report("lkgd_layernorm", f"C={C},L={L_},NV={NV}", w)


# ================================================================================================== row softmax
@pytest.mark.parametrize("cols", npb.SM_COLS)
def test_softmax_rows(cols):
    from lkgd_amd import ops
    w = 0.0
    for kind, rows in [(k, r) for k in ("uniform", "weighted") for r in npb.SM_ROWS] + [("onehot", 0)]:
        p = npb.SmProbe(kind, rows, cols)
        ref, bound = p.ref()
        whole, _ = npb.padded(p.x, 16, col0=8, fill=60000.0)        # a column read outside the row becomes its maximum
        out = _Out(p.rows, cols, pad=8, col0=8)
        ops.softmax_rows(whole.to(DEV)[:, 8:8 + cols], out.view)
        w = max(w, npb.worst(out.get("softmax"), ref, bound, f"softmax_rows {kind} {p.rows}x{cols}"))
    _report("lkgd_softmax_rows", f"cols={cols}", w)


def test_zz_worst_per_entry_point():
    """(runs last) the worst err / bound every entry point showed in this session"""
    for entry in sorted(WORST):
        print(f"PROBE WORST {entry} {WORST[entry]:.4f}")
    assert all(v <= 1.0 for v in WORST.values())
