"""The probes of tests/norm_probes.py without a GPU: an fp32 emulation of each kernel's arithmetic - written from norm.hip
(gn_stats_kernel / gn_finalize_kernel / gn_apply_kernel / gn_cols_kernel / gn_finalize_parts_kernel / layernorm_kernel), vae_ops.hip
(softmax_rows_kernel) and cogvae.hip (spatial_norm3d_kernel) - stays within HALF of every bound, and every fault the probes are
meant for is rejected.  Every test prints the emulation's worst err / bound (`EMU ...`, visible with -s)."""
import pytest
import torch

import norm_probes as npb
from norm_probes import F16, F32, F64

EPS = 1e-5


def _report(what, r):
    print(f"EMU {what} {r:.4f}")
    assert r <= 0.5, (what, r)


# ================================================================================================== emulations (norm.hip)
def emu_gn_sums(p, fault=None):
    """gn_stats_kernel + gn_sums_kernel: fp32 sums per (chunk, group), fp64 across the chunks; the float32 (sum, sumsq) [ns, 32, 2]
    and the fp64 pair.  Faults: the last row of the first chunk left out, the first row of the last chunk counted twice, the second
    source's channels read at the first source's column numbers"""
    x = p.x.to(F32).reshape(p.ns, p.rows, p.C)
    if fault == "second_source_at_first_offset":
        x = x.clone()
        x[:, :, p.c0:] = x[:, :, p.c0 + (torch.arange(p.c0, p.C) % p.c1)]        # x1[row, c] instead of x1[row, c - c0]
    rs = npb.gn_stats_rows(p.C, p.rows, p.ns)
    nch = (p.rows + rs - 1) // rs
    tot = torch.zeros(p.ns, 32, 2, dtype=F64)
    for ch in range(nch):
        r0, r1 = ch * rs, min((ch + 1) * rs, p.rows)
        rows = list(range(r0, r1))
        if fault == "drop_last_row" and ch == 0:
            rows = rows[:-1]
        if fault == "double_row" and ch == nch - 1:
            rows = rows + rows[:1]
        xs = x[:, rows].reshape(p.ns, len(rows), 32, p.gs)
        tot[..., 0] += xs.sum((1, 3), dtype=F32).to(F64)
        tot[..., 1] += (xs * xs).sum((1, 3), dtype=F32).to(F64)
    return tot.to(F32), tot


def emu_finalize(tot, count, eps):
    """gn_finalize_kernel: fp64, var = E[x^2] - mean^2, two float roundings"""
    inv = 1.0 / count
    mean = tot[..., 0] * inv
    var = (tot[..., 1] * inv - mean * mean).clamp(min=0.0)
    return torch.stack([mean.to(F32), (1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=F32)))).to(F32)], -1)


def _silu32(f):
    return f / (1.0 + torch.exp(-f))


def emu_gn_apply(p, stats, gamma, beta, silu):
    """gn_apply_kernel (= gn_apply_segments_kernel, gn_small_kernel's second half): A = rstd * gamma, B = beta - mean * A, x * A + B"""
    mean, rstd = p._per_channel(stats[..., 0]), p._per_channel(stats[..., 1])
    A = rstd * gamma
    B = beta - mean * A
    f = p.x.to(F32) * A + B
    return (_silu32(f) if silu else f).to(F16)


def emu_spatial(sp, src, silu=False):
    """spatial_norm3d_kernel: the arithmetic of gn_apply_kernel, then n * y + b, one rounding"""
    A = sp.gn._per_channel(sp.stats[..., 1]) * sp.gamma
    n = sp.gn.x.to(F32) * A + (sp.beta - sp.gn._per_channel(sp.stats[..., 0]) * A)
    yb = sp.yb.to(F32)
    f = n * yb[src, :sp.C] + yb[src, sp.C:]
    return (_silu32(f) if silu else f).to(F16)


def emu_layernorm(p, eps, fault=None):
    """layernorm_kernel<L, AFF, NV>: lane li holds the vectors li + L v; per-lane sums in (v, e) order, xor butterfly, mean =
    s * (1 / C), sum of (x - mean)^2 likewise, rsqrt.  Faults: the last channel left out of both sums; the clamped lanes' vector
    (C/8 - 1, as the gamma load clamps it) added in"""
    L, NV = npb.ln_plan(p.C)
    C8 = p.C // 8
    T = p.T
    x = p.x.to(F32)
    xv = torch.zeros(T, NV, L, 8, dtype=F32)
    live = torch.zeros(NV, L, dtype=torch.bool)
    for v in range(NV):
        for li in range(L):
            cv = li + L * v
            if cv < C8:
                live[v, li] = True
                xv[:, v, li] = x[:, cv * 8:cv * 8 + 8]
            elif fault == "clamped_added":
                xv[:, v, li] = x[:, (C8 - 1) * 8:C8 * 8]
    counted = live.clone()
    if fault == "clamped_added":
        counted[:] = True
    counted = counted[:, :, None].repeat(1, 1, 8)
    if fault == "drop_channel":
        counted[(C8 - 1) // L, (C8 - 1) % L, 7] = False

    def lanes(val):
        acc = torch.zeros(T, L, dtype=F32)
        for v in range(NV):
            for e in range(8):
                acc = acc + val[:, v, :, e] * counted[v, :, e].to(F32)
        o = L // 2
        while o > 0:
            acc = acc + acc[:, torch.arange(L) ^ o]
            o >>= 1
        return acc[:, :1]
    invC = torch.tensor(1.0, dtype=F32) / torch.tensor(float(p.C), dtype=F32)
    mean = lanes(xv) * invC
    d = xv - mean[:, None, :, None]
    q = lanes(d * d)
    rstd = (1.0 / torch.sqrt((q * invC + torch.tensor(eps, dtype=F32)).to(F64))).to(F32)
    y = (x - mean) * rstd
    if p.gamma is not None:
        y = y * p.gamma + p.beta
    return y.to(F16)


def emu_softmax(p, fault=None):
    """softmax_rows_kernel: fp32 max, p = exp2(fma(x, log2e, -max * log2e)), fp32 sum of the UNROUNDED p, p kept as fp16, times
    1 / sum, rounded.  Fault: vector slot i = 7 left out of max and sum (its columns are still normalised)"""
    x = p.x.to(F32)
    cols = torch.arange(p.cols)
    seen = torch.ones(p.cols, dtype=torch.bool) if fault is None else (cols // 8) // npb.SM_NT != 7
    log2e = torch.tensor(1.4426950408889634, dtype=F32)
    mx = x[:, seen].max(1, keepdim=True).values
    mb = mx * log2e
    arg = (x.to(F64) * log2e.to(F64) - mb.to(F64)).to(F32)                     # fmaf: one rounding
    pr = torch.exp2(arg.to(F64)).to(F32)
    inv = torch.tensor(1.0, dtype=F32) / pr[:, seen].sum(1, keepdim=True, dtype=F32)
    return (pr.to(F16).to(F32) * inv).to(F16)


# ================================================================================================== GroupNorm
EMU_GN = [(2, 100, 64, None), (3, 77, 320, 8), (2, 64, 1920, None), (1, 50, 2560, None), (1, 523, 1280, None), (3, 65, 32, None),
          (2, 10, 2080, None)]


@pytest.mark.parametrize("ns,rows,C,c0", EMU_GN)
def test_groupnorm_emulation_uses_half_the_bounds(ns, rows, C, c0):
    p = npb.GnProbe(ns, rows, C, c0)
    sums, tot = emu_gn_sums(p)
    p.check_sums(sums)
    stats = emu_finalize(tot, rows * p.gs, EPS)
    _report(f"gn stats {ns}x{rows}x{C}", p.check_stats(stats, EPS))
    gamma, beta = p.affine()
    for silu in (False, True):
        ref, bound = p.out_ref(gamma, beta, EPS, silu)
        _report(f"gn out silu={silu} {ns}x{rows}x{C}", npb.worst(emu_gn_apply(p, stats, gamma, beta, silu), ref, bound, "gn out"))
    st, ga, be = p.given()
    ref, bound = p.given_ref(st, ga, be)
    got = emu_gn_apply(p, st, ga, be, False)
    assert torch.equal(got, ref.to(F16))                                      # exact: the reference rounded once
    _report(f"gn given {ns}x{rows}x{C}", npb.worst(got, ref, bound, "gn given"))
    sref, sbound = npb.silu_of_exact(ref)
    _report(f"gn given silu {ns}x{rows}x{C}", npb.worst(emu_gn_apply(p, st, ga, be, True), sref, sbound, "gn given silu"))


def test_every_groupnorm_case_builds_and_names_its_path():
    """the case tables reach every path: one and two slots, a ragged second slot, every access width of gn_small_kernel, its refusals"""
    vecs, slots = set(), set()
    for ns, rows, C, c0, why in npb.GN_CASES:
        c0_ = C if c0 is None else c0
        vecs.add((npb.gn_small_vec(c0_, C - c0_, c0_ + 8, C - c0_ + 8, C + 16, ns, rows), (C // 32)))
        slots.add(npb.gn_map(C)[2])
        assert ns * rows * C * 2 <= 9 * 1024 * 1024, why
    assert slots == {1, 2}
    assert {v for v, _ in vecs} == {0, 2, 4, 8}
    assert (0, 1) in vecs and (0, 3) in vecs and (0, 65) in vecs              # C = 32, 96, 2080: no vector width divides the group
    assert {(2, 2), (4, 4), (8, 8)} <= vecs                                   # one access per row: C = 64, 128, 256
    assert npb.gn_small_vec(256, 0, 264, 0, 272, 2, 3072) == 8 and npb.gn_small_vec(256, 0, 264, 0, 272, 2, 3073) == 0
    assert npb.gn_chunks(64, 2400, 28) <= npb.gn_chunks_bound(64, 2400)       # longer chunks never overrun the caller's scratch
    for ns, rows, C, c0, why in npb.GN_CASES:                                 # every builder assertion holds: exact partials,
        p = npb.GnProbe(ns, rows, C, c0)                                      # x != 0, adjacent (m, a) differ, |mean| <= 4 std
        assert p.x.shape == (ns * rows, C), why


@pytest.mark.parametrize("ns,rows,C,c0", [(3, 77, 320, 8), (3, 100, 1280, 648)])
def test_groupnorm_faults_are_rejected(ns, rows, C, c0):
    p = npb.GnProbe(ns, rows, C, c0)
    sums, tot = emu_gn_sums(p)
    stats = emu_finalize(tot, rows * p.gs, EPS)
    gamma, beta = p.affine()
    ref, bound = p.out_ref(gamma, beta, EPS, False)
    st, ga, be = p.given()
    gref, gbound = p.given_ref(st, ga, be)
    for d in (1, -1):
        for shift, name in ((npb.shift_groups, "group"), (npb.shift_samples, "sample")):
            rej = npb.rejected(emu_gn_apply(p, shift(stats, d), gamma, beta, False), ref, bound)
            print(f"FAULT statistics of {name} {d:+d}: {100 * rej:.2f} % of the elements rejected")
            assert rej > 0.995, (name, d, rej)
            assert npb.rejected(emu_gn_apply(p, shift(st, d), ga, be, False), gref, gbound) > 0.9, (name, d)
    for fault in ("drop_last_row", "double_row", "second_source_at_first_offset"):
        bad, _ = emu_gn_sums(p, fault)
        with pytest.raises(AssertionError, match="differ from the exact"):
            p.check_sums(bad)
        wrong = (bad != p.sums_ref())[..., 1]
        assert bool(wrong.all()) if fault != "second_source_at_first_offset" else bool(wrong.any()), fault   # sum(x^2) of EVERY group


@pytest.mark.parametrize("case", npb.COLS_CASES, ids=str)
def test_column_sum_tables(case):
    """gn_cols_kernel on integer tables: fp64 sums are exact; a straddling group clipped to one source, or the second source read
    at the first source's channel numbers, changes the sums"""
    cp = npb.ColsProbe(*case)
    S, Q = cp.group_sums()
    tot = torch.stack([S, Q], -1).to(F64)
    _report(f"cols stats {case}", npb.check_finalized(emu_finalize(tot, cp.rows * cp.gs, EPS), S, Q, cp.rows * cp.gs, EPS, "cols"))
    if cp.c1:
        S2, Q2 = cp.group_sums(second_at_first_offset=True)
        assert not torch.equal(Q2, Q)
        with pytest.raises(AssertionError):
            npb.check_finalized(emu_finalize(torch.stack([S2, Q2], -1).to(F64), cp.rows * cp.gs, EPS), S, Q, cp.rows * cp.gs, EPS, "x")
    if cp.straddles():
        S1, Q1 = cp.group_sums(clip_to_first=True)
        g = cp.c0 // cp.gs
        assert bool((Q1[:, g] != Q[:, g]).all()) and torch.equal(Q1[:, :g], Q[:, :g])
        with pytest.raises(AssertionError):
            npb.check_finalized(emu_finalize(torch.stack([S1, Q1], -1).to(F64), cp.rows * cp.gs, EPS), S, Q, cp.rows * cp.gs, EPS, "x")
    assert any(npb.ColsProbe(*c).straddles() for c in npb.COLS_CASES)


def test_rank_parts():
    parts, ps, ss, S, Q, count = npb.parts_probe(3, 2, 40, 16)
    live = parts.view(3, ps)[:, :2 * ss].reshape(3, 2, ss)[:, :, :64].to(F64)
    tot = torch.stack([live[..., 0::2].sum(0), live[..., 1::2].sum(0)], -1)
    _report("parts stats", npb.check_finalized(emu_finalize(tot, count, EPS), S, Q, count, EPS, "parts"))
    with pytest.raises(AssertionError):                                       # a rank left out
        npb.check_finalized(emu_finalize(tot - torch.stack([live[0, ..., 0::2], live[0, ..., 1::2]], -1), count, EPS), S, Q, count, EPS, "x")


# ================================================================================================== spatial norm
@pytest.mark.parametrize("C,sh,Tz,T", [(64, 0, 3, 5), (128, 1, 2, 8), (384, 3, 3, 9), (64, 1, 3, 5)])
def test_spatial_norm_emulation_and_faults(C, sh, Tz, T):
    sp = npb.SpatialProbe(C, sh, Tz, T)
    ref, bound = sp.ref()
    got = emu_spatial(sp, sp.src())
    assert torch.equal(got, ref.to(F16))
    _report(f"spatial C={C} sh={sh} ({Tz}, {T})", npb.worst(got, ref, bound, "spatial"))
    sref, sbound = npb.silu_of_exact(ref)
    _report(f"spatial silu C={C} sh={sh} ({Tz}, {T})", npb.worst(emu_spatial(sp, sp.src(), True), sref, sbound, "spatial silu"))
    faults = {"tmap ignored": sp.src(tmap=[0] * T), "tmap off by one": sp.src(tmap=[min(t + 1, Tz - 1) for t in sp.tmap]),
              "Tz / T confused": sp.src(frames=T)}
    if sh:
        faults["latent pixel without the shift"] = sp.src(shift=0)
        faults["Y >> sh rounded up at the cell border"] = sp.src()     # replaced below
        B, H, W = sp.B, sp.H, sp.W
        h, w = H >> sh, W >> sh
        b, t, Y, X = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
        up = (((b * Tz + torch.tensor(sp.tmap)[t]) * h + ((Y + 1) >> sh).clamp(max=h - 1)) * w + (X >> sh)).reshape(-1)
        faults["Y >> sh rounded up at the cell border"] = up
    for name, src in faults.items():
        moved = src != sp.src()
        if not bool(moved.any()):
            continue
        r = npb.ratio(emu_spatial(sp, src), ref, bound)
        bad_rows = (r > 1).any(1)
        assert torch.equal(bad_rows, moved), name                       # an O(1) error on exactly the pixels concerned
        print(f"FAULT spatial {name}: {int(moved.sum())} rows moved, all rejected, no other")
    for d, shift in ((1, npb.shift_groups), (1, npb.shift_samples)):
        keep = sp.stats
        sp.stats = shift(keep, d)
        rej = npb.rejected(emu_spatial(sp, sp.src()), ref, bound)
        sp.stats = keep
        assert rej > 0.9, rej


# ================================================================================================== LayerNorm
@pytest.mark.parametrize("C", npb.LN_CS)
def test_layernorm_emulation_uses_half_the_bounds(C):
    probes = [npb.LnProbe("onehot", C, C, affine=True), npb.LnProbe("onehot", min(C, 64), C, affine=False)]
    probes += [npb.LnProbe("balanced", T, C, affine=a) for T in npb.ln_rows(C) for a in (True, False)]
    w = 0.0
    for p in probes:
        ref, bound = p.ref(EPS)
        w = max(w, npb.worst(emu_layernorm(p, EPS), ref, bound, f"layernorm {p.kind} T={p.T} C={C}"))
    _report(f"layernorm C={C} (L, NV)={npb.ln_plan(C)}", w)


@pytest.mark.parametrize("C", [64, 72, 104, 328, 1544, 2056, 3072])
def test_layernorm_faults_are_rejected(C):
    L, NV = npb.ln_plan(C)
    p = npb.LnProbe("onehot", C, C)
    ref, bound = p.ref(EPS)
    r = npb.ratio(emu_layernorm(p, EPS, "drop_channel"), ref, bound)
    assert bool((r > 1).any(1).all())                                          # a channel left out: rejected on EVERY row
    if C // 8 < L * NV:                                                        # the dispatch leaves clamped lanes
        assert bool((npb.ratio(emu_layernorm(p, EPS, "clamped_added"), ref, bound) > 1).any(1).all()), "clamped lane added in"
    q = npb.LnProbe("balanced", 37, C)                                         # (m, a) of the neighbouring row: every row rejects
    qref, qbound = q.ref(EPS)
    assert bool((npb.ratio(emu_layernorm(q, EPS).roll(1, 0), qref, qbound) > 1).any(1).all())


def test_layernorm_rowbias_rebuilds_the_probe_row():
    p = npb.LnProbe("balanced", 61, 328)
    xp, table, idx = p.rowbias(10, 3)
    assert torch.equal((xp + table[idx]), p.x) and len(set(idx.tolist())) == 3


# ================================================================================================== row softmax
@pytest.mark.parametrize("cols", npb.SM_COLS)
def test_softmax_emulation_and_faults(cols):
    w = 0.0
    for kind, rows in (("uniform", 5), ("weighted", 5), ("weighted", 1), ("onehot", 0)):
        p = npb.SmProbe(kind, rows, cols)
        ref, bound = p.ref()
        w = max(w, npb.worst(emu_softmax(p), ref, bound, f"softmax {kind} cols={cols}"))
        if cols > 7 * npb.SM_NT * 8:                                           # slot i = 7 exists: left out of the sums
            r = npb.ratio(emu_softmax(p, "drop_slot"), ref, bound)
            assert bool((r > 1).any(1).all()) if kind != "onehot" else bool((r > 1).any()), kind
    _report(f"softmax cols={cols}", w)
    hot = npb.sm_hot_columns(cols)
    assert cols - 1 in hot
    if cols >= 2048:
        assert {(c // 8) % npb.SM_NT for c in hot} == set(range(npb.SM_NT))    # every thread
    if cols == 16384:
        assert {(c // 8) // npb.SM_NT for c in hot} == set(range(8))           # every vector slot
