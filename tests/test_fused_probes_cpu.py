"""The probes of tests/fused_probes.py without a GPU: for every launch of tests/test_fused_probes_gpu.py the fp32 emulation of the kernel
stays inside half of the bound (and is bit for bit the reference for ln_qkv), and each fault the probes exist for, put into the
emulation, is rejected: the low half of the bias dropped, a channel or one lane's 8-channel vector left out of the row sums, a
later panel normalised with the previous panel's statistics, the row-bias row off by one at a boundary, hidden tile f0 multiplied
with gate tile f1, the W2 k-slots in plain order, res2 in the store layout, a clamped dead row stored over the last live one with
another row's data, tanh-GELU.  A fault's test stays only while >= 99 % of the cases it applies to reject it."""
import pytest
import torch

import attn_probes as ap
import fused_probes as fp

CUS = fp.NOMINAL_CUS
FF_CASES = fp.ff_cases(CUS)
QKV_CASES = fp.qkv_cases(CUS)


# ================================================================================================== rows, maps, the GELU term
@pytest.mark.parametrize("C", [320, 640])
def test_rows_normalise_to_z_exactly(C):
    rows = fp.rows_of(C)
    z, mean, sigma = fp.ln_emulate(rows.xp)
    assert torch.equal(z, rows.z) and not mean.any()
    assert torch.unique(rows.z, dim=0).shape[0] == rows.n
    a = rows.amp
    assert ((sigma - torch.sqrt(a * a + fp.EPS)).abs() <= 2.0 ** -22 * a).all()
    for v in (0.5, 1.0, 2.0, 4.0):
        assert (a == v).sum() > rows.n // 8


def test_rows_are_the_construction_of_the_fused_attention_probe():
    """attn_probes.FusedProbe's rows (a z, sum z = 0, a in 1/2 .. 4) go through the same emulated LayerNorm to exactly z"""
    p = ap.fused_probe("uniform", 1, 7, 3)
    z, mean, _ = fp.ln_emulate(p.x.double())
    assert torch.equal(z, p.z) and not mean.any()
    assert set(p.amp.tolist()) <= set(fp.rows_of(320).amp.tolist())


@pytest.mark.parametrize("cus", [8, 255, 256, 304])
def test_source_map_shares_no_row_inside_a_workgroups_reach(cus):
    T = fp.many_panels_T(cus)
    src = fp.source_map(T, cus)
    assert src.max() < fp.NSRC and (T + fp.PANEL - 1) // fp.PANEL == 2 * cus + 2 and T % fp.PANEL == 5
    pad = torch.full((-T % fp.PANEL,), -1)
    pan = torch.cat([src, pad]).reshape(-1, fp.PANEL)
    for p in range(pan.shape[0]):
        for q in (p, p + 1, p + cus, p + 2 * cus):
            if q < pan.shape[0]:
                both = torch.cat([pan[p], pan[q]]) if q != p else pan[p]
                both = both[both >= 0]
                assert torch.unique(both).numel() == both.numel(), (p, q)
        assert torch.unique(pan[p][pan[p] >= 0] % fp.PANEL).numel() == (pan[p] >= 0).sum()          # all 128 low code patterns


def test_gelu_term_is_the_measured_one():
    """the approximation term of the curve bound is measured here, not chosen: the fp32 chain against fp64 on the grid"""
    x = fp.GRID
    ref = fp.gelu64(x)
    for form in ("asm", "erf2"):
        err = (fp.gelu_chain(x, form) - ref).abs()
        rel = (err[x != 0] / x[x != 0].abs()).max().item()
        print(f"GELU {form}: max abs {err.max().item():.3e}, max / |gate| {rel:.3e}")
        assert err.max().item() <= fp.GELU_ABS and rel <= fp.GELU_REL
        if form == "asm":           # the constants are this chain's figures, not a round number above them
            assert err.max().item() >= 0.9 * fp.GELU_ABS and rel >= 0.9 * fp.GELU_REL
        assert (err <= fp.gelu_term(x) / 2).all()
    err = (fp.gelu_chain(x, "erff") - ref).abs()
    assert (err <= fp.gelu_term(x, "erff") / 2).all()
    # the switch probe's two points: gelu(8) = 8 exactly; gelu(-8) * hidden flushes to zero at the fp16 pack
    ends = fp.gelu_chain(torch.tensor([8.0, -8.0], dtype=torch.float64))
    assert ends[0] == 8.0 and -1e-14 < ends[1] < 0 and fp.r16(ends[1:] * 256) == 0
    for form in ("erf2", "erff"):
        ends = fp.gelu_chain(torch.tensor([8.0, -8.0], dtype=torch.float64), form)
        assert ends[0] == 8.0 and fp.r16(ends[1:] * 256) == 0


def test_curve_probe_covers_the_grid_on_every_hidden_channel():
    seen = []
    values = set()
    for v in range(fp.CURVE_VARIANTS):
        p = fp.ff_probe("curve", v)
        assert (p.grid_coverage() == 128).all()
        seen.append(p.sel)
        values |= set(p.gate[:fp.PANEL, p.sel[0]].tolist())
        assert set(p.hidden[:, p.sel].unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}
    for half in (seen[:4], seen[4:]):
        assert torch.equal(torch.cat(half).sort().values, torch.arange(fp.FF_INNER))       # all 40 tiles x 16 registers x 2 half-waves
    assert values == set(fp.GRID.tolist())                                                  # 0, +-1/8, ..., +-8
    assert any(c.kind == "curve" and c.T >= fp.PANEL for c in FF_CASES)
    ran = {c.variant for c in FF_CASES if c.kind == "curve" and c.T >= fp.PANEL}
    assert ran == set(range(fp.CURVE_VARIANTS))


# ================================================================================================== A. ln_qkv
@pytest.mark.parametrize("C", [320, 640])
@pytest.mark.parametrize("kind", ["dense", "select"])
def test_qkv_emulation_is_the_reference_bit_for_bit(kind, C):
    p = fp.qkv_probe(kind, C)
    fp.first_mismatch(p.emulate(), p.ref16, f"{kind} C={C}")
    if kind == "dense":
        print(f"QKV dense C={C}: max |W z| = {p.max_wz}")
        assert p.max_wz < 256


def _late_rows(T, grid):
    """a sample of rows of the panels a workgroup runs after its first: the first and last 40 of them, and the ragged tail"""
    first = fp.PANEL * grid
    if T <= first:
        return None
    rows = torch.arange(first, T)
    return torch.unique(torch.cat([rows[:40], rows[fp.PANEL * grid:fp.PANEL * grid + 40], rows[-40:]])) if rows.numel() > 120 else rows


@pytest.mark.parametrize("C", [320, 640])
@pytest.mark.parametrize("kind", ["dense", "select"])
def test_qkv_faults_are_rejected(kind, C):
    p = fp.qkv_probe(kind, C)
    ref = p.ref16
    cases = [c for c in QKV_CASES if c[0] == kind and c[1] == C]
    assert len(cases) == len(fp.T_SMALL) + 1
    tally = {}

    def count(fault, hit):
        n, k = tally.get(fault, (0, 0))
        tally[fault] = (n + 1, k + bool(hit))

    skipped = {name: p.emulate(skip=m) for name, m in fp.stat_skips(C).items()}
    no_lo = p.emulate(drop_b_lo=True)
    if kind == "dense":          # a dropped channel: every row, most elements
        changed = skipped["channel"] != ref
        print(f"QKV dense C={C}: a channel left out of the sums changes {changed.float().mean().item():.1%} of the elements")
        assert changed.any(1).all() and changed.float().mean() > 0.75          # (one channel of 640 moves z half as far as one of 320)
    for _, _, T, grid, _, _ in cases:
        src = fp.source_map(T, grid)
        for name, emu in skipped.items():
            count(name, (emu[src] != ref[src]).any())
        if kind == "select":
            count("b_lo", (no_lo[src] != ref[src]).any())
        if T % 32 and T > 1:       # a dead lane's row (clamped to T - 1) arrives with another row's data
            count("dead row", (ref[src[T - 2]] != ref[src[T - 1]]).any())
        late = _late_rows(T, grid)
        if late is not None:       # the later-panel LayerNorm takes (mean, rstd) of the panel before
            emu = p.emulate(xp=p.rows.xp[src[late]], stat_rows=p.rows.xp[src[late - fp.PANEL * grid]])
            count("previous panel's statistics", (emu != ref[src[late]]).any())
    print(f"QKV {kind} C={C} faults (cases, rejected): {tally}")
    assert set(tally) >= {"channel", "vector", "dead row", "previous panel's statistics"} | ({"b_lo"} if kind == "select" else set())
    for fault, (n, k) in tally.items():
        assert k >= 0.99 * n, f"{fault}: rejected by {k} of {n} cases"


# ================================================================================================== B. ff_fused
def _ff_id(c):
    return c.id


@pytest.mark.parametrize("case", FF_CASES, ids=_ff_id)
def test_ff_emulation_within_half_of_the_bound(case):
    p, form = case.probe, case.form
    ref, bound = p.ref(form), p.bound(form)
    src = case.src
    used = torch.unique(src)
    ratio = fp.check_bound(p.emulate_sources(form)[used], ref[used], bound[used], f"emulation, {case.id}", limit=0.5)
    print(f"EMU ff_fused {case.id} {ratio:.4f}")
    x = case.x()                                     # asserts that a z - pe is an fp16 matrix
    assert x.shape == (case.T, fp.FF_C)
    if form.rb:
        d1, md = form.rb
        assert int(case.idx.max()) < md and (case.T <= d1 or md == 1 or case.idx.unique().numel() > 1)
    if form.r2:
        r = case.res2_rows()
        assert (r.double() == p.res2(form)[src]).all()


def _ff_faults(case, count):
    """every fault that applies to the case: count(fault, rejected)"""
    p, form, T = case.probe, case.form, case.T
    ref, bound = p.ref(form), p.bound(form)
    src = case.src
    used = torch.unique(src)
    for fault in fp.FF_FAULTS:
        if fault == "res2_unswapped" and not form.r2 or fault == "tanh" and p.kind != "curve":
            continue
        if fault == "tanh" and T < 31:
            continue            # one row meets one gate per channel: below 31 rows the tanh form's deviations need not be met
        count(fault, fp.rejected(p.emulate_sources(form, fault)[used], ref[used], bound[used]))
    if T % 32 and T > 1:        # a dead lane's row (clamped to T - 1) arrives with another row's data
        good = p.emulate_sources(form)
        count("dead row", fp.rejected(good[src[T - 2]][None], ref[src[T - 1]][None], bound[src[T - 1]][None]))
    late = _late_rows(T, case.grid)
    if late is not None:
        emu = p.emulate(form, xp=p.rows.xp[src[late]], stat_rows=p.rows.xp[src[late - fp.PANEL * case.grid]],
                        res2=p.res2(form)[src[late]] if form.r2 else None)
        count("previous panel's statistics", fp.rejected(emu, ref[src[late]], bound[src[late]]))
    if form.rb and form.rb[1] > 1 and T > form.rb[0]:
        d1, md = form.rb
        edge = torch.arange(d1, T, d1)[:48]                              # the first row behind a boundary takes the row before's entry
        pe = fp.pe_table(md)
        xp = p.rows.xp[src[edge]] - pe[case.idx[edge]] + pe[case.idx[edge - 1]]
        emu = p.emulate(form, xp=xp, res2=p.res2(form)[src[edge]] if form.r2 else None)
        count("row-bias row off by one", fp.rejected(emu, ref[src[edge]], bound[src[edge]]))


@pytest.mark.parametrize("kind", ["switch", "curve"])
def test_ff_faults_are_rejected(kind):
    tally = {}
    for case in FF_CASES:
        if case.kind == kind:
            _ff_faults(case, lambda fault, hit, case=case: tally.setdefault(fault, []).append((case.id, bool(hit))))
    want = (set(fp.FF_FAULTS) - ({"tanh"} if kind == "switch" else set())) | {"dead row", "previous panel's statistics", "row-bias row off by one"}
    assert set(tally) == want, want ^ set(tally)
    for fault, hits in tally.items():
        n, k = len(hits), sum(h for _, h in hits)
        print(f"FF {kind} fault {fault}: rejected by {k} of {n} cases")
        assert k >= 0.99 * n, f"{fault}: rejected by {k} of {n} cases; missed by {[i for i, h in hits if not h][:5]}"


# ================================================================================================== the GEGLU epilogue of ops.gemm
@pytest.mark.parametrize("M,half,program,form", fp.GEGLU_GEMM)
def test_geglu_gemm_emulation_and_plan(M, half, program, form):
    from lkgd_amd import ops
    e = torch.empty
    plan = ops.gemm_plan(e(M, 320, dtype=torch.float16), e(2560, 320, dtype=torch.float16), e(M, 1280, dtype=torch.float16), cus=CUS,
                         M=M, N=2560, K=320, bias=e(2560), geglu=half)
    assert plan.program == program, f"planned program {plan.program}: the bound is derived for {program} ({form})"
    sw = fp.ff_probe("switch")
    assert torch.equal(sw.geglu_emulate(form)[:M], fp.r16(8 * sw.hidden * (sw.gate > 0))[:M])
    for v in (0, 4):
        cv = fp.ff_probe("curve", v)
        ratio = fp.check_bound(cv.geglu_emulate(form)[:M], cv.g[:M], cv.geglu_bound(form)[:M], f"geglu emulation {form}", limit=0.5)
        print(f"EMU geglu {form} curve{v} {ratio:.4f}")
        assert fp.rejected(cv.geglu_emulate(form, tanh=True)[:M], cv.g[:M], cv.geglu_bound(form)[:M])
