"""lkgd_ln_qkv_c320 / _c640 and lkgd_ff_fused_c320 (all four forms) on the probes of tests/fused_probes.py:

  ln_qkv    dense and selection probe: the output is the int64 / exact reference BIT FOR BIT
  ff_fused  switch probe (every gate +-8: g is 8 hidden or 0, y exact) and curve probe (one g per output, gates on a grid of 1/8 over
            [-8, 8]) per element against fp64 within the bounds derived in fused_probes.py
  ops.gemm  the GEGLU epilogue on the same two probes (the 128x128 and the 256x320 program, asserted through ops.gemm_plan)

Rows: 1, 31, 32, 33, 127, 128, 129, 901, and 128 (2 CUs + 1) + 5 - workgroup 0 runs three panels, the others two, the last one
ragged: the later-panel LayerNorm and the prefetch of the next panel's rows.  x, out and res2 sit inside larger buffers (guard rows
above and below, guard columns where the pitch exceeds the width) whose sentinels must survive; out is pre-filled with NaN; every
launch runs twice and must give the same bits.  That the probes reject the faults they exist for is shown without a GPU in
test_fused_probes_cpu.py.  Every case prints the worst err / bound it saw (`PROBE ...`, visible with -s)."""
import pytest
import torch

import fused_probes as fp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
SENTINEL = 7.0

FF_SMALL = [c for c in fp.ff_cases() if c.T <= fp.NSRC]            # (these do not depend on the CU count)
QKV_SMALL = [c for c in fp.qkv_cases() if c[2] <= fp.NSRC]
_dev_cache = {}


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _once(key, make):
    if key not in _dev_cache:
        _dev_cache[key] = make()
    return _dev_cache[key]


class _Guarded:
    """a [T, width] fp16 view inside a [T + 2, ld (+ 8)] buffer of sentinels: a guard row above and below, guard columns on the
    right where ld > width and, then, 8 on the left as well (the view starts 16 bytes into its row)"""

    def __init__(self, T, width, ld, rows=None, fill=NAN):
        left = 8 if ld > width else 0
        assert ld % 8 == 0 and ld >= width + left
        self.buf = torch.full((T + 2, ld), SENTINEL, dtype=torch.float16, device=DEV)
        self.view = self.buf[1:T + 1, left:left + width]
        if rows is None:
            self.view.fill_(fill)
        else:
            self.view.copy_(rows)

    def assert_guards(self, what):
        inside = torch.zeros_like(self.buf, dtype=torch.bool)
        inside[1:-1, self.view.storage_offset() % self.buf.shape[1]:][:, :self.view.shape[1]] = True
        assert bool(((self.buf == SENTINEL) | inside).all()), f"{what}: a guard row or column was written"


def _twice(launch, T, width, ld, what):
    """two launches into fresh NaN-filled guarded buffers: the same bits, the guards intact; returns the first output (a view)"""
    outs = []
    for _ in range(2):
        o = _Guarded(T, width, ld)
        launch(o.view)
        torch.cuda.synchronize()
        o.assert_guards(what)
        outs.append(o.view)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{what}: a second launch gives other bits"
    return outs[0]


# ================================================================================================== A. ln_qkv
def _run_qkv(kind, C, T, grid, ldx, ldo):
    from lkgd_amd import ops
    from lkgd_amd.packing import pack_ln_proj
    p = fp.qkv_probe(kind, C)
    ws = _once(("qkv-ws", kind, C), lambda: pack_ln_proj(p.w.float(), p.b.float()).to(DEV))
    xsrc = _once(("qkv-x", C), lambda: p.rows.xp.half().to(DEV))
    ref = _once(("qkv-ref", kind, C), lambda: p.ref16.to(DEV))
    src = fp.source_map(T, grid).to(DEV)
    x = _Guarded(T, C, ldx, xsrc[src])
    what = f"ln_qkv {kind} C={C} T={T} ldx={ldx} ldo={ldo}"
    out = _twice(lambda o: ops.ln_qkv(x.view, ws, o), T, 3 * C, ldo, what)
    x.assert_guards(what + " (x)")
    fp.first_mismatch(out, ref[src], what, row_of=lambda r: f" (source row {int(src[r])}, panel {r // fp.PANEL})")
    print(f"PROBE ln_qkv_c{C} {kind} T={T} exact")


@pytest.mark.parametrize("kind,C,T,grid,ldx,ldo", QKV_SMALL, ids=[f"{c[0]}-C{c[1]}-T{c[2]}" for c in QKV_SMALL])
def test_ln_qkv(kind, C, T, grid, ldx, ldo):
    """one lane, clamped half-waves, ragged and full panels; at T = 129 and 901 x with ldx > C and out as columns of a wider buffer"""
    _run_qkv(kind, C, T, grid, ldx, ldo)


@pytest.mark.parametrize("C", [320, 640])
@pytest.mark.parametrize("kind", ["dense", "select"])
def test_ln_qkv_two_and_three_panels_per_workgroup(kind, C):
    """128 (2 CUs + 1) + 5 rows: the later-panel LayerNorm, the statement's fetch of the next panel's rows, a ragged last panel;
    every row is checked"""
    cus = _cus()
    big = [c for c in fp.qkv_cases(cus) if c[0] == kind and c[1] == C and c[2] > fp.NSRC]
    assert len(big) == 1 and big[0][2] == fp.many_panels_T(cus)
    _run_qkv(*big[0])


# ================================================================================================== B. ff_fused
def _run_ff(case):
    from lkgd_amd import ops
    from lkgd_amd.packing import pack_ff_fused
    p, form, T = case.probe, case.form, case.T
    ws = _once(("ff-ws", p.kind, p.variant), lambda: pack_ff_fused(p.w1.float(), p.b1.float(), p.w2.float()).to(DEV))
    b2 = _once(("ff-b2", p.kind, p.variant), lambda: p.b2.float().to(DEV))
    x = _Guarded(T, fp.FF_C, case.ldx, case.x().to(DEV))
    kw = dict(s_acc=form.s_acc)
    guards = [x]
    if form.rb:
        d1, md = form.rb
        table = _Guarded(md, fp.FF_C, fp.FF_C + 16, fp.pe_table(md).half().to(DEV))
        guards.append(table)
        kw.update(rowbias=table.view, rowmap=(d1, 1, 1, md))
    if form.r2:
        res2 = _Guarded(T, fp.FF_C, case.ldr2, case.res2_rows().to(DEV))
        guards.append(res2)
        kw.update(res2=res2.view, r2=form.r2v)
    what = f"ff_fused {case.id}"
    out = _twice(lambda o: ops.ff_fused(x.view, ws, b2, o, **kw), T, fp.FF_C, case.ldo, what)
    for gd in guards:
        gd.assert_guards(what + " (an input)")
    ratio = fp.check_rows(out.cpu(), p.ref(form), p.bound(form), case.src, what)
    print(f"PROBE ff_fused {form.name} {p.kind}{p.variant} T={T} {form!r} {ratio:.4f}")
    return ratio


@pytest.mark.parametrize("case", FF_SMALL, ids=[c.id for c in FF_SMALL])
def test_ff_fused(case):
    """plain, row bias, second residual and both, on the switch and the curve probe; row maps with a boundary inside a wave (50), on
    a panel border (128) and beyond the rows (4096), tables of 1, 3 and 14 rows; s_acc and r2 powers of two, and 0.3 / 0.7"""
    _run_ff(case)


@pytest.mark.parametrize("form", range(4), ids=["plain", "rowbias", "res2", "rowbias+res2"])
def test_ff_fused_two_and_three_panels_per_workgroup(form):
    """128 (2 CUs + 1) + 5 rows through each of the four kernels: the later-panel LayerNorm (with the table: boundaries of the row
    map inside a workgroup's second panel), the prefetch of the next panel's rows under the epilogue, a ragged last panel"""
    cus = _cus()
    big = [c for c in fp.ff_cases(cus) if c.T > fp.NSRC]
    assert len(big) == 8 and all(c.T == fp.many_panels_T(cus) for c in big)
    names = {c.form.name for c in big[2 * form:2 * form + 2]}
    assert names == {["plain", "rowbias", "res2", "rowbias+res2"][form]}
    for case in big[2 * form:2 * form + 2]:
        _run_ff(case)


# ================================================================================================== the GEGLU epilogue of ops.gemm
@pytest.mark.parametrize("M,half,program,form", fp.GEGLU_GEMM, ids=[f"M{c[0]}-half{c[1]}" for c in fp.GEGLU_GEMM])
def test_geglu_gemm(M, half, program, form):
    """the switch and the curve probe through ops.gemm(..., geglu=half) on the rows z: K = C = 320, the planned program asserted"""
    from lkgd_amd import ops
    from lkgd_amd.packing import pack_geglu
    for kind, v in (("switch", 0), ("curve", 0), ("curve", 4)):
        p = fp.ff_probe(kind, v)
        a = p.rows.z[:M].half().to(DEV)
        wp, bp, h = pack_geglu(p.w1.float().to(DEV), p.b1.float().to(DEV), half=half)
        kw = dict(M=M, N=2 * fp.FF_INNER, K=fp.FF_C, bias=bp, geglu=h)
        what = f"geglu gemm M={M} interleave {half}, {kind}{v}"
        plan = ops.gemm_plan(a, wp, torch.empty(M, fp.FF_INNER, dtype=torch.float16, device=DEV), **kw)
        assert plan.program == program, f"{what}: planned program {plan.program}, the bound is derived for {program} ({form})"
        out = _twice(lambda o: ops.gemm(a, wp, o, **kw), M, fp.FF_INNER, fp.FF_INNER, what)
        if kind == "switch":
            fp.first_mismatch(out.cpu(), (8 * p.hidden * (p.gate > 0))[:M].half(), what)
            print(f"PROBE geglu_gemm program{program} {kind} M={M} exact")
        else:
            ratio = fp.check_bound(out.cpu(), p.g[:M], p.geglu_bound(form)[:M], what)
            print(f"PROBE geglu_gemm program{program} {kind}{v} M={M} {ratio:.4f}")
