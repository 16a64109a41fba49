"""GEMM census of the CogVideoX path: the lkgd_gemm_f16 descriptors of the DiT at 1920 and 3072 channels, of the 1.5 model and of
the T5-XXL encoder at their real row counts and widths (tools/gemm_census.py: two-layer / one-layer models with seeded weights
through the product's own ``forward``), the modulation GEMM at real depth (N = 695 040 and 1 554 432: hand-written signatures,
a two-layer model does not issue it), a row ladder over the block linears (the row counts at which the dispatcher's choice for
these widths changes) and the ``lkgd_gemm_fp8`` calls of the 2B forward after ``quantize_to_float8``.

Every lkgd_gemm_f16 signature goes through ``check_signature`` of tests/test_gemm_census_gpu.py as it is: sampled rows against the
fp64 descriptor oracle under the derived bound, the -7 sentinel around the output and in the ldc gaps, every row written, the
whole output against a second program.  ``lkgd_gemm_fp8`` takes no descriptor; ``check_fp8_signature`` below replays its recorded
calls on seeded random e4m3 bytes and scales (the operand distributions of test_gemm_fp8_random_e4m3, cast to e4m3 on the device:
35 552 x 7680 bytes through the table search of tests/fp8_oracle.py would take minutes) and checks 128 rows against the decoded
fp64 product under that test's bound, 2^-11 |ref| + 2^-13 S with |bias| in S, plus the sentinel and never-written checks.

Wall time on the MI355X box (`pytest -m gpu` over test_gemm_census_gpu.py, this file, test_fp8_gpu.py and
test_cogvideox_rope_gpu.py in one process: 49.6 s, of which the tests this file and the row-loop tests of the other two add take
about 13 s): dit2b 1.2 s (9 signatures, 21 launches; its recording, shared with the FP8 census, included), dit5b 0.5 s (9, 21), dit15
2.7 s (9, 17: 90 212 rows), t5xxl 0.4 s (4, 4), the modulation GEMM at real depth 0.05 s (4 signatures; W is filled on the device,
the oracle sees 36 tile columns), the ladder 0.2 s (2B half, 16 signatures) and 1.2 s (5B half, 16), the FP8 census 0.6 s (3
signatures, 12 launches), the wrong-tile-column test 0.02 s.  A replay is one launch of a few milliseconds, the operands are filled
on the device and the fp64 oracle takes 64 rows: no test here comes near a tenth of the 36 s these files took before, so none
carries the marker `slow`; the plans are re-derived without a GPU by tests/test_host_cpu.py on every run as well."""
import time
import zlib

import pytest
import torch

import fp8_oracle as fo
import gemm_oracle as go
from test_gemm_census_gpu import DEV, GUARD, SENTINEL, _census, _lib, _recorded, _view, check_signature
from lkgd_amd import ops
from tools import gemm_census as gc

pytestmark = pytest.mark.gpu

FP8_ROWS = 128
_fp8_calls = []


def _dit2b():
    """the 2B forward is recorded once for both of its censuses: fp16 descriptors and, after quantize_to_float8, the FP8 calls"""
    if gc.FP8_FORWARD not in _recorded:
        t0 = time.time()
        _recorded[gc.FP8_FORWARD], calls = gc.record_dit(gc.FP8_FORWARD, fp8=True)
        _fp8_calls.extend(calls)
        print(f"\nrecorded {gc.FP8_FORWARD} as fp16 and as FP8: {len(_recorded[gc.FP8_FORWARD])} + {len(calls)} launches, "
              f"{time.time() - t0:.1f} s")
    return _fp8_calls


# ------------------------------------------------------------------------------------------------------------- lkgd_gemm_f16
def test_census_dit2b():
    _dit2b()
    _census(None, ("dit2b_2x17776",))


def test_census_dit5b():
    _census(None, ("dit5b_2x17776",))


def test_census_dit15():
    _census(None, ("dit15_2x45106",))


def test_census_t5xxl():
    _census(None, (gc.T5_FORWARD,))


def test_census_modulation_at_real_depth():
    rows = [e for e in gc.load_table() if gc.MOD_FORWARD in e["launches"]]
    assert sorted((e["fields"]["M"], e["fields"]["N"], e["fields"]["K"]) for e in rows) == \
        [(1, 695040, 512), (1, 1554432, 512), (2, 695040, 512), (2, 1554432, 512)]
    for e in rows:            # 192x320 tiles, the last tile column ragged: 695 040 = 2172 x 320, 1 554 432 = 4857 x 320 + 192
        assert (e["plan"]["program"], e["plan"]["tile_m"], e["plan"]["tile_n"]) == (4, 192, 320), e["plan"]
    _census(None, (gc.MOD_FORWARD,))


def test_census_notices_a_wrong_tile_column(monkeypatch):
    """the sampled tile columns can fail: against an oracle whose LAST tile column (the ragged one of N = 1 554 432) is taken one
    column to the left, the modulation signature reports findings there and nowhere else (and none against the true oracle)"""
    sig = next(e for e in gc.load_table() if gc.MOD_FORWARD in e["launches"] and e["fields"]["N"] == 1554432 and e["fields"]["M"] == 2)
    assert check_signature(sig)[0] == []
    N, tn = sig["fields"]["N"], sig["plan"]["tile_n"]
    last = (N - 1) // tn * tn
    true_rows = go.gemm_rows

    def wrong(d, bufs, rows, cols=None, block=None):
        assert cols is not None and int((cols >= last).sum()) == N - last == 192          # the census asked for that tile column
        return true_rows(d, bufs, rows, cols=torch.where(cols >= last, cols - 1, cols), block=block)
    monkeypatch.setattr(go, "gemm_rows", wrong)
    bad = check_signature(sig)[0]
    print("\nlast tile column shifted by one:", bad[0][:300])
    assert len(bad) == 1 and "over the bound" in bad[0]
    n_over = int(bad[0].split(":")[1].split()[0])
    assert 192 <= n_over <= 2 * 192, n_over                   # (almost) every element of that tile column in both rows, no other


#: what the ladder is there to reach: (program, tile rows, tile columns or None = any, K slices > 1)
LADDER_PLANS = {"program 7 with K slices": lambda p: p["program"] == ops.GEMM_MID and p["k_slices"] > 1,
                "program 4 with K slices": lambda p: p["program"] == ops.GEMM_WIDE and p["k_slices"] > 1,
                "program 4 at 256x256": lambda p: (p["program"], p["tile_m"], p["tile_n"]) == (4, 256, 256),
                "program 4 at 192x320": lambda p: (p["program"], p["tile_m"], p["tile_n"]) == (4, 192, 320),
                "program 1": lambda p: p["program"] == ops.GEMM_TILE128}


def _ladder(D):
    return [e for e in gc.load_table() if gc.LADDER_FORWARD in e["launches"] and D in (e["fields"]["N"], e["fields"]["K"])]


def test_ladder_reaches_the_plans_it_is_there_for():
    rows = _ladder(1920) + _ladder(3072)
    assert len(rows) == 2 * 4 * len(gc.LADDER_ROWS) and {e["fields"]["M"] for e in rows} == set(gc.LADDER_ROWS)
    missing = [name for name, pred in LADDER_PLANS.items() if not any(pred(e["plan"]) for e in rows)]
    assert not missing, f"the row ladder no longer reaches: {missing} (the dispatcher changed: pick rows that do)"
    # this device plans what the table's 256-CU plans say (else the replay below would test other programs)
    for e in rows:
        assert gc.plan(gc.desc_from_signature(e), 0) == e["plan"], gc.sig_key(e)


def _census_ladder(D):
    """one model's half of the ladder"""
    _census(None, (gc.LADDER_FORWARD,), only=lambda e: D in (e["fields"]["N"], e["fields"]["K"]))


def test_census_row_ladder_2b():
    _census_ladder(1920)


def test_census_row_ladder_5b():
    _census_ladder(3072)


# ------------------------------------------------------------------------------------------------------------- lkgd_gemm_fp8
def fp8_sample_rows(M, key):
    rows = {0, M - 1}
    nt = (M + 127) // 128
    for t in (1, nt // 2, nt - 1):                      # both sides of the first, a middle and the last 128-row tile edge
        if 0 < t * 128 < M:
            rows |= {t * 128 - 1, t * 128}
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()) ^ 0xF8)
    while len(rows) < min(FP8_ROWS, M):
        rows |= set(torch.randint(0, M, (FP8_ROWS,), generator=g).tolist()[:min(FP8_ROWS, M) - len(rows)])
    return torch.tensor(sorted(rows), dtype=torch.int64)


def _e4m3_bytes(rows, ld, width, off, g):
    """[rows, width] seeded e4m3 bytes (N(0, 60^2) clamped to +-448, rounded by the device's cast) in a buffer of row stride ld"""
    buf = _view(rows * ld, torch.uint8, off, fill=0).view(rows, ld)
    v = (torch.randn(rows, width, generator=g, device=DEV) * 60).clamp(-448, 448)
    buf[:, :width] = v.to(torch.float8_e4m3fn).view(torch.uint8)
    assert not bool(((buf[:, :width] & 0x7F) == 0x7F).any())
    return buf


def check_fp8_signature(sig):
    """replay one recorded lkgd_gemm_fp8 call; returns the list of findings (empty = all checks passed)"""
    f, ptr = sig["fields"], sig["ptr"]
    M, N, K = f["M"], f["N"], f["K"]
    key = gc.sig_key(sig)
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(key.encode()))
    a = _e4m3_bytes(M, f["lda"], K, ptr["a"], g)
    w = _e4m3_bytes(N, f["ldw"], K, ptr["w"], g)
    a_s, w_s = _view(M, torch.float32, ptr["a_scale"]), _view(N, torch.float32, ptr["w_scale"])
    a_s.copy_(torch.rand(M, generator=g, device=DEV) * 0.02 + 1e-3)
    w_s.copy_(torch.rand(N, generator=g, device=DEV) * 0.01 + 1e-4)
    bias = None
    if "bias" in ptr:
        bias = _view(N, torch.float32, ptr["bias"], gen=g)
    n = M * f["ldc"]
    flat = _view(n + 2 * GUARD, torch.float16, ptr["out"], fill=SENTINEL)
    out = flat[GUARD:GUARD + n].view(M, f["ldc"])
    rc = _lib().lkgd_gemm_fp8(a.data_ptr(), f["lda"], a_s.data_ptr(), w.data_ptr(), f["ldw"], w_s.data_ptr(),
                              None if bias is None else bias.data_ptr(), out.data_ptr(), f["ldc"], M, N, K,
                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"lkgd_gemm_fp8 returned {rc}"
    torch.cuda.synchronize()
    bad = []
    rows = fp8_sample_rows(M, key)
    da = fo.decode(a[:, :K].index_select(0, rows.to(DEV))).double()
    dw = fo.decode(w[:, :K]).double()
    sc = a_s.index_select(0, rows.to(DEV)).cpu().double()[:, None] * w_s.cpu().double()[None, :]
    ref, S = (da @ dw.t()) * sc, (da.abs() @ dw.abs().t()) * sc
    if bias is not None:
        ref, S = ref + bias.cpu().double()[None, :], S + bias.cpu().double().abs()[None, :]
    got = out[:, :N].index_select(0, rows.to(DEV)).cpu().double()
    lim = 2.0 ** -11 * ref.abs() + 2.0 ** -13 * S
    ratio = (got - ref).abs() / lim
    worst = float(ratio.max())
    print(f"  fp8 {M} x {N} x {K}: {rows.numel()} rows, max |err| / bound = {worst:.3f}")
    if not bool(torch.isfinite(got).all()):
        bad.append("non-finite outputs in the sampled rows")
    elif not worst <= 1.0:
        r, c = divmod(int(ratio.argmax()), N)
        bad.append(f"{int((ratio > 1).sum())} elements of {ratio.numel()} over the bound, worst {worst:.3f} x at row {int(rows[r])} col {c}: "
                   f"got {got[r, c]:.6g} ref {ref[r, c]:.6g}; rows hit {sorted({int(rows[i]) for i in torch.nonzero((ratio > 1).any(1)).flatten()})[:12]}")
    if not (bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + n:] == SENTINEL).all())):
        bad.append("sentinel around the output overwritten")
    if f["ldc"] > N and not bool((out[:, N:] == SENTINEL).all()):
        bad.append("sentinel in the ldc - width gap overwritten")
    if bool((out[:, :N] == SENTINEL).all(dim=1).any()):
        bad.append("an output row was never written")
    return bad


def test_census_fp8_dit2b():
    t0 = time.time()
    rows = gc.reduce_fp8(_dit2b())
    table = gc.load_fp8_table()
    assert [gc.sig_key(e) for e in rows] == [gc.sig_key(e) for e in table] and len(table) >= 3, \
        "recorded lkgd_gemm_fp8 signatures differ from tests/golden/gemm_census.json (tools/gemm_census.py --write regenerates it)"
    assert [e["launches"] for e in rows] == [e["launches"] for e in table]
    # the six linears of both layers, at the real row count and the three (N, K) of a block
    assert sum(e["launches"][gc.FP8_FORWARD] for e in table) == 12
    assert {(e["fields"]["M"], e["fields"]["N"], e["fields"]["K"]) for e in table} == {(35552, 1920, 1920), (35552, 7680, 1920),
                                                                                       (35552, 1920, 7680)}
    t1 = time.time()
    findings = []
    for e in rows:
        try:
            findings += [f"{m}\n    {gc.sig_key(e)}" for m in check_fp8_signature(e)]
        except AssertionError:
            raise
        except Exception as err:      # a HIP error: nothing more may be started on a device that has just faulted
            pytest.exit(f"GPU error while replaying {gc.sig_key(e)}: {err!r}", returncode=3)
        torch.cuda.empty_cache()
    print(f"\ncensus fp8 {gc.FP8_FORWARD}: {sum(e['launches'][gc.FP8_FORWARD] for e in rows)} launches, {len(rows)} signatures, "
          f"record {t1 - t0:.1f} s, replay {time.time() - t1:.1f} s")
    assert not findings, f"{len(findings)} findings:\n" + "\n".join(findings)
