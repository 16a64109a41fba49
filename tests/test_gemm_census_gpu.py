"""GEMM census: every lkgd_gemm_f16 descriptor the real forwards issue (tools/gemm_census.py: UNet full forward and the slices of
a rank of 2 / 4 / 8, the ControlNet encoder, the VAE) is replayed IN ISOLATION under automatic dispatch and held against the fp64
descriptor oracle (tests/gemm_oracle.py) - the real M, leading dimensions, column-slice outputs and epilogue combinations, under
the dispatcher's own choice of program, so that a fault is localised to one launch instead of diluting in a whole-model golden.

Per signature:
  * sampled rows, all N columns, against the oracle.  Non-GEGLU bound, derived and not measured:
        |got - ref| <= 2^-10 |ref| + (K + 16) 2^-24 S + 2^-24,   S[m,n] = sum_k |A(m,k) W[n,k]|
    (fp16 store rounding with one ulp of slack; fp32 accumulation in any order plus the epilogue).  Where s_acc != 1 scales the
    accumulator and nothing is added behind it (no rowbias, res1, res2: T5's closing projections, s_acc = 2^-6) the accumulation
    term is |s_acc| (K + 16) 2^-24 S - the rounding error of the sum is scaled with the sum; every other descriptor keeps the
    bound above.  GEGLU: the `_close` tolerance of tests/test_kernels_gpu.py (4e-3 of scale + 2e-3, rel-L2 < 3e-3).
    N > 2^17 (the real-depth modulation GEMM): the oracle sees the first two and the last two tile columns in full and
    ORACLE_TILE_COLUMNS seeded random tile columns (tests/gemm_oracle.py ``cols``); every other check sees every column;
  * the -7 sentinel around the output and in the ld - width gap of every row is intact;
  * the whole output against a second program (forced 128x128 two-stage; 256x320 <-> resident-weight for the 80-wide GEGLU)
    within 4e-3 max|out| (as test_gemm_split_k_few_rows); only LayerNorm-fold descriptors and 80-wide GEGLU ones the resident-
    weight program does not cover have no second program - they get 512 random rows instead of 64;
  * `colstats`, where the recorded descriptor asked for it, against fp64 sums of the rounded output.
The recorded signatures must equal tests/golden/gemm_census.json (tools/gemm_census.py --write regenerates it).

Wall time on the MI355X box (`pytest -m gpu` over this file, test_kernels_gpu.py and test_footprint_gpu.py: 38.6 s, of which the
other two files take 14.5 s): the real-width fixture 13.6 s, the full forward 2.1 s (105 signatures, 253 launches), the ControlNet
0.5 s, the three rank slices 6.6 s (306 signatures), the VAE 1.2 s.  The full-forward and ControlNet censuses run by default; the
slices and the VAE lengthen the selection by more than a tenth and run with LKGD_SLOW=1 (marker `slow`) - their plans are still
re-derived without a GPU by tests/test_host_cpu.py on every run.  The CogVideoX rows of the table (DiT, T5, the real-depth modulation
GEMM, the row ladder, the FP8 calls) are replayed by tests/test_gemm_census_dit_gpu.py through ``check_signature`` and ``_census``
below; its docstring has their wall times (about 7 s for all of them)."""
import ctypes as C
import time
import zlib

import pytest
import torch

import gemm_oracle as go
from tools import gemm_census as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.0
GUARD = 4096                      # sentinel elements in front of and behind every output
RANDOM_ROWS, RANDOM_ROWS_NO_SECOND = 64, 512
ORACLE_ALL_COLUMNS_UP_TO = 1 << 17       # wider outputs: the oracle checks whole tile columns, see oracle_columns
ORACLE_TILE_COLUMNS = 32


def _lib():
    from lkgd_amd import _lib as L
    return L.lib()


def _view(n, dtype, off_bytes, fill=None, gen=None, scale=1.0, shift=0.0):
    """n elements starting `off_bytes` past a 256-byte aligned address (+ slack behind them)"""
    item = torch.empty((), dtype=dtype).element_size()
    assert off_bytes % item == 0
    flat = torch.empty(n + 256 + 16, dtype=dtype, device=DEV)
    v = flat[off_bytes // item: off_bytes // item + n]
    assert v.data_ptr() % 16 == off_bytes
    if gen is not None:
        v.copy_((torch.randn(n, generator=gen, device=DEV, dtype=torch.float32) * scale + shift).to(dtype))
        flat[off_bytes // item + n:].zero_()
    elif fill is not None:
        flat.fill_(fill)
    return v


def _row_index(f, m):
    """the row map of include/lkgd_hip.h section 1, restated here: it sizes the rowbias table, which must not follow a
    (deliberately) wrong oracle"""
    return ((m // f["rb_d1"]) * f.get("rb_m1", 0) + m % f["rb_d2"] + f.get("rb_c0", 0)) % f["rb_md"]


def _a_source_rows(f):
    M, mode = f["M"], f.get("mode", 0)
    if mode == go.A_CONV3X3:
        return (M // (f["Hout"] * f["Wout"])) * f["Hin"] * f["Win"]
    if mode == go.A_TCONV3:
        return (M // (f["Floc"] * f["HW"])) * f["F"] * f["HW"]
    return M


class Replay:
    """a signature's descriptor on fresh seeded tensors of the descriptor's own dimensions and the recorded alignment classes"""

    def __init__(self, sig):
        from lkgd_amd import ops
        f, ptr = sig["fields"], sig["ptr"]
        self.sig, self.f = sig, f
        M, N, K = f["M"], f["N"], f["K"]
        self.M, self.N, self.K = M, N, K
        self.n_out = N // 2 if f.get("geglu") else N
        g = torch.Generator(device=DEV).manual_seed(zlib.crc32(gc.sig_key(sig).encode()))
        bufs, p = {}, {}
        rows_a = _a_source_rows(f)
        ln = "ln_colsum" in ptr
        a0 = _view(rows_a * f["lda0"], torch.float16, ptr["a0"], gen=g, scale=1.3 if ln else 1.0, shift=0.4 if ln else 0.0)
        bufs["a0"] = a0.view(rows_a, f["lda0"])
        if "a1" in ptr:
            bufs["a1"] = _view(rows_a * f["lda1"], torch.float16, ptr["a1"], gen=g).view(rows_a, f["lda1"])
        k_eff = 72 if f.get("mode", 0) == go.A_CONV3X3_C8 else K
        w = _view(N * K, torch.float16, ptr["w"], gen=g, scale=1.0 / k_eff ** 0.5).view(N, K)
        if k_eff != K:
            w[:, k_eff:] = 0                                     # the packer's zero padding (pack_conv3x3_c8)
        bufs["w"] = w
        if "bias" in ptr:
            bufs["bias"] = _view(N, torch.float32, ptr["bias"], gen=g, scale=0.5, shift=0.1)
        if "rowbias" in ptr:
            idx = _row_index(f, torch.arange(M, device=DEV))
            nrb = int(idx.max().item()) + 1
            self.map_idx = idx
            bufs["rowbias"] = _view(nrb * f["ldrb"], torch.float16, ptr["rowbias"], gen=g, scale=0.5).view(nrb, f["ldrb"])
        for r, ld in (("res1", "ldr1"), ("res2", "ldr2")):
            if r in ptr:
                bufs[r] = _view(M * f[ld], torch.float16, ptr[r], gen=g).view(M, f[ld])
        if ln:
            cs = _view(N, torch.float32, ptr["ln_colsum"])
            cs.copy_(w.float().sum(1))
            bufs["ln_colsum"] = cs
        self.zeros = _view(256, torch.float16, ptr["zeros"], fill=0.0)
        self.bufs = bufs
        p = {k: v.data_ptr() for k, v in bufs.items()}
        p["zeros"] = self.zeros.data_ptr()
        if "workspace" in ptr:
            ws = ops.splitk_workspace(torch.device(DEV))
            assert ws.numel() * 4 >= f["workspace_bytes"] and ws.data_ptr() % 16 == ptr["workspace"]
            p["workspace"] = ws.data_ptr()
        self.p = p
        self.out_off = ptr["out"]
        self.has_colstats = "colstats" in ptr

    def _out(self):
        n = self.M * self.f["ldc"]
        flat = _view(n + 2 * GUARD, torch.float16, self.out_off, fill=SENTINEL)
        return flat, flat[GUARD:GUARD + n].view(self.M, self.f["ldc"])

    def _run(self, d, out):
        return _lib().lkgd_gemm_f16(C.byref(d), torch.cuda.current_stream().cuda_stream)

    def launch(self, variant=0, colstats=True):
        """-> (flat, out view [M, ldc], colstats buffer or None, blk, plan)"""
        lib = _lib()
        p = dict(self.p)
        flat, out = self._out()
        assert GUARD * 2 % 16 == 0
        p["out"] = out.data_ptr()
        cs, blk = None, 0
        sig = self.sig
        if not (colstats and self.has_colstats):
            sig = dict(sig, ptr={k: v for k, v in sig["ptr"].items() if k != "colstats"})
        lib.lkgd_debug_set_gemm_variant(variant)
        try:
            if "colstats" in sig["ptr"]:
                probe = gc.desc_from_signature(dict(sig, ptr={k: v for k, v in sig["ptr"].items() if k != "colstats"}), p)
                blk = gc.plan(probe, 0)["colstats_block"]
                assert blk > 0, "the recorded descriptor carried column sums, the plan offers none"
                nb = (self.M + blk - 1) // blk
                cs_flat = _view(nb * self.N + 2 * GUARD, torch.float32, sig["ptr"]["colstats"], fill=SENTINEL)
                cs = cs_flat[GUARD:GUARD + nb * self.N].view(nb, self.N // 2, 2)
                p["colstats"] = cs.data_ptr()
                self.cs_flat = cs_flat
            d = gc.desc_from_signature(sig, p)
            plan = gc.plan(d, 0)
            rc = self._run(d, out)
        finally:
            lib.lkgd_debug_set_gemm_variant(0)
        assert rc == 0, f"lkgd_gemm_f16 returned {rc}"
        return flat, out, cs, blk, plan


def sample_rows(rp, plan, n_random):
    f, M = rp.f, rp.M
    rows = {0, M - 1}
    tm = plan["tile_m"]
    nt = (M + tm - 1) // tm
    for t in (1, nt // 2, nt - 1):                      # both sides of the first, a middle and the last tile boundary
        if 0 < t * tm < M:
            rows |= {t * tm - 1, t * tm}
    mode = f.get("mode", 0)
    if mode in (go.A_CONV3X3, go.A_CONV3X3_C8):
        Ho, Wo = f["Hout"], f["Wout"]
        nimg = M // (Ho * Wo)
        px = [(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1), (0, Wo // 2), (Ho - 1, Wo // 2), (Ho // 2, 0), (Ho // 2, Wo - 1)]
        for n in {0, nimg - 1}:
            rows |= {(n * Ho + y) * Wo + x for y, x in px}
    if mode == go.A_TCONV3:
        Floc, HW = f["Floc"], f["HW"]
        nb = M // (Floc * HW)
        for b in {0, nb - 1}:
            for fl in {0, Floc - 1}:
                rows |= {(b * Floc + fl) * HW + s for s in (0, HW // 2, HW - 1)}
    if "rowbias" in rp.sig["ptr"]:
        idx = rp.map_idx
        cut = (torch.nonzero(idx[1:] != idx[:-1]).flatten() + 1).cpu()
        if cut.numel():
            for b in {int(cut[0]), int(cut[-1])}:
                rows |= {b - 1, b}
    g = torch.Generator().manual_seed(zlib.crc32(gc.sig_key(rp.sig).encode()) ^ 0x5EED)
    rows |= set(torch.randint(0, M, (n_random,), generator=g).tolist())
    return torch.tensor(sorted(rows), dtype=torch.int64)


def oracle_columns(sig, plan):
    """None = every column; for N > ORACLE_ALL_COLUMNS_UP_TO the columns of the first two and last two tile columns of the plan
    (the last one ragged where tile_n does not divide N) and of ORACLE_TILE_COLUMNS seeded random tile columns, ascending"""
    N, tn = sig["fields"]["N"], plan["tile_n"]
    if N <= ORACLE_ALL_COLUMNS_UP_TO or sig["fields"].get("geglu"):
        return None
    nt = (N + tn - 1) // tn
    g = torch.Generator().manual_seed(zlib.crc32(gc.sig_key(sig).encode()) ^ 0xC015)
    tiles = {0, 1, nt - 2, nt - 1} | set(torch.randint(0, nt, (ORACLE_TILE_COLUMNS,), generator=g).tolist())
    return torch.cat([torch.arange(t * tn, min(N, (t + 1) * tn)) for t in sorted(t for t in tiles if 0 <= t < nt)])


def accumulation_scale(sig):
    """the factor on the accumulation term of the bound: |s_acc| where the scaled accumulator is all that is stored"""
    s_acc = float(sig["fields"].get("s_acc", 1.0))
    if s_acc != 1.0 and not any(k in sig["ptr"] for k in ("res1", "res2", "rowbias")):
        return abs(s_acc)
    return 1.0


def check_signature(sig):
    """replay one signature; returns the list of findings (empty = all checks passed)"""
    bad = []
    f = sig["fields"]
    rp = Replay(sig)
    flat, out, cs, blk, plan = rp.launch(0)
    variant, why = gc.second_program(sig)
    rows = sample_rows(rp, plan, RANDOM_ROWS if variant is not None else RANDOM_ROWS_NO_SECOND)
    cols = oracle_columns(sig, plan)
    ref, S = go.gemm_rows(go.desc(**f), rp.bufs, rows, cols=cols)
    got = out[:, :rp.n_out].index_select(0, rows.to(DEV))
    if cols is not None:
        got = got.index_select(1, cols.to(DEV))
    got = got.cpu().double()
    width = got.shape[1]
    col_of = (lambda c: c) if cols is None else (lambda c: int(cols[c]))                  # noqa: E731
    tag = f"program {plan['program']} {plan['tile_m']}x{plan['tile_n']} ks {plan['k_slices']}"
    if not torch.isfinite(got).all():
        bad.append(f"{tag}: non-finite outputs in the sampled rows")
    elif S is not None:
        bound = 2.0 ** -10 * ref.abs() + accumulation_scale(sig) * (rp.K + 16) * 2.0 ** -24 * S + 2.0 ** -24
        over = (got - ref).abs() - bound
        if (over > 0).any():
            r, c = divmod(int(over.argmax()), width)
            bad.append(f"{tag}: {int((over > 0).sum())} elements of {over.numel()} over the bound, worst at row {int(rows[r])} "
                       f"col {col_of(c)}: got {got[r, c]:.6g} ref {ref[r, c]:.6g} bound {bound[r, c]:.3g}; rows hit "
                       f"{sorted({int(rows[i]) for i in torch.nonzero((over > 0).any(1)).flatten()})[:12]}")
    else:
        err = (got - ref).abs().max().item()
        scale = ref.abs().max().item() + 1e-6
        rel = ((got - ref).norm() / (ref.norm() + 1e-12)).item()
        if err > 4e-3 * scale + 2e-3 or rel >= 3e-3:
            bad.append(f"{tag}: GEGLU max abs err {err:.4g} vs scale {scale:.4g}, rel L2 {rel:.4g}")
    # the sentinel: guards in front and behind, and the ld - width gap of every row
    n = rp.M * f["ldc"]
    if not (bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + n:] == SENTINEL).all())):
        bad.append(f"{tag}: sentinel around the output overwritten")
    if f["ldc"] > rp.n_out and not bool((out[:, rp.n_out:] == SENTINEL).all()):
        bad.append(f"{tag}: sentinel in the ldc - width gap overwritten")
    if bool((out[:, :rp.n_out] == SENTINEL).all(dim=1).any()):
        bad.append(f"{tag}: an output row was never written")
    # the whole output against a second program
    if variant is not None:
        flat2, out2, _, _, plan2 = rp.launch(variant, colstats=False)
        a, b = out[:, :rp.n_out].float(), out2[:, :rp.n_out].float()
        lim = 4e-3 * float(b.abs().max())
        diff = (a - b).abs()
        worst = float(diff.max())
        if not worst <= lim:
            r, c = divmod(int(diff.argmax()), rp.n_out)
            bad.append(f"{tag} vs program {plan2['program']} ks {plan2['k_slices']}: max |diff| {worst:.4g} > {lim:.4g} at row {r} "
                       f"col {c}; {int((diff > lim).sum())} elements over")
        del flat2, out2
    # column sums of the ROUNDED outputs
    if cs is not None:
        nb = (rp.M + blk - 1) // blk
        x = out[:, :rp.N].double()
        pad = nb * blk - rp.M
        if pad:
            x = torch.cat([x, torch.zeros(pad, rp.N, dtype=torch.float64, device=DEV)])
        x = x.view(nb, blk, rp.N // 2, 2)
        cnt = torch.full((nb,), 2.0 * blk, dtype=torch.float64, device=DEV)
        cnt[-1] = 2.0 * (rp.M - (nb - 1) * blk)
        ref_cs = torch.stack([x.sum(dim=(1, 3)), (x * x).sum(dim=(1, 3))], dim=-1) / cnt[:, None, None]
        got_cs = cs.double() / cnt[:, None, None]
        # (the tolerance of test_groupnorm_statistics_from_gemm_epilogues, on the means the sums stand for)
        if not torch.allclose(got_cs, ref_cs, rtol=1e-3, atol=1e-4):
            e = (got_cs - ref_cs).abs()
            bad.append(f"{tag}: colstats (block {blk}) off by up to {float(e.max()):.4g} at {divmod(int(e.argmax()), rp.N)}")
        nel = nb * rp.N
        if not (bool((rp.cs_flat[:GUARD] == SENTINEL).all()) and bool((rp.cs_flat[GUARD + nel:] == SENTINEL).all())):
            bad.append(f"{tag}: sentinel around colstats overwritten")
    return bad, variant, why


# ------------------------------------------------------------------------------------------------------------------------ tests
_checked = {}          # signature key -> (findings, second variant, reason): a signature shared by several forwards runs once
_recorded = {}


def _records(unet, forwards):
    miss = [f for f in forwards if f not in _recorded]
    if miss:
        _recorded.update(gc.record_all(unet, miss))
    return {f: _recorded[f] for f in forwards}


def _census(unet, forwards, only=None):
    """record `forwards`, hold their signatures against the committed table, replay every signature not yet checked.  ``only``
    (a predicate on a table row): the census of that part of the forwards' signatures"""
    t0 = time.time()
    only = only or (lambda e: True)
    rows = [e for e in gc.reduce(_records(unet, forwards)) if only(e)]
    table = {gc.sig_key(e): e for e in gc.load_table() if any(f in e["launches"] for f in forwards) and only(e)}
    got = {gc.sig_key(e): e for e in rows}
    assert set(got) == set(table), (f"recorded signatures differ from tests/golden/gemm_census.json: {len(set(got) - set(table))} "
                                    f"new, {len(set(table) - set(got))} gone (tools/gemm_census.py --write regenerates it)\n"
                                    + "\n".join(sorted(set(got) ^ set(table))[:6]))
    for k, e in got.items():
        assert e["launches"] == {f: n for f, n in table[k]["launches"].items() if f in forwards}, k
        assert e["plan"] == table[k]["plan"], (k, e["plan"], table[k]["plan"])
        assert e["second_program"] == table[k]["second_program"], k
        assert gc.plan(gc.desc_from_signature(e), 0) == e["plan"], "this device's plan differs from the table's 256-CU plan"
    t1 = time.time()
    findings, no_second = [], {}
    for i, k in enumerate(sorted(got)):
        if i % 25 == 0:
            print(f"  census {forwards[0]}: signature {i} of {len(got)}, {time.time() - t1:.0f} s", flush=True)
        if k not in _checked:
            try:
                _checked[k] = check_signature(got[k])
            except AssertionError:
                raise
            except Exception as e:      # a HIP error: nothing more may be started on a device that has just faulted
                pytest.exit(f"GPU error while replaying {k}: {e!r}", returncode=3)
            torch.cuda.empty_cache()
        bad, variant, why = _checked[k]
        if variant is None:
            no_second[k] = why
        findings += [f"{m}\n    {k}" for m in bad]
    # the only signatures without a second program: the two classes of NO_SECOND, exactly as the table states them
    assert set(no_second.values()) <= set(gc.NO_SECOND)
    assert {k: v for k, v in no_second.items()} == {k: e["no_second_program"] for k, e in table.items() if e.get("no_second_program")}
    print(f"\ncensus {'+'.join(forwards)}: {sum(sum(e['launches'].values()) for e in rows)} launches, {len(rows)} signatures, "
          f"record {t1 - t0:.1f} s, replay {time.time() - t1:.1f} s")
    assert not findings, f"{len(findings)} findings:\n" + "\n".join(findings)


def test_census_unet_full_forward(c1_hip_model):
    _census(c1_hip_model, ("unet_2x14",))


@pytest.mark.slow
def test_census_unet_rank_slices(c1_hip_model):
    _census(c1_hip_model, ("unet_1x14", "unet_1x7", "unet_1x4"))


def test_census_controlnet(c1_hip_model):
    _census(c1_hip_model, ("controlnet_2x14",))


@pytest.mark.slow
def test_census_vae(c1_hip_model):
    _census(c1_hip_model, ("vae_decode", "vae_encode"))


def _first(forward, pred):
    for e in gc.load_table():
        if forward in e["launches"] and pred(e):
            return e
    raise AssertionError("the table has no such signature")


def test_census_notices_a_wrong_oracle(monkeypatch):
    """the census can fail: against an oracle with ONE row-map parameter or ONE tap offset perturbed, the sampled-row check of a
    signature that uses it reports findings (and none against the unperturbed oracle)"""
    rowmap = _first("unet_2x14", lambda e: "rowbias" in e["ptr"] and e["fields"].get("mode", 0) == go.A_PLAIN)
    conv = _first("unet_2x14", lambda e: e["fields"].get("mode", 0) == go.A_CONV3X3 and "colstats" not in e["ptr"])
    for sig in (rowmap, conv):
        assert check_signature(sig)[0] == []
    true_index, true_rows = go.rowmap_index, go.a_rows
    wrong_index = lambda d, rows: true_index(go.desc(**dict(vars(d), rb_d1=d.rb_d1 + 1)), rows)          # noqa: E731
    m = torch.arange(rowmap["fields"]["M"])
    d0 = go.desc(**rowmap["fields"])
    assert int(wrong_index(d0, m).max()) <= int(true_index(d0, m).max())          # the wrong map stays inside the table
    monkeypatch.setattr(go, "rowmap_index", wrong_index)
    bad = check_signature(rowmap)[0]
    print("\nrow map with rb_d1 + 1:", bad[0][:300])
    assert bad and "over the bound" in bad[0]
    monkeypatch.setattr(go, "rowmap_index", true_index)
    # every tap one pixel further down / right (pad_off flipped): only the oracle's gather moves
    monkeypatch.setattr(go, "a_rows", lambda d, bufs, rows: true_rows(go.desc(**dict(vars(d), pad_off=1 - d.pad_off)), bufs, rows))
    bad = check_signature(conv)[0]
    print("taps shifted by one pixel:", bad[0][:300])
    assert bad and "over the bound" in bad[0]


def test_gemm_family_flop_replayed_equals_eager(c1_hip_model):
    """bench.py's roofline line reads the algorithmic FLOP of every GEMM-family launch from `ops.GEMM_EVENTS` in an eager forward
    and from `Plan.run(events)` in a replayed one: the full forward gives the same list both ways, element by element, and the
    fused kernels of the family are in it with the FLOP of their matrix products"""
    from lkgd_amd import ops, replay
    unet = c1_hip_model
    tok, emb, ids, t = gc._unet_inputs(unet.device, 2, 14)
    run = lambda: unet.forward_tokens(tok, 2, 14, gc.H, gc.W, t, emb, ids)      # noqa: E731
    run()                                       # (first-use packs and cached tables)
    torch.cuda.synchronize()
    eager = []
    ops.GEMM_EVENTS = eager
    try:
        run()
    finally:
        ops.GEMM_EVENTS = None
    torch.cuda.synchronize()
    with replay.strict(False):
        with replay.record(replay.Arena()) as plan:
            plan.result = run()
    try:
        replayed = []
        plan.run(replayed)
        torch.cuda.synchronize()
        family = [(name, flop) for fn, args, name, flop in plan.calls if flop is not None]
    finally:
        plan.release()
        torch.cuda.empty_cache()
    assert len(eager) == len(replayed) == len(family) > 200
    assert [f for _, _, f in eager] == [f for _, _, f in replayed] == [f for _, f in family]
    assert all(e.elapsed_time(e2) >= 0 for e, e2, _ in replayed[:4])
    T320, T640 = 2 * 14 * gc.H * gc.W, 2 * 14 * (gc.H // 2) * (gc.W // 2)
    want = {"lkgd_ff_fused_c320": 2.0 * T320 * (2560 * 320 + 320 * 1280),
            "lkgd_tattn_block_c320": 2.0 * T320 * (960 * 320 + 320 * 320) + 4.0 * T320 * 16 * 320,
            "lkgd_ln_qkv_c320": 2.0 * T320 * 3 * 320 * 320,
            "lkgd_ln_qkv_c640": 2.0 * T640 * 3 * 640 * 640}
    for name, flop in want.items():
        got = {f for n, f in family if n == name}
        assert got == {flop}, (name, got, flop)
    # conv_in (A_CONV3X3_C8: K = 128 zero padded in memory) counts its 72 real taps
    assert 2.0 * T320 * 320 * 72 in {f for n, f in family if n == "lkgd_gemm_f16"}
