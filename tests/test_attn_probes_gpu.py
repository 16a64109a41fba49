"""Every attention entry point on the two probes of tests/attn_probes.py, per element against an fp64 reference:

  uniform   q = 0: every output row is the mean of its value rows; |got - ref| <= 2^-9 |ref| + 2^-20
  identity  sign-code keys, every query selects one key by >= 22 nats: the row is that value row; <= 2^-9 |ref| + 2^-16

The bounds are derived in attn_probes.py (two fp16 roundings of 2^-11 - the probability and the output - doubled); that the probes
reject a dropped / doubled key, exchanged value rows, unmasked duplicate keys, an inverted kv map, exchanged temporal pairs and
a wrong cross-attention context is shown without a GPU in test_attn_probes_cpu.py.  Outputs are pre-filled with NaN, the K / V
of a batch entry that no query selects are NaN, and the debug knobs are reset in `finally`.  Every case prints the worst
err / bound it saw (`PROBE ...`, visible with -s).

The fused temporal kernels (ops.tattn_block, ops.tattn_front) take x and packed weights, not q / k / v: attn_probes.FusedProbe
builds both forms on rows and signed-selection weights that keep every intermediate exact, with the bounds derived in that module's
docstring.  ops.attn_dense_relbias runs the two probes under a zero table, and an offset and a weighted probe of the table itself."""
import pytest
import torch

import attn_probes as ap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _lib():
    from lkgd_amd import _lib
    return _lib.lib()


def _dev(p, poison=True):
    """the probe's q, k, v on the device; the K / V rows of a batch entry that the kv map never selects are NaN"""
    q, k, v = p.q.to(DEV), p.k.to(DEV), p.v.to(DEV)
    lay = p.lay
    if poison and lay.kvmap is not None:
        rows = lay.kv_rows // lay.nb
        for b in set(range(lay.nb)) - set(lay.kvmap):
            k[b * rows:(b + 1) * rows] = NAN
            v[b * rows:(b + 1) * rows] = NAN
    return q, k, v


def _map(kvmap):
    return torch.tensor(kvmap, dtype=torch.int32, device=DEV) if kvmap is not None else None


def _report(entry, program, case, kind, ratio):
    print(f"PROBE {entry} {program} {case} {kind} {ratio:.4f}")


# ================================================================================================== attn_spatial
PROGRAMS = {            # name -> (attn_pipe, attn_waves, attn_kvb), as tests/test_footprint_gpu.py::attn_mode sets them
    "rule": (0, 0, 0), "waves8": (0, 8, 0), "waves8_kvb128": (0, 8, 128), "waves16": (0, 16, 0), "waves16_kvb64": (0, 16, 64),
    "never_pipe": (1, 0, 0), "pipe": (2, 0, 0)}
SPATIAL = [(prog, S, Sq) for prog in PROGRAMS for S, Sq in (ap.SPATIAL_PIPE if prog == "pipe" else ap.SPATIAL_PLAIN)]
assert all(S >= 128 for prog, S, _ in SPATIAL if prog == "pipe")


class _program:
    def __init__(self, name):
        self.knobs = PROGRAMS[name]

    def __enter__(self):
        L = _lib()
        L.lkgd_debug_set_attn_pipe(self.knobs[0])
        L.lkgd_debug_set_attn_waves(self.knobs[1])
        L.lkgd_debug_set_attn_kvb(self.knobs[2])

    def __exit__(self, *exc):
        L = _lib()
        L.lkgd_debug_set_attn_pipe(0)
        L.lkgd_debug_set_attn_waves(0)
        L.lkgd_debug_set_attn_kvb(0)
        return False


@pytest.mark.parametrize("kvmap", ap.KVMAPS_SPATIAL, ids=lambda m: "kv" + ("".join(map(str, m)) if m else "none"))
@pytest.mark.parametrize("program,S,Sq", SPATIAL, ids=[f"{p}-S{S}-Sq{Sq}" for p, S, Sq in SPATIAL])
def test_attn_spatial(program, S, Sq, kvmap):
    """4 / 8 / 16 waves x 32 queries against 64- / 128-key stages (S around one and two stages, a last stage of 1, 63 and 8 keys,
    Sq down to one row and one row past a tile) and the software-pipelined program: one stage, every ring buffer, a wrapped ring,
    and the masked last stage with 127, 1, 56, 84 and 24 duplicate keys"""
    from lkgd_amd import ops
    nb, heads = ap.SPATIAL_NB, ap.SPATIAL_HEADS
    with _program(program):
        for kind in ("uniform", "identity"):
            p = ap.spatial_probe(kind, S, Sq, kvmap)
            q, k, v = _dev(p)
            out = torch.full((nb * Sq, heads * 64), NAN, dtype=torch.float16, device=DEV)
            ops.attn_spatial(q, k, v, out, nb, S, heads, kv_batch_map=_map(kvmap), Sq=Sq)
            _report("attn_spatial", program, f"S={S},Sq={Sq},kv={kvmap}", kind, p.check(out.cpu(), f"attn_spatial[{program}] S={S} Sq={Sq} kv map {kvmap}"))


@pytest.mark.parametrize("program", ["rule", "waves16", "pipe"])
def test_attn_spatial_packed_qkv(program):
    """q | k | v as column blocks of one [T, 3C] matrix (the UNet's projection output): row pitch 3C on all three"""
    from lkgd_amd import ops
    nb, heads = ap.SPATIAL_NB, ap.SPATIAL_HEADS
    S = ap.SPATIAL_PACKED["pipe" if program == "pipe" else "plain"]
    C = heads * 64
    with _program(program):
        for kind in ("uniform", "identity"):
            p = ap.spatial_probe(kind, S, S, (1, 2, 0))
            qkv = torch.cat([p.q, p.k, p.v], dim=1).to(DEV)
            out = torch.full((nb * S, C), NAN, dtype=torch.float16, device=DEV)
            ops.attn_spatial(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, nb, S, heads, kv_batch_map=_map((1, 2, 0)))
            _report("attn_spatial", program, f"S={S},packed", kind, p.check(out.cpu(), f"attn_spatial[{program}] packed q|k|v S={S}"))


# ================================================================================================== attn_temporal
@pytest.mark.parametrize("S,heads", ap.TEMPORAL_SH)
@pytest.mark.parametrize("F", ap.TEMPORAL_F)
def test_attn_temporal(F, S, heads):
    """both instantiations (F <= 16 / <= 32) and the 16 / 17 edge, odd F (the unpaired last frame of the two-frame P.V), 16 / 15 / 1
    (pixel, head) pairs (a full workgroup, clamped lanes, a single pair), Fq = F, 1, F - 1.  The identity probe draws codes and targets
    per (batch entry, pixel, head): a pair that reads another pair's swizzled chunk meets foreign codes and a foreign frame order.
    The probability is normalised and rounded to fp16 before P.V (one of the two roundings of the bound)"""
    from lkgd_amd import ops
    B = ap.TEMPORAL_B
    for Fq in ap.temporal_fqs(F):
        for kvmap in ap.KVMAPS_TEMPORAL:
            for kind in ("uniform", "identity"):
                p = ap.temporal_probe(kind, F, Fq, S, heads, kvmap)
                q, k, v = _dev(p)
                out = torch.full((B * Fq * S, heads * 64), NAN, dtype=torch.float16, device=DEV)
                ops.attn_temporal(q, k, v, out, B, F, S, heads, kv_b_map=_map(kvmap), Fq=Fq)
                _report("attn_temporal", "-", f"F={F},Fq={Fq},S={S},heads={heads},kv={kvmap}", kind,
                        p.check(out.cpu(), f"attn_temporal F={F} Fq={Fq} S={S} heads={heads} kv map {kvmap}"))


# ================================================================================================== attn_cross
@pytest.mark.parametrize("T,heads,NC,Lk,rowmap,ld", ap.CROSS, ids=[f"T{c[0]}-Lk{c[3]}" for c in ap.CROSS])
def test_attn_cross(T, heads, NC, Lk, rowmap, ld):
    """block-constant and interleaved row maps, a table that starts at a later context, ragged T, one and two keys; row m of the
    identity probe targets key m % Lk of its context, the codes are distinct across all contexts of a head.  Row pitch ld >= C: the
    columns beyond C stay untouched"""
    from lkgd_amd import ops
    C = heads * 64
    for kind in ap.kinds(Lk):
        p = ap.cross_probe(kind, T, heads, NC, Lk, rowmap)
        q, k, v = (torch.zeros(x.shape[0], ld, dtype=torch.float16, device=DEV) for x in (p.q, p.k, p.v))
        q[:, :C], k[:, :C], v[:, :C] = p.q.to(DEV), p.k.to(DEV), p.v.to(DEV)
        out = torch.full((T, ld), NAN, dtype=torch.float16, device=DEV)
        ops.attn_cross(q[:, :C], k[:, :C], v[:, :C], out[:, :C], heads, NC, Lk, rowmap)
        _report("attn_cross", "-", f"T={T},heads={heads},NC={NC},Lk={Lk}", kind, p.check(out[:, :C].cpu(), f"attn_cross T={T} Lk={Lk} row map {rowmap}"))
        assert torch.isnan(out[:, C:]).all()


# ================================================================================================== attn_dense
@pytest.mark.parametrize("nb,S,heads,hd", ap.DENSE)
def test_attn_dense(nb, S, heads, hd):
    """16 query rows per workgroup, keys by lane in rounds of 64: S = 1, 17, 50, 63, 64, 65, 257; head_dim 8, 64, 80, 128"""
    from lkgd_amd import ops
    for kind in ap.kinds(S):
        p = ap.dense_probe(kind, nb, S, heads, hd)
        q, k, v = _dev(p)
        out = torch.full((nb * S, heads * hd), NAN, dtype=torch.float16, device=DEV)
        ops.attn_dense(q, k, v, out, nb, S, heads, hd)
        _report("attn_dense", "-", f"nb={nb},S={S},heads={heads},hd={hd}", kind, p.check(out.cpu(), f"attn_dense S={S} head_dim {hd}"))


# ================================================================================================== fused temporal blocks
def _pitched(t, ld, fill=0.0):
    """t's rows in a [T, ld] device buffer (row pitch ld > width): the view of its first columns, and the buffer"""
    buf = torch.full((t.shape[0], ld), fill, dtype=torch.float16, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]], buf


def _fused_case(B, HW, F):
    return f"B={B},HW={HW},F={F}"


def _run_tattn_block(p, ldx=None, ldo=None):
    from lkgd_amd import ops
    from lkgd_amd.packing import pack_tblock
    ws = pack_tblock(p.wqkv.float(), p.bqkv.float(), p.wo.float()).to(DEV)
    x = _pitched(p.x, ldx)[0] if ldx else p.x.to(DEV)
    out, buf = _pitched(torch.full((p.T, 320), NAN, dtype=torch.float16), ldo or 320, NAN)
    kw = {}
    if p.table is not None:
        kw = dict(rowbias=p.table.half().to(DEV), rowmap=p.rowmap)
    ops.tattn_block(x, ws, p.bo.float().to(DEV), out, p.B, p.F, p.HW, **kw)
    assert torch.isnan(buf[:, 320:]).all(), "columns beyond the row were written"
    return out.cpu()


@pytest.mark.parametrize("F", ap.FUSED_F)
def test_tattn_block(F):
    """lkgd_tattn_block_c320 on exact inputs (attn_probes.FusedProbe): 14 -> 16 frame-slot padding (F = 13, 14, 15 against 16), a
    single pixel, a ragged / full / one-past-full panel, odd HW with B > 1 (a wave's pixel pair on a batch border), the (b_hi, b_lo)
    bias k-step, the per-head value and out-projection chunk order, the rebuilt residual at four row amplitudes; x and out with a
    row pitch of their own in one case each"""
    for B, HW in ap.TBLOCK_BHW:
        for kind in ap.fused_kinds(F):
            p = ap.fused_probe(kind, B, HW, F)
            ldx = 328 if (B, HW, F) == ap.TBLOCK_LDX else None
            ldo = 336 if (B, HW, F) == ap.TBLOCK_LDO else None
            out = _run_tattn_block(p, ldx, ldo)
            _report("tattn_block", f"ldx={ldx or 320},ldo={ldo or 320}", _fused_case(B, HW, F), kind,
                    p.check_block(out, f"tattn_block {_fused_case(B, HW, F)}"))


def test_tattn_block_row_bias():
    """the row-bias table (entries in multiples of 1/4) behind the row map of test_tblock_row_bias_and_sharp_scores"""
    B, HW, F = ap.TBLOCK_ROWBIAS
    for kind in ("uniform", "identity"):
        p = ap.fused_probe(kind, B, HW, F, True)
        _report("tattn_block", "rowbias", _fused_case(B, HW, F), kind, p.check_block(_run_tattn_block(p), f"tattn_block row bias {_fused_case(B, HW, F)}"))


def test_tattn_block_more_panels_than_cus():
    """515 panels, the last one ragged: the grid-stride panel loop, its token-row prefetch and the weight chunks issued across panel
    borders"""
    B, HW, F = ap.TBLOCK_MANY
    assert (B * HW + 7) // 8 > torch.cuda.get_device_properties(0).multi_processor_count and (B * HW) % 8
    for kind in ("uniform", "identity"):
        p = ap.fused_probe(kind, B, HW, F)
        _report("tattn_block", "panels>CUs", _fused_case(B, HW, F), kind, p.check_block(_run_tattn_block(p), f"tattn_block {_fused_case(B, HW, F)}"))


@pytest.mark.parametrize("F", ap.FUSED_F)
def test_tattn_front(F):
    """lkgd_tattn_front (the A/B fallback and the sharded path) on the same inputs: its own padding mask, softmax and fp32 bias"""
    from lkgd_amd import ops
    from lkgd_amd.packing import pack_tfront
    for B, HW in ap.TFRONT_BHW:
        for kind in ap.fused_kinds(F):
            p = ap.fused_probe(kind, B, HW, F)
            ldx = 328 if (B, HW, F) == ap.TFRONT_LDX else None
            ldo = 336 if (B, HW, F) == ap.TFRONT_LDO else None
            x = _pitched(p.x, ldx)[0] if ldx else p.x.to(DEV)
            out, buf = _pitched(torch.full((p.T, 320), NAN, dtype=torch.float16), ldo or 320, NAN)
            ops.tattn_front(x, pack_tfront(p.wqkv.half().to(DEV), 5), p.bqkv.float().to(DEV), out, B, F, HW, 5)
            assert torch.isnan(buf[:, 320:]).all(), "columns beyond the row were written"
            _report("tattn_front", f"ldx={ldx or 320},ldo={ldo or 320}", _fused_case(B, HW, F), kind,
                    p.check_front(out.cpu(), f"tattn_front {_fused_case(B, HW, F)}"))


# ================================================================================================== attn_dense_relbias
@pytest.mark.parametrize("nb,S,heads,hd", ap.RELBIAS_SHAPES)
def test_attn_dense_relbias(nb, S, heads, hd):
    """the RELBIAS instantiation: both plain probes under an all-zero table at scale 1.0 (T5's) and hd^-0.5; one-entry tables that
    shift every row by d = 0, +-1, +-(S - 1), +-64 and a seeded offset (a different one per head); a table of ln(w), whose rows are
    w-weighted means.  One key, one wave of keys +- 1, the T5 length, the LDS-heaviest legal shape"""
    from lkgd_amd import ops
    case = f"nb={nb},S={S},heads={heads},hd={hd}"
    probes = [(f"zero,scale={scale}", ap.relbias_zero_probe(kind, nb, S, heads, hd, scale)) for scale in (1.0, None) for kind in ap.kinds(S)]
    probes += [(f"d={list(o)}", ap.relbias_offset_probe(nb, S, heads, hd, o)) for o in ap.relbias_offsets(S, heads, hd)]
    probes.append(("ln(w)", ap.relbias_weighted_probe(nb, S, heads, hd)))
    for name, p in probes:
        q, k, v = _dev(p)
        out = torch.full((nb * S, heads * hd), NAN, dtype=torch.float16, device=DEV)
        ops.attn_dense_relbias(q, k, v, out, nb, S, heads, hd, p.table.to(DEV), scale=p.scale)
        _report("attn_dense_relbias", name, case, p.kind, p.check(out.cpu(), f"attn_dense_relbias {case} {name}"))
