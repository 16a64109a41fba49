"""Every attention entry point on the two probes of tests/attn_probes.py, per element against an fp64 reference:

  uniform   q = 0: every output row is the mean of its value rows; |got - ref| <= 2^-9 |ref| + 2^-20
  identity  sign-code keys, every query selects one key by >= 22 nats: the row is that value row; <= 2^-9 |ref| + 2^-16

The bounds are derived in attn_probes.py (two fp16 roundings of 2^-11 - the probability and the output - doubled); that the probes
reject a dropped / doubled key, exchanged value rows, unmasked duplicate keys, an inverted kv map, exchanged temporal pairs and
a wrong cross-attention context is shown without a GPU in test_attn_probes_cpu.py.  Outputs are pre-filled with NaN, the K / V
of a batch entry that no query selects are NaN, and the debug knobs are reset in `finally`.  Every case prints the worst
err / bound it saw (`PROBE ...`, visible with -s)."""
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
