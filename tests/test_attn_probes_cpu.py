"""The attention probes (tests/attn_probes.py) would catch the faults they are built for.  No GPU and no kernel here: a kernel is
emulated by rounding an fp64 attention to fp16, a faulty kernel by an fp64 attention with one deliberate mistake.

This is a condition on the TEST: the only quantity that has to stay inside a bound is the fp16-rounded reference (within half of it);
every injected fault has to be rejected by the pair of probes that every GPU case runs.  Two faults are visible to one probe only, by
construction: a key counted twice cannot move the identity probe (its target already holds all the weight of the row) and is the
uniform probe's to find; value rows exchanged cannot move the uniform probe (a mean does not depend on the order) and are the
identity probe's.  Every other fault is rejected by both probes wherever both run."""
import math

import pytest
import torch
import torch.nn.functional as F

import attn_probes as ap

CASES = ap.all_cases()


def _kernel(x):
    """what a correct kernel returns: the reference rounded to fp16"""
    return x.to(torch.float16)


def _rejects(probe, out, what):
    with pytest.raises(AssertionError, match="err / bound"):
        probe.check(_kernel(out), what)


# ================================================================================================== the probes themselves
@pytest.mark.parametrize("make", [c[1] for c in CASES], ids=[c[0] for c in CASES])
def test_rounded_reference_uses_at_most_half_the_bound(make):
    p = make()
    assert p.check(_kernel(p.ref), "fp16-rounded reference", limit=0.5) <= 0.5
    assert p.q.dtype == p.k.dtype == p.v.dtype == torch.float16
    if p.kind == "uniform":
        assert not p.q.any()
        return
    # the builder's conditions: distinct codes, a power-of-two c <= 64, the margin, and the weight left for foreign keys
    codes, c, D = p.info["codes"], p.info["c"], p.lay.hd
    gram = codes @ codes.transpose(1, 2)
    off = gram - 2 * D * torch.eye(p.lay.Lk, dtype=gram.dtype)
    assert (gram.diagonal(dim1=1, dim2=2) == D).all() and off.max() < D, "codes not distinct within a key set"
    assert c in (1, 2, 4, 8, 16, 32, 64)
    assert p.info["margin"] >= ap.MARGIN_NATS
    if p.lay.Lk > 1:
        assert math.isclose(p.info["margin"], c * (D - float(off.max())) / math.sqrt(D))
    assert p.info["one_minus_p"] < 2.0 ** -20
    assert torch.equal(p.k.double().abs(), torch.full_like(p.k, c, dtype=torch.float64))
    # to fp64 rounding the reference IS the value row of the target key
    vt = torch.gather(p.lay.kv_groups(p.v.double())[p.lay.gmap()], 1, p.info["targets"][:, :, None].expand(-1, -1, D))
    assert (p.ref - p.lay.out_tokens(vt)).abs().max() <= 2.0 ** -18


def test_cross_codes_are_distinct_across_contexts():
    """a row sent to the wrong context must meet none of its own codes"""
    for T, heads, NC, Lk, rowmap, _ in ap.CROSS:
        if Lk < 2:
            continue
        p = ap.cross_probe("identity", T, heads, NC, Lk, rowmap)
        per_head = p.info["codes"].reshape(NC, heads, Lk, 64).permute(1, 0, 2, 3).reshape(heads, NC * Lk, 64)
        for h in range(heads):
            assert torch.unique(per_head[h], dim=0).shape[0] == NC * Lk
        assert torch.equal(p.info["targets"].reshape(T, heads)[:, 0], torch.arange(T) % Lk)


def test_sdpa64_against_torch_sdpa():
    """the reference's own index maps (kv map, Sq != S, the temporal regroup) against F.scaled_dot_product_attention in fp64"""
    g = torch.Generator().manual_seed(1)
    nb, heads, S, Sq = 3, 2, 37, 11
    q = torch.randn(nb * Sq, heads * 64, generator=g).half()
    k, v = torch.randn(nb * S, heads * 64, generator=g).half(), torch.randn(nb * S, heads * 64, generator=g).half()
    for kvmap in (None, [1, 2, 0], [2, 0, 0]):
        qf, kf, vf = (t.double().reshape(nb, -1, heads, 64).transpose(1, 2) for t in (q, k, v))
        if kvmap is not None:
            kf, vf = kf[kvmap], vf[kvmap]
        ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(nb * Sq, heads * 64)
        assert (ap.sdpa64(q, k, v, nb, heads, kvmap=kvmap) - ref).abs().max() < 1e-12
    B, Fq, Fk, S, heads = 3, 4, 7, 5, 3
    q = torch.randn(B * Fq * S, heads * 64, generator=g).half()
    k, v = torch.randn(B * Fk * S, heads * 64, generator=g).half(), torch.randn(B * Fk * S, heads * 64, generator=g).half()
    for kvmap in (None, [1, 2, 0], [2, 2, 2]):
        def split(x, Fr):
            return x.double().reshape(B, Fr, S, heads, 64).permute(0, 2, 3, 1, 4)
        qq, kk, vv = split(q, Fq), split(k, Fk), split(v, Fk)
        if kvmap is not None:
            kk, vv = kk[kvmap], vv[kvmap]
        ref = F.scaled_dot_product_attention(qq, kk, vv).permute(0, 3, 1, 2, 4).reshape(B * Fq * S, heads * 64)
        assert (ap.sdpa64(q, k, v, B, heads, kvmap=kvmap, temporal=(Fq, Fk, S)) - ref).abs().max() < 1e-12
    # head_dim != 64 takes its own default scale
    q, k, v = (torch.randn(2 * 9, 2 * 80, generator=g).half() for _ in range(3))
    qf, kf, vf = (t.double().reshape(2, 9, 2, 80).transpose(1, 2) for t in (q, k, v))
    ref = F.scaled_dot_product_attention(qf, kf, vf).transpose(1, 2).reshape(18, 160)
    assert (ap.sdpa64(q, k, v, 2, 2, hd=80) - ref).abs().max() < 1e-12


def test_check_reports_the_worst_element():
    ref = torch.linspace(-1, 1, 6 * 128, dtype=torch.float64).reshape(6, 128)
    got = ref.to(torch.float16)
    assert ap.check(got, ref, ap.UNIFORM_FLOOR, "clean") <= 0.25 + 1e-9
    bad = got.clone()
    bad[4, 70] += 0.25
    with pytest.raises(AssertionError) as e:
        ap.check(bad, ref, ap.UNIFORM_FLOOR, "one element off", rows_per_entry=2)
    msg = str(e.value)
    assert "row 4" in msg and "column 70" in msg and "batch entry 2 row 0" in msg and "err / bound" in msg and "1 of 768" in msg
    bad = got.clone()
    bad[1, 3] = float("nan")
    with pytest.raises(AssertionError, match="row 1.*column 3"):
        ap.check(bad, ref, ap.UNIFORM_FLOOR, "NaN left in the output")
    with pytest.raises(AssertionError, match="shape"):
        ap.check(got[:5], ref, ap.UNIFORM_FLOOR, "a row short")


# ================================================================================================== injected faults
S_BIG, SQ_BIG = max(ap.SPATIAL_PLAIN + ap.SPATIAL_PIPE)           # the largest S of the GPU file


def _key_indices(S):
    """first, last and both sides of every 64-key boundary"""
    return sorted({0, S - 1} | {j for m in range(64, S, 64) for j in (m - 1, m)})


@pytest.fixture(scope="module", params=[(S_BIG, SQ_BIG), (16, 16)], ids=lambda a: f"S{a[0]}")
def big(request):
    S, Sq = request.param
    out = {}
    for kind in ("uniform", "identity"):
        p = ap.spatial_probe(kind, S, Sq, None)
        out[kind] = (p, p.parts())
    return S, out


def _targeted(p, j):
    """does any row of the identity probe select key j?  (Sq < S leaves a few keys of a group without a query)"""
    return bool((p.info["targets"] == j).any())


def test_one_key_dropped(big):
    S, probes = big
    for j in _key_indices(S) if S > 64 else range(S):
        for kind, (p, parts) in probes.items():
            assert kind == "uniform" or _targeted(p, j)
            _rejects(p, parts.out_key_weight(j, 0.0), f"key {j} dropped")


def test_one_key_counted_twice(big):
    """seen by the uniform probe alone: the identity probe's target already holds all the weight of its row"""
    S, probes = big
    p, parts = probes["uniform"]
    for j in _key_indices(S) if S > 64 else range(S):
        _rejects(p, parts.out_key_weight(j, 2.0), f"key {j} counted twice")


def test_value_rows_exchanged(big):
    """seen by the identity probe alone: the uniform probe's rows are means, which do not depend on the order of the value rows"""
    S, probes = big
    p, parts = probes["identity"]
    for j in _key_indices(S) if S > 64 else range(S):
        j = min(j, S - 2)
        assert _targeted(p, j) or _targeted(p, j + 1)
        _rejects(p, parts.out_v_rows_exchanged(j), f"value rows {j} and {j + 1} exchanged")


@pytest.mark.parametrize("S,Sq", [c for c in ap.SPATIAL_PIPE if c[0] % 128])
def test_overlap_of_the_last_stage_counted_twice(S, Sq):
    """the masked pipelined program loads keys [S - 128, S) as its last stage; the first 128 - S % 128 of them are the last keys of
    the stage before it and have to be masked.  Unmasked, they count twice"""
    dup = 128 - S % 128
    w = torch.ones(S, dtype=torch.float64)
    w[S - 128:S - 128 + dup] = 2.0
    assert S - 128 + dup == (S // 128) * 128
    p = ap.spatial_probe("uniform", S, Sq, None)
    _rejects(p, p.parts().out(w), f"{dup} duplicate keys unmasked")
    w[S - 128:S - 128 + dup] = 1.0
    w[S - 128 + dup - 1] = 2.0                                   # a mask one key short
    _rejects(p, p.parts().out(w), "the last duplicate key unmasked")
    for kind in ("uniform", "identity"):                         # a mask one key long: the first new key of the last stage lost
        w = torch.ones(S, dtype=torch.float64)
        w[S - 128 + dup] = 0.0
        p = ap.spatial_probe(kind, S, Sq, None)
        _rejects(p, p.parts().out(w), "a mask one key too long")


@pytest.mark.parametrize("kind", ["uniform", "identity"])
def test_kv_map_replaced_by_its_inverse(kind):
    kvmap, inverse = (1, 2, 0), (2, 0, 1)
    assert [kvmap[i] for i in inverse] == [0, 1, 2] and kvmap != inverse
    for S, Sq in [(129, 129), (200, 72), (1152, 1100)]:
        p = ap.spatial_probe(kind, S, Sq, kvmap)
        _rejects(p, p.parts(gmap=p.lay.gmap(inverse)).out(), "spatial: map^-1[b] for map[b]")
    for F_, S, heads in [(14, 8, 2), (17, 5, 3)]:
        p = ap.temporal_probe(kind, F_, F_, S, heads, kvmap)
        _rejects(p, p.parts(gmap=p.lay.gmap(inverse)).out(), "temporal: map^-1[b] for map[b]")


@pytest.mark.parametrize("kind", ["uniform", "identity"])
@pytest.mark.parametrize("F_,S,heads", [(14, 8, 2), (17, 5, 3), (2, 8, 2), (32, 5, 3)])
def test_temporal_pairs_exchanged(kind, F_, S, heads):
    """two neighbouring (pixel, head) pairs of a workgroup read each other's K / V (a wrong XOR in the LDS swizzle)"""
    for Fq in ap.temporal_fqs(F_):
        p = ap.temporal_probe(kind, F_, Fq, S, heads, None)
        gm = p.lay.gmap()
        per = S * heads
        pair = gm % per
        partner = torch.where((pair ^ 1) < per, pair ^ 1, pair)
        _rejects(p, p.parts(gmap=gm - pair + partner).out(), "pairs 2i and 2i + 1 exchanged")
        one = gm.clone()                                         # a single pair of the last batch entry reads its neighbour
        one[-2] = gm[-1]
        _rejects(p, p.parts(gmap=one).out(), "one pair reads its neighbour")


@pytest.mark.parametrize("T,heads,NC,Lk,rowmap", [c[:5] for c in ap.CROSS])
def test_cross_row_sent_to_the_next_context(T, heads, NC, Lk, rowmap):
    for kind in ap.kinds(Lk):
        p = ap.cross_probe(kind, T, heads, NC, Lk, rowmap)
        wrong = ap.Layout("ctx", NC, heads, 64, 1, Lk, ctx=(p.lay.ctx + 1) % NC)
        _rejects(p, p.parts(gmap=wrong.gmap()).out(), "every row -> ctx + 1")
        ctx = p.lay.ctx.clone()                                  # one row alone, the last of the first workgroup or of T
        m = min(T, 256) - 1
        ctx[m] = (ctx[m] + 1) % NC
        _rejects(p, p.parts(gmap=ap.Layout("ctx", NC, heads, 64, 1, Lk, ctx=ctx).gmap()).out(), f"row {m} -> ctx + 1")
