"""The attention probes (tests/attn_probes.py) would catch the faults they are built for.  No GPU and no kernel here: a kernel is
emulated by rounding an fp64 attention to fp16, a faulty kernel by an fp64 attention with one deliberate mistake.

This is a condition on the TEST: the only quantity that has to stay inside a bound is the fp16-rounded reference (within half of it);
every injected fault has to be rejected by the pair of probes that every GPU case runs.  Two faults are visible to one probe only, by
construction: a key counted twice cannot move the identity probe (its target already holds all the weight of the row) and is the
uniform probe's to find; value rows exchanged cannot move the uniform probe (a mean does not depend on the order) and are the
identity probe's.  Every other fault is rejected by both probes wherever both run.

The second half of the file does the same for the probes of the fused temporal kernels (here the emulation is the kernels' own
chain in fp32 with their fp16 roundings, inside half of each bound) and of the relative-position-bias table."""
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


# ================================================================================================== fused temporal blocks
# lkgd_tattn_block_c320 and lkgd_tattn_front: the probe's conditions, an fp32 emulation of each kernel's chain with exactly its fp16
# roundings (attn_probes' docstring) inside HALF of each bound, and the faults of the fused machinery.  A fault has to be rejected
# in every unit it touches - a token row of the block's result, a (token row, head) of the front's output: a touched unit is one
# in which the faulty fp64 chain differs from the reference at all, and rejected means at least one of its elements misses the
# bound after fp16 rounding.  Where the fault leaves the softmax one-hot (identity form), every single touched ELEMENT has to
# miss it: there the references differ by multiples of 1/4.
TBLOCK_CASES = [(B, HW, Fr, rb, kind) for B, HW, Fr, rb in ap.tblock_cases() for kind in ap.fused_kinds(Fr)]
TFRONT_CASES = [(B, HW, Fr, kind) for B, HW, Fr in ap.tfront_cases() for kind in ap.fused_kinds(Fr)]
LOG2E = 1.4426950408889634


def _ln_onepass(x, ulps=0):
    """the kernels' LayerNorm: one pass, var = E[x^2] - mean^2, a reciprocal square root (moved by `ulps` here), eps = 1e-5"""
    xf = x.float()
    mean = xf.sum(1) * torch.tensor(1.0 / 320, dtype=torch.float32)
    var = ((xf * xf).sum(1) * torch.tensor(1.0 / 320, dtype=torch.float32) - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + ap.TB_EPS)
    for _ in range(abs(ulps)):
        rstd = torch.nextafter(rstd, torch.full_like(rstd, math.inf if ulps > 0 else 0.0))
    z = (xf * rstd[:, None] + (-mean * rstd)[:, None]).half()
    return z, mean, (var + ap.TB_EPS) * rstd


def _emulate(p, front):
    """fp32 with the fp16 roundings of attn_tfront.hip (front) / attn_tblock.hip: z, the packed q | k | v, P, the packed attention
    output, the stored result; the front scales q by log2(e) / 8 BEFORE packing it, the block scales the fp32 scores"""
    z, mean, sigma = _ln_onepass(p.x)
    qkv = z.float() @ p.wqkv.half().float().T + p.bqkv.float()
    q, k, v = qkv.split(320, dim=1)
    scl = torch.tensor(0.125 * LOG2E, dtype=torch.float32)
    if front:
        q = q * scl
    lay = p.lay
    qg, kg, vg = lay.q_groups(q.half().float()), lay.kv_groups(k.half().float()), lay.kv_groups(v.half().float())
    s = qg @ kg.transpose(1, 2)
    if not front:
        s = s * scl
    e = torch.exp2(s - s.amax(-1, keepdim=True))
    pr = (e * (1.0 / e.sum(-1, keepdim=True))).half().float()
    att = lay.out_tokens(pr @ vg).half()
    if front:
        return att
    out = att.float() @ p.wo.half().float().T + p.bo.float() + (z.float() * sigma[:, None] + mean[:, None])
    if p.table is not None:
        out = out + p.table.half().float()[p.idx]
    return out.half()


def _fused_conditions(p):
    x = p.x
    assert x.dtype == torch.float16 and torch.equal(x.double(), p.x64) and not p.x64.sum(1).any()
    assert torch.equal(F.layer_norm(x.float(), (320,)).half().double(), p.z), "LayerNorm(x) is not exactly +-1 in fp16"
    for ulps in (-2, 0, 2):
        assert torch.equal(_ln_onepass(x, ulps)[0].double(), p.z), f"one-pass LayerNorm, rsq moved by {ulps} ulp"
    for t in (p.wqkv, p.bqkv, p.wo, p.bo) + ((p.table,) if p.table is not None else ()):
        assert torch.equal(t.half().double(), t), "a weight or bias is not an fp16 number"
    assert p.bqkv[:320].eq(0).all() and p.bqkv[320:].ne(0).all()
    assert int(p.wo.ne(0).sum()) == 320 and p.wo.abs().sum(0).eq(1).all() and p.wo.abs().sum(1).eq(1).all()
    if p.kind == "uniform":
        assert not p.wqkv[:320].any()
        return
    assert p.one_minus_p < 2.0 ** -20 and p.margin >= ap.MARGIN_NATS and p.c in (1, 2, 4, 8, 16, 32, 64)
    # the identity form's reference is the target's value row; chained through the block it is an fp16 number
    vg = p.lay.kv_groups(p.qkv64()[2])
    ideal = p.lay.out_tokens(torch.gather(vg, 1, p.targets[:, :, None].expand(-1, -1, 64)))
    assert torch.equal(ideal.half().double(), ideal) and (p.att_ref - ideal).abs().max() <= 2.0 ** -18
    out = p.block64(ideal)[1]
    assert torch.equal(out.half().double(), out) and (p.out_ref - out).abs().max() <= 2.0 ** -18
    assert torch.equal(out * 4, (out * 4).round())


@pytest.mark.parametrize("B,HW,Fr,rowbias,kind", TBLOCK_CASES, ids=[f"B{c[0]}-HW{c[1]}-F{c[2]}{'-rb' if c[3] else ''}-{c[4]}" for c in TBLOCK_CASES])
def test_tattn_block_probe_conditions_and_half_bound(B, HW, Fr, rowbias, kind):
    p = ap.fused_probe(kind, B, HW, Fr, rowbias)
    _fused_conditions(p)
    assert p.check_block(_emulate(p, front=False), "fp32 emulation of attn_tblock.hip", limit=0.5) <= 0.5


@pytest.mark.parametrize("B,HW,Fr,kind", TFRONT_CASES, ids=[f"B{c[0]}-HW{c[1]}-F{c[2]}-{c[3]}" for c in TFRONT_CASES])
def test_tattn_front_probe_conditions_and_half_bound(B, HW, Fr, kind):
    p = ap.fused_probe(kind, B, HW, Fr)
    _fused_conditions(p)
    assert p.check_front(_emulate(p, front=True), "fp32 emulation of attn_tfront.hip", limit=0.5) <= 0.5


def _units(t, width):
    return t.reshape(t.shape[0], -1, width).any(-1)


def _touched_rejected(faulty, ref, bound, width, what, every_element=False, expect=None, floor=ap.IDENTITY_FLOOR):
    """every unit (`width` columns of a row) in which the faulty fp64 chain differs from the reference misses the bound once it is
    rounded to fp16; expect: [rows, units] bool, units that have to be among the touched ones.  Returns the touched units.
    (Differs = by more than the floor, which is what the e^-22 of the foreign keys may move an element that is otherwise the same)"""
    touched = (faulty - ref).abs() > floor
    oob = ap.out_of_bound(_kernel(faulty), ref, bound)
    tu, ou = _units(touched, width), _units(oob, width)
    assert tu.any(), f"{what}: the fault touches nothing"
    assert (ou | ~tu).all(), f"{what}: {int((tu & ~ou).sum())} of {int(tu.sum())} touched units stay inside the bound"
    if every_element:
        assert (oob | ~touched).all(), f"{what}: {int((touched & ~oob).sum())} touched elements stay inside the bound"
    if expect is not None:
        assert (tu | ~expect).all(), f"{what}: {int((expect & ~tu).sum())} units the fault should reach are untouched"
    return tu


def _fused_rejects(p, att, what, every_element=False, rows=None, front=True, block=True):
    """the attention output `att` of a faulty chain, as lkgd_tattn_front stores it and carried through the block"""
    sharp = every_element and p.kind == "identity"
    if front:
        _touched_rejected(att, p.att_ref, p.front_bound, 64, f"front, {what}", sharp, None if rows is None else rows[:, None].expand(-1, 5), p.floor)
    if block:
        _touched_rejected(p.block64(att)[1], p.out_ref, p.block_bound, 320, f"block, {what}", sharp, None if rows is None else rows[:, None], p.floor)


def _pixels(p, t):
    """token rows [T, C] -> [B * HW, F, C] by global pixel, and back"""
    return t.reshape(p.B, p.F, p.HW, -1).permute(0, 2, 1, 3).reshape(p.B * p.HW, p.F, -1)


def _tokens(p, t):
    return t.reshape(p.B, p.HW, p.F, -1).permute(0, 2, 1, 3).reshape(p.T, -1)


def _partner(npix):
    """the other pixel of a wave's pair (pixels 2i, 2i + 1 of the clip batch); an unpaired last pixel is its own"""
    g = torch.arange(npix)
    return torch.where((g ^ 1) < npix, g ^ 1, g)


FAULT_SHAPES = [(B, HW, Fr) for Fr in (2, 3, 13, 14, 15) for B, HW in ((1, 7), (1, 9), (3, 13), (2, 24))]


@pytest.mark.parametrize("B,HW,Fr", FAULT_SHAPES + [(1, 16, 14), (3, 48, 3)])
def test_fused_padded_slot_counted_as_a_key(B, HW, Fr):
    """slots >= F reload the last frame's row: unmasked, the last frame counts 17 - F times.  The identity form cannot see it (key
    and value of the duplicate are the target's own or carry no weight): it is the uniform form's fault"""
    p = ap.fused_probe("uniform", B, HW, Fr)
    w = torch.ones(Fr, dtype=torch.float64)
    w[Fr - 1] = 17 - Fr
    _fused_rejects(p, p.parts().out(w), f"last frame counted {17 - Fr} times", rows=torch.ones(p.T, dtype=torch.bool), front=HW % 16 == 0)


@pytest.mark.parametrize("B,HW,Fr", FAULT_SHAPES + [(1, 8, 1), (1, 16, 1), (2, 32, 16)])
def test_fused_other_pixels_keys_unmasked(B, HW, Fr):
    """without the block-diagonal mask a row is the mean over the 2 F rows of both pixels of its wave (uniform form; in the
    identity form the foreign codes stay >= 22 nats behind, by construction)"""
    p = ap.fused_probe("uniform", B, HW, Fr)
    a = _pixels(p, p.att_ref)
    pr = _partner(a.shape[0])
    paired = (pr != torch.arange(a.shape[0]))[:, None, None].expand(-1, Fr, 1)
    _fused_rejects(p, _tokens(p, (a + a[pr]) / 2), "both pixels' keys in one softmax", rows=_tokens(p, paired)[:, 0], front=HW % 16 == 0)


@pytest.mark.parametrize("kind", ["uniform", "identity"])
@pytest.mark.parametrize("B,HW,Fr", FAULT_SHAPES + [(2, 32, 16)])
def test_fused_pixels_of_a_wave_exchanged(B, HW, Fr, kind):
    p = ap.fused_probe(kind, B, HW, Fr)
    a = _pixels(p, p.att_ref)
    pr = _partner(a.shape[0])
    paired = (pr != torch.arange(a.shape[0]))[:, None, None].expand(-1, Fr, 1)
    _fused_rejects(p, _tokens(p, a[pr]), "the two pixels of a wave exchanged", every_element=True, rows=_tokens(p, paired)[:, 0], front=HW % 16 == 0)


@pytest.mark.parametrize("kind", ["uniform", "identity"])
@pytest.mark.parametrize("B,HW,Fr", FAULT_SHAPES + [(1, 1, 16), (3, 48, 2)])
def test_fused_head_reads_its_neighbours_value_rows(B, HW, Fr, kind):
    p = ap.fused_probe(kind, B, HW, Fr)
    v = torch.roll(p.qkv64()[2], -64, dims=1)                    # head h multiplies its probabilities with head h + 1's rows
    _fused_rejects(p, p.parts(v=v).out(), "V rows of head h + 1", every_element=True, rows=torch.ones(p.T, dtype=torch.bool), front=HW % 16 == 0)


@pytest.mark.parametrize("B,HW,Fr", [c for c in FAULT_SHAPES if c[2] >= 13] + [(2, 32, 16)])
def test_fused_key_bias_reaches_only_some_keys(B, HW, Fr):
    """b_k on every key is softmax-invariant; on the keys of the even frames alone it reorders the scores (identity form; the
    uniform form has q = 0).  A (row, head) whose selection it changes is an O(1) error; one whose target merely loses part of its
    lead moves by less than the bound, so the condition here is on the rows that select another frame.  (F >= 13: two or three
    random codes are nearly orthogonal, their margin of about 8 c nats is out of the bias's reach)"""
    p = ap.fused_probe("identity", B, HW, Fr)
    q, k, v = p.qkv64()
    odd = (torch.arange(p.T) // HW % Fr % 2 == 1)[:, None]
    parts = ap.Parts(p.lay, q, k - odd * p.bqkv[320:640], v)
    att = parts.out()
    moved = p.lay.out_tokens((parts.e.argmax(-1) != p.targets)[:, :, None].expand(-1, -1, 64).double())[:, ::64].bool()   # [T, heads]
    assert moved.any(), "the partial bias changes no selection"
    oob = _units(ap.out_of_bound(_kernel(att), p.att_ref, p.front_bound), 64)
    assert (oob | ~moved).all()
    oob = ap.out_of_bound(_kernel(p.block64(att)[1]), p.out_ref, p.block_bound).any(1)
    assert (oob | ~moved.any(1)).all()


@pytest.mark.parametrize("kind", ["uniform", "identity"])
@pytest.mark.parametrize("B,HW,Fr", FAULT_SHAPES + [(1, 1, 1), (1, 8, 16)])
def test_tblock_out_projection_columns_of_two_heads_exchanged(B, HW, Fr, kind):
    if Fr < 2 and kind == "identity":
        return
    p = ap.fused_probe(kind, B, HW, Fr)
    for h in range(4):
        wo = p.wo.clone()
        wo[:, 64 * h:64 * h + 64], wo[:, 64 * h + 64:64 * h + 128] = p.wo[:, 64 * h + 64:64 * h + 128], p.wo[:, 64 * h:64 * h + 64]
        _touched_rejected(p.block64(p.att_ref, wo=wo)[1], p.out_ref, p.block_bound, 320, f"W_o chunks of heads {h} and {h + 1} exchanged",
                          p.kind == "identity", torch.ones(p.T, 1, dtype=torch.bool), p.floor)


@pytest.mark.parametrize("kind", ["uniform", "identity"])
@pytest.mark.parametrize("B,HW,Fr", [c for c in FAULT_SHAPES if (c[0] * c[1]) % 8])
def test_tblock_dead_pixel_stored_over_a_live_one(B, HW, Fr, kind):
    """the dead pixels of a ragged last panel are clamped to the last live pixel; their rows are never stored.  Stored one pixel
    slot early, they replace the rows of the last pixel's neighbour"""
    p = ap.fused_probe(kind, B, HW, Fr)
    o = _pixels(p, p.out_ref).clone()
    o[-2] = o[-1]
    hit = torch.zeros(B * HW, Fr, 1, dtype=torch.bool)
    hit[-2] = True
    _touched_rejected(_tokens(p, o), p.out_ref, p.block_bound, 320, "clamped pixel over its neighbour", p.kind == "identity", _tokens(p, hit), p.floor)


@pytest.mark.parametrize("kind", ["uniform", "identity"])
@pytest.mark.parametrize("Fr", [2, 3, 13, 14, 15, 16])
def test_tblock_batch_index_of_a_straddling_pair_from_its_first_pixel(Fr, kind):
    """B = 3, HW = 13: pixels 12 and 13 of the clip batch share a wave, 12 = (entry 0, pixel 12), 13 = (entry 1, pixel 0).  With the
    first pixel's entry, pixel 13 becomes 'pixel 13 of entry 0': its rows are read HW rows too early"""
    B, HW = 3, 13
    p = ap.fused_probe(kind, B, HW, Fr)
    src = torch.arange(p.T)
    f = torch.arange(Fr)
    rows = (1 * Fr + f) * HW + 0
    src[rows] = (0 * Fr + f) * HW + HW
    out = p.block64(p.parts(z=p.z[src]).out(), x=p.x64[src])[1]
    hit = torch.zeros(p.T, 1, dtype=torch.bool)
    hit[rows] = True
    _touched_rejected(out, p.out_ref, p.block_bound, 320, "straddling pair", False, hit, p.floor)


@pytest.mark.parametrize("kind", ["uniform", "identity"])
def test_tblock_row_bias_index_off_by_one_row(kind):
    B, HW, Fr = ap.TBLOCK_ROWBIAS
    p = ap.fused_probe(kind, B, HW, Fr, True)
    for shift in (1, -1):
        idx = ap.rowmap_index(p.T, p.rowmap, shift)
        assert (idx != p.idx).all()
        _touched_rejected(p.block64(p.att_ref, idx=idx)[1], p.out_ref, p.block_bound, 320, f"table row of token row {shift:+d}", True,
                          torch.ones(p.T, 1, dtype=torch.bool), p.floor)


# ================================================================================================== relative-position bias
RELBIAS_CASES = ap.relbias_cases()


@pytest.mark.parametrize("make", [c[1] for c in RELBIAS_CASES], ids=[c[0] for c in RELBIAS_CASES])
def test_relbias_rounded_reference_uses_at_most_half_the_bound(make):
    p = make()
    assert p.check(_kernel(p.ref), "fp16-rounded reference", limit=0.5) <= 0.5
    lay, S = p.lay, p.lay.Lk
    assert p.table.dtype == torch.float32 and tuple(p.table.shape) == (lay.heads, 2 * S - 1)
    if p.kind in ("uniform", "identity"):
        # a zero table changes nothing, and scale 1.0 only sharpens the identity probe's selection
        assert not p.table.any()
        assert (p.ref - ap.dense_probe(p.kind, lay.nb, S, lay.heads, lay.hd).ref).abs().max() <= 2.0 ** -18
        return
    assert not p.q.any() and p.scale == lay.hd ** -0.5
    if p.kind == "weighted":
        # row i is sum_j w[h, j - i + S - 1] v_j / sum_j w[h, j - i + S - 1] (the table is ln w rounded to fp32)
        i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
        w = p.info["w"].double()[:, j - i + S - 1].repeat(lay.nb, 1, 1)
        want = lay.out_tokens((w @ lay.kv_groups(p.v.double())) / w.sum(-1, keepdim=True))
        assert (p.ref - want).abs().max() < 2.0 ** -20


def test_relbias_offsets_cover_the_edges():
    for nb, S, heads, hd in ap.RELBIAS_SHAPES:
        tables = ap.relbias_offsets(S, heads, hd)
        seen = {d for t in tables for d in t}
        assert all(len(t) == heads for t in tables)
        assert {d for d in (0, 1, -1, S - 1, 1 - S, 64, -64) if abs(d) < S} <= seen and all(abs(d) < S for d in seen)
        if S > 2:
            assert all(len(set(t)) > 1 for t in tables[:-1]), "a table whose heads all share one offset cannot tell the heads apart"


def _flat(table, pad):
    return torch.cat([table.reshape(-1), torch.zeros(pad)])


RELBIAS_FAULTS = {
    # fault -> (table the faulty kernel effectively uses, heads it must touch in the weighted probe)
    "table transposed (i - j for j - i)": lambda t, S, scale: t.flip(1),
    "head stride 2S": lambda t, S, scale: torch.stack([_flat(t, t.shape[0])[h * 2 * S:h * 2 * S + 2 * S - 1] for h in range(t.shape[0])]),
    "base off by one": lambda t, S, scale: torch.stack([_flat(t, 1)[h * (2 * S - 1) + 1:(h + 1) * (2 * S - 1) + 1] for h in range(t.shape[0])]),
    "bias multiplied by scale": lambda t, S, scale: t * scale,
}


@pytest.mark.parametrize("fault", list(RELBIAS_FAULTS))
@pytest.mark.parametrize("nb,S,heads,hd", [c for c in ap.RELBIAS_SHAPES if c[1] > 1], ids=lambda v: str(v))
def test_relbias_faults_are_rejected(nb, S, heads, hd, fault):
    """every (row, head) whose fp64 result the fault changes misses the bound; the weighted probe is touched in every head the fault
    can reach, the offset tables together in every head"""
    probes = [ap.relbias_weighted_probe(nb, S, heads, hd)] + [ap.relbias_offset_probe(nb, S, heads, hd, o) for o in ap.relbias_offsets(S, heads, hd)]
    first = 1 if fault == "head stride 2S" else 0
    reached = torch.zeros(heads, dtype=torch.bool)
    for p in probes:
        bad = RELBIAS_FAULTS[fault](p.table, S, p.scale)
        if torch.equal(bad, p.table):
            continue
        out = p.parts(bias=ap.relbias_scores(bad, p.lay)).out()
        if not ((out - p.ref).abs() > p.floor).any():
            assert p.kind == "offset"                       # (d = 0 is its own transpose)
            continue
        tu = _touched_rejected(out, p.ref, ap.REL * p.ref.abs() + p.floor, hd, f"{p.kind} probe, {fault}", floor=p.floor)
        if p.kind == "weighted":
            assert tu[:, first:].all() and not tu[:, :first].any()
        reached |= tu.any(0)
    assert reached[first:].all()
