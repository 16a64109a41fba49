"""Probe inputs for the attention kernels: data on which EVERY key of EVERY row is individually decisive, an fp64 reference and
per-element bounds that are derived, not tuned.  CPU only; imports no kernel (tests/test_attn_probes_cpu.py shows that the probes
reject the faults they are meant for, tests/test_attn_probes_gpu.py runs them on every attention entry point).

Uniform probe: q = 0, so every score is 0, exp2(0) = 1 exactly, and an output row is the plain mean of the value rows of its
(kv-mapped batch entry, head).  The sums are exact (to fp32 accumulation); what is left are at most two fp16 roundings of 2^-11,
the probability and the output.  Bound: |got - ref| <= 2^-9 |ref| + 2^-20, twice their sum.  A key that is dropped or counted
twice moves a row by |v| / S, tens to thousands of times the bound.

Identity probe: distinct sign codes s_j in {-1, +1}^D, k_j = c s_j, q_i = s_pi(i).  With scale D^-0.5 the target key outscores
every other by c (D - max offdiag) / sqrt(D) nats; c is the smallest power of two that makes this >= 22 nats, so that
1 - p_target < 2^-20 and the output row is the value row pi(i).  Bound: |got - ref| <= 2^-9 |ref| + 2^-16: the same two
roundings; the floor covers what S e^-22 of foreign keys can add.  A wrong key is an O(1) error.

Relative-position bias (lkgd_attn_dense_relbias, attn_dense.h with RELBIAS): Parts takes an additive score term, built from
relbias[h, j - i + S - 1].  Three probes: the two above under an all-zero table (scale 1.0 and hd^-0.5; bounds unchanged); the
offset probe (q = 0, one table entry of 32 nats per head at offset d_h: row i is value row i + d_h, or the mean of all value rows
where that row does not exist; S e^-32 < 2^-37, so the identity bound holds with room); the weighted probe (q = 0, table = ln w,
integer w in 1..8: a row is the w-weighted mean).  attn_dense.h keeps score, exponential, sum and P.V in fp32 and normalises in
fp32: the one fp16 rounding is the store, so the uniform bound (which allows two) holds for the weighted probe.

Fused temporal blocks (lkgd_tattn_block_c320 = attn_tblock.hip + attn_tblock_loop.inc, lkgd_tattn_front = attn_tfront.hip): q, k, v
are not inputs, x and the packed weights are, so FusedProbe builds x and signed-selection weights for which every intermediate is
an fp16 number: LayerNorm(x) = z in {-1, +1}^320 exactly, k = c P_h s + b_k, q = P_h s_target (identity) or 0 (uniform),
v = sigma_h * z[64 h : 64 h + 64] + b_v, W_o a signed permutation, b_o and the row-bias table in multiples of 1/4.  The fp16
roundings left in the sources:
  attn_tfront.hip   q * (log2(e) / 8) is packed to fp16 - the same factor on every entry (|q| = 1), so it rescales all scores of
                    the probe alike and leaves uniform scores 0; P = p * (1 / l) packed as the B operand of V^T . P (2^-11); the
                    head's output packed for the store (2^-11).  Twice the sum: the bounds of the plain probes,
                    2^-9 |ref| + floor.
  attn_tblock.hip   the scale multiplies the fp32 scores; P = e * rcp(l) packed (v_cvt_pk_f16_f32, 2^-11 |o|); O^T packed as the B
                    operand of the out-projection (2^-11 |o|); W_o is a signed permutation, so y = +-o exactly; y + b_o + x
                    (+ table row) in fp32, one rounding at the store (2^-11 |out|).  The residual x is REBUILT in the epilogue as
                    z * sigma + mean with sigma = (var + eps) * rsq(var + eps) = sqrt(a^2 + eps) for a row of amplitude a: it
                    exceeds |x| = a by sqrt(a^2 + eps) - a (about eps / 2a: 10^-5 at a = 1/2), plus the rsq's ulp and three fp32
                    roundings (< 2^-21 a).  Twice the sum:
                        2^-9 |o_ref| + 2^-10 |out_ref| + 2 (sqrt(a^2 + eps) - a + 2^-21 a) + floor
                    o_ref = the out-projected attention term before bias and residual (the result can cancel against x).  The
                    rebuild term only matters where the result cancels to less than about 2^-6.
The uniform form sees what the identity form cannot: a padded frame slot that is not masked repeats the LAST frame's own key and
value (the last frame counted 17 - F times), and the other pixel's keys, >= 22 nats behind in the identity form, make a row the
mean over 2 F rows."""
import math
import zlib

import torch

REL = 2.0 ** -9
UNIFORM_FLOOR = 2.0 ** -20
IDENTITY_FLOOR = 2.0 ** -16
MARGIN_NATS = 22.0


def seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode())


def _gen(*key):
    return torch.Generator().manual_seed(seed_of(*key))


def _h(x):
    return x.to(torch.float16)


# ================================================================================================== layouts
class Layout:
    """how the token matrices of an entry point fall into attention groups (one group = the rows that share a key set)

    seq     q [nb*Lq, heads*hd], k / v [nb*Lk, heads*hd]; group = (batch entry, head)             attn_spatial, attn_dense
    frames  q [nb*Lq*S, heads*hd], row = (b*Lq + f)*S + s, k / v likewise with Lk frames;
            group = (batch entry, pixel, head), the sequence is the frame axis                    attn_temporal
    ctx     q [T, heads*hd], k / v [nb*Lk, heads*hd] (nb contexts); group = (row, head), one query each,
            against the keys of context ctx[row]                                                  attn_cross"""

    def __init__(self, kind, nb, heads, hd, Lq, Lk, kvmap=None, S=1, ctx=None):
        assert kind in ("seq", "frames", "ctx")
        self.kind, self.nb, self.heads, self.hd, self.Lq, self.Lk, self.S = kind, nb, heads, hd, Lq, Lk, S
        self.kvmap = list(kvmap) if kvmap is not None else None
        self.ctx = ctx
        self.T = len(ctx) if kind == "ctx" else None

    # rows of q / out that belong to one batch entry (for the failure report)
    @property
    def rows_per_entry(self):
        return {"seq": self.Lq, "frames": self.Lq * self.S, "ctx": 1}[self.kind]

    @property
    def q_rows(self):
        return self.T if self.kind == "ctx" else self.nb * self.Lq * self.S

    @property
    def kv_rows(self):
        return self.nb * self.Lk * self.S

    @property
    def width(self):
        return self.heads * self.hd

    @property
    def n_kv_groups(self):
        return self.nb * self.S * self.heads

    def _groups(self, x, L):
        nb, H, D, S = self.nb, self.heads, self.hd, self.S
        if self.kind == "frames":
            return x.reshape(nb, L, S, H, D).permute(0, 2, 3, 1, 4).reshape(nb * S * H, L, D)
        return x.reshape(nb, L, H, D).permute(0, 2, 1, 3).reshape(nb * H, L, D)

    def q_groups(self, x):
        if self.kind == "ctx":
            return x.reshape(self.T * self.heads, 1, self.hd)
        return self._groups(x, self.Lq)

    def kv_groups(self, x):
        return self._groups(x, self.Lk)

    def _tokens(self, g, L):
        nb, H, D, S = self.nb, self.heads, self.hd, self.S
        if self.kind == "frames":
            return g.reshape(nb, S, H, L, D).permute(0, 3, 1, 2, 4).reshape(nb * L * S, H * D)
        return g.reshape(nb, H, L, D).permute(0, 2, 1, 3).reshape(nb * L, H * D)

    def out_tokens(self, g):
        if self.kind == "ctx":
            return g.reshape(self.T, self.heads * self.hd)
        return self._tokens(g, self.Lq)

    def kv_tokens(self, g):
        return self._tokens(g, self.Lk)

    def gmap(self, kvmap="own"):
        """kv group of every query group"""
        H = self.heads
        if self.kind == "ctx":
            return (self.ctx.long()[:, None] * H + torch.arange(H)[None, :]).reshape(-1)
        kvmap = self.kvmap if kvmap == "own" else kvmap
        per = self.S * H                                   # groups per batch entry
        m = torch.tensor(kvmap if kvmap is not None else list(range(self.nb)), dtype=torch.long)
        return (m[:, None] * per + torch.arange(per)[None, :]).reshape(-1)


# ================================================================================================== fp64 attention
class Parts:
    """the pieces of an fp64 softmax attention, per group: e = exp(score - row max) [G, Lq, Lk], the value rows vv [G, Lk, D],
    numerator N = e . vv and denominator Z = sum e.  A fault that reweights a key or moves a value row is a rank-one change."""

    def __init__(self, lay, q, k, v, scale=None, gmap=None, bias=None):
        """bias: [G, Lq, Lk] (or anything that broadcasts against it), added to the scaled scores"""
        self.lay = lay
        scale = lay.hd ** -0.5 if scale is None else scale
        gm = lay.gmap() if gmap is None else gmap
        qg = lay.q_groups(q.double())
        kk = lay.kv_groups(k.double())[gm]
        self.vv = lay.kv_groups(v.double())[gm]
        s = qg @ kk.transpose(1, 2) * scale
        if bias is not None:
            s = s + bias
        self.e = torch.exp(s - s.amax(-1, keepdim=True))
        self.Z = self.e.sum(-1, keepdim=True)
        self.N = self.e @ self.vv

    def out(self, w=None):
        """attention with key j counted w[j] times (w: [Lk], or anything that broadcasts against [G, Lq, Lk])"""
        if w is None:
            return self.lay.out_tokens(self.N / self.Z)
        e = self.e * w
        return self.lay.out_tokens((e @ self.vv) / e.sum(-1, keepdim=True))

    def out_key_weight(self, j, w):
        """key j counted w times (0 = dropped, 2 = doubled)"""
        ej = self.e[:, :, j:j + 1] * (w - 1.0)
        return self.lay.out_tokens((self.N + ej * self.vv[:, None, j, :]) / (self.Z + ej))

    def out_v_rows_exchanged(self, j):
        """probability j paired with value row j + 1 and the other way round"""
        d = (self.e[:, :, j:j + 1] - self.e[:, :, j + 1:j + 2]) * (self.vv[:, None, j + 1, :] - self.vv[:, None, j, :])
        return self.lay.out_tokens((self.N + d) / self.Z)


def attend64(lay, q, k, v, scale=None, gmap=None, w=None):
    return Parts(lay, q, k, v, scale, gmap).out(w)


def sdpa64(q, k, v, nb, heads, hd=64, kvmap=None, temporal=None, scale=None):
    """softmax(q k^T scale) v in fp64 on token matrices: q [nb*Sq, heads*hd], k / v [nb*S, heads*hd] (Sq != S allowed), the K / V
    of batch entry kvmap[b] for the queries of entry b.  temporal = (Fq, F, S): rows are (b*Fr + f)*S + s and the attention runs
    over the frames of every (pixel, head) - the index map of attn_temporal.  scale defaults to hd^-0.5"""
    if temporal is not None:
        Fq, Fk, S = temporal
        lay = Layout("frames", nb, heads, hd, Fq, Fk, kvmap, S=S)
    else:
        lay = Layout("seq", nb, heads, hd, q.shape[0] // nb, k.shape[0] // nb, kvmap)
    return attend64(lay, q, k, v, scale)


def cross_ctx(T, rowmap):
    d1, m1, d2, md = rowmap[:4]
    c0 = rowmap[4] if len(rowmap) > 4 else 0
    rows = torch.arange(T)
    return ((rows // d1) * m1 + rows % d2 + c0) % md


# ================================================================================================== the check
def worst(got, ref, floor, rel=REL):
    """(ratio, flat index) of the element with the largest err / bound; a non-finite output counts as infinitely wrong"""
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    ratio = err / (rel * ref.abs() + floor)
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.reshape(-1).argmax())
    return float(ratio.reshape(-1)[i]), i


def check(got, ref, floor, what, rel=REL, rows_per_entry=None, limit=1.0):
    """every element: |got - ref| <= limit * (rel |ref| + floor).  Returns the worst err / bound; on failure names its row, column
    and batch entry"""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    ratio, i = worst(got, ref, floor, rel)
    if not ratio <= limit:
        row, col = divmod(i, ref.shape[1])
        g, r = float(got[row, col]), float(ref[row, col])
        entry = f", batch entry {row // rows_per_entry} row {row % rows_per_entry}" if rows_per_entry else ""
        n_bad = int((~((got.detach().double().cpu() - ref).abs() <= limit * (rel * ref.abs() + floor))).sum())
        raise AssertionError(f"{what}: err / bound = {ratio:.4g} (limit {limit:g}) at row {row}{entry}, column {col}: got {g!r}, "
                             f"ref {r!r}; {n_bad} of {ref.numel()} elements out of bound")
    return ratio


# ================================================================================================== builders
class Probe:
    def __init__(self, kind, lay, q, k, v, floor, ref=None, scale=None, table=None, **info):
        """scale: None = hd^-0.5; table: fp32 [heads, 2 Lk - 1], relbias[h, j - i + Lk - 1] joins the score of query i and key j"""
        self.kind, self.lay, self.q, self.k, self.v, self.floor = kind, lay, q, k, v, floor
        self.scale, self.table = scale, table
        self.info = info
        self._ref = ref

    def parts(self, gmap=None, bias="own"):
        """the softmax pieces, for a test that injects a fault (not kept: [groups, Lq, Lk] in fp64)"""
        if isinstance(bias, str):
            bias = relbias_scores(self.table, self.lay) if self.table is not None else None
        return Parts(self.lay, self.q, self.k, self.v, scale=self.scale, gmap=gmap, bias=bias)

    @property
    def ref(self):
        """fp64 softmax attention of the probe's inputs, computed once"""
        if self._ref is None:
            self._ref = self.parts().out()
        return self._ref

    def check(self, got, what, limit=1.0, floor=None, rel=REL):
        return check(got, self.ref, self.floor if floor is None else floor, f"{self.kind} probe, {what}", rel=rel,
                     rows_per_entry=self.lay.rows_per_entry, limit=limit)


def uniform_probe(lay, *key):
    g = _gen("uniform", *key)
    q = torch.zeros(lay.q_rows, lay.width, dtype=torch.float16)
    k = _h(torch.randn(lay.kv_rows, lay.width, generator=g))
    v = _h(torch.randn(lay.kv_rows, lay.width, generator=g))
    return Probe("uniform", lay, q, k, v, UNIFORM_FLOOR)


def _distinct_codes(n, D, g):
    """n distinct rows of {-1, +1}^D"""
    assert n <= 2 ** min(D, 30), f"{n} distinct sign codes do not exist in {D} dimensions"
    if D <= 16:
        idx = torch.randperm(2 ** D, generator=g)[:n]
        bits = (idx[:, None] >> torch.arange(D)[None, :]) & 1
        return (2 * bits - 1).double()
    while True:
        c = torch.randint(0, 2, (n, D), generator=g) * 2 - 1
        if torch.unique(c, dim=0).shape[0] == n:
            return c.double()


def identity_probe(lay, *key, targets=None, code_scope="group"):
    """code_scope: "group" draws the Lk codes of every kv group independently; "head" draws nb * Lk codes per head that are
    distinct across the batch entries / contexts too (attn_cross: a row sent to the wrong context meets none of its own codes).
    targets: [query groups, Lq] key index of every query row; default: per group a seeded permutation (Lq <= Lk) or map"""
    assert lay.Lk >= 2 or lay.kind == "frames", "one key: the identity probe says nothing the uniform probe does not"
    g = _gen("identity", *key)
    D, Lk, Gk = lay.hd, lay.Lk, lay.n_kv_groups
    if code_scope == "head":
        assert lay.S == 1
        per_head = torch.stack([_distinct_codes(lay.nb * Lk, D, g) for _ in range(lay.heads)])      # [H, nb*Lk, D]
        codes = per_head.reshape(lay.heads, lay.nb, Lk, D).permute(1, 0, 2, 3).reshape(Gk, Lk, D)
    else:
        codes = torch.stack([_distinct_codes(Lk, D, g) for _ in range(Gk)])                          # [Gk, Lk, D]
    gm = lay.gmap()
    G = gm.shape[0]
    if targets is None:
        if lay.Lq <= Lk:
            targets = torch.stack([torch.randperm(Lk, generator=g)[:lay.Lq] for _ in range(G)])
        else:
            targets = torch.randint(0, Lk, (G, lay.Lq), generator=g)
    gram = codes @ codes.transpose(1, 2)
    gram.diagonal(dim1=1, dim2=2).fill_(-float("inf"))
    maxoff = float(gram.max()) if Lk > 1 else -float(D)
    assert maxoff < D, "codes are not distinct"
    c = 1
    while c * (D - maxoff) / math.sqrt(D) < MARGIN_NATS:
        c *= 2
    assert c <= 64, f"no c <= 64 separates the codes by {MARGIN_NATS} nats (max off-diagonal {maxoff} of {D})"
    qg = torch.gather(codes[gm], 1, targets[:, :, None].expand(G, lay.Lq, D))
    q = _h(lay.out_tokens(qg))
    k = _h(lay.kv_tokens(c * codes))
    v = _h(torch.randn(lay.kv_rows, lay.width, generator=g))
    p = Probe("identity", lay, q, k, v, IDENTITY_FLOOR, c=c, margin=c * (D - maxoff) / math.sqrt(D), codes=codes, targets=targets)
    # the builder's own condition: every row puts all but 2^-20 of its weight on its target key
    parts = p.parts()
    e_t = torch.gather(parts.e, 2, targets[:, :, None])
    rest = ((parts.Z - e_t) / parts.Z).max().item()
    assert rest < 2.0 ** -20, f"1 - p_target = {rest:.3g} (c = {c}, margin {p.info['margin']:.1f} nats)"
    p.info["one_minus_p"] = rest
    p._ref = parts.out()
    return p


# ================================================================================================== the cases of the GPU file
KVMAPS_SPATIAL = (None, (1, 2, 0), (2, 0, 0))          # (1, 2, 0) is not its own inverse
KVMAPS_TEMPORAL = (None, (1, 2, 0), (2, 2, 2))
SPATIAL_NB, SPATIAL_HEADS = 3, 2
# (S, Sq) of the compiler-scheduled programs and of the software-pipelined one (unmasked, masked, Sq != S)
SPATIAL_PLAIN = [(16, 16), (64, 64), (65, 65), (129, 129), (200, 200), (255, 255), (256, 256), (577, 577),
                 (200, 72), (577, 1), (256, 129)]
SPATIAL_PIPE = [(128, 128), (256, 256), (384, 384), (640, 640),
                (129, 129), (255, 255), (200, 200), (300, 300), (1000, 1000),
                (777, 100), (1152, 1100)]
SPATIAL_PACKED = {"plain": 200, "pipe": 300}           # q | k | v as column blocks of one [T, 3C] matrix
TEMPORAL_B = 3
TEMPORAL_F = [1, 2, 3, 14, 16, 17, 25, 32]
TEMPORAL_SH = [(8, 2), (5, 3), (1, 1)]                 # 16, 15 and 1 (pixel, head) pairs
# (T, heads, NC, Lk, rowmap, ld): the four of test_attn_cross_short_contexts and T = 257 against two keys
CROSS = [(700, 2, 3, 5, (250, 1, 1, 1 << 30), 128), (513, 3, 2, 77, (1 << 20, 0, 2, 2), 200),
         (300, 1, 4, 1, (60, 7, 1, 4, 2), 64), (40, 5, 2, 128, (16, 1, 1, 2), 320),
         (257, 2, 3, 2, (100, 1, 1, 1 << 30), 136)]
# (nb, S, heads, head_dim)
DENSE = [(2, 257, 2, 80), (1, 17, 2, 80), (3, 50, 2, 128), (2, 64, 2, 64), (2, 65, 1, 64), (1, 63, 1, 8), (1, 1, 2, 8)]

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def temporal_fqs(F):
    return sorted({F, 1, max(F - 1, 1)})


def spatial_probe(kind, S, Sq, kvmap):
    """the reference is computed once per (S, Sq, kv map) and shared by every program that runs the case"""
    key = ("spatial", kind, S, Sq, kvmap)
    lay = Layout("seq", SPATIAL_NB, SPATIAL_HEADS, 64, Sq, S, kvmap)
    return _cached(key, lambda: (uniform_probe if kind == "uniform" else identity_probe)(lay, *key))


def temporal_probe(kind, F, Fq, S, heads, kvmap):
    """identity: codes and targets drawn independently per (batch entry, pixel, head)"""
    key = ("temporal", kind, F, Fq, S, heads, kvmap)
    lay = Layout("frames", TEMPORAL_B, heads, 64, Fq, F, kvmap, S=S)
    return _cached(key, lambda: (uniform_probe if kind == "uniform" else identity_probe)(lay, *key))


def cross_probe(kind, T, heads, NC, Lk, rowmap):
    """identity: row m targets key m % Lk of the context its row map selects; codes distinct across all NC * Lk keys of a head"""
    key = ("cross", kind, T, heads, NC, Lk, rowmap)
    lay = Layout("ctx", NC, heads, 64, 1, Lk, ctx=cross_ctx(T, rowmap))
    if kind == "uniform":
        return _cached(key, lambda: uniform_probe(lay, *key))
    targets = (torch.arange(T) % Lk)[:, None].expand(T, heads).reshape(T * heads, 1)
    return _cached(key, lambda: identity_probe(lay, *key, targets=targets, code_scope="head"))


def dense_probe(kind, nb, S, heads, hd):
    key = ("dense", kind, nb, S, heads, hd)
    lay = Layout("seq", nb, heads, hd, S, S)
    return _cached(key, lambda: (uniform_probe if kind == "uniform" else identity_probe)(lay, *key))


# ================================================================================================== relative-position bias
def relbias_scores(table, lay):
    """table [heads, 2S - 1] -> the additive score term [nb * heads, S, S]: entry [b * heads + h, i, j] = table[h, j - i + S - 1]"""
    S = lay.Lk
    assert lay.kind == "seq" and lay.Lq == S and tuple(table.shape) == (lay.heads, 2 * S - 1)
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    return table.double()[:, j - i + S - 1].repeat(lay.nb, 1, 1)


RELBIAS_SHAPES = [(2, 1, 2, 8), (1, 7, 3, 64), (2, 63, 2, 64), (2, 64, 2, 64), (1, 65, 3, 80), (2, 226, 2, 64), (1, 257, 2, 128)]
RELBIAS_PEAK = 32.0           # nats: S e^-32 < 2^-37 is left for the other keys


def relbias_zero_probe(kind, nb, S, heads, hd, scale):
    """the plain probes of dense_probe with an all-zero table; scale 1.0 is what T5 passes.  The identity probe's c is chosen for
    hd^-0.5, so scale 1.0 only widens its margin"""
    base = dense_probe(kind, nb, S, heads, hd)
    key = ("relbias-zero", kind, nb, S, heads, hd, scale)
    assert scale is None or scale >= hd ** -0.5

    def make():
        p = Probe(kind, base.lay, base.q, base.k, base.v, base.floor, scale=scale, table=torch.zeros(heads, 2 * S - 1), **base.info)
        return p
    return _cached(key, make)


def relbias_offsets(S, heads, hd):
    """the offset tables of a shape: a list of per-head offset lists that jointly cover 0, +-1, +-(S - 1), +-64 and a seeded one;
    the heads of one table get different offsets wherever the shape has two"""
    ds = [0, 1, -1, S - 1, -(S - 1), 64, -64, int(torch.randint(-(S - 1), S, (1,), generator=_gen("relbias-d", S, heads, hd)))]
    ds = list(dict.fromkeys(d for d in ds if abs(d) <= S - 1))
    n = len(ds)
    while len(ds) % heads:                                 # the last table is filled up from the front of the list
        ds.append(ds[(len(ds) - n) % n])
    return [ds[t:t + heads] for t in range(0, len(ds), heads)]


def relbias_offset_probe(nb, S, heads, hd, offsets):
    """q = 0, table[h, d_h + S - 1] = 32 and 0 elsewhere: row i is value row i + d_h where that exists, else the mean of all.
    Checked with the identity floor; the scale argument (hd^-0.5) must not reach the table"""
    key = ("relbias-offset", nb, S, heads, hd, tuple(offsets))

    def make():
        lay = Layout("seq", nb, heads, hd, S, S)
        u = uniform_probe(lay, *key)
        table = torch.zeros(heads, 2 * S - 1)
        for h, d in enumerate(offsets):
            table[h, d + S - 1] = RELBIAS_PEAK
        p = Probe("offset", lay, u.q, u.k, u.v, IDENTITY_FLOOR, scale=hd ** -0.5, table=table, offsets=tuple(offsets))
        # the builder's own condition: the reference IS the selected value row, or the mean
        vg = lay.kv_groups(u.v.double())                                             # [nb * heads, S, hd]
        want = vg.mean(1, keepdim=True).expand(-1, S, -1).clone()
        for h, d in enumerate(offsets):
            i = torch.arange(max(0, -d), min(S, S - d))
            want[h::heads, i] = vg[h::heads, i + d]
        assert (p.ref - lay.out_tokens(want)).abs().max() < 2.0 ** -30
        return p
    return _cached(key, make)


def relbias_weighted_probe(nb, S, heads, hd):
    """q = 0, table[h, d] = ln w with seeded integers 1 <= w <= 8: a row is the w-weighted mean of its value rows.  attn_dense.h
    keeps scores, probabilities and sums in fp32 and rounds once, at the store: the uniform bound"""
    key = ("relbias-weighted", nb, S, heads, hd)

    def make():
        lay = Layout("seq", nb, heads, hd, S, S)
        u = uniform_probe(lay, *key)
        w = torch.randint(1, 9, (heads, 2 * S - 1), generator=_gen(*key, "w"))
        return Probe("weighted", lay, u.q, u.k, u.v, UNIFORM_FLOOR, scale=hd ** -0.5, table=torch.log(w.double()).float(), w=w)
    return _cached(key, make)


def relbias_cases():
    """(id, thunk) of every probe test_attn_dense_relbias runs"""
    out = []
    for nb, S, heads, hd in RELBIAS_SHAPES:
        for scale in (1.0, None):
            for kind in kinds(S):
                out.append((f"relbias-zero-{kind}-S{S}-hd{hd}-scale{scale}", lambda a=(kind, nb, S, heads, hd, scale): relbias_zero_probe(*a)))
        for offs in relbias_offsets(S, heads, hd):
            out.append((f"relbias-offset-S{S}-hd{hd}-d{offs}", lambda a=(nb, S, heads, hd, offs): relbias_offset_probe(*a)))
        out.append((f"relbias-weighted-S{S}-hd{hd}", lambda a=(nb, S, heads, hd): relbias_weighted_probe(*a)))
    return out


# ================================================================================================== fused temporal blocks
TB_C, TB_HEADS, TB_HD = 320, 5, 64
TB_EPS = 1e-5
FUSED_F = [1, 2, 3, 13, 14, 15, 16]
TBLOCK_BHW = [(1, 1), (1, 7), (1, 8), (1, 9), (3, 13), (2, 24)]
TBLOCK_MANY = (3, 1371, 5)                   # (B, HW, F): 515 panels, more than CUs, the last one ragged
TBLOCK_ROWBIAS = (2, 24, 14)                 # (B, HW, F) of the case with the row-bias table
TBLOCK_LDX = (3, 13, 13)                     # x with a row pitch of its own
TBLOCK_LDO = (1, 9, 15)                      # out with a row pitch of its own
TFRONT_BHW = [(1, 16), (2, 32), (3, 48)]
TFRONT_LDX = (2, 32, 13)
TFRONT_LDO = (1, 16, 15)


def tblock_rowmap(F, HW):
    """the row map of tests/test_tblock_gpu.py::test_tblock_row_bias_and_sharp_scores: ((row / d1) * m1 + row % d2 + c0) % md"""
    return (F * HW, HW, HW, 4, 3)


def rowmap_index(T, rowmap, shift=0):
    rows = torch.arange(T) + shift
    return ((rows // rowmap[0]) * rowmap[1] + rows % rowmap[2] + rowmap[4]) % rowmap[3]


def _quarters(shape, g, lo=-4, hi=4, nonzero=False):
    """seeded multiples of 1/4"""
    t = torch.randint(lo, hi + 1, shape, generator=g)
    if nonzero:
        t = torch.where(t == 0, torch.ones_like(t), t)
    return t.double() / 4


class FusedProbe:
    """Inputs of lkgd_tattn_block_c320 / lkgd_tattn_front on which every intermediate of the fused chain is exact.

    x [B*F*HW, 320], row = (b*F + f)*HW + pixel, every row a_row * z with z in {-1, +1}^320, sum(z) = 0 and a_row a power of two:
    mean = 0 and E[x^2] = a^2 are exact, so LayerNorm gives z / sqrt(1 + eps / a^2), which rounds to z in fp16.  Channels of z:
    [0, 64) the token's key code s(b, pixel, f), [64, 128) / [128, 192) the codes of its target frames pi_A(f) / pi_B(f) (even / odd
    heads), [192, 256) a payload, [256, 320) the entries that balance the sum.  The weights are signed selections (module
    docstring), so q, k, v are small multiples of 1/4 and their fp16 packing is exact; W_q = 0 in the uniform form."""

    def __init__(self, kind, B, F, HW, rowbias=False):
        assert kind in ("uniform", "identity") and 1 <= F <= 16 and (kind == "uniform" or F >= 2)
        self.kind, self.B, self.F, self.HW = kind, B, F, HW
        self.T = T = B * F * HW
        npix = B * HW
        self.lay = Layout("frames", B, TB_HEADS, TB_HD, F, F, S=HW)
        self.floor = UNIFORM_FLOOR if kind == "uniform" else IDENTITY_FLOOR
        g = _gen("fused", B, F, HW)                       # both forms share x, W_v, b_v, W_o, b_o
        D = TB_HD
        # ---- codes: F distinct sign rows per pixel, drawn independently per pixel
        codes = torch.randint(0, 2, (npix, F, D), generator=g) * 2 - 1
        while True:
            gram = (codes.double() @ codes.double().transpose(1, 2)) - 2.0 * D * torch.eye(F, dtype=torch.float64)
            bad = (gram.amax((1, 2)) >= D).nonzero().reshape(-1)
            if not len(bad):
                break
            codes[bad] = torch.randint(0, 2, (len(bad), F, D), generator=g) * 2 - 1
        self.maxoff = float(gram.max()) if F > 1 else -float(D)
        pi_a = torch.argsort(torch.rand(npix, F, generator=g), dim=1)
        pi_b = torch.roll(pi_a, -1, dims=1)                # pi_B(f) = pi_A(f + 1): differs from pi_A in every frame (F >= 2)
        self.codes, self.pi = codes, (pi_a, pi_b)

        def rows(t):                                       # [npix, F, n] (b, pixel, f) -> token rows (b, f, pixel)
            return t.reshape(B, HW, F, -1).permute(0, 2, 1, 3).reshape(T, -1)
        own = rows(codes)
        ta = rows(torch.gather(codes, 1, pi_a[:, :, None].expand(-1, -1, D)))
        tb = rows(torch.gather(codes, 1, pi_b[:, :, None].expand(-1, -1, D)))
        pay = torch.randint(0, 2, (T, D), generator=g) * 2 - 1
        while True:
            t = (own + ta + tb + pay).sum(1)
            bad = (t.abs() > D).nonzero().reshape(-1)
            if not len(bad):
                break
            pay[bad] = torch.randint(0, 2, (len(bad), D), generator=g) * 2 - 1
        npos = (D - t) // 2                                # +1 entries of the balancing block: their sum is -t
        order = torch.argsort(torch.rand(T, D, generator=g), dim=1)
        bal = torch.where(order < npos[:, None], 1, -1)
        self.z = torch.cat([own, ta, tb, pay, bal], dim=1).double()
        assert not self.z.sum(1).any() and self.z.abs().eq(1).all()
        self.amp = 2.0 ** torch.randint(-1, 3, (T,), generator=g).double()      # 1/2, 1, 2, 4
        self.x64 = self.z * self.amp[:, None]
        self.x = _h(self.x64)
        # ---- weights: signed selections
        c = 1
        while c * (D - self.maxoff) / math.sqrt(D) < MARGIN_NATS:
            c *= 2
        assert c <= 64
        self.c, self.margin = c, c * (D - self.maxoff) / math.sqrt(D)
        wq, wk, wv = (torch.zeros(TB_C, TB_C, dtype=torch.float64) for _ in range(3))
        for h in range(TB_HEADS):
            perm = torch.randperm(D, generator=g)
            sign = (torch.randint(0, 2, (D,), generator=g) * 2 - 1).double()
            sig_v = (torch.randint(0, 2, (D,), generator=g) * 2 - 1).double()
            r = torch.arange(D) + D * h
            wk[r, perm] = c * sign
            if kind == "identity":
                wq[r, D * (1 + h % 2) + perm] = sign
            wv[r, r] = sig_v
        self.wqkv = torch.cat([wq, wk, wv])
        # b_q = 0; b_k = c * (+-1 .. +-4): q . b_k is the same for every key of a row, so the softmax does not see it - but it is of the
        # size of the margin (a sum of 64 terms +-c m / 8, m = 1 .. 4: sd about 2.7 c nats against a margin of at most 8 c), so a K
        # bias that reaches only some of the keys moves the selection; b_v in multiples of 1/4
        self.bqkv = torch.cat([torch.zeros(TB_C, dtype=torch.float64), 4 * c * _quarters((TB_C,), g, nonzero=True), _quarters((TB_C,), g, nonzero=True)])
        self.operm = torch.randperm(TB_C, generator=g)
        self.osign = (torch.randint(0, 2, (TB_C,), generator=g) * 2 - 1).double()
        self.wo = torch.zeros(TB_C, TB_C, dtype=torch.float64)
        self.wo[torch.arange(TB_C), self.operm] = self.osign
        self.bo = _quarters((TB_C,), g)
        self.table = _quarters((4, TB_C), g) if rowbias else None
        self.rowmap = tblock_rowmap(F, HW) if rowbias else None
        self.idx = rowmap_index(T, self.rowmap) if rowbias else None
        # ---- the fp64 reference: attention output (lkgd_tattn_front), out-projected term and result (lkgd_tattn_block_c320)
        parts = self.parts()
        self.att_ref = parts.out()
        self.o_ref, self.out_ref = self.block64(self.att_ref)
        self.targets = torch.stack([pi_b if h % 2 else pi_a for h in range(TB_HEADS)], 1).reshape(npix * TB_HEADS, F)
        if kind == "identity":
            e_t = torch.gather(parts.e, 2, self.targets[:, :, None])
            self.one_minus_p = ((parts.Z - e_t) / parts.Z).max().item()
            assert self.one_minus_p < 2.0 ** -20, f"1 - p_target = {self.one_minus_p:.3g} (c = {c}, margin {self.margin:.1f} nats)"

    # ---- the chain in fp64, piecewise, so that a test can put one mistake into it
    def qkv64(self, z=None):
        y = (self.z if z is None else z) @ self.wqkv.T + self.bqkv
        return y.split(TB_C, dim=1)

    def parts(self, z=None, gmap=None, v=None):
        q, k, v0 = self.qkv64(z)
        return Parts(self.lay, q, k, v0 if v is None else v, gmap=gmap)

    def block64(self, att, x=None, wo=None, idx=None):
        """(out-projected attention term, result) of the block for the attention output att"""
        o = att @ (self.wo if wo is None else wo).T
        out = o + self.bo + (self.x64 if x is None else x)
        if self.table is not None:
            out = out + self.table[self.idx if idx is None else idx]
        return o, out

    # ---- bounds
    @property
    def front_bound(self):
        """lkgd_tattn_front: P (the fp16 B operand of V^T . P) and the stored row - the bound of the plain probes"""
        return REL * self.att_ref.abs() + self.floor

    @property
    def block_bound(self):
        """lkgd_tattn_block_c320 (module docstring): P, the packed O^T, the stored result, the rebuilt residual"""
        a = self.amp[:, None]
        resid = (torch.sqrt(a * a + TB_EPS) - a) + 2.0 ** -21 * a
        return REL * self.o_ref.abs() + REL / 2 * self.out_ref.abs() + 2 * resid + self.floor

    def where(self, row):
        bf, pix = divmod(row, self.HW)
        return f", batch entry {bf // self.F} pixel {pix} frame {bf % self.F}"

    def check_front(self, got, what, limit=1.0):
        return check_bound(got, self.att_ref, self.front_bound, f"{self.kind} probe, {what}", limit, self.where,
                           lambda col: f" (head {col // TB_HD} channel {col % TB_HD})")

    def check_block(self, got, what, limit=1.0):
        return check_bound(got, self.out_ref, self.block_bound, f"{self.kind} probe, {what}", limit, self.where,
                           lambda col: f" (= {self.osign[col]:+.0f} x head {int(self.operm[col]) // TB_HD} channel {int(self.operm[col]) % TB_HD})")


def out_of_bound(got, ref, bound, limit=1.0):
    """[rows, columns] bool: the elements that miss limit * bound (a non-finite output misses it)"""
    got = got.detach().double().cpu()
    return ~((got - ref).abs() <= limit * bound)


def check_bound(got, ref, bound, what, limit=1.0, where=None, column=None):
    """every element: |got - ref| <= limit * bound[element].  Returns the worst err / bound; a failure names its row (with
    where(row): batch entry, pixel, frame) and its column"""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    g = got.detach().double().cpu()
    ratio = (g - ref).abs() / bound
    ratio = torch.where(torch.isfinite(g), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.reshape(-1).argmax())
    worst_ratio = float(ratio.reshape(-1)[i])
    if not worst_ratio <= limit:
        row, col = divmod(i, ref.shape[1])
        n_bad = int(out_of_bound(got, ref, bound, limit).sum())
        raise AssertionError(f"{what}: err / bound = {worst_ratio:.4g} (limit {limit:g}) at row {row}{where(row) if where else ''}, "
                             f"column {col}{column(col) if column else ''}: got {float(g[row, col])!r}, ref {float(ref[row, col])!r}; "
                             f"{n_bad} of {ref.numel()} elements out of bound")
    return worst_ratio


def fused_probe(kind, B, HW, F, rowbias=False):
    return _cached(("fused", kind, B, HW, F, rowbias), lambda: FusedProbe(kind, B, F, HW, rowbias))


def fused_kinds(F):
    return ("uniform", "identity") if F >= 2 else ("uniform",)


def tblock_cases():
    """(B, HW, F, rowbias) of every shape test_tattn_block runs"""
    out = [(B, HW, F, False) for F in FUSED_F for B, HW in TBLOCK_BHW]
    return out + [TBLOCK_MANY + (False,), TBLOCK_ROWBIAS + (True,)]


def tfront_cases():
    return [(B, HW, F) for F in FUSED_F for B, HW in TFRONT_BHW]


def kinds(Lk):
    """both probes, except against a single key (then the identity probe is the uniform one)"""
    return ("uniform", "identity") if Lk >= 2 else ("uniform",)


def all_cases():
    """(id, builder thunk) of every probe the GPU file runs - the CPU file checks each of them"""
    out = []
    for S, Sq in sorted(set(SPATIAL_PLAIN + SPATIAL_PIPE)):
        for kvmap in KVMAPS_SPATIAL:
            for kind in kinds(S):
                out.append((f"spatial-{kind}-S{S}-Sq{Sq}-kv{kvmap}", lambda a=(kind, S, Sq, kvmap): spatial_probe(*a)))
    for F in TEMPORAL_F:
        for S, heads in TEMPORAL_SH:
            for Fq in temporal_fqs(F):
                for kvmap in KVMAPS_TEMPORAL:
                    for kind in ("uniform", "identity"):
                        out.append((f"temporal-{kind}-F{F}-Fq{Fq}-S{S}-h{heads}-kv{kvmap}",
                                    lambda a=(kind, F, Fq, S, heads, kvmap): temporal_probe(*a)))
    for T, heads, NC, Lk, rowmap, _ in CROSS:
        for kind in kinds(Lk):
            out.append((f"cross-{kind}-T{T}-Lk{Lk}", lambda a=(kind, T, heads, NC, Lk, rowmap): cross_probe(*a)))
    for nb, S, heads, hd in DENSE:
        for kind in kinds(S):
            out.append((f"dense-{kind}-S{S}-hd{hd}", lambda a=(kind, nb, S, heads, hd): dense_probe(*a)))
    return out
