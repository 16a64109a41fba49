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
roundings; the floor covers what S e^-22 of foreign keys can add.  A wrong key is an O(1) error."""
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

    def __init__(self, lay, q, k, v, scale=None, gmap=None):
        self.lay = lay
        scale = lay.hd ** -0.5 if scale is None else scale
        gm = lay.gmap() if gmap is None else gmap
        qg = lay.q_groups(q.double())
        kk = lay.kv_groups(k.double())[gm]
        self.vv = lay.kv_groups(v.double())[gm]
        s = qg @ kk.transpose(1, 2) * scale
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
    def __init__(self, kind, lay, q, k, v, floor, ref=None, **info):
        self.kind, self.lay, self.q, self.k, self.v, self.floor = kind, lay, q, k, v, floor
        self.info = info
        self._ref = ref

    def parts(self, gmap=None):
        """the softmax pieces, for a test that injects a fault (not kept: [groups, Lq, Lk] in fp64)"""
        return Parts(self.lay, self.q, self.k, self.v, gmap=gmap)

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
