"""Probe inputs for the fused LayerNorm + projection kernels (lkgd_ln_qkv_c320 / _c640 = qkv_fused.hip) and the one-launch feed-forward
(lkgd_ff_fused_c320 = ff_fused.hip, all four forms), with int64 / fp64 references, per-element bounds that are derived, not tuned, and
fp32 emulations of the kernels' arithmetic into which one mistake at a time can be put.  CPU only; imports no kernel
(tests/test_fused_probes_cpu.py shows that the emulations stay inside half of each bound and that the faults are rejected,
tests/test_fused_probes_gpu.py runs the probes on the device).

Rows.  Every row of x' is a * z, z in {-1, +1}^C with sum(z) = 0 and a in {1/2, 1, 2, 4} - the construction of
attn_probes.FusedProbe at any width: mean = 0 and E[x^2] = a^2 are exact in fp32 in any order of summation, and the kernels' one-pass
LayerNorm (rstd = rsq(var + eps), fmaf(x, rstd, -mean * rstd), eps = 1e-5) gives z / sqrt(1 + eps / a^2), which rounds to z in fp16.
24 channels of z are the bits of a code of the row index and 24 their complements (no two rows of a case agree; the low seven bits
are the row index mod 128), the rest is seeded and balanced; one seeded permutation spreads the channels over the k-steps.  With a
row-bias table the input is x = a z - pe[idx(row)], pe in multiples of 1/4: the kernel's fp32 x + pe is exact, and a wrong table row
unbalances the whole row.  Cases of more than 1024 rows draw their rows through a seeded map from 1024 source rows (eight classes of
128): no two rows of one panel, of adjacent panels or of panels a multiple of the grid apart share a source.

A. ln_qkv, bit for bit.
  dense   W in {-2 .. 2}, b in non-zero multiples of 1/4: the int64 reference W z + b (units of 1/4) stays below 512, so it is an fp16
          number, and fp32 accumulation of integers below 2^24 is exact in any order: the kernel must return exactly that.
  select  one entry +-1 per output row, b = +-(1 + 2^-12): b_hi = +-1, b_lo = +-2^-12 through pack_ln_proj's bias k-step.  The exact
          sum is +-2^-12 or +-(2 + 2^-12); the second rounds to +-2 (far from a tie), the first is an fp16 number.  A lost b_lo
          gives 0 where 2^-12 is due.  Output row m of block j (q, k, v) selects k-step (m + 7 j) mod C/16 and slot
          (m div C/16 + m + 7 j) mod 16: every channel three times; a tile of 32 rows meets every (half, slot) pair and 32
          consecutive k-steps - all 20 at C = 320; 32 of the 40 at C = 640, where a tile has fewer rows than k-steps (the window
          moves with the tile, and every (k-step, half, slot) is met three times over the matrix).

B. ff_fused: out = s_acc (W2 g + b2 + x') + r2 res2, g = fp16(hidden * gelu(gate)).
  switch  hidden rows dense in {-1, 0, 1} with integer bias, gate rows 8 * (+-selection): every gate is +-8.  In the kernel's
          arithmetic gelu(8) = 8 exactly and gelu(-8) * hidden (about -5e-15 |hidden|) flushes to 0 at the fp16 pack, so g is
          8 hidden or 0, exact in fp16 (|hidden| <= 256 asserted); W2 in {0, +-2^-8}: y is exact in fp32.  What is left
          (ff_fused.hip, epilogue): the residual REBUILT as z sigma + mean, sigma = (var + eps) rsq(var + eps) = sqrt(a^2 + eps) -
          above a by sqrt(a^2 + eps) - a, plus the rsq's ulp and the roundings of sigma and the fmaf (< 2^-21 a), as in
          attn_tblock.hip; four fp32 roundings of (y + b2 + x') s_acc + res2 r2, each below 2^-24 S with
          S = |s_acc| (|y| + |b2| + a) + |r2 res2|; one fp16 rounding at the store.  Twice the sum:
              bound = 2 (2^-11 |out_ref| + |s_acc| (sqrt(a^2 + eps) - a + 2^-21 a) + 2^-22 S) + 2^-24 (1 + |s_acc|)
          (the last term: an fp16-subnormal result or g is rounded by 2^-25 absolute).
  curve   hidden = b + w z_c in {+-1, +-2}; gate = b_g + sum_k +-2^(2 - k) z_code(k), k = 0 .. 6, over the seven low code bits with
          b_g = +-1/16: every multiple of 1/8 in (-8, 8] (b_g > 0) or [-8, 8) (b_g < 0), each hidden channel meeting all 128 values
          in any 128 consecutive source rows; W2 a signed selection, so an output element is one g.  Eight variants: four
          selections that together observe all 1280 hidden channels (every tile, every accumulator register, both half-waves) x the
          two signs of b_g.  Reference: hidden * x erfc(-x / sqrt 2) / 2 in fp64.  In the forms with a second residual
          res2 = -(s_acc / r2) x' where that ratio is a power of two (-x' / 2 otherwise), so the output is s_acc (g + b2) to the
          rebuild error and the store rounding is that of g, not of the residual.
              bound = switch bound + 2 * 2^-11 |s_acc y_ref| + |s_acc| |hidden| * 2 * gelu_term(gate)
          gelu_term is MEASURED: the fp32 emulation of the generated chain (gen_ff_asm.py::geglu_items; the same arithmetic as
          common.h::gelu_erf2) against fp64 erfc on the grid - GELU_ABS absolute, GELU_REL |gate| relative to the gate; the smaller
          of the two, doubled, enters the bound.  test_fused_probes_cpu.py re-measures both.
  The GEGLU epilogue of ops.gemm runs the same two probes on the rows z themselves: switch exact, curve within
  2 * 2^-11 |g_ref| + |hidden| * gelu_term(gate) + 2^-24.  M = 700 with interleave 80 plans the 256x320 program (gelu_erf2: the measured
  term); M = 260 with interleave 32 plans the 128x128 program, which evaluates 0.5 x (1 + erff(x / sqrt 2)) - its term is reasoned in
  gelu_term, not measured."""
import math

import torch

from attn_probes import _gen, _quarters, check_bound, out_of_bound, rowmap_index

EPS = 1e-5
PANEL = 128
NSRC = 1024
CODE_BITS = 24
NOMINAL_CUS = 256                      # what the CPU file plans the many-panel case with (the MI355X's count)
T_SMALL = [1, 31, 32, 33, 127, 128, 129, 128 * 7 + 5]
GELU_ABS = 3.3e-7                      # measured (test_gelu_term_is_the_measured_one): max |chain - fp64| over the grid
GELU_REL = 1.12e-7                     # measured: max |chain - fp64| / |gate|


def many_panels_T(cus):
    """workgroup 0 runs three panels, the others two, the last panel is ragged"""
    return PANEL * (2 * cus + 1) + 5


def r32(t):
    """round to fp32, keep fp64 storage"""
    return t.float().double()


def r16(t):
    """fp32 -> fp16 as the kernels convert, kept in fp64"""
    return t.float().half().double()


def f32c(v):
    return float(torch.tensor(v, dtype=torch.float64).float())


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ================================================================================================== rows
class Rows:
    """NSRC source rows of width C: z [n, C] in {-1, +1}, amp [n], the channel of code bit k"""

    def __init__(self, C, n=NSRC):
        g = _gen("fused-rows", C, n)
        i = torch.arange(n)
        hi = ((i >> 7) * 40503 + 977) % (1 << (CODE_BITS - 7))          # odd multiplier: injective in i >> 7
        code = (i & 127) | (hi << 7)
        assert torch.unique(code).numel() == n
        s = 2 * ((code[:, None] >> torch.arange(CODE_BITS)[None, :]) & 1) - 1
        rest = C - 2 * CODE_BITS
        order = torch.argsort(torch.rand(n, rest, generator=g), dim=1)
        bal = torch.where(order < rest // 2, 1, -1)
        perm = torch.randperm(C, generator=g)
        self.z = torch.cat([s, -s, bal], 1)[:, perm].double()
        self.code_channel = torch.argsort(perm)[:CODE_BITS]             # z[:, code_channel[k]] = 2 bit_k(code) - 1
        assert not self.z.sum(1).any() and self.z.abs().eq(1).all()
        assert (self.z[:, self.code_channel] == s.double()).all()
        self.amp = 2.0 ** torch.randint(-1, 3, (n,), generator=g).double()
        self.xp = self.z * self.amp[:, None]
        self.C, self.n = C, n


def rows_of(C):
    return _cached(("rows", C), lambda: Rows(C))


def source_map(T, grid):
    """row -> source row.  T <= NSRC: the identity.  Otherwise source = 128 * class(panel) + a seeded permutation of the row's place
    in its panel, class = (panel mod grid) mod 2 + 2 ((panel div grid) mod 4): it differs between adjacent panels and between the
    panels p, p + grid, p + 2 grid, p + 3 grid that one workgroup runs"""
    rows = torch.arange(T)
    if T <= NSRC:
        return rows
    npan = (T + PANEL - 1) // PANEL
    assert npan <= 4 * grid, "a workgroup would meet a class twice"
    p = torch.arange(npan)
    cls = (p % grid) % 2 + 2 * ((p // grid) % 4)
    for step in (1, grid, 2 * grid, 3 * grid):
        assert (cls[step:] != cls[:-step]).all(), f"panels {step} apart share a class (grid {grid})"
    sigma = torch.argsort(torch.rand(npan, PANEL, generator=_gen("source-map", T, grid)), dim=1)
    return (cls[:, None] * PANEL + sigma).reshape(-1)[:T]


def ln_emulate(xp, skip=None, stat_rows=None, eps=EPS):
    """the kernels' LayerNorm (qkv_fused.hip / ff_fused.hip::layernorm_rows) in fp32 steps: xp [n, C] the fp32 values of x' in fp64
    storage.  Every partial sum of x and x^2 is a small dyadic number, exact in fp32 in the lane order (asserted), so the order of
    summation is not emulated.  skip: [C] bool, channels left out of the sums (a fault); stat_rows: [n, C] rows whose statistics are
    used instead of the rows' own (a fault).  Returns (z as fp16 values, mean, sigma)"""
    C = xp.shape[1]
    st = xp if stat_rows is None else stat_rows
    if skip is not None:
        st = st * (~skip).double()[None, :]
    s, q = st.sum(1), (st * st).sum(1)
    assert (r32(s) == s).all() and (r32(q) == q).all() and q.max() < 2.0 ** 20
    inv = f32c(f32c(1.0) / C)
    mean = r32(s * inv)
    var = r32(r32(q * inv) - mean * mean).clamp_min(0.0)
    ve = r32(var + f32c(eps))
    rstd = r32(1.0 / torch.sqrt(ve))
    nm = r32(-mean * rstd)
    sigma = r32(ve * rstd)
    z = r16(r32(xp * rstd[:, None] + nm[:, None]))
    return z, mean, sigma


def stat_skips(C):
    """the channel sets a fault leaves out of the row sums: one channel; the 16-byte vector of one lane (channels 16 ks + 8 h + 0..7)"""
    one = torch.zeros(C, dtype=torch.bool)
    one[C // 2 + 3] = True
    vec = torch.zeros(C, dtype=torch.bool)
    ks, h = C // 16 - 3, 1
    vec[16 * ks + 8 * h:16 * ks + 8 * h + 8] = True
    return {"channel": one, "vector": vec}


def split_bias(b):
    """(b_hi, b_lo) as pack_ln_proj / pack_ff_fused split an fp32 bias"""
    b32 = r32(b)
    hi = r16(b32)
    return hi, r16(b32 - hi)


# ================================================================================================== A. ln_qkv
class QkvProbe:
    def __init__(self, kind, C):
        assert kind in ("dense", "select") and C in (320, 640)
        self.kind, self.C, self.rows = kind, C, rows_of(C)
        g = _gen("qkv", kind, C)
        z = self.rows.z
        if kind == "dense":
            self.w = torch.randint(-2, 3, (3 * C, C), generator=g).double()
            self.b = _quarters((3 * C,), g, -16, 16, nonzero=True)
            ref4 = 4 * (self.w.long() @ z.long().T).T + (4 * self.b).long()[None, :]          # int64, units of 1/4
            assert int(ref4.abs().max()) < 4 * 512, "the reference is not an fp16 number"
            self.max_wz = int((self.w.long() @ z.long().T).abs().max())
            self.exact = ref4.double() / 4
        else:
            m = torch.arange(C)
            nks = C // 16
            self.sel = torch.cat([16 * ((m + 7 * j) % nks) + (m // nks + m + 7 * j) % 16 for j in range(3)])
            self.sign = (torch.randint(0, 2, (3 * C,), generator=g) * 2 - 1).double()
            self.w = torch.zeros(3 * C, C, dtype=torch.float64)
            self.w[torch.arange(3 * C), self.sel] = self.sign
            self.b = (torch.randint(0, 2, (3 * C,), generator=g) * 2 - 1).double() * (1 + 2.0 ** -12)
            assert (torch.bincount(self.sel, minlength=C) == 3).all()
            slot = torch.bincount(self.sel % 16 + 16 * (torch.arange(3 * C) // 32), minlength=16 * 3 * C // 32)
            assert (slot >= 1).all(), "a tile misses a (half, slot) pair"
            ksteps = [torch.unique(self.sel[32 * t:32 * t + 32] // 16).numel() for t in range(3 * C // 32)]
            assert min(ksteps) >= min(C // 16, 32), "a tile meets too few k-steps"
            hi, lo = split_bias(self.b)
            assert lo.abs().eq(2.0 ** -12).all() and hi.abs().eq(1).all()
            self.exact = z @ self.w.T + self.b
            small = self.exact.abs() == 2.0 ** -12
            assert (small | (self.exact.abs() == 2 + 2.0 ** -12)).all() and small.float().mean() > 0.4
        self.ref16 = self.exact.float().half()                    # [NSRC, 3C]: what the kernel must return, bit for bit
        if kind == "dense":
            assert (self.ref16.double() == self.exact).all()

    def emulate(self, xp=None, skip=None, stat_rows=None, drop_b_lo=False):
        """the kernel on rows xp (default: all source rows): fp16 [n, 3C]"""
        z, _, _ = ln_emulate(self.rows.xp if xp is None else xp, skip, stat_rows)
        hi, lo = split_bias(self.b)
        return r32(z @ self.w.T + hi + (0 if drop_b_lo else lo)).float().half()


def qkv_probe(kind, C):
    return _cached(("qkv", kind, C), lambda: QkvProbe(kind, C))


def first_mismatch(got, ref, what, row_of=None):
    """bit-for-bit check of fp16 matrices; a failure names row and column"""
    assert got.shape == ref.shape and got.dtype == ref.dtype == torch.float16, what
    if torch.equal(got.view(torch.int16), ref.view(torch.int16)) or torch.equal(got, ref):       # (-0 == 0 passes)
        return
    bad = (got != ref) | torch.isnan(got)
    i = int(bad.reshape(-1).nonzero()[0])
    row, col = divmod(i, ref.shape[1])
    raise AssertionError(f"{what}: row {row}{row_of(row) if row_of else ''}, column {col}: got {float(got[row, col])!r}, "
                         f"expected exactly {float(ref[row, col])!r}; {int(bad.sum())} of {ref.numel()} elements differ")


# ================================================================================================== B. ff_fused
FF_C, FF_INNER = 320, 1280
KIDX = torch.tensor([(e & 3) + 8 * (e >> 2) + 4 * h for h in range(2) for e in range(8)])      # k-slot (h, e) -> channel of 16
CURVE_VARIANTS = 8
GRID = torch.arange(-64, 65).double() / 8


def gelu64(x):
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_tanh64(x):
    return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_chain(x, form="asm"):
    """fp32 emulation of gelu as the kernels evaluate it: "asm" = tools/gen_ff_asm.py::geglu_items, "erf2" = common.h::gelu_erf2
    (max(x, 0) - |x| q t e, Abramowitz-Stegun 7.1.26; rcp and exp2 correctly rounded here, about an ulp on the device)"""
    if form == "erff":
        return r32(r32(0.5 * x) * r32(1.0 + r32(torch.erf(r32(x * f32c(0.70710678118654752440))))))
    ax = x.abs()
    a1, a2, a3, a4, a5 = (f32c(0.5 * f32c(c)) for c in (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429))
    c1 = f32c(f32c(0.3275911) * f32c(0.70710678118654752440))
    t = r32(1.0 / r32(ax * c1 + 1.0))
    if form == "asm":
        zz = r32(f32c(0.5 * 1.4426950408889634) * r32(x * x))
    else:
        zz = r32(ax * f32c(0.84932180028801904272))
        zz = r32(zz * zz)
    e = r32(torch.exp2(-zz))
    q = r32(t * a5 + a4)
    for a in (a3, a2, a1):
        q = r32(q * t + a)
    q = r32(r32(q * t) * e)
    return r32(x.clamp_min(0.0) - q * ax)


def gelu_term(gate, form="asm"):
    """the approximation term of the curve bound.  "asm" / "erf2": twice the measured error of the fp32 chain (module docstring).
    "erff": the 128x128 GEMM program evaluates 0.5 x (1 + erff(x / sqrt 2)) (gemm_common.h, common.h::gelu_erf_f) - erff to 4 ulp of
    a value below 1 (2^-22 absolute on 1 + erf, which cancels in the negative tail), times |x| / 2, plus three fp32 roundings"""
    if form == "erff":
        return 0.5 * gate.abs() * 2.0 ** -22 + 3 * 2.0 ** -24 * gelu64(gate).abs()
    return 2 * torch.minimum(torch.full_like(gate, GELU_ABS), GELU_REL * gate.abs())


FF_FAULTS = ("channel", "vector", "gate_of_f1", "kslot_e", "res2_unswapped", "tanh")


class FFProbe:
    """weights of one probe and everything of the chain that does not depend on the form: hidden, gate, g, y per source row"""

    def __init__(self, kind, variant=0):
        assert kind in ("switch", "curve")
        self.kind, self.variant, self.rows = kind, variant, rows_of(FF_C)
        z = self.rows.z
        g = _gen("ff", kind)                                   # the variants of the curve probe share W1 up to the gate bias
        w1 = torch.zeros(2 * FF_INNER, FF_C, dtype=torch.float64)
        b1 = torch.zeros(2 * FF_INNER, dtype=torch.float64)
        j = torch.arange(FF_INNER)
        if kind == "switch":
            w1[:FF_INNER] = torch.randint(-1, 2, (FF_INNER, FF_C), generator=g).double()
            b1[:FF_INNER] = torch.randint(-3, 4, (FF_INNER,), generator=g).double()
            w1[FF_INNER + j, torch.randint(0, FF_C, (FF_INNER,), generator=g)] = 8.0 * (torch.randint(0, 2, (FF_INNER,), generator=g) * 2 - 1).double()
            self.w2 = torch.randint(-1, 2, (FF_C, FF_INNER), generator=g).double() * 2.0 ** -8
        else:
            opt = torch.tensor([[1.5, 0.5], [-1.5, 0.5], [0.5, 1.5], [-0.5, 1.5]], dtype=torch.float64)[torch.randint(0, 4, (FF_INNER,), generator=g)]
            b1[:FF_INNER] = opt[:, 0]
            w1[j, torch.randint(0, FF_C, (FF_INNER,), generator=g)] = opt[:, 1] * (torch.randint(0, 2, (FF_INNER,), generator=g) * 2 - 1).double()
            wt = 2.0 ** (2 - torch.argsort(torch.rand(FF_INNER, 7, generator=g), dim=1).double())       # a permutation of 4 .. 1/16 per channel
            sg = (torch.randint(0, 2, (FF_INNER, 7), generator=g) * 2 - 1).double()
            w1[FF_INNER:, self.rows.code_channel[:7]] = wt * sg
            b1[FF_INNER:] = (1.0 if variant < 4 else -1.0) / 16
            order = torch.randperm(FF_INNER, generator=g)
            self.sel = order[FF_C * (variant & 3):FF_C * (variant & 3) + FF_C]             # the hidden channel of every output
            self.sel_sign = (torch.randint(0, 2, (FF_C,), generator=_gen("ff-curve-sign", variant)) * 2 - 1).double()
            self.w2 = torch.zeros(FF_C, FF_INNER, dtype=torch.float64)
            self.w2[torch.arange(FF_C), self.sel] = self.sel_sign
        self.w1, self.b1 = w1, b1
        self.b2 = _quarters((FF_C,), _gen("ff-b2", kind, variant))
        hg = z @ w1.T + b1
        self.hidden, self.gate = hg[:, :FF_INNER], hg[:, FF_INNER:]
        if kind == "switch":
            assert self.gate.abs().eq(8).all() and self.hidden.abs().max() <= 256
            self.max_hidden = int(self.hidden.abs().max())
        else:
            assert self.hidden.abs().ge(1).all() and self.hidden.abs().le(2).all() and (self.hidden == self.hidden.round()).all()
            assert (self.gate * 8 == (self.gate * 8).round()).all() and self.gate.abs().max() <= 8
        self.g = self.hidden * gelu64(self.gate)
        self.y = self.g @ self.w2.T

    def grid_coverage(self):
        """curve: per observed hidden channel, the number of distinct gate values met in source rows 0 .. 127"""
        gs = self.gate[:PANEL, self.sel]
        return torch.tensor([torch.unique(gs[:, c]).numel() for c in range(FF_C)])

    # ---- the fp64 reference and the bound of a form
    def res2(self, form):
        if not form.r2:
            return None
        if self.kind == "curve":          # cancels the residual where s_acc / r2 is a power of two
            ratio = f32c(form.s_acc) / f32c(form.r2v)
            return -self.rows.xp * (ratio if math.log2(ratio) == round(math.log2(ratio)) else 0.5)
        return _quarters((NSRC, FF_C), _gen("ff-res2", self.kind), -16, 16)

    def ref(self, form):
        sa, r2 = f32c(form.s_acc), f32c(form.r2v)
        out = sa * (self.y + self.b2 + self.rows.xp)
        if form.r2:
            out = out + r2 * self.res2(form)
        return out

    def bound(self, form):
        sa, r2 = abs(f32c(form.s_acc)), abs(f32c(form.r2v))
        a = self.rows.amp[:, None]
        resid = torch.sqrt(a * a + EPS) - a + 2.0 ** -21 * a
        S = sa * (self.y.abs() + self.b2.abs() + a) + (r2 * self.res2(form).abs() if form.r2 else 0.0)
        b = 2 * (2.0 ** -11 * self.ref(form).abs() + sa * resid + 2.0 ** -22 * S) + 2.0 ** -24 * (1 + sa)
        if self.kind == "curve":
            b = b + 2.0 ** -10 * sa * self.y.abs() + sa * self.hidden[:, self.sel].abs() * gelu_term(self.gate[:, self.sel])
        return b

    # ---- the kernel in fp32 steps
    def core(self, xp=None, skip=None, stat_rows=None, gate_of_f1=False, kslot_e=False, tanh=False):
        """the form-independent part of the kernel on rows xp (x' = x + pe as the kernel forms it; default: every source row):
        (y, z, mean, sigma).  Faults: skip / stat_rows (ln_emulate); gate_of_f1: the hidden tile f0 of every unit multiplied with gelu
        of gate tile f1; kslot_e: the W2 k-slots of a 16-channel k-step taken as 8 h + e instead of (e & 3) + 8 (e >> 2) + 4 h; tanh:
        the tanh form of GELU"""
        xp = self.rows.xp if xp is None else xp
        z, mean, sigma = ln_emulate(xp, skip, stat_rows)
        hi, lo = split_bias(self.b1)
        hg = r32(z @ self.w1.T + hi + lo)
        hid, gate = hg[:, :FF_INNER], hg[:, FF_INNER:]
        if gate_of_f1:
            jj = torch.arange(FF_INNER)
            gate = gate[:, torch.where(jj % 64 < 32, jj + 32, jj)]
        act = r32(gelu_tanh64(gate)) if tanh else gelu_chain(gate)
        g16 = r16(r32(hid * act))
        w2 = self.w2
        if kslot_e:
            w2 = w2.reshape(FF_C, FF_INNER // 16, 16)[:, :, torch.argsort(KIDX)].reshape(FF_C, FF_INNER)
        return r32(g16 @ w2.T), z, mean, sigma

    def finish(self, core, form, res2=None, res2_unswapped=False):
        """the epilogue of ff_fused.hip on a core: fp16 values [n, 320] (in fp64).  res2: the second-residual rows (default: the
        probe's, for every source row); res2_unswapped (a fault): res2 used in the store layout, channels 4..7 and 8..11 of every 16
        exchanged"""
        y, z, mean, sigma = core
        xs = r32(z * sigma[:, None] + mean[:, None])
        sa, r2 = f32c(form.s_acc), f32c(form.r2v)
        out = r32(r32(r32(y + self.b2) + xs) * sa)
        if form.r2:
            rr = self.res2(form) if res2 is None else res2
            if res2_unswapped:
                c = torch.arange(FF_C)
                k = c % 16
                rr = rr[:, torch.where((k >= 4) & (k < 8), c + 4, torch.where((k >= 8) & (k < 12), c - 4, c))]
            out = r32(out + rr * r2)                            # (contracted: one rounding)
        return r16(out)

    def emulate(self, form, res2=None, res2_unswapped=False, **core_args):
        return self.finish(self.core(**core_args), form, res2, res2_unswapped)

    def emulate_sources(self, form, fault=None):
        """the kernel on every source row, with one of FF_FAULTS; the core is computed once per (probe, fault)"""
        if fault == "res2_unswapped":
            return self.finish(self.emulate_core(None), form, res2_unswapped=True)
        return self.finish(self.emulate_core(fault), form)

    def emulate_core(self, fault):
        args = {None: {}, "channel": dict(skip=stat_skips(FF_C)["channel"]), "vector": dict(skip=stat_skips(FF_C)["vector"]),
                "gate_of_f1": dict(gate_of_f1=True), "kslot_e": dict(kslot_e=True), "tanh": dict(tanh=True)}[fault]
        return _cached(("ff-core", self.kind, self.variant, fault), lambda: self.core(**args))

    # ---- the GEGLU epilogue of ops.gemm on the rows z
    def geglu_bound(self, form="erf2"):
        return 2.0 ** -10 * self.g.abs() + self.hidden.abs() * gelu_term(self.gate, form) + 2.0 ** -24

    def geglu_emulate(self, form="erf2", tanh=False):
        act = r32(gelu_tanh64(self.gate)) if tanh else gelu_chain(self.gate, form)
        return r16(r32(self.hidden * act))


def ff_probe(kind, variant=0):
    return _cached(("ff", kind, variant), lambda: FFProbe(kind, variant))


class Form:
    """one of the four forms of lkgd_ff_fused_c320 with its scalars: rb = (rb_d1, rb_md) or None; r2v = None: no second residual"""

    def __init__(self, rb=None, s_acc=1.0, r2v=None):
        self.rb, self.s_acc, self.r2 = rb, s_acc, r2v is not None
        self.r2v = 0.0 if r2v is None else r2v

    @property
    def name(self):
        return ("rowbias" if self.rb else "") + ("+" if self.rb and self.r2 else "") + ("res2" if self.r2 else "") or "plain"

    def __repr__(self):
        return f"{self.name}(rb={self.rb},s_acc={self.s_acc},r2={self.r2v if self.r2 else None})"


def pe_table(md):
    return _cached(("pe", md), lambda: _quarters((md, FF_C), _gen("ff-pe", md), -8, 8))


class FFCase:
    """one launch: probe, form, T rows (drawn through source_map for the many-panel case), the row pitches"""

    def __init__(self, kind, variant, T, form, grid, ldx=FF_C, ldo=FF_C, ldr2=FF_C):
        self.kind, self.variant, self.T, self.form, self.grid = kind, variant, T, form, grid
        self.ldx, self.ldo, self.ldr2 = ldx, ldo, ldr2
        self.id = f"{kind}{variant}-T{T}-{form!r}-ld{ldx},{ldo},{ldr2}"

    @property
    def probe(self):
        return ff_probe(self.kind, self.variant)

    @property
    def src(self):
        return _cached(("src", self.T, self.grid), lambda: source_map(self.T, self.grid))

    @property
    def idx(self):
        """the row-bias table row of every token row"""
        d1, md = self.form.rb
        return rowmap_index(self.T, (d1, 1, 1, md, 0))

    def x(self):
        """fp16 [T, 320]: a z, minus the table row where the form has one"""
        xp = self.probe.rows.xp[self.src]
        if self.form.rb:
            xp = xp - pe_table(self.form.rb[1])[self.idx]
        x = xp.half()
        assert (x.double() == xp).all()
        return x

    def res2_rows(self):
        return self.probe.res2(self.form)[self.src].half()


def ff_forms(i):
    """the four forms for the i-th shape: the row maps and scalars rotate with i"""
    rbs = [(50, 3), (128, 14), (4096, 3), (50, 1), (128, 3), (4096, 14), (50, 14), (128, 1)]
    scal = [(1.0, 1.0), (0.5, 2.0), (2.0, 0.25), (0.3, 0.7)]
    sa1, r1 = scal[i % 4]
    sa2, r2 = scal[(i + 1) % 4]
    return [Form(), Form(rb=rbs[i % 8], s_acc=(1.0, 0.5)[i % 2]), Form(s_acc=sa1, r2v=r1), Form(rb=rbs[(i + 3) % 8], s_acc=sa2, r2v=r2)]


def ff_cases(cus=NOMINAL_CUS):
    """every launch of the GPU file.  Shapes x the four forms, the switch probe and one curve variant each (the variants rotate; all
    eight run at T = 901); pitched x / out / res2 at T = 129 and T = 901; the many-panel case with boundaries of the row map inside
    a workgroup's second panel"""
    out = []
    n = 0
    for i, T in enumerate(T_SMALL):
        grid = min((T + PANEL - 1) // PANEL, cus)
        pitched = T in (129, 901)
        ld = (FF_C + 8, FF_C + 64, FF_C + 24) if pitched else (FF_C, FF_C, FF_C)
        for f, form in enumerate(ff_forms(i)):
            out.append(FFCase("switch", 0, T, form, grid, *ld))
            for v in (range(CURVE_VARIANTS) if T == 901 and f in (0, 3) else [n % CURVE_VARIANTS]):
                out.append(FFCase("curve", v, T, form, grid, *ld))
            n += 1
    T = many_panels_T(cus)
    forms = [Form(), Form(rb=(4096, 14)), Form(s_acc=0.5, r2v=2.0), Form(rb=(50, 3), s_acc=0.3, r2v=0.7)]
    for f, form in enumerate(forms):
        out.append(FFCase("switch", 0, T, form, cus))
        out.append(FFCase("curve", (3 + 5 * f) % CURVE_VARIANTS, T, form, cus))
    return out


def qkv_cases(cus=NOMINAL_CUS):
    """(kind, C, T, grid, ldx, ldo) of every ln_qkv launch"""
    out = []
    for C in (320, 640):
        for kind in ("dense", "select"):
            for T in T_SMALL:
                pitched = T in (129, 901)
                out.append((kind, C, T, min((T + PANEL - 1) // PANEL, cus), C + 8 if pitched else C, 3 * C + 64 if pitched else 3 * C))
            out.append((kind, C, many_panels_T(cus), cus, C, 3 * C))
    return out


# (M, interleave, planned program, its GELU) at K = C = 320: the 128x128 program (gemm_common.h: gelu_erf_f) and the 256x320 one
# (gemm_wide.hip: gelu_erf2)
GEGLU_GEMM = [(260, 32, 1, "erff"), (700, 80, 4, "erf2")]


# ================================================================================================== checks
def check_rows(got, ref, bound, src, what, limit=1.0, chunk=8192):
    """attn_probes.check_bound on got [T, n] against ref[src], bound[src] (per source row), in chunks of rows; returns the worst
    err / bound"""
    worst = 0.0
    for r0 in range(0, got.shape[0], chunk):
        s = src[r0:r0 + chunk]
        worst = max(worst, check_bound(got[r0:r0 + chunk], ref[s], bound[s], what, limit,
                                       where=lambda r, r0=r0, s=s: f" (+ {r0}; source row {int(s[r])})"))
    return worst


def rejected(got, ref, bound, limit=1.0):
    return bool(out_of_bound(got, ref, bound, limit).any())
