"""Probe inputs for GroupNorm, LayerNorm and the row softmax: data on which every element, every (sample, group) and every channel
is individually decisive, fp64 / integer references and per-element bounds that are derived, not tuned.  CPU only; imports no kernel
(tests/test_norm_probes_cpu.py shows that an fp32 emulation of each kernel's arithmetic uses at most half of every bound and that
the faults the probes are meant for are rejected, tests/test_norm_probes_gpu.py runs them on the entry points).

Why: on iid `randn * a + b` every (sample, group) has the same statistics to about 1 %, one row of 9216 moves a mean by 1e-4 of a
standard deviation, and every probability of a 9216-column softmax is below an absolute tolerance of 2e-3 - a kernel that reads its
neighbour's statistics, drops a row or a column slot stays inside the global tolerances of the plain tests.

GroupNorm, exact-sums probe (GnProbe): x = m[s, g] + a[s, g] * z, m in multiples of 1/4 within [-2, 2], a in {1/2, 1, 2}, z in
multiples of 1/2 within [-1.5, 1.5], x != 0 everywhere, (m, a) different between adjacent groups and adjacent samples, |m| <= 3 a so
that |mean| <= 4 std (the subject is indexing, not conditioning: the statistics stay E[x^2] - mean^2).  x is a multiple of 1/4 and
x^2 of 1/16, |x| <= 5: every fp32 partial sum a kernel can form (a statistics chunk's group share, at most 2048 elements; a whole
group of gn_small_kernel, at most 24 576) stays below 2^24 units of 1/16 and is exact in any order, the fp64 sums across chunks are
exact, and
  sums    (lkgd_groupnorm_sums) are the float32 rounding of the int64 sums BIT FOR BIT - an element lost, counted twice or credited
          to another group changes sum(x^2), because x^2 > 0 everywhere;
  stats   |mean - ref| <= 2^-22 max(|ref|, a), |rstd - ref| <= 2^-22 ref against fp64 with eps as its float32 value: the kernel's
          fp64 mean / variance are exact to 2^-48 (|mean| <= 4 std), what is left is the rounding to float32 (2^-24); the same
          bounds hold gn_cols_kernel and gn_finalize_parts_kernel, which add integer tables in fp64;
  output  silu = 0: |got - ref| <= 2^-10 |ref| + 2^-20 (|x A| + |mean A| + |beta|) + 2^-24, A = rstd gamma.  norm.hip:239-249:
          A = rstd * gamma, B = beta - mean * A and x * A + B are fp32, contracted or not (2^-24 of |A|, of |mean A| + |beta| and of
          |x A| + |B|), rstd and mean are one float rounding of fp64 values (2^-24 each, on |x A| + |mean A|), the store rounds to
          fp16 (2^-11 |ref|, 2^-25 in the subnormal range); twice the sum is below the bound.
  silu    f -> f / (1 + __expf(-f)) (common.h:24).  With e_f the fp32 share of the bound above, the error reaches the result through
          SiLU's slope (<= 1.1); __expf is v_exp_f32 of f * log2(e) - the product's rounding is 2^-24 |f| in the exponent, the
          instruction 1 ulp - and the division (v_rcp_f32 based) 2.5 ulp: together below 2^-21 (1 + |f|) |silu(f)|; one fp16
          rounding.  Twice the sum: 2^-10 |silu(f)| + 1.1 * 2^-20 (|x A| + |mean A| + |beta|) + 2^-20 (1 + |f|) |silu(f)| + 2^-24.

GroupNorm, given-statistics probe (lkgd_groupnorm_apply, lkgd_groupnorm_apply_segments, lkgd_spatial_norm3d take `stats`): the same
x with synthetic statistics mean = m[s, g], rstd = 2^-k[s, g], gamma = +-2^j, beta in multiples of 1/4 - and for the spatial norm yb
rows with y = +-2^j and b in multiples of 1/4 that encode the latent pixel they belong to in every 8-channel vector.  Every
intermediate is exact in fp32; the output is the reference rounded once: |got - ref| <= 2^-11 |ref| + 2^-24 (with SiLU on top: the
SiLU bound above with e_f = 0).  A neighbour's
statistics, a wrong tmap entry, Y >> sh off by one at a cell border or Tz / T confused are O(1) errors on exactly the rows concerned.

LayerNorm (LnProbe; layernorm_kernel of norm.hip is two-pass: mean, then sum((x - mean)^2)):
  one-hot   row r = m_r (a non-zero multiple of 1/4, |m_r| <= 1) except channel r mod C, which carries m_r + A_r, A_r in
            {2, 4, 8, 16}; T = C rows make every channel the decisive one once: left out of the sums, rstd goes to eps^-1/2; counted
            twice, it is off by sqrt(2).  A FLAT channel left out moves the mean by m_r / C, as much as the flat channels' own
            distance A_r / C from it: every row rejects it (which is why m_r is never 0).
  balanced  x = m_r + a_r z, z in {-1, +1}^C with sum z = 0, neighbouring rows with different (m_r, a_r), random gamma / beta.
  bound     2^-10 |ref| + 2^-20 ((|x| + |mean|) rstd |gamma| + |beta|) + 2^-24: sum(x) is exact, mean = s * (1 / C) carries two fp32
            roundings on |mean| - (x - mean) cancels on the flat channels of the one-hot rows, hence the |mean| term -, the variance
            sum, * invC, + eps, v_rsq_f32 and the two products a few 2^-24 on (|x| + |mean|) rstd |gamma|, the affine add 2^-24 on
            |ref| + |beta|, the store 2^-11 |ref|; twice the sum is below the bound.
  The row-bias table is added in fp16 before the norm (norm.hip:639); the probe hands the kernel x - table[idx(row)] with table
  entries in multiples of 1/4, so the biased row is the probe row exactly.  The 64-bit row-map branch (norm.hip:629) needs 2^31
  rows and stays untested.

Row softmax (softmax_rows_kernel of vae_ops.hip), per element against fp64, bound 2^-9 |ref| + 2^-24 / l with l the fp64 row sum
of exp(x - max): the kernel rounds p = exp2(x log2e - max log2e) to fp16 BEFORE it normalises (vae_ops.hip:49: 2^-11 p, or 2^-25
absolute below 2^-14) and rounds p / l once more at the store (2^-11 |ref|); the fp32 terms - the fmaf against the rounded
max * log2(e) (2^-24 * 12 in the exponent for |x| <= 8), v_exp_f32 (1 ulp), the fp32 sum and 1.0f / l - stay below 2^-20 relative.
Twice (2^-11 + 2^-11 + 2^-20) |ref| + 2^-25 / l is below the bound.  One term more, which the fp32 emulation needs at 16376 and
16384 columns: a RESULT below 2^-14 is an fp16 subnormal, so the store (vae_ops.hip:63) rounds it by up to 2^-25 absolute, not
2^-11 relative - the bound carries + 2^-24 on exactly the elements whose reference is below 2^-14.
  uniform   x = c, another c per row: every element 1 / cols;   weighted  x = fp16(ln w), w in 1..8, reference from the rounded x;
  one-hot   one column 24 above the rest, swept over every thread, every one of the 8 vector slots and the last column."""
import zlib

import torch

GN_GROUPS = 32
F64, F32, F16 = torch.float64, torch.float32, torch.float16
SENTINEL = -7.0
HUGE = 1.0e30


def seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode())


def _gen(*key):
    return torch.Generator().manual_seed(seed_of(*key))


def ratio(got, ref, bound):
    """err / bound per element (fp64); a non-finite result counts as infinitely wrong"""
    r = (got.to(F64) - ref).abs() / bound
    return torch.where(torch.isfinite(got.to(F64)), r, torch.full_like(r, float("inf")))


def worst(got, ref, bound, what=""):
    """the largest err / bound; an AssertionError that names the worst element if it exceeds 1"""
    r = ratio(got, ref, bound)
    w = r.max().item()
    if not w <= 1.0:
        i = int(r.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))
        raise AssertionError(f"{what}: err / bound = {w:.3g} at {idx}: got {got[idx].item()!r}, ref {ref[idx].item()!r}, "
                             f"bound {bound[idx].item():.3g}; {(r > 1).sum().item()} of {r.numel()} elements outside")
    return w


def rejected(got, ref, bound):
    """fraction of elements outside the bound"""
    return (ratio(got, ref, bound) > 1.0).to(F64).mean().item()


# ================================================================================================== launch plans (norm.hip)
GN_APPLY_KB, GN_STATS_KB, GN_TARGET_WGS = 32, 128, 1024
GN_SMALL_LDS = 48 * 1024
GN_SMALL_MAX_BYTES = 10 * 1024 * 1024 + 512 * 1024
GN_SMALL_NT = 512


def gn_rows_kb(C, kb, rows, ns, target=GN_TARGET_WGS):
    """gn_rows_kb of norm.hip: rows of one sample per workgroup"""
    rmax = min(max(kb * 1024 // (C * 2), 8), 1024)
    rmin = min(max(8 * 1024 // (C * 2), 8), rmax)
    want = (rows * ns + target - 1) // target
    return min(max(want, rmin), rmax)


def gn_stats_rows(C, rows, ns):
    return gn_rows_kb(C, GN_STATS_KB, rows, ns)


def gn_apply_rows(C, rows, ns):
    return gn_rows_kb(C, GN_APPLY_KB, rows, ns)


def gn_chunks(C, rows, ns):
    rs = gn_stats_rows(C, rows, ns)
    return (rows + rs - 1) // rs


def gn_chunks_bound(C, rows):
    """lkgd_groupnorm_chunks: what the caller sizes `partial` by"""
    r = min(gn_apply_rows(C, rows, 1), gn_stats_rows(C, rows, 1))
    return (rows + r - 1) // r


def gn_map(C):
    """(C8, rows_par, nslot) of gn_map in norm.hip"""
    C8 = C // 8
    return (C8, 256 // C8, 1) if C8 <= 256 else (C8, 1, (C8 + 255) // 256)


def gn_small_vec(c0, c1, ld0, ld1, ldo, ns, rows, on=True, max_bytes=GN_SMALL_MAX_BYTES):
    """gn_small_vec of norm.hip for a 16-byte aligned output: halfs per access of the one-launch kernel, 0 = three launches"""
    C = c0 + c1
    gs = C // GN_GROUPS
    if not on or rows * gs * 2 > GN_SMALL_LDS or ns * rows * C * 2 > max_bytes or ns * GN_GROUPS < 64:
        return 0
    vec = 8 if gs % 8 == 0 else 4 if gs % 4 == 0 else 2 if gs % 2 == 0 else 0
    if not vec or gs // vec > GN_SMALL_NT or c0 % vec or ld0 % vec or (c1 > 0 and ld1 % vec) or ldo % vec:
        return 0
    return vec


def ln_plan(C):
    """(L, NV) of lkgd_layernorm's dispatch: lanes per row, 16-byte vectors per lane"""
    C8 = C // 8
    if C8 > 64 * 4:
        return 64, 6
    if C8 > 64 * 3:
        return 64, 4
    L = 4
    while L < 64 and L * 3 < C8:
        L *= 2
    return L, 3


# ================================================================================================== GroupNorm: exact sums
_COMBOS = [(i / 4.0, a) for a in (0.5, 1.0, 2.0) for i in range(-8, 9) if abs(i / 4.0) <= 3 * a]      # 47 of them (a prime)


class GnProbe:
    """x [ns * rows, C] fp16 of the exact-sums construction; c0 splits the channels into the two sources of a concatenated input"""

    def __init__(self, ns, rows, C, c0=None):
        assert C % GN_GROUPS == 0 and C % 8 == 0
        self.ns, self.rows, self.C, self.gs = ns, rows, C, C // GN_GROUPS
        self.c0 = C if c0 is None else c0
        self.c1 = C - self.c0
        g = _gen("gn", ns, rows, C)
        perm = torch.randperm(len(_COMBOS), generator=g)
        base = int(torch.randint(0, len(_COMBOS), (1,), generator=g))
        s_i, g_i = torch.meshgrid(torch.arange(ns), torch.arange(GN_GROUPS), indexing="ij")
        code = perm[(base + 7 * g_i + 11 * s_i) % len(_COMBOS)]
        tab = torch.tensor(_COMBOS, dtype=F64)
        self.m, self.a = tab[code, 0], tab[code, 1]                    # [ns, 32]
        for d in ((0, 1), (1, 0)):                                      # adjacent groups / samples never share (m, a)
            c2 = code.roll(-1, d.index(1))
            sl = (slice(None), slice(0, -1)) if d == (0, 1) else (slice(0, -1), slice(None))
            assert bool((code[sl] != c2[sl]).all())
        z = (torch.randint(0, 7, (ns, rows, GN_GROUPS, self.gs), generator=g).to(F64) - 3.0) / 2.0
        m4, a4 = self.m[:, None, :, None], self.a[:, None, :, None]
        zero = (m4 + a4 * z) == 0
        z = torch.where(zero, torch.where(z < 1.5, z + 0.5, z - 0.5), z)
        x = m4 + a4 * z
        assert bool((x != 0).all()) and x.abs().max().item() <= 5.0
        self.x64 = x.reshape(ns * rows, C)
        self.x = self.x64.to(F16)
        assert torch.equal(self.x.to(F64), self.x64)
        xi = (x * 4).round().to(torch.int64)
        self.s4 = xi.sum((1, 3))                                        # sum x   in units of 1/4   [ns, 32] int64
        self.q16 = (xi * xi).sum((1, 3))                                # sum x^2 in units of 1/16
        # the largest fp32 partial a kernel can form is exact: a statistics chunk's group share, or gn_small_kernel's whole group
        share = min(rows, gn_stats_rows(C, rows, ns)) * self.gs
        assert share <= 2048
        if rows * self.gs * 2 <= GN_SMALL_LDS:
            share = max(share, rows * self.gs)
        assert share * int((xi * xi).max()) < 2 ** 24
        n = rows * self.gs
        self.mean = self.s4.to(F64) / 4.0 / n
        self.var = self.q16.to(F64) / 16.0 / n - self.mean ** 2
        big = n >= 64                  # (a handful of elements may be flat: their cases check indexing of the output, not stats)
        assert not big or bool((self.mean.abs() <= 4 * self.var.sqrt()).all()), "|mean| <= 4 std"

    # ---- references
    def sums_ref(self):
        """float32 rounding of the exact (sum x, sum x^2)   [ns, 32, 2]"""
        return torch.stack([self.s4.to(F64) / 4.0, self.q16.to(F64) / 16.0], -1).to(F32)

    def stats_ref(self, eps):
        eps = float(torch.tensor(eps, dtype=F32))
        return self.mean, 1.0 / torch.sqrt(self.var + eps)

    def check_sums(self, got, what="sums"):
        ref = self.sums_ref()
        got = got.reshape(ref.shape).cpu()
        if not torch.equal(got, ref):
            bad = (got != ref).any(-1).nonzero()
            s, g = (int(v) for v in bad[0])
            raise AssertionError(f"{what}: {len(bad)} of {ref.shape[0] * 32} (sample, group) sums differ from the exact ones; first "
                                 f"(sample {s}, group {g}): got {got[s, g].tolist()}, exact {ref[s, g].tolist()}")
        return 0.0

    def check_stats(self, got, eps, what="stats"):
        mean, rstd = self.stats_ref(eps)
        got = got.reshape(self.ns, GN_GROUPS, 2).cpu()
        return max(worst(got[..., 0], mean, 2.0 ** -22 * torch.maximum(mean.abs(), self.a), what + " mean"),
                   worst(got[..., 1], rstd, 2.0 ** -22 * rstd, what + " rstd"))

    def _per_channel(self, t):
        """[ns, 32] -> [ns * rows, C]"""
        return t[:, None, :, None].expand(self.ns, self.rows, GN_GROUPS, self.gs).reshape(self.ns * self.rows, self.C)

    def out_ref(self, gamma, beta, eps=None, silu=False, stats=None):
        """(ref, bound) of the output in fp64: statistics from the data (eps) or given ones (stats = (mean, rstd) [ns, 32])"""
        mean, rstd = self.stats_ref(eps) if stats is None else stats
        mean, rstd = self._per_channel(mean.to(F64)), self._per_channel(rstd.to(F64))
        A = rstd * gamma.to(F64)
        f = (self.x64 - mean) * A + beta.to(F64)
        e_f = 2.0 ** -20 * ((self.x64 * A).abs() + (mean * A).abs() + beta.to(F64).abs())
        if not silu:
            return f, 2.0 ** -10 * f.abs() + e_f + 2.0 ** -24
        s = f * torch.sigmoid(f)
        return s, 2.0 ** -10 * s.abs() + 1.1 * e_f + 2.0 ** -20 * (1 + f.abs()) * s.abs() + 2.0 ** -24

    def affine(self):
        g = _gen("gn affine", self.C)
        return (torch.randn(self.C, generator=g) * 0.5 + 1.0).to(F32), torch.randn(self.C, generator=g).to(F32)

    # ---- given statistics: every intermediate exact, the output the reference rounded once
    def given(self):
        """(stats [ns, 32, 2] fp32 with mean = m and rstd = 2^-k, gamma = +-2^j, beta in multiples of 1/4)"""
        g = _gen("gn given", self.ns, self.C)
        s_i, g_i = torch.meshgrid(torch.arange(self.ns), torch.arange(GN_GROUPS), indexing="ij")
        k = (g_i + 2 * s_i + int(torch.randint(0, 3, (1,), generator=g))) % 3          # differs between adjacent groups / samples
        stats = torch.stack([self.m, 2.0 ** -k.to(F64)], -1).to(F32)
        gamma = (2.0 ** (torch.randint(0, 4, (self.C,), generator=g) - 1).to(F64)) * (torch.randint(0, 2, (self.C,), generator=g) * 2 - 1)
        beta = (torch.randint(0, 17, (self.C,), generator=g) - 8).to(F64) / 4.0
        return stats, gamma.to(F32), beta.to(F32)

    def given_ref(self, stats, gamma, beta):
        mean, rstd = self._per_channel(stats[..., 0].to(F64)), self._per_channel(stats[..., 1].to(F64))
        ref = (self.x64 - mean) * rstd * gamma.to(F64) + beta.to(F64)
        assert torch.equal(ref.to(F32).to(F64), ref)
        return ref, exact_bound(ref)


def exact_bound(ref):
    return 2.0 ** -11 * ref.abs() + 2.0 ** -24


def silu_of_exact(f):
    """(ref, bound) of SiLU on a pre-activation the kernel holds exactly: the SiLU terms of the module docstring with e_f = 0"""
    s = f * torch.sigmoid(f)
    return s, 2.0 ** -10 * s.abs() + 2.0 ** -20 * (1 + f.abs()) * s.abs() + 2.0 ** -24


def shift_groups(stats, d):
    """fault: every group normalised with the statistics of group g + d"""
    return stats.roll(-d, 1)


def shift_samples(stats, d):
    """fault: every sample normalised with the statistics of sample s + d"""
    return stats.roll(-d, 0)


def padded(t, pad, col0=0, fill=SENTINEL):
    """t [rows, C] inside a [rows, col0 + C + pad] matrix of sentinels: (whole, view)"""
    whole = torch.full((t.shape[0], col0 + t.shape[1] + pad), fill, dtype=t.dtype)
    whole[:, col0:col0 + t.shape[1]] = t
    return whole, whole[:, col0:col0 + t.shape[1]]


def _gn_cases():
    cases = []

    def add(ns, rows, C, c0=None, why=""):
        if rows >= 1 and (ns, rows, C, c0) not in [c[:4] for c in cases]:
            cases.append((ns, rows, C, c0, why))
    for C in (32, 64, 96, 128, 256, 320, 512, 640, 1280, 1920, 2080, 2560, 4096):
        rp, rmin = gn_map(C)[1], gn_rows_kb(C, 8, 1, 1)
        add(3, rp + 1, C, why="rows_par + 1")
        add(3, rp - 1, C, why="rows_par - 1")
        # small tensors are cut into 8-KiB chunks by both passes (read from gn_rows_kb): one row beyond a chunk
        assert gn_stats_rows(C, rmin + 1, 3) == rmin == gn_apply_rows(C, rmin + 1, 3)
        add(3, rmin + 1, C, why="one row beyond a statistics / apply chunk")
    for C in (256, 1280, 4096):
        add(1, 1, C, why="a single row")
    add(3, 1, 640, why="a single row per sample")
    add(1, 523, 1280, why="66 statistics chunks: more than the 64 lanes of gn_reduce_pair")
    assert gn_chunks(1280, 523, 1) == 66
    add(2, 3072, 256, why="a gn_small group of exactly 48 KiB")
    add(2, 3073, 256, why="one row beyond 48 KiB: three launches")
    add(2, 192, 4096, why="a gn_small group of exactly 48 KiB, 16 accesses per row")
    add(2, 193, 4096, why="one row beyond 48 KiB: three launches")
    add(28, 2400, 64, why="28 samples: gn_rows_kb picks longer chunks than lkgd_groupnorm_chunks assumed")
    assert gn_stats_rows(64, 2400, 28) > gn_stats_rows(64, 2400, 1) and gn_apply_rows(64, 2400, 28) > gn_apply_rows(64, 2400, 1)
    add(28, 9, 1280, why="28 samples")
    add(3, 77, 320, 8, why="two sources, c0 = 8 inside group 0")
    add(3, 50, 1280, 648, why="two sources, c0 in the middle of group 16 (16-byte accesses)")
    add(2, 64, 640, 328, why="two sources, c0 in the middle of group 16 (8-byte accesses)")
    add(2, 10, 2560, 1280, why="two sources on a group border, two slots")
    return cases


GN_CASES = _gn_cases()
GN_SILU_CASES = [(3, 77, 320, 8), (2, 64, 640, None), (3, 9, 2560, None)]      # one-launch and three-launch forms of each
GN_SEGMENTS = [(320, [(77, 2), (5, 0), (1, 3), (30, 1)]), (1280, [(9, 1), (3, 0)]), (2560, [(5, 0), (20, 1)])]   # C, [(rows, sample)]


# ================================================================================================== GroupNorm: column-sum tables
class ColsProbe:
    """integer column-sum tables as the producing GEMMs leave them: cs[block, pair, (sum, sumsq)] per source, row blocks of blk0 /
    blk1 rows, table widths ld0 / ld1 (floats per block row / 2 pairs) beyond the channels, everything outside the live entries HUGE"""

    def __init__(self, ns, rows, c0, c1, blk0, blk1, pad0=8, pad1=4):
        C = c0 + c1
        assert C % GN_GROUPS == 0 and (C // GN_GROUPS) % 2 == 0 and c0 % 2 == 0 and c1 % 2 == 0 and rows % blk0 == 0
        self.ns, self.rows, self.c0, self.c1, self.C, self.gs = ns, rows, c0, c1, C, C // GN_GROUPS
        self.blk, self.ld = (blk0, blk1), (c0 + pad0, (c1 + pad1) if c1 else 0)
        g = _gen("cols", ns, rows, c0, c1, blk0, blk1)
        self.tab, self.ints = [], []
        for c, blk, ld in zip((c0, c1), self.blk, self.ld):
            if not c:
                self.tab.append(None); self.ints.append(None)
                continue
            assert rows % blk == 0
            nb = ns * rows // blk
            cnt = 2 * blk                                                        # elements behind one (block, pair) entry
            s = torch.randint(-cnt, cnt + 1, (nb, c // 2), generator=g)          # |mean| <= 1
            q = torch.randint(2 * cnt, 5 * cnt, (nb, c // 2), generator=g)       # E[x^2] in [2, 5): std >= 1
            t = torch.full((nb + 1, ld // 2, 2), HUGE, dtype=F32)                # (one guard block behind the last sample)
            t[:nb, :c // 2, 0], t[:nb, :c // 2, 1] = s.to(F32), q.to(F32)
            self.tab.append(t); self.ints.append((s, q))

    def group_sums(self, clip_to_first=False, second_at_first_offset=False):
        """int64 (sum, sumsq) [ns, 32]; the two flags are the faults of a straddling group clipped to its first source and of the
        second source's pairs read at the first source's channel numbers"""
        S = torch.zeros(self.ns, GN_GROUPS, dtype=torch.int64)
        Q = torch.zeros_like(S)
        for src, (c, blk) in enumerate(zip((self.c0, self.c1), self.blk)):
            if not c:
                continue
            s, q = self.ints[src]
            nb = self.rows // blk
            for g in range(GN_GROUPS):
                lo, hi = g * self.gs - (self.c0 if src else 0), (g + 1) * self.gs - (self.c0 if src else 0)
                if clip_to_first and src == 1 and lo < 0 < hi:
                    continue
                if second_at_first_offset and src == 1:
                    lo, hi = lo + self.c0, hi + self.c0
                lo, hi = max(lo, 0), min(hi, c)
                if hi <= lo:
                    continue
                for smp in range(self.ns):
                    S[smp, g] += s[smp * nb:(smp + 1) * nb, lo // 2:hi // 2].sum()
                    Q[smp, g] += q[smp * nb:(smp + 1) * nb, lo // 2:hi // 2].sum()
        return S, Q

    def straddles(self):
        return self.c1 > 0 and self.c0 % self.gs != 0


COLS_CASES = [  # ns, rows, c0, c1, blk0, blk1
    (3, 96, 320, 0, 32, 0), (2, 96, 328, 312, 32, 48), (3, 64, 64, 0, 64, 0), (2, 128, 1282, 1278, 16, 128), (1, 256, 66, 62, 256, 1)]


def finalize_ref(S, Q, count, eps):
    """fp64 (mean, rstd) from exact integer sums"""
    mean = S.to(F64) / count
    var = Q.to(F64) / count - mean ** 2
    return mean, 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=F32)))


def check_finalized(got, S, Q, count, eps, what):
    mean, rstd = finalize_ref(S, Q, count, eps)
    std = (Q.to(F64) / count - mean ** 2).sqrt()
    assert bool((mean.abs() <= 4 * std).all())
    got = got.reshape(S.shape + (2,)).cpu()
    return max(worst(got[..., 0], mean, 2.0 ** -22 * torch.maximum(mean.abs(), std), what + " mean"),
               worst(got[..., 1], rstd, 2.0 ** -22 * rstd, what + " rstd"))


def parts_probe(nparts, ns, part_pad, sample_pad):
    """(parts fp32 flat, part_stride, sample_stride, S, Q int64 [ns, 32], count): integer rank sums with gaps of HUGE"""
    g = _gen("parts", nparts, ns)
    count = 4096 * nparts
    s = torch.randint(-4096, 4097, (nparts, ns, GN_GROUPS), generator=g)
    q = torch.randint(2 * 4096, 5 * 4096, (nparts, ns, GN_GROUPS), generator=g)
    sample_stride = 64 + sample_pad
    part_stride = ns * sample_stride + part_pad
    parts = torch.full((nparts, part_stride), HUGE, dtype=F32)
    live = parts[:, :ns * sample_stride].view(nparts, ns, sample_stride)
    live[:, :, 0:64:2], live[:, :, 1:64:2] = s.to(F32), q.to(F32)
    return parts.reshape(-1), part_stride, sample_stride, s.sum(0), q.sum(0), count


# ================================================================================================== spatial norm
NORM_PAIRS = [(1, 1), (2, 2), (2, 8), (3, 3), (3, 5), (3, 9)]
SPATIAL_CASES = [(C, sh, Tz, T) for C in (64, 128, 384) for sh in (0, 1, 3) for Tz, T in NORM_PAIRS
                 if (C, sh) in ((64, 0), (128, 1), (384, 3)) or (Tz, T) == (3, 5)]


def tmap_ref(Tz, T):
    """latent frame of every frame: nearest resize, the first frame apart when T is odd and above one"""
    if T > 1 and T % 2 == 1:
        return [0] + [1 + (i * (Tz - 1)) // (T - 1) for i in range(T - 1)]
    return [(t * Tz) // T for t in range(T)]


class SpatialProbe:
    """f = a GnProbe's x over B samples of T*H*W rows, given statistics, yb rows that name their latent pixel in every vector"""

    def __init__(self, C, sh, Tz, T, B=2, H=8, W=16):
        self.C, self.sh, self.Tz, self.T, self.B, self.H, self.W = C, sh, Tz, T, B, H, W
        self.gn = GnProbe(B, T * H * W, C)
        self.stats, self.gamma, self.beta = self.gn.given()
        h, w = H >> sh, W >> sh
        npx = B * Tz * h * w
        assert npx < 33 * 33
        p = torch.arange(npx)[:, None]
        c = torch.arange(C)[None, :]
        digit = torch.where(c % 2 == 0, p % 33, p // 33)
        self.yb_b = ((digit + c) % 33 - 16).to(F64) / 4.0
        self.yb_y = 2.0 ** (((p + c) % 4) - 1).to(F64) * (1 - 2 * ((p // 4 + c) % 2)).to(F64)
        self.yb = torch.cat([self.yb_y, self.yb_b], 1).to(F16)
        assert torch.equal(self.yb.to(F64), torch.cat([self.yb_y, self.yb_b], 1))
        assert len({tuple(r[:8].tolist()) for r in self.yb_b}) == npx              # no two latent pixels share a vector
        self.tmap = tmap_ref(Tz, T)

    def src(self, tmap=None, shift=None, frames=None):
        """latent pixel of every row [B * T * H * W]; the arguments inject faults"""
        B, T, H, W, sh = self.B, self.T, self.H, self.W, self.sh if shift is None else shift
        h, w = self.H >> self.sh, self.W >> self.sh
        tm = torch.tensor(self.tmap if tmap is None else tmap)
        b, t, Y, X = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
        Tz = self.Tz if frames is None else frames
        s = ((b * Tz + tm[t]) * h + (Y >> sh).clamp(max=h - 1)) * w + (X >> sh).clamp(max=w - 1)
        return s.reshape(-1).clamp(max=self.yb.shape[0] - 1)

    def ref(self, src=None):
        n, _ = self.gn.given_ref(self.stats, self.gamma, self.beta)
        src = self.src() if src is None else src
        r = n * self.yb_y[src] + self.yb_b[src]
        assert torch.equal(r.to(F32).to(F64), r)
        return r, exact_bound(r)


# ================================================================================================== LayerNorm
# (640 and 768 are the L = 32 rows: 49 <= C / 8 <= 96, which no other width here reaches)
LN_CS = (8, 64, 72, 96, 104, 320, 328, 640, 768, 1536, 1544, 1920, 2048, 2056, 3072)
assert {ln_plan(C)[0] for C in LN_CS} == {4, 8, 16, 32, 64} and {ln_plan(C)[1] for C in LN_CS} == {3, 4, 6}
assert any(C // 8 == ln_plan(C)[0] * ln_plan(C)[1] for C in LN_CS) and any((C // 8) % ln_plan(C)[0] for C in LN_CS)
_LN_COMBOS = [(i / 4.0, a) for i in range(-4, 5) for a in (0.5, 1.0, 2.0, 4.0)]


def ln_rows(C):
    """T values of the balanced probe: one row, one short of a wave's rows, one beyond a workgroup's rows"""
    rpw = 64 // ln_plan(C)[0]
    return sorted({1, rpw - 1, 4 * rpw + 1} - {0})


class LnProbe:
    def __init__(self, kind, T, C, affine=True):
        assert kind in ("onehot", "balanced")
        self.kind, self.T, self.C = kind, T, C
        g = _gen("ln", kind, T, C)
        r = torch.arange(T)
        if kind == "onehot":
            m = torch.randint(1, 5, (T,), generator=g).to(F64) / 4.0 * (torch.randint(0, 2, (T,), generator=g) * 2 - 1).to(F64)
            A = 2.0 ** (1 + (r + int(torch.randint(0, 4, (1,), generator=g))) % 4).to(F64)
            x = m[:, None].repeat(1, C)
            x[r, r % C] += A
        else:
            perm = torch.randperm(len(_LN_COMBOS), generator=g)
            tab = torch.tensor(_LN_COMBOS, dtype=F64)[perm[r % len(_LN_COMBOS)]]
            z = torch.ones(T, C, dtype=F64)
            order = torch.rand(T, C, generator=g).argsort(1)
            z.scatter_(1, order[:, :C // 2], -1.0)
            assert bool((z.sum(1) == 0).all())
            x = tab[:, :1] + tab[:, 1:] * z
        self.x64 = x
        self.x = x.to(F16)
        assert torch.equal(self.x.to(F64), x)
        if affine:
            self.gamma = (torch.randn(C, generator=g) * 0.5 + 1.0).to(F32)
            self.beta = torch.randn(C, generator=g).to(F32)
        else:
            self.gamma = self.beta = None

    def ref(self, eps):
        eps = float(torch.tensor(eps, dtype=F32))
        x = self.x64
        mean = x.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
        ga = self.gamma.to(F64) if self.gamma is not None else torch.ones(self.C, dtype=F64)
        be = self.beta.to(F64) if self.beta is not None else torch.zeros(self.C, dtype=F64)
        ref = (x - mean) * rstd * ga + be
        bound = 2.0 ** -10 * ref.abs() + 2.0 ** -20 * ((x.abs() + mean.abs()) * rstd * ga.abs() + be.abs()) + 2.0 ** -24
        return ref, bound

    def rowbias(self, div, mod):
        """(x', table [mod, C] fp16): x' + table[(row // div) % mod] is the probe row exactly"""
        g = _gen("ln table", self.T, self.C, div, mod)
        table = (torch.randint(-8, 9, (mod, self.C), generator=g).to(F64) / 4.0)
        idx = (torch.arange(self.T) // div) % mod
        xp = self.x64 - table[idx]
        assert torch.equal(xp.to(F16).to(F64), xp)
        return xp.to(F16), table.to(F16), idx


# ================================================================================================== row softmax
SM_COLS = (8, 96, 2040, 2048, 2056, 9216, 16376, 16384)
SM_ROWS = (1, 5)
SM_NT = 256
_SM_C = (8.0, -8.0, -3.5, 0.0, 2.25)


def sm_hot_columns(cols):
    """the one-hot sweep: every thread (with the slot and the element moving along), every slot, the last column"""
    full = max(1, cols // (8 * SM_NT))                                # slots that every thread owns at this width
    want = [((t % full) * SM_NT + t) * 8 + (t // 8) % 8 for t in range(SM_NT)]
    want += [(i * SM_NT + t) * 8 + e for i in range(8) for t, e in ((0, 0), (SM_NT - 1, 7))]
    seen, out = set(), []
    for c in want + [cols - 1]:
        c = c if c < cols else c % cols
        if c not in seen:
            seen.add(c); out.append(c)
    return out


class SmProbe:
    def __init__(self, kind, rows, cols):
        assert kind in ("uniform", "weighted", "onehot")
        self.kind, self.cols = kind, cols
        g = _gen("sm", kind, rows, cols)
        if kind == "uniform":
            x = torch.tensor(_SM_C[:rows], dtype=F64)[:, None].repeat(1, cols)
        elif kind == "weighted":
            x = torch.log(torch.randint(1, 9, (rows, cols), generator=g).to(F64)).to(F16).to(F64)
        else:
            hot = sm_hot_columns(cols)
            rows = len(hot)
            x = (torch.randint(-8, 9, (rows, 1), generator=g).to(F64) / 2.0).repeat(1, cols)
            x[torch.arange(rows), torch.tensor(hot)] += 24.0
            self.hot = hot
        self.rows = rows
        self.x64 = x
        self.x = x.to(F16)
        assert torch.equal(self.x.to(F64), x)

    def ref(self):
        e = torch.exp(self.x64 - self.x64.max(1, keepdim=True).values)
        l = e.sum(1, keepdim=True)
        ref = e / l
        return ref, 2.0 ** -9 * ref + 2.0 ** -24 / l + 2.0 ** -24 * (ref < 2.0 ** -14)
