// The host-side planner of lkgd_gemm_f16 (include/lkgd_hip.h section 1): descriptor check, choice of tile program, K slices and
// tile form, and the A/B knobs that override them.  Pure arithmetic on the descriptor's numbers and on NULL-ness / alignment of
// its pointers: no HIP, no device (g++ -std=c++17 -I include compiles it; tools/gemm_plan_sweep.cpp walks it under sanitizers).
#include "gemm_plan.h"

#include "../../include/lkgd_hip_debug.h"

namespace lkgd_gemm {

// The A/B knobs (include/lkgd_hip_debug.h; not part of the reference-facing ABI), per host thread.
struct gemm_knobs {
  int variant = 0;             // 0 = auto, else the gemm_program to force where it applies
  bool splitk = true;          // false = never cut K into slices
  // cost model of GEMM_MID's K slicing (mid_split)
  float mid_tk_us = 0.75f, mid_fix_us = 6.0f, mid_red_us = 5.0f, mid_red_tbs = 3.5f;
  int mid_ksplit_forced = 0;
  int wide_ksplit = 0;         // tools/micro/ksplit_sweep.py: force this slice count on GEMM_WIDE where it is legal
  int wide_lds_out = -1;       // 0 = direct 8-byte stores everywhere, 1 / -1 = rows through LDS where used
  int wide_tile_n = 0;         // tools/micro/wide_tile_n.py: 256 / 320 where that width divides N, 0 = the rule
  int wide_tile_m = 0;         // 192 / 256 tile rows (0 = the rule of gemm_wide_form)
};
static thread_local gemm_knobs knobs;

int check_desc(const lkgd_gemm_desc* d) {
  if (!d || !d->a0 || !d->w || !d->out || !d->zeros) return LKGD_E_NULL;
  if (d->M <= 0 || d->N <= 0 || d->K <= 0) return LKGD_E_SHAPE;
  if (d->K % BK) return LKGD_E_SHAPE;
  if (d->N % 4) return LKGD_E_SHAPE;
  if (d->geglu != 0 && d->geglu != 32 && d->geglu != 80) return LKGD_E_MODE;
  if (d->geglu && (d->N % (4 * d->geglu) || d->rowbias || d->res1 || d->res2)) return LKGD_E_SHAPE;
  if (d->ldc % 4 || d->lda0 % 8) return LKGD_E_ALIGN;
  if (!aligned16(d->a0) || !aligned16(d->w) || !aligned16(d->zeros) || ((uintptr_t)d->out & 7)) return LKGD_E_ALIGN;
  if (d->a1 && (!aligned16(d->a1) || d->lda1 % 8)) return LKGD_E_ALIGN;
  if (d->bias && !aligned16(d->bias)) return LKGD_E_ALIGN;
  if (d->rowbias && (d->ldrb % 4 || d->rb_d1 <= 0 || d->rb_d2 <= 0 || d->rb_md <= 0 || d->rb_c0 < 0)) return LKGD_E_SHAPE;
  if (d->res1 && d->ldr1 % 4) return LKGD_E_ALIGN;
  if (d->res2 && d->ldr2 % 4) return LKGD_E_ALIGN;
  switch (d->mode) {
    case LKGD_A_PLAIN:
      if (d->csplit % 8 || d->csplit <= 0) return LKGD_E_SHAPE;
      if (d->csplit < d->K && !d->a1) return LKGD_E_NULL;
      if (d->csplit < d->K && d->csplit % BK) return LKGD_E_SHAPE;
      break;
    case LKGD_A_CONV3X3:
      if (d->Cin <= 0 || d->Cin % BK || d->K != 9 * d->Cin) return LKGD_E_SHAPE;
      if (d->csplit <= 0 || d->csplit % BK) return LKGD_E_SHAPE;
      if (d->csplit < d->Cin && !d->a1) return LKGD_E_NULL;
      if (d->Hout <= 0 || d->Wout <= 0 || d->Hin <= 0 || d->Win <= 0) return LKGD_E_SHAPE;
      if (d->stride != 1 && d->stride != 2) return LKGD_E_SHAPE;
      if (d->ups != 0 && d->ups != 1) return LKGD_E_SHAPE;
      if (d->M % (d->Hout * d->Wout)) return LKGD_E_SHAPE;
      if (d->pad_off != 0 && d->pad_off != 1) return LKGD_E_SHAPE;
      // output size must match: pad 1 on every side: floor((Hv + 2 - 3)/stride) + 1;  pad_off (0 top/left, 1 bottom/right):
      // floor((Hv + 1 - 3)/stride) + 1
      if (d->Hout != (((d->Hin << d->ups) - 1 - d->pad_off) / d->stride) + 1) return LKGD_E_SHAPE;
      if (d->Wout != (((d->Win << d->ups) - 1 - d->pad_off) / d->stride) + 1) return LKGD_E_SHAPE;
      break;
    case LKGD_A_TCONV3:
      if (d->Cin <= 0 || d->Cin % BK || d->K != 3 * d->Cin) return LKGD_E_SHAPE;
      if (d->F <= 0 || d->HW <= 0 || d->Floc <= 0 || d->f_off < 0 || d->f_off + d->Floc > d->F) return LKGD_E_SHAPE;
      if (d->M % (d->Floc * d->HW)) return LKGD_E_SHAPE;
      break;
    case LKGD_A_CONV3X3_C8:
      if (d->Cin != 8 || d->K != 128 || d->lda0 != 8 || d->stride != 1 || d->ups != 0 || d->pad_off != 0) return LKGD_E_SHAPE;
      if (d->Hout != d->Hin || d->Wout != d->Win || d->M % (d->Hout * d->Wout)) return LKGD_E_SHAPE;
      break;
    case LKGD_A_CCONV3:
      if (d->Cin <= 0 || d->Cin % BK || d->K != 27 * d->Cin || d->csplit != d->Cin) return LKGD_E_SHAPE;
      if (d->Hout <= 0 || d->Wout <= 0 || d->Hout != d->Hin || d->Wout != d->Win) return LKGD_E_SHAPE;
      if (d->stride != 1 || d->ups != 0 || d->pad_off != 0) return LKGD_E_SHAPE;
      if (d->Floc <= 0 || d->F != d->Floc + 2 || d->f_off != 0) return LKGD_E_SHAPE;   // two context frames, then the chunk
      if (d->M % (d->Floc * d->Hout * d->Wout)) return LKGD_E_SHAPE;
      if ((long long)(d->M / d->Floc) * d->F >= (1LL << 31)) return LKGD_E_SHAPE;      // 32-bit source row index
      if (d->geglu) return LKGD_E_SHAPE;
      break;
    default:
      return LKGD_E_MODE;
  }
  return LKGD_OK;
}

// Split-K for the 256x320 kernel on problems whose tiles leave CUs idle (fewer tiles than CUs): EQUAL K slices (a divisor
// c <= 8 of K / 64, slices of >= 10 K-tiles, K >= 48 K-tiles in all, partials within the caller's workspace) as virtual
// tiles.  Of the legal c the one whose virtual tiles best fill the CU rounds they occupy wins (ties: fewer slices), if that
// fill is >= 70 % and at least 15 points above the unsplit fill; 0 = none.  Measured per slice count
// (tools/micro/ksplit_sweep.py, profiles/r02_gemm_ksplit_sweep.txt): 64 tiles (4032 x 1280) want 4 slices - 3x3 conv 0.272
// unsplit / 0.122 at 3 / 0.114 at 4, temporal conv 0.104 / 0.062 / 0.060; 128 tiles (8064 rows, the 18x32 level of a
// CFG-parallel rank) want 2 - 3x3 conv 0.274 -> 0.200, FF-out 0.135 -> 0.108; 36 tiles (a rank of 8) want 5-6 even at
// 10-K-tile slices (temporal conv 0.046 vs 0.050 on 128x128 tiles); below 48 K-tiles the fp32 partials cost more than the idle
// CUs (9216 x 640 x 1920: 0.046 split vs 0.039 on 128x128 tiles).
static int wide_split(const lkgd_gemm_desc* d, long long tiles_wide, int cus) {
  if (d->geglu || !d->workspace || !aligned16(d->workspace)) return 0;
  const int nk = d->K / BK;
  if (knobs.wide_ksplit) {
    const int c = knobs.wide_ksplit;
    return (c >= 2 && nk % c == 0 && (long long)c * d->M * d->N * 4 <= d->workspace_bytes) ? c : 0;
  }
  if (!knobs.splitk || tiles_wide >= cus || nk < 48) return 0;
  const double unsplit = (double)tiles_wide / cus;
  int best = 0;
  double best_fill = 0.0;
  // measured tile counts: 36, 64, 128 (slices 5-6, 4, 2).  Elsewhere - e.g. ~200 tiles, where the fill rule would pick 5 - the
  // partial traffic c * M * N * 4 bytes is kept within what the measured cases moved (4 slices at 64 tiles = 66 MB x 4)
  for (int c = 2; c <= 8 && c * 10 <= nk; ++c) {
    if (nk % c || (long long)c * d->M * d->N * 4 > d->workspace_bytes) continue;
    if (tiles_wide > 128 && c > 2) continue;
    const long long vt = tiles_wide * c, rounds = (vt + cus - 1) / cus;
    const double fill = (double)vt / (double)(rounds * cus);
    if (fill > best_fill + 1e-9) { best_fill = fill; best = c; }
  }
  return (best_fill >= 0.70 && best_fill >= unsplit + 0.15) ? best : 0;
}

// K slices of the four-stage 128x128 kernel (one workgroup per CU): the slice count with the smallest MODELLED time.  A
// workgroup costs a fixed part (prologue, pipeline fill, epilogue or partial-tile store) plus its K-tiles; slicing adds the
// reduce pass, which reads ks fp32 copies of the output.  Constants from tools/micro/mid_knobs.py (time over K at 2304 x 1280:
// 0.75 us per K-tile, 5-6 us fixed; profiles/r05_gemm_mid_knobs.txt); 1 = unsplit.
static int mid_split(const lkgd_gemm_desc* d, long long nwg, int nk, int cus) {
  if (!d->workspace || !aligned16(d->workspace) || d->N % 4) return 1;
  const long long fit = d->workspace_bytes / ((long long)d->M * d->N * 4);
  if (knobs.mid_ksplit_forced) return (knobs.mid_ksplit_forced <= nk && knobs.mid_ksplit_forced <= fit) ? knobs.mid_ksplit_forced : 1;
  if (!knobs.splitk || nk < 16) return 1;
  int best = 1;
  float best_t = 1e30f;
  for (int ks = 1; ks <= 16 && ks <= fit && ks * 8 <= nk; ++ks) {
    const int per = (nk + ks - 1) / ks;
    const long long blocks = nwg * ((nk + per - 1) / per), rounds = (blocks + cus - 1) / cus;
    float t = (float)rounds * (knobs.mid_fix_us + per * knobs.mid_tk_us);
    if (ks > 1) t += knobs.mid_red_us + (float)ks * (float)d->M * (float)d->N * 4.0f / (knobs.mid_red_tbs * 1e6f);
    if (t < best_t * 0.97f) { best_t = t; best = ks; }      // more slices only for a clear gain
  }
  return best;
}

// K slices of the two-stage 128x128 program.  Split-K when the tiles leave workgroup slots (2 per CU) idle: the smallest slice
// count whose blocks fill >= 85 % of the rounds they occupy, slices of >= 4 K-tiles when less than half the slots are filled
// (few-row problems: the reduce pass is tiny) and of >= 32 K-tiles otherwise (the 3x3 convs of the full model's 9x16 level:
// 320 tiles on 512 slots -> 3 slices, 0.172 -> 0.150 ms; its K = 3840 temporal convs lose more in the reduce pass than they
// gain); bounded by the caller's workspace (include/lkgd_hip.h: lkgd_gemm_desc.workspace).  *per_out = K-tiles per slice
static int tile128_split(const lkgd_gemm_desc* d, long long nwg, int cus, int* per_out) {
  int ksplit = 1, per = d->K / BK;
  const int nk = d->K / BK;
  const long long slots = 2LL * cus;
  if (knobs.splitk && d->workspace && aligned16(d->workspace) && d->N % 4 == 0 && nk >= 8 &&
      nwg * 10 < slots * 7) {
    const bool few = nwg * 2 <= slots;
    const int min_slice = few ? 4 : 32;
    long long cap = nk / min_slice;
    if (cap > 16) cap = 16;
    const long long fit = d->workspace_bytes / ((long long)d->M * d->N * 4);
    if (cap > fit) cap = fit;
    long long want = 1;
    for (long long ks = 2; ks <= cap; ++ks) {
      const long long blocks = nwg * ks, rounds = (blocks + slots - 1) / slots;
      if (blocks * 100 >= rounds * slots * 85 || (few && ks == cap)) { want = ks; break; }
    }
    if (few && slots / nwg > want && slots / nwg <= cap) want = slots / nwg;   // fill one whole round
    if (want >= 2) {
      per = (int)((nk + want - 1) / want);
      ksplit = (nk + per - 1) / per;           // every slice non-empty
    }
  }
  *per_out = per;
  return ksplit;
}

// may a launch of this descriptor on the resident-weight kernel carry column statistics?
bool gemm_resw_colstats_ok(const lkgd_gemm_desc* d) {
  const int src = (d->rowbias ? 1 : 0) | (d->res1 ? 2 : 0) | (d->res2 ? 4 : 0);
  return !d->geglu && resw_has_cs(d->K / 64, src);
}

// does the resident-weight kernel cover this problem on a device with `cus` compute units?  (lkgd_gemm_f16's dispatch)
bool gemm_resw_ok(const lkgd_gemm_desc* d, int cus) {
  const int nk = d->K / 64;
  if (nk < 1 || nk > 5 || d->K % 64 || d->mode != LKGD_A_PLAIN || d->csplit < d->K) return false;
  if (d->N % RW_SLAB || (d->geglu != 0 && d->geglu != 80) || d->N / RW_SLAB > cus / 8) return false;
  if (d->geglu && (d->rowbias || d->res1 || d->res2)) return false;
  const int src = (d->rowbias ? 1 : 0) | (d->res1 ? 2 : 0) | (d->res2 ? 4 : 0);
  if (!d->geglu && !resw_has(nk, src)) return false;
  // 16-byte row pieces of out, 8-byte pieces of the sources, 16-byte token fragments; 32-bit row arithmetic
  if (d->ldc % 8 || !aligned16(d->out) || d->lda0 % 8 || !aligned16(d->a0) || !aligned16(d->w)) return false;
  if ((d->res1 && (d->ldr1 % 4 || ((uintptr_t)d->res1 & 7))) || (d->res2 && (d->ldr2 % 4 || ((uintptr_t)d->res2 & 7))) ||
      (d->rowbias && (d->ldrb % 4 || ((uintptr_t)d->rowbias & 7))))
    return false;
  return d->M >= 1 && d->M < (1 << 26);
}

// the 256x256 form serves channel counts that are whole 256-column tiles and not whole 320-column ones (256, 512, 768 ...)
// and would leave more than a tenth of the 320-wide tile columns idle (3072 = 9.6 x 320 stays on 320)
static int wide_tile_n(int N) {
  if (knobs.wide_tile_n && N % knobs.wide_tile_n == 0) return knobs.wide_tile_n;
  return (N % WBN != 0 && N % 256 == 0 && (long long)((N + WBN - 1) / WBN) * WBN * 10 > (long long)N * 11) ? 256 : WBN;
}

int gemm_wide_lds_out(const lkgd_gemm_desc* d, int ksplit, int wn) {
  // plain linears without GEGLU, whole tile columns, 16-byte aligned output rows: the rows leave through LDS (see the epilogue)
  // (the convolutions only when column statistics are asked for: they are summed from the rows in LDS)
  const bool lds_ok = ksplit == 1 && !d->geglu && d->N % wn == 0 && d->ldc % 8 == 0 && aligned16(d->out);
  if (d->colstats && !lds_ok) return LKGD_E_SHAPE;
  return lds_ok && (d->colstats ? true : (knobs.wide_lds_out != 0 && d->mode == LKGD_A_PLAIN)) ? 1 : 0;
}

// tile-program choice for a checked descriptor; *wide_ks_out = K slices of GEMM_WIDE (1 = none); negative = LKGD_E_*
static int gemm_pick(const lkgd_gemm_desc* d, int cus, int* wide_ks_out) {
  // GEGLU weights are packed for one tile family (interleave width 80 -> 256x320 tiles, 32 -> 128-wide tiles)
  // the persistent kernels move epilogue rows as 16-byte chunks: 8-channel granularity and 16-byte aligned rows
  const bool rows16 = d->N % 8 == 0 && d->ldc % 8 == 0 && aligned16(d->out) &&
                      (!d->res1 || (d->ldr1 % 8 == 0 && aligned16(d->res1))) &&
                      (!d->res2 || (d->ldr2 % 8 == 0 && aligned16(d->res2)));
  // ---- tile-program choice.  Rules are the per-shape winners of the interleaved A/B runs (tools/gemm_shapes_bench.py ab,
  //      profiles/r01_gemm_shapes_ab*.txt), expressed through the quantities that explain them: how many workgroup
  //      slots a tiling fills (a 256-row tiling of M = 16 128 x N = 640 is 126 tiles for 256 CUs), K depth (amortises
  //      the epilogue and the pipeline fill), and N granularity (320-wide tiles for N = 320 / 640 / 1280).
  const int v = knobs.variant;
  const bool plain = d->mode == LKGD_A_PLAIN;
  const bool rp_ok = rows16 && plain && d->K <= 320 && d->csplit >= d->K && d->geglu != 80;
  // (the GEGLU epilogue of the 256x320 kernel is compiled into its plain-linear instantiation only)
  const bool wide_ok = (d->geglu == 0 || (d->geglu == 80 && plain)) && d->mode != LKGD_A_CONV3X3_C8 &&
                       d->M < (1 << 24);
  const bool stream_ok = rows16 && d->geglu != 80;
  // resident-weight kernel: a 160-row slab of W[N][K] in LDS per workgroup, every XCD runs all N / 160 slabs
  const bool rw_ok = gemm_resw_ok(d, cus);
  const int wide_n = wide_tile_n(d->N);
  const long long tiles_wide = (long long)((d->M + 255) / 256) * ((d->N + wide_n - 1) / wide_n);
  // N tiles by 320 (by 256 where that divides N and 320 does not: the VAE decoder's 256 / 512) with at most a fifth of all
  // tile columns idle
  const bool n320 = d->N % wide_n == 0 || (long long)((d->N + 319) / 320) * 320 * 4 <= (long long)d->N * 5;
  int pick = 0;
  int wide_ks = 1;
  if (d->mode == LKGD_A_CCONV3) {
    // the causal 3x3x3 gather exists in the 256x320 program only (its kernels are instantiated per mode; the runtime-mode gathers of
    // the other programs do not know it), unsliced: whatever variant a knob forces
    if (!wide_ok || d->ln_colsum) return LKGD_E_SHAPE;
    *wide_ks_out = 1;
    return GEMM_WIDE;
  }
  if (d->geglu == 80) {
    if (!wide_ok) return LKGD_E_SHAPE;
    // 80-wide GEGLU interleave: the 256x320 kernel, or - at K <= 320 from 32k rows - the resident-weight kernel (a slab = one
    // wave's 160 packed rows): its waves run their erf epilogues beside each other's K-loops (72x128 level 0.485 vs 0.533 ms,
    // a CFG-parallel rank's 0.246 vs 0.274; profiles/r03_resw_ab.txt)
    pick = (rw_ok && (v == GEMM_RESW || (v == 0 && d->M >= 32768))) ? GEMM_RESW : GEMM_WIDE;
  } else if (v != 0) {
    pick = v;
  } else if (rw_ok && d->res1 && d->M >= 32768) {
    // K <= 320 projections that carry a residual (attention out, proj_out at the 72x128 level): 0.125 ms against 0.138
    // (row-panel) / 0.152 (256x320) at 258k rows, 0.053 vs 0.059 at 129k.  Without a residual the 256x320 kernel stays
    // ahead (QKV 0.225 vs 0.264, bias-only 0.089 vs 0.096): there the resident-weight kernel's token loads (64 different
    // rows per instruction) and its eight in-order waves do not hide what they wait for
    pick = GEMM_RESW;
  } else if (rp_ok && d->M >= 4096 && d->K >= 192 && (d->res1 || (d->N != 320 && d->M >= 196608))) {
    // K <= 320 projections at 258k rows: A read exactly once.  The 320 x 320 ones only when they carry a residual (its
    // row-coalesced epilogue wins there; without one the 256x320 kernel is ahead).  Without a residual (QKV) the two
    // programs tie at 258k rows since the 256x320 kernel writes its rows through LDS, and at a sharded rank's row counts
    // (129k / 65k / 37k: 504 / 252 / 144 row panels for 256 CUs) the 256x320 tiles fill the CUs better: 0.118 vs 0.125,
    // 0.039 vs 0.052 ms (profiles/r02_gemm_shapes_ab_shards.txt)
    pick = GEMM_ROWPANEL;
  } else if (wide_ok && d->geglu == 0 && d->N % 320 == 0 && d->M >= 1024 && (wide_ks = wide_split(d, tiles_wide, cus)) >= 2) {
    pick = GEMM_WIDE;                                    // fewer tiles than CUs, deep K: 256x320 tiles over equal K slices
                                                         // (the 9x16 level; the 18x32 / 36x64 levels of sharded ranks)
  } else if (wide_ok && d->geglu == 0 && n320 && d->K >= 320 && tiles_wide * 2 >= cus - 16) {
    pick = GEMM_WIDE;                                    // every N = 320 / 640 / 960 / 1280 / 1920 / 3840 shape of the model
                                                         // whose 256x320 tiles fill at least half the CUs; N = 256 / 512 (the
                                                         // VAE decoder) on the 256x256 form of the same program
                                                         // (tools/micro/vae_shapes_bench.py)
  } else if (d->M < 12288) {
    wide_ks = 1;
    // the 9x16 level (M = 4032; also the 9216-row 36x64 level of a rank of 8): 256-row tilings leave most CUs idle; 128x128
    // at two workgroups per CU fills best, except for the wide-N projections (QKV: 16 x 12 tiles of 256x320)
    pick = (wide_ok && plain && d->geglu == 0 && d->N % 320 == 0 && d->N >= 2560 && d->M >= 2048 && !d->res1) ? GEMM_WIDE : GEMM_TILE128;
    // 128x128 tiles that give a CU one workgroup at most (the 18x32 / 9x16 levels of a frame-sharded rank, the full model's
    // 9x16 level): the four-stage ring instead of the two-stage kernel, whose K-steps then wait out every load - 2304 x 1280 x
    // 1280 0.022 vs 0.036 ms, the 576-row temporal conv 0.025 vs 0.033, ff-out 0.029 vs 0.036 (profiles/r05_gemm_mid_ab.txt)
    if (pick == GEMM_TILE128 && d->geglu == 0 && (long long)((d->M + BM - 1) / BM) * ((d->N + BN - 1) / BN) <= cus) pick = GEMM_MID;
  } else {
    pick = GEMM_STREAM;
  }
  // applicability (forced variants fall back the same way)
  if (pick == GEMM_RESW && !rw_ok) pick = d->geglu == 80 ? GEMM_WIDE : GEMM_TILE128;
  if (pick == GEMM_ROWPANEL && !rp_ok) pick = GEMM_TILE128;
  if (d->ln_colsum) {          // LayerNorm fold: only the row-panel program holds whole rows in registers
    if (!rp_ok || d->geglu || d->K % 64 || !aligned16(d->ln_colsum) || !(d->ln_eps > 0.f)) return LKGD_E_SHAPE;
    pick = GEMM_ROWPANEL;
  }
  if (pick == GEMM_WIDE && !wide_ok) pick = GEMM_STREAM;
  // deep-K problems (3x3 / temporal convs, K >= 960) take the 256x128 three-stage ring: its two K-tiles in flight hide
  // the HBM latency the two-stage kernel exposes every K-step.  Short-K GEMMs (K = 320/640 projections at 258k rows) are
  // epilogue-bound; they keep 128x128 tiles at two workgroups per CU so one workgroup's epilogue overlaps the other's
  // main loop (measured per shape: tools/gemm_shapes_bench.py, profiles/r01_gemm_shapes.txt).
  if (pick == GEMM_STREAM && (!stream_ok || d->M <= 256)) pick = (d->K >= 960 && d->M > 256) ? GEMM_TILE256 : GEMM_TILE128;
  if (d->geglu == 80 && pick != GEMM_WIDE && pick != GEMM_RESW) return LKGD_E_SHAPE;   // 80-wide interleave: 256x320 / resident-weight kernels
  *wide_ks_out = wide_ks;
  return pick;
}

// wide_split() for a forced 256x320 variant follows the same slicing rule as the automatic one
static int gemm_wide_slices(const lkgd_gemm_desc* d, int cus, int wide_ks) {
  if (d->mode == LKGD_A_CCONV3) return 1;
  if (knobs.variant == GEMM_WIDE) {
    const int wide_n = wide_tile_n(d->N);
    const long long tiles_wide = (long long)((d->M + 255) / 256) * ((d->N + wide_n - 1) / wide_n);
    wide_ks = wide_n == 320 ? wide_split(d, tiles_wide, cus) : 1;
  }
  return wide_ks >= 2 ? wide_ks : 1;
}

// Tile form of an unsliced 256x320-program launch: tile rows wm (256 | 192: wave tile 64 | 48 rows) x tile columns wn (320 | 256).
// The N-only rule (lkgd_gemm_wide_tile_n) fixes wn where only one width divides N; a plain linear whose channel count BOTH widths
// divide (1280, 3840) may take either.  Among the candidates the one with the smallest MODELLED time wins: rounds over the CUs
// x the cost of one tile of that form relative to 256x320 - 1.00 | 0.85 (256x256) | 0.83 (192x320) | 0.72 (192x256), measured
// on one-round shapes (tools/micro/wide_tile_m.py, profiles/r05_wide_tile_m.txt: 36 864 x 320 x 2880 conv 88.8 -> 75.5 us,
// 16 128 x 640 x 5760 conv 154.7 -> 127.7, 8064 x 1280 x 1280 51.6 -> 43.7 / 42.5 / 37.1) - and a smaller tile must win by 3 %.
// On the full forward every large shape keeps 256x320 (1008 tiles = 4 rounds against 1344 = 6 x 0.83); the smaller forms are
// for the levels of a sharded rank, where 256-row tiles leave CUs idle.
static void gemm_wide_form(const lkgd_gemm_desc* d, int cus, int slices, int* wn_out, int* wm_out) {
  const int fn = knobs.wide_tile_n, fm = knobs.wide_tile_m;
  int wn0 = wide_tile_n(d->N);
  // the causal 3x3x3 convolutions run on this program whatever N is: up to 256 channels (the CogVideoX VAE decoder's 128 at its
  // 480 x 720 level, where most of its FLOP are) one 256-column tile idles fewer columns than one 320-column tile
  if (d->mode == LKGD_A_CCONV3 && d->N <= 256 && !fn) wn0 = 256;
  *wn_out = wn0;
  *wm_out = 256;
  if (slices != 1) return;
  if (fn || fm) {                                  // A/B knobs: no rule
    if (fm) *wm_out = fm;
    return;
  }
  const bool both = wn0 == 320 && d->mode == LKGD_A_PLAIN && !d->geglu && d->N % 320 == 0 && d->N % 256 == 0;   // (GEGLU: 80-wide interleave)
  float best = 0.f;
  for (int pass = 0; pass < 4; ++pass) {           // 256x wn0 first: the default, to which the others are compared
    const int wm = (pass & 1) ? 192 : 256, wn = (pass & 2) ? 256 : wn0;
    if ((pass & 2) && !both) continue;
    if (pass && d->cs_rows > 0 && d->cs_rows % wm) continue;       // column sums: whole tiles per GroupNorm sample
    const long long tiles = (long long)((d->M + wm - 1) / wm) * ((d->N + wn - 1) / wn);
    const long long rounds = (tiles + cus - 1) / cus;
    const float unit = (wn == 256 ? 0.85f : 1.0f) * (wm == 192 ? (wn == 256 ? 0.72f / 0.85f : 0.83f) : 1.0f);
    const float cost = (float)rounds * unit;
    if (pass == 0) best = cost;
    else if (cost < best * 0.97f) { best = cost; *wn_out = wn; *wm_out = wm; }
  }
}

int gemm_make_plan(const lkgd_gemm_desc* d, int cus, gemm_plan* pl) {
  int wide_ks = 1;
  const int pick = gemm_pick(d, cus, &wide_ks);
  if (pick < 0) return pick;
  pl->program = (gemm_program)pick;
  pl->ks = 1;
  pl->per = d->K / BK;
  pl->wm = BM;
  pl->wn = BN;
  pl->cs_blk = 0;
  pl->lds_out = 0;
  const bool cs_shape = !d->geglu && d->N % 8 == 0;
  switch (pl->program) {
    case GEMM_RESW:
      pl->wm = 32; pl->wn = RW_SLAB;               // a wave's 32 token rows x a 160-row weight slab (gemm_resw.hip)
      if (cs_shape && gemm_resw_colstats_ok(d)) pl->cs_blk = 32;
      break;
    case GEMM_ROWPANEL:
      pl->wm = 256; pl->wn = 64;                   // gemm_rowpanel.hip
      break;
    case GEMM_WIDE:
      pl->ks = gemm_wide_slices(d, cus, wide_ks);
      gemm_wide_form(d, cus, pl->ks, &pl->wn, &pl->wm);
      pl->per = (d->K / BK) / pl->ks;
      // the 256x320 program sums the columns of the row segments it parks in LDS: whole 320-column tiles, unsliced K
      if (cs_shape && pl->ks == 1 && d->ldc % 8 == 0 && aligned16(d->out) && d->N % pl->wn == 0) pl->cs_blk = pl->wm;
      pl->lds_out = gemm_wide_lds_out(d, pl->ks, pl->wn) > 0 ? 1 : 0;
      break;
    case GEMM_STREAM:
    case GEMM_TILE256:
      pl->wm = BM2;                                // gemm_stream.hip / lkgd_gemm_kernel_256
      if (pl->program == GEMM_TILE256 && (long long)((d->M + BM2 - 1) / BM2) * ((d->N + BN - 1) / BN) > 0x7fffffffLL) return LKGD_E_SHAPE;
      break;
    case GEMM_TILE128:
    case GEMM_MID: {
      const long long nwg = (long long)((d->M + BM - 1) / BM) * ((d->N + BN - 1) / BN);
      if (nwg > 0x7fffffffLL) return LKGD_E_SHAPE;
      const int nk = d->K / BK;
      if (pl->program == GEMM_MID) {
        const int ksplit = mid_split(d, nwg, nk, cus);
        if (ksplit > 1) {
          pl->per = (nk + ksplit - 1) / ksplit;
          pl->ks = (nk + pl->per - 1) / pl->per;           // every slice non-empty
        }
      } else {
        pl->ks = tile128_split(d, nwg, cus, &pl->per);
      }
      break;
    }
  }
  return LKGD_OK;
}

}  // namespace lkgd_gemm

using namespace lkgd_gemm;

extern "C" {

int lkgd_gemm_plan(const lkgd_gemm_desc* d, int32_t cus, lkgd_gemm_plan_info* out) {
  if (!out) return LKGD_E_NULL;
  int rc = check_desc(d);
  if (rc != LKGD_OK) return rc;
  if (cus < 0) return LKGD_E_SHAPE;
  int n = cus;
  if (n == 0 && (rc = gemm_device_cus(&n)) != LKGD_OK) return rc;
  gemm_plan pl;
  if ((rc = gemm_make_plan(d, n, &pl)) != LKGD_OK) return rc;
  out->program = pl.program;
  out->k_slices = pl.ks;
  out->tile_m = pl.wm;
  out->tile_n = pl.wn;
  out->colstats_block = pl.cs_blk;
  out->lds_out = pl.lds_out;
  return LKGD_OK;
}

int lkgd_gemm_colstats_block(const lkgd_gemm_desc* d) {
  if (!d || check_desc(d) != LKGD_OK) return 0;
  int cus = 0;
  if (gemm_device_cus(&cus) != LKGD_OK) return 0;
  gemm_plan pl;
  return gemm_make_plan(d, cus, &pl) == LKGD_OK ? pl.cs_blk : 0;
}

int lkgd_gemm_wide_tile_n(int N) { return wide_tile_n(N); }

// ---- the knobs' setters (include/lkgd_hip_debug.h)
void lkgd_debug_set_gemm_variant(int32_t v) { knobs.variant = (v >= GEMM_TILE128 && v <= GEMM_MID) ? v : 0; }
void lkgd_debug_set_gemm_splitk(int32_t on) { knobs.splitk = on != 0; }
void lkgd_debug_set_mid_model(float tk, float fix, float red, float tbs, int32_t forced) {
  if (tk > 0) knobs.mid_tk_us = tk;
  if (fix > 0) knobs.mid_fix_us = fix;
  if (red > 0) knobs.mid_red_us = red;
  if (tbs > 0) knobs.mid_red_tbs = tbs;
  knobs.mid_ksplit_forced = forced < 0 ? 0 : forced;
}
void lkgd_debug_set_wide_ksplit(int32_t k) { knobs.wide_ksplit = k < 0 ? 0 : k; }
void lkgd_debug_set_wide_lds_out(int32_t on) { knobs.wide_lds_out = on; }
void lkgd_debug_set_wide_tile_n(int32_t wn) { knobs.wide_tile_n = (wn == 256 || wn == WBN) ? wn : 0; }
void lkgd_debug_set_wide_tile_m(int32_t wm) { knobs.wide_tile_m = (wm == 192 || wm == WBM) ? wm : 0; }

}  // extern "C"
