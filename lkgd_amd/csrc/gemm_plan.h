// What lkgd_gemm_f16 decides on the host, and the seams between the planner (gemm_plan.cpp: pure arithmetic, no HIP) and the
// five kernel files that launch from its plan.  Everything here has C++ linkage and hidden visibility: the shared library
// exports only what the headers under include/ declare.
#pragma once
#include <stdint.h>

#include "../../include/lkgd_hip.h"
#include "aligned16.h"

namespace lkgd_gemm __attribute__((visibility("hidden"))) {

// tile sizes the rules reason about; the kernel files take them from here
constexpr int BK = 64;                  // K-tile of every program
constexpr int BM = 128, BN = 128;       // gemm.hip: the two 128x128 programs
constexpr int BM2 = 256;                // gemm.hip: the 256x128 ring
constexpr int WBM = 256, WBN = 320;     // gemm_wide.hip (forms: 256 | 192 rows x 320 | 256 columns)
constexpr int RW_SLAB = 160;            // gemm_resw.hip: weight rows per resident slab

// the tile programs (values frozen: include/lkgd_hip.h, tests/golden/gemm_census.json)
enum gemm_program {
  GEMM_TILE128 = LKGD_GEMM_TILE128,     // gemm.hip::lkgd_gemm_kernel: 128x128, two LDS stages
  GEMM_TILE256 = LKGD_GEMM_TILE256,     // gemm.hip::lkgd_gemm_kernel_256: 256x128 three-stage ring
  GEMM_STREAM = LKGD_GEMM_STREAM,       // gemm_stream.hip: persistent 256x128
  GEMM_WIDE = LKGD_GEMM_WIDE,           // gemm_wide.hip: persistent 256x320 family
  GEMM_ROWPANEL = LKGD_GEMM_ROWPANEL,   // gemm_rowpanel.hip: register-resident row panel
  GEMM_RESW = LKGD_GEMM_RESW,           // gemm_resw.hip: resident weights
  GEMM_MID = LKGD_GEMM_MID              // gemm.hip::lkgd_gemm_mid_kernel: 128x128 on the four-stage ring
};

// Everything lkgd_gemm_f16 decides on the host for a CHECKED descriptor, in one place: lkgd_gemm_f16 launches from it and
// lkgd_gemm_plan / lkgd_gemm_colstats_block report it, so what they say is what runs.
struct gemm_plan {
  gemm_program program;
  int ks, per;     // K slices (1 = none) and K-tiles per slice (GEMM_TILE128 and GEMM_MID; GEMM_WIDE's slices are equal)
  int wm, wn;      // tile rows x columns
  int cs_blk;      // rows per colstats block, 0 = no column sums
  int lds_out;     // GEMM_WIDE: rows leave through LDS
};

int check_desc(const lkgd_gemm_desc* d);                                   // LKGD_OK or the LKGD_E_* lkgd_gemm_f16 returns
int gemm_make_plan(const lkgd_gemm_desc* d, int cus, gemm_plan* pl);       // d checked; LKGD_OK or LKGD_E_*
// do the output rows of a GEMM_WIDE launch leave through LDS?  1 = yes, 0 = direct 8-byte stores, LKGD_E_SHAPE = column sums asked
// for where the rows cannot go through LDS
int gemm_wide_lds_out(const lkgd_gemm_desc* d, int ksplit, int wn);
// does the resident-weight kernel cover this problem on a device with `cus` compute units, and may that launch carry column sums?
bool gemm_resw_ok(const lkgd_gemm_desc* d, int cus);
bool gemm_resw_colstats_ok(const lkgd_gemm_desc* d);

// Which (K, epilogue sources) instantiations of the resident-weight kernel exist: the ones hipcc allocates WITHOUT scratch spills
// inside the 96-register budget (tests/test_host_cpu.py compiles gemm_resw.hip with -Rpass-analysis and checks it).  A spill would be
// more than slow there: the residual loads are issued and awaited by hand, and spill code placed between a load and its wait would
// save a register whose data has not arrived yet.
constexpr bool resw_has(int nk, int src) { return nk >= 4 ? src <= 5 : (src == 0 || src == 1 || src == 2 || src == 4 || src == 6); }
constexpr bool resw_has_cs(int nk, int src) { return src == 0 || src == 2; }      // bare / bias, + one residual (proj_out)

// CU count of the current device for lkgd_gemm_plan(cus = 0) and lkgd_gemm_colstats_block: LKGD_OK, or LKGD_E_LAUNCH when there
// is no device to ask.  The planner's one question to the device; gemm.hip answers it (common.h::lkgd_cu_query).
int gemm_device_cus(int* cus);

// the programs that live in files of their own; each checks what its kernels assume.  GEMM_WIDE with pl.ks > 1 leaves fp32
// partials in d->workspace: the caller runs the reduce pass
int gemm_stream_launch(const lkgd_gemm_desc* d, lkgd_stream_t stream, int cus, const gemm_plan& pl);
int gemm_wide_launch(const lkgd_gemm_desc* d, lkgd_stream_t stream, int cus, const gemm_plan& pl);
int gemm_rowpanel_launch(const lkgd_gemm_desc* d, lkgd_stream_t stream, int cus, const gemm_plan& pl);
int gemm_resw_launch(const lkgd_gemm_desc* d, lkgd_stream_t stream, int cus, const gemm_plan& pl);

}  // namespace lkgd_gemm
