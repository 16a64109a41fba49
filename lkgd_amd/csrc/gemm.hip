// MFMA fp16 GEMM with implicit-convolution A operand and fused epilogue (include/lkgd_hip.h section 1).
//
// Design (gfx950 / CDNA4):
//   * 128x128 output tile per 256-thread workgroup (4 waves as 2x2, 64x64 per wave = 2x2 v_mfma_f32_32x32x16_f16,
//     64 fp32 accumulator VGPRs), BK = 64, two LDS stages of 32 KiB -> 2 workgroups per CU.
//   * both operands are K-contiguous ([M][K] tokens, [N][K] weights), so A and B fragments are one ds_read_b128 each.
//   * staging is LDS-DMA (global_load_lds_dwordx4): the LDS image is lane-linear, the bank-conflict swizzle
//     (16-byte chunk ^= (row>>1)&7 inside each 128-byte row) is applied to the per-lane SOURCE address and to the
//     fragment read.  The per-lane source address is also what makes the A operand an implicit convolution: every
//     lane computes where "its" 16 bytes live (3x3 tap with halo, stride-2, nearest-2x upsample, frame shift,
//     two-tensor channel concat) and out-of-image lanes read a zero page.
//   * one barrier per K-tile (stage t+1 is issued before the MFMAs of tile t).
//   * epilogue: accumulators -> LDS (fp32, reusing the staging buffers) -> row-contiguous 8-byte stores with bias,
//     row-indexed bias (time embedding / positional / cross-attention), GEGLU, two scaled residuals (AlphaBlender).
//   * blockIdx -> tile map is XCD-aware (each XCD's L2 sees a contiguous range of tiles, n fastest).
#include "gemm_common.h"

// BM x BN = 128 x 128, BM2 = 256 (rows of the large-M tile), BK: gemm_plan.h
#define STAGE_BYTES (2 * BM * BK * 2)  // A 16 KiB + B 16 KiB
#define GEMM_LDS (2 * STAGE_BYTES)     // 64 KiB (also holds the fp32 C tile in the epilogue)

// ksplit > 1: blockIdx.y owns K-tiles [y*per, (y+1)*per) and leaves its fp32 partial tile in ws[y][M][N]
__global__ __launch_bounds__(256, 2) void lkgd_gemm_kernel(const lkgd_gemm_desc p, int tiles_m, int tiles_n, int ksplit,
                                                           int per, float* ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int w = t >> 6;
  const int wr = w >> 1, wc = w & 1;

  const int nwg = tiles_m * tiles_n;
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- per-thread staging rows: thread t fills LDS slots t + 256*i (slot = row*8 + chunk), i = 0..3
  const int srow = t >> 3;                               // + 32*i
  const int schunk = (t & 7) ^ ((t >> 4) & 7);           // logical 16-byte chunk this thread fetches (swizzled)
  AGather<4> ag;
  const half_t* brow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ag.row[i] = a_row(p, m0 + srow + 32 * i);
    int n = n0 + srow + 32 * i;
    brow[i] = n < p.N ? (const half_t*)p.w + (long long)n * p.K + schunk * 8 : nullptr;
  }
  const int nk_all = p.K / BK;
  const int kb = ksplit > 1 ? (int)blockIdx.y * per : 0;
  const int ke = ksplit > 1 ? (kb + per < nk_all ? kb + per : nk_all) : nk_all;
  a_segment<4>(p, ag, kb * BK, schunk);

  auto stage = [&](int buf, int kt) {
    char* sa = smem + buf * STAGE_BYTES;
    char* sb = sa + BM * BK * 2;
    const int k0 = kt * BK;
    if (k0 >= ag.seg_end) a_segment<4>(p, ag, k0, schunk);      // wave-uniform: K-tiles are staged in order
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(a_chunk<4>(ag, i, k0), sa + (w * 64 + 256 * i) * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      glds16(brow[i] ? brow[i] + k0 : (const half_t*)p.zeros, sb + (w * 64 + 256 * i) * 16);
  };

  float16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fragment read addresses (bytes inside a stage): row*128 + ((ks*2 + h) ^ ((row>>1)&7))*16
  const int h = lane >> 5;
  int a_off[2], b_off[2], a_sw[2], b_sw[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int ra = wr * 64 + i * 32 + (lane & 31);
    int rb = wc * 64 + i * 32 + (lane & 31);
    a_off[i] = ra * 128; a_sw[i] = (ra >> 1) & 7;
    b_off[i] = BM * BK * 2 + rb * 128; b_sw[i] = (rb >> 1) & 7;
  }

  stage(0, kb);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = kb; kt < ke; ++kt) {
    const int cur = (kt - kb) & 1;
    if (kt + 1 < ke) stage(cur ^ 1, kt + 1);
    const char* sbase = smem + cur * STAGE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      half8_t af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = *(const half8_t*)(sbase + a_off[i] + (((ks * 2 + h) ^ a_sw[i]) << 4));
        bf[i] = *(const half8_t*)(sbase + b_off[i] + (((ks * 2 + h) ^ b_sw[i]) << 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // ---- epilogue: accumulators -> LDS fp32 tile [128][128] -> row-contiguous stores
  float* ct = (float*)smem;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int row = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        int col = wc * 64 + j * 32 + (lane & 31);
        ct[row * BN + col] = acc[i][j][r];
      }
  __syncthreads();

  if (ksplit > 1) {
    // partial tile -> workspace, 16-byte row-contiguous stores; the epilogue runs in lkgd_gemm_splitk_reduce
    float* dst = ws + (long long)blockIdx.y * p.M * p.N;
    const int col = (t & 31) * 4;
    if (n0 + col < p.N) {
      for (int row = t >> 5; row < BM && m0 + row < p.M; row += 8)
        *(float4_t*)(dst + (long long)(m0 + row) * p.N + n0 + col) = *(const float4_t*)(ct + row * BN + col);
    }
    return;
  }
  gemm_epilogue<BM, BN, 256>(p, ct, t, m0, n0, tn);
}

// ------------------------------------------------------------------------------------------------------------------
// Few-row variant (round 5): the same 128x128 tile and wave layout on a FOUR-stage LDS ring (128 KiB, one workgroup per
// CU), three K-tiles of LDS-DMA in flight behind a counted s_waitcnt vmcnt.  The two-stage kernel above waits for every
// K-tile's loads before its MFMAs (vmcnt(0) + barrier per K-step): with a second workgroup on the CU that latency is
// hidden, but the problems of a frame-sharded rank (576 - 9216 rows) give a CU ONE workgroup or none, and a K-step then
// costs the whole L2 / fabric round trip - 1.3-1.8 us per K-tile measured (profiles/r05_plan_profile_base.txt: 2304 x
// 1280 x 1280 in 36 us unsplit).  ksplit > 1 as above: blockIdx.y owns K-tiles [y*per, (y+1)*per).
#define MID_NST 4
#define MID_NT 512
#define MID_LDS (MID_NST * STAGE_BYTES)   // 128 KiB (holds the 64 KiB fp32 C tile in the epilogue)
#define MID_LOADS 4                       // LDS-DMA instructions per thread and stage (2 A + 2 B)

__global__ __launch_bounds__(MID_NT, 2) void lkgd_gemm_mid_kernel(const lkgd_gemm_desc p, int tiles_m, int tiles_n, int ksplit,
                                                                  int per, float* ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int w = t >> 6;              // 0..7: two waves per SIMD, so one wave's fragment reads and LDS-DMA issue run under
  const int wr = w >> 1, wc = w & 1; // the other's MFMAs; wave tile 32 x 64 (4 x 2 waves)

  const int nwg = tiles_m * tiles_n;
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;

  // staging: slot = row*8 + chunk; thread t fills A slots t + 512*i and B slots t + 512*i (i < 2): row = (t>>3) + 64*i
  const int srow = t >> 3;
  const int schunk = (t & 7) ^ ((t >> 4) & 7);           // logical 16-byte chunk this thread fetches (swizzled)
  AGather<2> ag;
  const half_t* brow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ag.row[i] = a_row(p, m0 + srow + 64 * i);
    int n = n0 + srow + 64 * i;
    brow[i] = n < p.N ? (const half_t*)p.w + (long long)n * p.K + schunk * 8 : nullptr;
  }
  const int nk_all = p.K / BK;
  const int kb = ksplit > 1 ? (int)blockIdx.y * per : 0;
  const int ke = ksplit > 1 ? (kb + per < nk_all ? kb + per : nk_all) : nk_all;
  const int nkt = ke - kb;
  a_segment<2>(p, ag, kb * BK, schunk);

  auto stage = [&](int buf, int kt) {
    char* sa = smem + buf * STAGE_BYTES;
    char* sb = sa + BM * BK * 2;
    const int k0 = kt * BK;
    if (k0 >= ag.seg_end) a_segment<2>(p, ag, k0, schunk);      // wave-uniform: K-tiles are staged in order
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16(a_chunk<2>(ag, i, k0), sa + (w * 64 + 512 * i) * 16);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      glds16(brow[i] ? brow[i] + k0 : (const half_t*)p.zeros, sb + (w * 64 + 512 * i) * 16);
  };

  float16_t acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  // fragment read addresses (bytes inside a stage): row*128 + ((ks*2 + h) ^ ((row>>1)&7))*16
  const int h = lane >> 5;
  const int ra = wr * 32 + (lane & 31);
  const int a_off = ra * 128, a_sw = (ra >> 1) & 7;
  int b_off[2], b_sw[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    int rb = wc * 64 + j * 32 + (lane & 31);
    b_off[j] = BM * BK * 2 + rb * 128; b_sw[j] = (rb >> 1) & 7;
  }

  for (int s = 0; s < MID_NST - 1 && s < nkt; ++s) stage(s, kb + s);
  int cur = 0;
  for (int i = 0; i < nkt; ++i) {
    // tile i must have landed: this thread leaves only the (at most two) NEWER tiles' loads outstanding; the barrier then
    // makes every thread's tile-i loads visible and frees the buffer of tile i-1 for restaging
    const int newer = nkt - 1 - i;
#ifndef MID_X_NOBAR        /* MID_X_*: timing experiments only (tools/micro/mid_knobs.sh), results wrong by construction */
    if (newer >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (newer == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#endif
    const char* sbase = smem + cur * STAGE_BYTES;
    half8_t af[4], bf[4][2];                     // the whole K-tile's fragments: 12 reads in flight in front of the MFMAs
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
#ifdef MID_X_NOLDS
      af[ks] = (half8_t)(half_t)(float)(lane + i);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[ks][j] = (half8_t)(half_t)(float)(lane - i + j);
#else
      af[ks] = *(const half8_t*)(sbase + a_off + (((ks * 2 + h) ^ a_sw) << 4));
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[ks][j] = *(const half8_t*)(sbase + b_off[j] + (((ks * 2 + h) ^ b_sw[j]) << 4));
#endif
    }
#ifndef MID_X_NODMA
    if (i + MID_NST - 1 < nkt) {
      int nb = cur + MID_NST - 1; if (nb >= MID_NST) nb -= MID_NST;
      stage(nb, kb + i + MID_NST - 1);
    }
#endif
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#ifdef MID_X_NOMFMA
        acc[j][ks] += (float)af[ks][j] * (float)bf[ks][j][0];
#else
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[ks], bf[ks][j], acc[j], 0, 0, 0);
#endif
      }
    cur = cur + 1 == MID_NST ? 0 : cur + 1;
  }
  __syncthreads();   // all waves done reading the ring before it becomes the C tile

  float* ct = (float*)smem;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int row = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      int col = wc * 64 + j * 32 + (lane & 31);
      ct[row * BN + col] = acc[j][r];
    }
  __syncthreads();

  if (ksplit > 1) {
    float* dst = ws + (long long)blockIdx.y * p.M * p.N;
    const int col = (t & 31) * 4;
    if (n0 + col < p.N) {
      for (int row = t >> 5; row < BM && m0 + row < p.M; row += 16)
        *(float4_t*)(dst + (long long)(m0 + row) * p.N + n0 + col) = *(const float4_t*)(ct + row * BN + col);
    }
    return;
  }
  gemm_epilogue<BM, BN, MID_NT>(p, ct, t, m0, n0, tn);
}

// second pass of a split-K GEMM: 32 x 128 output tile per workgroup, partials added in slice order, then the shared epilogue
__global__ __launch_bounds__(256) void lkgd_gemm_splitk_reduce(const lkgd_gemm_desc p, int tiles_n, int ksplit,
                                                               const float* ws) {
  __shared__ __attribute__((aligned(16))) float ct[32 * BN];
  const int t = threadIdx.x;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int m0 = tm * 32, n0 = tn * BN;
  const int col = (t & 31) * 4;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int row = (t >> 5) + 8 * it;
    float4_t v = {0.f, 0.f, 0.f, 0.f};
    if (m0 + row < p.M && n0 + col < p.N) {
      const float* src = ws + (long long)(m0 + row) * p.N + n0 + col;
      for (int s = 0; s < ksplit; ++s) v += *(const float4_t*)(src + (long long)s * p.M * p.N);
    }
    *(float4_t*)(ct + row * BN + col) = v;
  }
  __syncthreads();
  gemm_epilogue<32, BN, 256>(p, ct, t, m0, n0, tn);
}

// ------------------------------------------------------------------------------------------------------------------
// Large-M variant: 256x128 tile, 512 threads (8 waves as 4x2, 64x64 per wave), BK = 64, THREE LDS stages of 48 KiB
// (144 KiB, one workgroup per CU, two waves per SIMD).  Two K-tiles of LDS-DMA stay in flight across the (single,
// raw) barrier of each K-step behind a COUNTED s_waitcnt vmcnt - the HBM latency that the two-stage kernel above
// exposes every K-step is covered by two K-steps of MFMA work.
#define NT2 512
#define STAGE2_BYTES ((BM2 + BN) * BK * 2)   // A 32 KiB + B 16 KiB
#define NSTAGE2 3
#define GEMM2_LDS (NSTAGE2 * STAGE2_BYTES)   // 144 KiB (holds the 128 KiB fp32 C tile in the epilogue)

__global__ __launch_bounds__(NT2, 2) void lkgd_gemm_kernel_256(const lkgd_gemm_desc p, int tiles_m, int tiles_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int w = t >> 6;              // 0..7
  const int wr = w >> 1, wc = w & 1;
  const int nwg = tiles_m * tiles_n;
  const int bid = xcd_remap(blockIdx.x, nwg);
  const int tm = bid / tiles_n, tn = bid - tm * tiles_n;
  const int m0 = tm * BM2, n0 = tn * BN;

  // staging: A slots t + 512*i (i<4): row = (t>>3) + 64*i; B slots t + 512*i (i<2)
  const int srow = t >> 3;
  const int schunk = (t & 7) ^ ((t >> 4) & 7);
  AGather<4> ag;
  const half_t* brow[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) ag.row[i] = a_row(p, m0 + srow + 64 * i);
  a_segment<4>(p, ag, 0, schunk);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int n = n0 + srow + 64 * i;
    brow[i] = n < p.N ? (const half_t*)p.w + (long long)n * p.K + schunk * 8 : nullptr;
  }
  auto stage = [&](int buf, int kt) {
    char* sa = smem + buf * STAGE2_BYTES;
    char* sb = sa + BM2 * BK * 2;
    const int k0 = kt * BK;
    if (k0 >= ag.seg_end) a_segment<4>(p, ag, k0, schunk);      // wave-uniform: K-tiles are staged in order
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(a_chunk<4>(ag, i, k0), sa + (w * 64 + 512 * i) * 16);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      glds16(brow[i] ? brow[i] + k0 : (const half_t*)p.zeros, sb + (w * 64 + 512 * i) * 16);
  };

  float16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int h = lane >> 5;
  int a_off[2], b_off[2], a_sw[2], b_sw[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int ra = wr * 64 + i * 32 + (lane & 31);
    int rb = wc * 64 + i * 32 + (lane & 31);
    a_off[i] = ra * 128; a_sw[i] = (ra >> 1) & 7;
    b_off[i] = BM2 * BK * 2 + rb * 128; b_sw[i] = (rb >> 1) & 7;
  }

  const int nk = p.K / BK;
  stage(0, 0);
  if (nk > 1) stage(1, 1);
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // tile kt must have landed: this thread leaves only the NEWER tile's 6 LDS-DMA ops outstanding, then the
    // barrier makes every thread's tile-kt loads visible and frees buffer (kt-1)%3 for restaging
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 2 < nk) {
      int nb = cur + 2; if (nb >= NSTAGE2) nb -= NSTAGE2;
      stage(nb, kt + 2);
    }
    const char* sbase = smem + cur * STAGE2_BYTES;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      half8_t af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = *(const half8_t*)(sbase + a_off[i] + (((ks * 2 + h) ^ a_sw[i]) << 4));
        bf[i] = *(const half8_t*)(sbase + b_off[i] + (((ks * 2 + h) ^ b_sw[i]) << 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    cur = cur + 1 == NSTAGE2 ? 0 : cur + 1;
  }
  __syncthreads();   // all waves done reading the ring before it becomes the C tile

  float* ct = (float*)smem;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int row = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        int col = wc * 64 + j * 32 + (lane & 31);
        ct[row * BN + col] = acc[i][j][r];
      }
  __syncthreads();
  gemm_epilogue<BM2, BN, NT2>(p, ct, t, m0, n0, tn);
}

// ------------------------------------------------------------------------------------------------------------------
// Host side: lkgd_gemm_f16 checks the descriptor, asks the planner (gemm_plan.cpp) and launches the plan's program.
int lkgd_gemm::gemm_device_cus(int* cus) { return lkgd_cu_query(cus) ? LKGD_OK : LKGD_E_LAUNCH; }

// second pass of a K-sliced launch (GEMM_TILE128, GEMM_MID, GEMM_WIDE): the partials in d->workspace, then the shared epilogue
static int splitk_reduce_launch(const lkgd_gemm_desc* d, hipStream_t stream, int ks) {
  const int tiles_n = (d->N + BN - 1) / BN;
  const unsigned rblocks = (unsigned)(((d->M + 31) / 32) * tiles_n);
  hipLaunchKernelGGL(lkgd_gemm_splitk_reduce, dim3(rblocks), dim3(256), 0, stream, *d, tiles_n, ks, (const float*)d->workspace);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// GEMM_TILE128 (two LDS stages) and GEMM_MID (four-stage ring): 128x128 tiles, pl.ks K slices of pl.per K-tiles + the reduce pass
static int tile128_launch(const lkgd_gemm_desc* d, hipStream_t stream, const gemm_plan& pl) {
  const int tiles_m = (d->M + BM - 1) / BM, tiles_n = (d->N + BN - 1) / BN;
  const unsigned nwg = (unsigned)(tiles_m * tiles_n);
  float* ws = pl.ks > 1 ? (float*)d->workspace : (float*)nullptr;
  const dim3 grid = pl.ks > 1 ? dim3(nwg, (unsigned)pl.ks) : dim3(nwg);
  if (pl.program == GEMM_MID)
    hipLaunchKernelGGL(lkgd_gemm_mid_kernel, grid, dim3(MID_NT), MID_LDS, stream, *d, tiles_m, tiles_n, pl.ks, pl.per, ws);
  else
    hipLaunchKernelGGL(lkgd_gemm_kernel, grid, dim3(256), GEMM_LDS, stream, *d, tiles_m, tiles_n, pl.ks, pl.per, ws);
  if (pl.ks > 1) return splitk_reduce_launch(d, stream, pl.ks);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

static int tile256_launch(const lkgd_gemm_desc* d, hipStream_t stream) {
  const int tiles_m = (d->M + BM2 - 1) / BM2, tiles_n = (d->N + BN - 1) / BN;
  hipLaunchKernelGGL(lkgd_gemm_kernel_256, dim3((unsigned)(tiles_m * tiles_n)), dim3(NT2), GEMM2_LDS, stream, *d, tiles_m, tiles_n);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_gemm_f16(const lkgd_gemm_desc* d, lkgd_stream_t stream) {
  int rc = check_desc(d);
  if (rc != LKGD_OK) return rc;
  LKGD_DEVICE_ONCE_BEGIN
    if (!lkgd_dynamic_lds(GEMM_LDS, lkgd_gemm_kernel) || !lkgd_dynamic_lds(GEMM2_LDS, lkgd_gemm_kernel_256) ||
        !lkgd_dynamic_lds(MID_LDS, lkgd_gemm_mid_kernel))
      return LKGD_E_LAUNCH;
  LKGD_DEVICE_ONCE_END
  int cus = 0;
  if ((rc = gemm_device_cus(&cus)) != LKGD_OK) return rc;
  gemm_plan pl;
  if ((rc = gemm_make_plan(d, cus, &pl)) != LKGD_OK) return rc;
  if (d->colstats && pl.cs_blk == 0) return LKGD_E_SHAPE;   // the chosen program produces no column sums
  switch (pl.program) {
    case GEMM_RESW: return gemm_resw_launch(d, stream, cus, pl);
    case GEMM_ROWPANEL: return gemm_rowpanel_launch(d, stream, cus, pl);
    case GEMM_WIDE:
      rc = gemm_wide_launch(d, stream, cus, pl);
      return (rc != LKGD_OK || pl.ks == 1) ? rc : splitk_reduce_launch(d, (hipStream_t)stream, pl.ks);
    case GEMM_STREAM: return gemm_stream_launch(d, stream, cus, pl);
    case GEMM_TILE256: return tile256_launch(d, (hipStream_t)stream);
    case GEMM_TILE128:
    case GEMM_MID: return tile128_launch(d, (hipStream_t)stream, pl);
  }
  return LKGD_E_MODE;   // (no such program)
}
