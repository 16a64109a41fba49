// lkgd_gemm_fp8 (include/lkgd_hip_fp8.h): out[m, n] = fp16((sum_k a[m, k] w[n, k]) a_scale[m] w_scale[n] + bias[n]) with e4m3fn
// operands, both K-contiguous, on the block-scaled matrix instruction v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 0: e4m3
// on both sides; every block scale the E8M0 byte 0x7f = 2^0).  Plain HIP, no inline assembly.
//
// Structure: a 128 x 128 output tile per 256-thread workgroup, K-steps of 128 bytes, both operands staged by 16-byte LDS-DMA
// into two LDS buffers (2 x 32 KB, ONE __shared__ array), 2 x 2 waves with 4 x 4 accumulators of 16 x 16 each.  One barrier per
// K-step: the DMA of step t + 1 is issued right after the barrier that retires step t and runs under step t's MFMAs; the buffer
// it overwrites was last read in step t - 1, which every wave has left once it is past that barrier.
//
// LDS image of an operand tile: [128 rows][8 chunks of 16 bytes], the chunk index XOR-ed with (row & 7).  An LDS-DMA writes
// wave-base + lane * 16, so the image is filled linearly and the swizzle sits on the per-lane SOURCE address; the fragment reads
// apply the same XOR.  Without it the 16 rows of a fragment read (128 B apart) meet on two 16-byte slots of the bank row.
//
// Operand roles: the WEIGHT tile is the instruction's A operand and the ACTIVATION tile its B operand, so an accumulator holds
// out^T: lane l has output row m = l & 15 and the four consecutive columns n = 4 (l >> 4) + j - one 8-byte store per 16 x 16
// tile.  A and B fragments use the same lane map (row l & 15, k bytes [32 (l >> 4), + 32)), so any k order is harmless as long
// as both sides share it; tests/test_fp8_gpu.py pins the whole map with one-hot rows against an asymmetric integer weight.
//
// M tail: rows past M - 1 are CLAMPED to M - 1 on load (a and a_scale are never read beyond their last row) and masked on store.
#include "common.h"
#include "../../include/lkgd_hip_fp8.h"

typedef int int8v_t __attribute__((ext_vector_type(8)));
typedef int int4v_t __attribute__((ext_vector_type(4)));

#define F8_BM 128
#define F8_BN 128
#define F8_BK 128                               // bytes = e4m3 elements per K-step
#define F8_TILE_BYTES (128 * F8_BK)             // one operand tile
#define F8_STAGE_BYTES (2 * F8_TILE_BYTES)      // activation tile, then weight tile
#define F8_UNIT_SCALE 0x7f7f7f7f                // E8M0 127 = 2^0 in every byte

__device__ __forceinline__ int8v_t f8_frag(const char* tile, int row, int g0) {
  const int sw = row & 7;
  const int4v_t lo = *(const int4v_t*)(tile + row * F8_BK + (((g0) ^ sw) << 4));
  const int4v_t hi = *(const int4v_t*)(tile + row * F8_BK + (((g0 + 1) ^ sw) << 4));
  return int8v_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

__global__ __launch_bounds__(256) void gemm_fp8_kernel(const uint8_t* __restrict__ a, int lda, const float* __restrict__ a_scale,
                                                       const uint8_t* __restrict__ w, int ldw, const float* __restrict__ w_scale,
                                                       const float* __restrict__ bias, half_t* __restrict__ out, int ldc, int M,
                                                       int K) {
  __shared__ __attribute__((aligned(16))) char smem[2 * F8_STAGE_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int brow = blockIdx.y * F8_BM, bcol = blockIdx.x * F8_BN;
  const int wr = wv >> 1, wc = wv & 1;          // the wave's 64 x 64 quadrant: rows wr, columns wc

  // staging: chunk c = i * 256 + tid of a tile is row c >> 3, LDS slot c & 7, and holds the row's 16-byte chunk slot ^ (row & 7)
  const uint8_t* asrc[4];
  const uint8_t* wsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = i * 256 + tid, r = c >> 3, g = (c & 7) ^ (r & 7);
    int ar = brow + r;
    ar = ar < M ? ar : M - 1;
    asrc[i] = a + (long long)ar * lda + g * 16;
    wsrc[i] = w + (long long)(bcol + r) * ldw + g * 16;
  }
  auto stage = [&](int buf, int k0) {
    char* sa = smem + buf * F8_STAGE_BYTES + wv * 1024;
    char* sw = sa + F8_TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(asrc[i] + k0, sa + i * 4096);
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(wsrc[i] + k0, sw + i * 4096);
  };

  float4_t acc[4][4];       // [activation 16-row tile][weight 16-column tile]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, g0 = (lane >> 4) * 2;
  const int nk = K / F8_BK;
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) stage(buf ^ 1, (kt + 1) * F8_BK);
    const char* ta = smem + buf * F8_STAGE_BYTES;
    const char* tw = ta + F8_TILE_BYTES;
    int8v_t fa[4], fw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = f8_frag(ta, wr * 64 + i * 16 + fr, g0);
#pragma unroll
    for (int j = 0; j < 4; ++j) fw[j] = f8_frag(tw, wc * 64 + j * 16 + fr, g0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[j], fa[i], acc[i][j], 0, 0, 0, F8_UNIT_SCALE, 0,
                                                                     F8_UNIT_SCALE);
  }

  // epilogue: acc[i][j][e] = sum for output row brow + wr 64 + i 16 + (lane & 15), column bcol + wc 64 + j 16 + 4 (lane >> 4) + e
  const int cq = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = brow + wr * 64 + i * 16 + fr;
    if (m >= M) continue;
    const float as = a_scale[m];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = bcol + wc * 64 + j * 16 + cq;
      const float4_t ws = *(const float4_t*)(w_scale + n);
      float4_t bs = {0.f, 0.f, 0.f, 0.f};
      if (bias) bs = *(const float4_t*)(bias + n);
      half4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (half_t)__builtin_fmaf(acc[i][j][e] * as, ws[e], bs[e]);
      *(half4_t*)(out + (long long)m * ldc + n) = o;
    }
  }
}

extern "C" int lkgd_gemm_fp8(const void* a, int32_t lda, const float* a_scale, const void* w, int32_t ldw, const float* w_scale,
                             const float* bias, void* out, int32_t ldc, int32_t M, int32_t N, int32_t K, lkgd_stream_t stream) {
  if (!a || !a_scale || !w || !w_scale || !out) return LKGD_E_NULL;
  if (M <= 0 || N <= 0 || K <= 0 || N % F8_BN || K % F8_BK || lda < K || ldw < K || ldc < N) return LKGD_E_SHAPE;
  if (lda % 16 || ldw % 16 || ldc % 8 || !aligned16(a) || !aligned16(w) || !aligned16(out) || !aligned16(w_scale) ||
      (bias && !aligned16(bias)))
    return LKGD_E_ALIGN;
  const long long mt = ((long long)M + F8_BM - 1) / F8_BM;
  if (mt > 65535) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(gemm_fp8_kernel, dim3((unsigned)(N / F8_BN), (unsigned)mt), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)a, lda, a_scale, (const uint8_t*)w, ldw, w_scale, bias, (half_t*)out, ldc, M, K);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
