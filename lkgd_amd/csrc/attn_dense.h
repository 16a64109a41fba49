// The kernel of the dense short-sequence attention, shared by its two entry points: lkgd_attn_dense (attn_dense.hip,
// include/lkgd_hip.h section 16) and lkgd_attn_dense_relbias (t5.hip, include/lkgd_hip_t5.h), which adds relbias[h, j - i + S - 1]
// to the scaled score of query i and key j before the softmax.  RELBIAS is a compile-time switch: the instantiation without it is
// the kernel as it was, statement for statement.
//
// A workgroup = one (image, head) and AD_QPB query rows; the head's K and V rows sit in LDS (row pitch head_dim + 2 halfs: an
// odd number of dwords, so the lanes of a wave - one key each - read their K rows without bank conflicts).  A wave takes one
// query at a time: scores with one key per lane (v_dot2_f32_f16 over the head channels), wave-wide max / sum, the
// unnormalised probabilities parked in LDS, then O = P . V with one channel PAIR per lane.  With RELBIAS the head's 2S - 1 table
// entries sit in LDS behind the query rows; lane `key` of query `qr` reads entry key - qr + S - 1 (consecutive lanes, consecutive
// dwords).
#pragma once
#include "common.h"

#define AD_NT 256
#define AD_WAVES 4
#define AD_QPB 16             // query rows per workgroup
#define AD_MAXD 128
#define AD_LDS_MAX (160 * 1024)

template <bool RELBIAS>
__global__ __launch_bounds__(AD_NT) void attn_dense_kernel(const half_t* __restrict__ q, int ldq, const half_t* __restrict__ k, int ldk,
                                                           const half_t* __restrict__ v, int ldv, half_t* __restrict__ out, int ldo,
                                                           int S, int heads, int D, float scale, const float* __restrict__ relbias) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int bh = blockIdx.x, n = bh / heads, h = bh - n * heads;
  const int D2 = D >> 1, P2 = D2 + 1;                   // dwords per row / LDS pitch in dwords
  half2_t* sk = (half2_t*)smem;                         // [S][P2]
  half2_t* sv = sk + (long long)S * P2;                 // [S][P2]
  float* sp = (float*)(sv + (long long)S * P2) + w * S; // [waves][S] probabilities of the wave's query
  half2_t* sq = (half2_t*)((float*)(sv + (long long)S * P2) + AD_WAVES * S) + w * (AD_MAXD / 2);   // [waves][64] its query row
  [[maybe_unused]] float* sb = (float*)(sv + (long long)S * P2) + AD_WAVES * S + AD_WAVES * (AD_MAXD / 2);   // [2S - 1] the head's table (RELBIAS)
  const half_t* kb = k + (long long)n * S * ldk + h * D;
  const half_t* vb = v + (long long)n * S * ldv + h * D;
  const int c8 = D >> 3;                                // 16-byte chunks per row
  for (int c = t; c < S * c8; c += AD_NT) {
    const int r = c / c8, cc = c - r * c8;
    const half8_t kx = *(const half8_t*)(kb + (long long)r * ldk + cc * 8);
    const half8_t vx = *(const half8_t*)(vb + (long long)r * ldv + cc * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sk[r * P2 + cc * 4 + e] = (half2_t){kx[2 * e], kx[2 * e + 1]};
      sv[r * P2 + cc * 4 + e] = (half2_t){vx[2 * e], vx[2 * e + 1]};
    }
  }
  if constexpr (RELBIAS) {
    const float* rb = relbias + (long long)h * (2 * S - 1);
    for (int c = t; c < 2 * S - 1; c += AD_NT) sb[c] = rb[c];
  }
  __syncthreads();
  const int q0 = blockIdx.y * AD_QPB;
  for (int qi = w; qi < AD_QPB; qi += AD_WAVES) {
    const int qr = q0 + qi;
    if (qr >= S) break;                                  // wave-uniform
    const half_t* qp = q + ((long long)n * S + qr) * ldq + h * D;
    if (lane < D2) sq[lane] = *(const half2_t*)(qp + 2 * lane);
    __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0): the wave's own LDS writes are visible to its reads below
    // ---- scores: key = lane, lane + 64, ...
    float mx = -INFINITY;
    for (int key = lane; key < S; key += 64) {
      const half2_t* kr = sk + key * P2;
      float s = 0.f;
      for (int c = 0; c < D2; ++c) s = __builtin_amdgcn_fdot2(kr[c], sq[c], s, false);
      s *= scale;
      if constexpr (RELBIAS) s += sb[key - qr + S - 1];
      sp[key] = s;
      mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float l = 0.f;
    for (int key = lane; key < S; key += 64) {
      const float p = __expf(sp[key] - mx);
      sp[key] = p;
      l += p;
    }
    l = wave_sum(l);
    __builtin_amdgcn_s_waitcnt(0xc07f);
    // ---- O = P . V: lane = channel pair
    if (lane < D2) {
      float a0 = 0.f, a1 = 0.f;
      for (int key = 0; key < S; ++key) {
        const half2_t vv = sv[key * P2 + lane];
        const float p = sp[key];
        a0 = fmaf(p, (float)vv.x, a0);
        a1 = fmaf(p, (float)vv.y, a1);
      }
      const float inv = 1.0f / l;
      *(half2_t*)(out + ((long long)n * S + qr) * ldo + h * D + 2 * lane) = (half2_t){(half_t)(a0 * inv), (half_t)(a1 * inv)};
    }
  }
}

// K and V of one head, the waves' probability and query rows; with the table, its 2S - 1 entries behind them
static inline size_t attn_dense_lds(int S, int D, bool relbias) {
  return (size_t)2 * S * (D / 2 + 1) * 4 + (size_t)AD_WAVES * S * 4 + (size_t)AD_WAVES * (AD_MAXD / 2) * 4 +
         (relbias ? ((size_t)2 * S - 1) * 4 : 0);
}

// the checks and the launch of both entry points; relbias NULL = the plain kernel
template <bool RELBIAS>
static int attn_dense_launch(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* out, int32_t ldo,
                             int32_t nbatch, int32_t S, int32_t heads, int32_t head_dim, const float* relbias, float scale,
                             lkgd_stream_t stream) {
  if (!q || !k || !v || !out || (RELBIAS && !relbias)) return LKGD_E_NULL;
  if (nbatch <= 0 || S <= 0 || heads <= 0 || head_dim <= 0 || head_dim > AD_MAXD || head_dim % 8) return LKGD_E_SHAPE;
  const size_t lds = attn_dense_lds(S, head_dim, RELBIAS);
  if (lds > AD_LDS_MAX) return LKGD_E_SHAPE;             // K and V of one head must fit the CU's LDS
  const int width = heads * head_dim;
  if (ldq < width || ldk < width || ldv < width || ldo < width) return LKGD_E_SHAPE;
  if (ldq % 8 || ldk % 8 || ldv % 8 || ldo % 2 || !aligned16(q) || !aligned16(k) || !aligned16(v) || ((uintptr_t)out & 3) ||
      ((uintptr_t)relbias & 3))
    return LKGD_E_ALIGN;
  LKGD_DEVICE_ONCE_BEGIN
    if (!lkgd_dynamic_lds(AD_LDS_MAX, attn_dense_kernel<RELBIAS>)) return LKGD_E_LAUNCH;
  LKGD_DEVICE_ONCE_END
  const long long nbh = (long long)nbatch * heads;
  if (nbh > 0x7fffffffLL) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(attn_dense_kernel<RELBIAS>, dim3((unsigned)nbh, (unsigned)((S + AD_QPB - 1) / AD_QPB)), dim3(AD_NT), lds,
                     (hipStream_t)stream, (const half_t*)q, ldq, (const half_t*)k, ldk, (const half_t*)v, ldv, (half_t*)out, ldo, S,
                     heads, head_dim, scale, relbias);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
