// The dynamic per-row e4m3 quantisers of the DiT's FP8 block linears (include/lkgd_hip_fp8.h): lkgd_quant_rows_fp8,
// lkgd_gelu_tanh_quant_fp8, lkgd_layernorm_quant_fp8.  One device function (fp8_common.h) holds the statement Q; the two fused
// forms first produce the fp16 values their un-fused kernel would have stored, with that kernel's own arithmetic, then apply Q:
// the fusion saves a round trip through memory, not a rounding point.
#include "common.h"
#include "fp8_common.h"
#include "../../include/lkgd_hip_fp8.h"

typedef uint32_t uint2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float amax8(half8_t h, float m) {
#pragma unroll
  for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)h[e]));
  return m;
}

__device__ __forceinline__ uint2_t quant8(half8_t h, float inv) {
  uint2_t o = {0u, 0u};
#pragma unroll
  for (int e = 0; e < 4; ++e) o.x |= lkgd_q_elem((float)h[e], inv) << (8 * e);
#pragma unroll
  for (int e = 0; e < 4; ++e) o.y |= lkgd_q_elem((float)h[4 + e], inv) << (8 * e);
  return o;
}

// ------------------------------------------------------------------------------------ rows of any width up to 12 288
// One 256-thread workgroup per row, the row in registers as NV x 8 halfs per thread (12 288 halfs = 6 vectors); the maximum is
// reduced by wave shuffles and one LDS exchange (two slots used in turn, so one barrier per row is enough).
#define QR_MAXV 6
template <int NV, bool GELU>
__global__ __launch_bounds__(256) void quant_rows_kernel(const half_t* __restrict__ x, int ldx, uint8_t* __restrict__ q, int ldq,
                                                         float* __restrict__ scale, long long T, int K8) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int it = 0;
  for (long long row = blockIdx.x; row < T; row += gridDim.x, it ^= 1) {
    half8_t h[NV];
    float m = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int cv = tid + 256 * v;
      if (cv < K8) {
        h[v] = *(const half8_t*)(x + row * ldx + cv * 8);
        if (GELU) {           // gelu_tanh_kernel's arithmetic (elementwise.hip), rounded to fp16 as that kernel stores it
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float f = (float)h[v][e];
            const float u = 0.7978845608028654f * (f + 0.044715f * f * f * f);
            const float t = 1.0f - 2.0f / (__builtin_amdgcn_exp2f(u * 2.885390081777927f) + 1.0f);
            h[v][e] = (half_t)(0.5f * f * (1.0f + t));
          }
        }
        m = amax8(h[v], m);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[it][wave] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[it][0], red[it][1]), fmaxf(red[it][2], red[it][3]));
    float inv, sc;
    lkgd_q_scales(m, &inv, &sc);
    if (tid == 0) scale[row] = sc;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int cv = tid + 256 * v;
      if (cv < K8) *(uint2_t*)(q + row * ldq + cv * 8) = quant8(h[v], inv);
    }
  }
}

template <bool GELU>
static int quant_rows_launch(const void* x, int32_t ldx, void* q, int32_t ldq, float* scale, int64_t T, int32_t K,
                             lkgd_stream_t stream) {
  if (!x || !q || !scale) return LKGD_E_NULL;
  if (T <= 0 || K <= 0 || K % 8 || K > 256 * 8 * QR_MAXV || ldx < K || ldq < K) return LKGD_E_SHAPE;
  if (ldx % 8 || ldq % 16 || !aligned16(x) || !aligned16(q)) return LKGD_E_ALIGN;
  const int K8 = K / 8;
  const long long blocks = T < 256 * 32 ? T : 256 * 32;
#define QR_GO(V)                                                                                                         \
  hipLaunchKernelGGL((quant_rows_kernel<V, GELU>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, \
                     ldx, (uint8_t*)q, ldq, scale, (long long)T, K8)
  if (K8 <= 256) QR_GO(1);
  else if (K8 <= 512) QR_GO(2);
  else if (K8 <= 1024) QR_GO(4);
  else QR_GO(6);
#undef QR_GO
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_quant_rows_fp8(const void* x, int32_t ldx, void* q, int32_t ldq, float* scale, int64_t T, int32_t K,
                                   lkgd_stream_t stream) {
  return quant_rows_launch<false>(x, ldx, q, ldq, scale, T, K, stream);
}

extern "C" int lkgd_gelu_tanh_quant_fp8(const void* x, int32_t ldx, void* q, int32_t ldq, float* scale, int64_t T, int32_t K,
                                        lkgd_stream_t stream) {
  return quant_rows_launch<true>(x, ldx, q, ldq, scale, T, K, stream);
}

// ------------------------------------------------------------------------------------------------- LayerNorm + Q
// layernorm_kernel of norm.hip without the row bias, statement for statement: the same L lanes per row and NV vectors per lane
// for a given C (lkgd_layernorm's dispatch, repeated below), the same element and shuffle order of both sums, the same
// expressions - so the fp16 values that enter Q have the bits lkgd_layernorm stores (tests/test_fp8_gpu.py compares the two
// bit for bit at every dispatch width).  A row lives in one wave, so its maximum is one more shuffle reduction over the group.
template <int L, bool AFF, int NV>
__global__ __launch_bounds__(256) void layernorm_quant_kernel(const half_t* x, int ldx, long long T, int C, const float* gamma,
                                                              const float* beta, float eps, uint8_t* q, int ldq, float* scale) {
  constexpr int RPW = 64 / L;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int sub = lane / L, li = lane % L;
  const int C8 = C >> 3;
  float g[AFF ? NV : 1][8], b[AFF ? NV : 1][8];
  if (AFF) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int cv = li + L * v;
      if (cv >= C8) cv = C8 - 1;        // clamped lanes never store
      const float4_t g0 = *(const float4_t*)(gamma + cv * 8), g1 = *(const float4_t*)(gamma + cv * 8 + 4);
      const float4_t b0 = *(const float4_t*)(beta + cv * 8), b1 = *(const float4_t*)(beta + cv * 8 + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        g[AFF ? v : 0][e] = e < 4 ? g0[e & 3] : g1[e & 3];
        b[AFF ? v : 0][e] = e < 4 ? b0[e & 3] : b1[e & 3];
      }
    }
  }
  const float invC = 1.0f / (float)C;
  const long long rows_per_block = 4 * RPW;
  for (long long row0 = (long long)blockIdx.x * rows_per_block + wave * RPW; row0 < T;
       row0 += (long long)gridDim.x * rows_per_block) {
    const long long row = row0 + sub;
    const bool live = row < T;
    float xv[NV][8];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int cv = li + L * v;
      if (live && cv < C8) {
        half8_t h = *(const half8_t*)(x + row * ldx + cv * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) { xv[v][e] = (float)h[e]; s += xv[v][e]; }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) xv[v][e] = 0.f;
      }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s * invC;
    float qs = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int cv = li + L * v;
      if (cv < C8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { float d = xv[v][e] - mean; qs += d * d; }
      }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) qs += __shfl_xor(qs, o, 64);
    const float rstd = rsqrtf(qs * invC + eps);
    half8_t y8[NV];
    float m = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int cv = li + L * v;
      if (live && cv < C8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float y = (xv[v][e] - mean) * rstd;
          if (AFF) y = y * g[AFF ? v : 0][e] + b[AFF ? v : 0][e];
          y8[v][e] = (half_t)y;
        }
        m = amax8(y8[v], m);
      }
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float inv, sc;
    lkgd_q_scales(m, &inv, &sc);
    if (live && li == 0) scale[row] = sc;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      int cv = li + L * v;
      if (live && cv < C8) *(uint2_t*)(q + row * ldq + cv * 8) = quant8(y8[v], inv);
    }
  }
}

// the (L, NV) of lkgd_layernorm for C channels (norm.hip: LN_MAXV 3, LN_MAXV_WIDE 4, LN_MAXV_XWIDE 6)
extern "C" int lkgd_layernorm_quant_fp8(const void* x, int32_t ldx, int64_t T, int32_t C, const float* gamma, const float* beta,
                                        float eps, void* q, int32_t ldq, float* scale, lkgd_stream_t stream) {
  if (!x || !q || !scale) return LKGD_E_NULL;
  if ((gamma == nullptr) != (beta == nullptr)) return LKGD_E_NULL;
  if (T <= 0 || C <= 0 || C % 8 || C > 64 * 8 * 6 || ldx < C || ldq < C) return LKGD_E_SHAPE;
  if (ldx % 8 || ldq % 16 || !aligned16(x) || !aligned16(q) || (gamma && (!aligned16(gamma) || !aligned16(beta))))
    return LKGD_E_ALIGN;
  const int C8 = C / 8;
  int L = 4;
  while (L < 64 && L * 3 < C8) L *= 2;
  const long long rows_per_block = 4 * (64 / L);
  long long blocks = (T + rows_per_block - 1) / rows_per_block;
  if (blocks > 256 * 16) blocks = 256 * 16;
#define LNQ_GO(LL, NVV)                                                                                                       \
  do {                                                                                                                        \
    if (gamma)                                                                                                                \
      hipLaunchKernelGGL((layernorm_quant_kernel<LL, true, NVV>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,  \
                         (const half_t*)x, ldx, (long long)T, C, gamma, beta, eps, (uint8_t*)q, ldq, scale);                  \
    else                                                                                                                      \
      hipLaunchKernelGGL((layernorm_quant_kernel<LL, false, NVV>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, \
                         (const half_t*)x, ldx, (long long)T, C, gamma, beta, eps, (uint8_t*)q, ldq, scale);                  \
  } while (0)
  if (C8 > 64 * 4) LNQ_GO(64, 6);
  else if (C8 > 64 * 3) LNQ_GO(64, 4);
  else if (L == 4) LNQ_GO(4, 3);
  else if (L == 8) LNQ_GO(8, 3);
  else if (L == 16) LNQ_GO(16, 3);
  else if (L == 32) LNQ_GO(32, 3);
  else LNQ_GO(64, 3);
#undef LNQ_GO
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
