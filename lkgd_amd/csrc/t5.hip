// The operators of the T5 text encoder in front of the CogVideoX loop (include/lkgd_hip_t5.h; lkgd_amd/t5.py): embedding lookup into
// an fp32 residual stream, T5LayerNorm (RMS norm, fp32 rows -> fp16), dense attention with a relative-position bias (the kernel of
// attn_dense.h with its table switch on), gated tanh-GELU, and the fp32 residual add.  The encoder runs once per clip; the four
// element-wise kernels are memory-bound passes with 16-byte accesses per lane, one 8-channel piece per thread.
#include "attn_dense.h"
#include "../../include/lkgd_hip_t5.h"

#define T5_NT 256
#define T5_MAXC 4096
#define T5_PIECES (T5_MAXC / 8 / T5_NT)      // 8-channel pieces of a row one thread of the norm holds in registers

static inline bool t5_grid(long long pieces, unsigned* nblk) {
  const long long n = (pieces + T5_NT - 1) / T5_NT;
  if (n > 0x7fffffffLL) return false;
  *nblk = (unsigned)n;
  return true;
}

// ---- lkgd_t5_embed_rows -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(T5_NT) void t5_embed_rows_kernel(const long long* __restrict__ ids, const half_t* __restrict__ table, int ldt,
                                                              int V, int D8, float* __restrict__ out, int ldo, long long T) {
  const long long i = (long long)blockIdx.x * T5_NT + threadIdx.x;
  if (i >= T * D8) return;
  const long long r = i / D8;
  const int c = (int)(i - r * D8) * 8;
  long long id = ids[r];
  id = id < 0 ? 0 : (id >= V ? V - 1 : id);            // the host has validated the ids: the clamp keeps ANY launch inside the table
  const half8_t x = *(const half8_t*)(table + id * ldt + c);
  float* o = out + r * ldo + c;
  *(float4_t*)o = (float4_t){(float)x[0], (float)x[1], (float)x[2], (float)x[3]};
  *(float4_t*)(o + 4) = (float4_t){(float)x[4], (float)x[5], (float)x[6], (float)x[7]};
}

extern "C" int lkgd_t5_embed_rows(const int64_t* ids, const void* table, int32_t ldt, int32_t V, int32_t D, float* out, int32_t ldo,
                                  int64_t T, lkgd_stream_t stream) {
  if (!ids || !table || !out) return LKGD_E_NULL;
  if (T <= 0 || V <= 0 || D <= 0 || D % 8 || ldt < D || ldo < D) return LKGD_E_SHAPE;
  if (!aligned16(table) || !aligned16(out) || ((uintptr_t)ids & 7) || ldt % 8 || ldo % 4) return LKGD_E_ALIGN;
  unsigned nblk;
  if (T > 0x7fffffffLL || !t5_grid((long long)T * (D / 8), &nblk)) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(t5_embed_rows_kernel, dim3(nblk), dim3(T5_NT), 0, (hipStream_t)stream, (const long long*)ids, (const half_t*)table,
                     ldt, V, D / 8, out, ldo, (long long)T);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// ---- lkgd_t5_rmsnorm ----------------------------------------------------------------------------------------------------------
// One workgroup per row.  A thread keeps its (up to T5_PIECES) 8-channel pieces in registers between the two passes, so a row is
// read once.  The sum of squares: per thread in channel order, wave_sum, then the four waves' sums added in wave order by everyone.
__global__ __launch_bounds__(T5_NT) void t5_rmsnorm_kernel(const float* __restrict__ x, int ldx, int C8, const float* __restrict__ weight,
                                                           float eps, half_t* __restrict__ out, int ldo) {
  __shared__ float wsum[T5_NT / 64];
  const int t = threadIdx.x;
  const float* xr = x + (long long)blockIdx.x * ldx;
  float4_t v[T5_PIECES][2];
  float ss = 0.f;
#pragma unroll
  for (int p = 0; p < T5_PIECES; ++p) {
    const int c = t + p * T5_NT;
    if (c < C8) {
      v[p][0] = *(const float4_t*)(xr + c * 8);
      v[p][1] = *(const float4_t*)(xr + c * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = fmaf(v[p][0][e], v[p][0][e], ss);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = fmaf(v[p][1][e], v[p][1][e], ss);
    }
  }
  ss = wave_sum(ss);
  if ((t & 63) == 0) wsum[t >> 6] = ss;
  __syncthreads();
  const float total = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  const float r = rsqrtf(total / (float)(C8 * 8) + eps);
  half_t* orow = out + (long long)blockIdx.x * ldo;
#pragma unroll
  for (int p = 0; p < T5_PIECES; ++p) {
    const int c = t + p * T5_NT;
    if (c < C8) {
      const float4_t w0 = *(const float4_t*)(weight + c * 8), w1 = *(const float4_t*)(weight + c * 8 + 4);
      half8_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (half_t)(w0[e] * (v[p][0][e] * r));
        o[4 + e] = (half_t)(w1[e] * (v[p][1][e] * r));
      }
      *(half8_t*)(orow + c * 8) = o;
    }
  }
}

extern "C" int lkgd_t5_rmsnorm(const float* x, int32_t ldx, int64_t T, int32_t C, const float* weight, float eps, void* out, int32_t ldo,
                               lkgd_stream_t stream) {
  if (!x || !weight || !out) return LKGD_E_NULL;
  if (T <= 0 || T > 0x7fffffffLL || C <= 0 || C % 8 || C > T5_MAXC || ldx < C || ldo < C) return LKGD_E_SHAPE;
  if (!aligned16(x) || !aligned16(weight) || !aligned16(out) || ldx % 4 || ldo % 8) return LKGD_E_ALIGN;
  hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((unsigned)T), dim3(T5_NT), 0, (hipStream_t)stream, x, ldx, C / 8, weight, eps, (half_t*)out,
                     ldo);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// ---- lkgd_attn_dense_relbias --------------------------------------------------------------------------------------------------
extern "C" int lkgd_attn_dense_relbias(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* out,
                                       int32_t ldo, int32_t nbatch, int32_t S, int32_t heads, int32_t head_dim, const float* relbias,
                                       float scale, lkgd_stream_t stream) {
  return attn_dense_launch<true>(q, ldq, k, ldk, v, ldv, out, ldo, nbatch, S, heads, head_dim, relbias, scale, stream);
}

// ---- lkgd_t5_gated_gelu -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(T5_NT) void t5_gated_gelu_kernel(const half_t* __restrict__ h, int ldh, int F8, half_t* __restrict__ out,
                                                              int ldo, long long T) {
  const long long i = (long long)blockIdx.x * T5_NT + threadIdx.x;
  if (i >= T * F8) return;
  const long long r = i / F8;
  const int c = (int)(i - r * F8) * 8;
  const half_t* hr = h + r * ldh + c;
  const half8_t a = *(const half8_t*)hr, b = *(const half8_t*)(hr + F8 * 8);
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float f = (float)a[e];
    const float u = 0.7978845608028654f * (f + 0.044715f * f * f * f);
    // tanh(u) = 1 - 2 / (exp(2u) + 1); exp2-based, saturates cleanly for |u| large (lkgd_gelu_tanh's form)
    const float th = 1.0f - 2.0f / (__builtin_amdgcn_exp2f(u * 2.885390081777927f) + 1.0f);
    o[e] = (half_t)((0.5f * f * (1.0f + th)) * (float)b[e]);
  }
  *(half8_t*)(out + r * ldo + c) = o;
}

extern "C" int lkgd_t5_gated_gelu(const void* h, int32_t ldh, int64_t T, int32_t F, void* out, int32_t ldo, lkgd_stream_t stream) {
  if (!h || !out) return LKGD_E_NULL;
  if (T <= 0 || F <= 0 || F % 8 || F > 0x3fffffff || ldh < 2 * F || ldo < F) return LKGD_E_SHAPE;
  if (!aligned16(h) || !aligned16(out) || ldh % 8 || ldo % 8) return LKGD_E_ALIGN;
  unsigned nblk;
  if (T > 0x7fffffffLL || !t5_grid((long long)T * (F / 8), &nblk)) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(t5_gated_gelu_kernel, dim3(nblk), dim3(T5_NT), 0, (hipStream_t)stream, (const half_t*)h, ldh, F / 8, (half_t*)out,
                     ldo, (long long)T);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// ---- lkgd_t5_residual_add -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(T5_NT) void t5_residual_add_kernel(float* __restrict__ x, int ldx, const half_t* __restrict__ y, int ldy,
                                                                int C8, float s, long long T) {
  const long long i = (long long)blockIdx.x * T5_NT + threadIdx.x;
  if (i >= T * C8) return;
  const long long r = i / C8;
  const int c = (int)(i - r * C8) * 8;
  float* xr = x + r * ldx + c;
  const half8_t yv = *(const half8_t*)(y + r * ldy + c);
  float4_t a = *(const float4_t*)xr, b = *(const float4_t*)(xr + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] += s * (float)yv[e];
    b[e] += s * (float)yv[4 + e];
  }
  *(float4_t*)xr = a;
  *(float4_t*)(xr + 4) = b;
}

extern "C" int lkgd_t5_residual_add(float* x, int32_t ldx, const void* y, int32_t ldy, int64_t T, int32_t C, float s,
                                    lkgd_stream_t stream) {
  if (!x || !y) return LKGD_E_NULL;
  if (T <= 0 || C <= 0 || C % 8 || ldx < C || ldy < C) return LKGD_E_SHAPE;
  if (!aligned16(x) || !aligned16(y) || ldx % 4 || ldy % 8) return LKGD_E_ALIGN;
  unsigned nblk;
  if (T > 0x7fffffffLL || !t5_grid((long long)T * (C / 8), &nblk)) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(t5_residual_add_kernel, dim3(nblk), dim3(T5_NT), 0, (hipStream_t)stream, x, ldx, (const half_t*)y, ldy, C / 8, s,
                     (long long)T);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
