// The latent-modulated norm of the CogVideoX 3-D causal VAE decoder (include/lkgd_hip_cogvae.h): GroupNorm apply, the gather of the
// conv_y | conv_b rows from the latent grid, the modulation and SiLU in one memory-bound pass.
#include "common.h"

#include "../../include/lkgd_hip_cogvae.h"

// One thread = 8 channels (16 bytes) of one row; consecutive threads walk a row's channels, then the next row, so a wave reads and
// writes whole rows (C = 128: four rows of 256 bytes per wave instruction, every lane busy).  The yb rows of a wave are at most
// 64 / (C/8) latent pixels: they come from L2 (the latent grid's [.., 2C] matrix is a few MB).
__global__ __launch_bounds__(256) void spatial_norm3d_kernel(const half_t* __restrict__ f, int ldf, const float* __restrict__ stats,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             const half_t* __restrict__ yb, int ldyb, const int* __restrict__ tmap,
                                                             half_t* __restrict__ out, int ldo, long long out_batch_rows, unsigned rows,
                                                             int T, int H, int W, int C, int Tz, int sh, int act) {
  const unsigned C8 = (unsigned)C >> 3;
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  const unsigned row = (unsigned)(i / C8);
  if (row >= rows) return;
  const unsigned c = ((unsigned)(i - (unsigned long long)row * C8)) << 3;
  const unsigned HW = (unsigned)(H * W), THW = (unsigned)T * HW;
  const unsigned b = row / THW, r = row - b * THW;
  const unsigned t = r / HW, px = r - t * HW;
  const unsigned Y = px / (unsigned)W, X = px - Y * (unsigned)W;
  int tz = tmap[t];
  tz = tz < 0 ? 0 : (tz >= Tz ? Tz - 1 : tz);
  const unsigned h = (unsigned)H >> sh, w = (unsigned)W >> sh;
  const unsigned long long src = ((unsigned long long)(b * (unsigned)Tz + (unsigned)tz) * h + (Y >> sh)) * w + (X >> sh);
  const half8_t v = *(const half8_t*)(f + (unsigned long long)row * ldf + c);
  const half8_t ys = *(const half8_t*)(yb + src * ldyb + c);
  const half8_t bs = *(const half8_t*)(yb + src * ldyb + C + c);
  const float4_t g0 = *(const float4_t*)(gamma + c), g1 = *(const float4_t*)(gamma + c + 4);
  const float4_t b0 = *(const float4_t*)(beta + c), b1 = *(const float4_t*)(beta + c + 4);
  const unsigned gs = (unsigned)C >> 5;          // channels per group: 2, 4, 6 ... (C % 64 == 0)
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned g = (c + e) / gs;
    const float mean = stats[(b * 32u + g) * 2], rstd = stats[(b * 32u + g) * 2 + 1];
    const float ga = e < 4 ? g0[e & 3] : g1[e & 3], be = e < 4 ? b0[e & 3] : b1[e & 3];
    const float A = rstd * ga;
    const float n = (float)v[e] * A + (be - mean * A);          // the arithmetic of lkgd_groupnorm_apply
    float x = n * (float)ys[e] + (float)bs[e];
    if (act) x = silu_f(x);
    o[e] = (half_t)x;
  }
  *(half8_t*)(out + ((unsigned long long)b * (unsigned long long)out_batch_rows + r) * ldo + c) = o;
}

extern "C" int lkgd_spatial_norm3d(const void* f, int32_t ldf, const float* stats, const float* gamma, const float* beta,
                                   const void* yb, int32_t ldyb, const int32_t* tmap, void* out, int32_t ldo, int64_t out_batch_rows,
                                   int32_t B, int32_t T, int32_t H, int32_t W, int32_t C, int32_t Tz, int32_t sh, int32_t act,
                                   lkgd_stream_t stream) {
  if (!f || !stats || !gamma || !beta || !yb || !tmap || !out) return LKGD_E_NULL;
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || Tz <= 0 || C <= 0 || C % 64) return LKGD_E_SHAPE;
  if (sh < 0 || sh > 3 || H % (1 << sh) || W % (1 << sh) || (act != 0 && act != 1)) return LKGD_E_SHAPE;
  if (ldf < C || ldo < C || ldyb < 2 * C) return LKGD_E_SHAPE;
  const long long thw = (long long)T * H * W;
  if (out_batch_rows < thw || (long long)B * thw >= (1LL << 31) || (long long)B * out_batch_rows >= (1LL << 31)) return LKGD_E_SHAPE;
  if (!aligned16(f) || !aligned16(yb) || !aligned16(out) || ldf % 8 || ldyb % 8 || ldo % 8) return LKGD_E_ALIGN;
  if (!aligned16(gamma) || !aligned16(beta) || ((uintptr_t)stats & 7u) || ((uintptr_t)tmap & 3u)) return LKGD_E_ALIGN;
  const long long total = (long long)B * thw * (C / 8);
  hipLaunchKernelGGL(spatial_norm3d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)f, ldf, stats, gamma, beta, (const half_t*)yb, ldyb, tmap, (half_t*)out, ldo,
                     (long long)out_batch_rows, (unsigned)((long long)B * thw), T, H, W, C, Tz, sh, act);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
