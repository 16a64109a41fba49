// The operators the encoder of the CogVideoX 3-D causal VAE adds (include/lkgd_hip_cogvae_enc.h): the tap rows of conv_in over the
// pixel channels, the temporal average pool of the downsamplers, and the posterior (mean, scaled sample) of conv_out's moment rows.
// All three are memory-bound passes.
#include "common.h"

#include "../../include/lkgd_hip_cogvae_enc.h"

#include <math.h>

// ---- lkgd_cogvae_pixel_taps ----------------------------------------------------------------------------------------------------------
// One thread = 8 columns (16 bytes) of one 128-column row; the 16 threads of a row are consecutive, so a wave writes four whole rows
// (1 KiB, contiguous when ldo == 128).  The clip has Cin <= 4 planes per frame: the 27*Cin gathers of a row and of its neighbours hit
// the same few cache lines, and the columns past 27*Cin cost no load at all.  CIN is a template argument: k -> (tap, c) is then a
// division by a constant.
template <int CIN>
__global__ __launch_bounds__(256) void pixel_taps_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, int ldo, unsigned rows,
                                                         int T, int H, int W, int t0, int Tc) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  const unsigned row = (unsigned)(i >> 4);
  if (row >= rows) return;
  const int k0 = ((int)(i & 15u)) << 3;
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)0.0f;
  if (k0 < 27 * CIN) {
    const unsigned HW = (unsigned)(H * W), THW = (unsigned)Tc * HW;
    const unsigned b = row / THW, r = row - b * THW;
    const unsigned tl = r / HW, px = r - tl * HW;
    const int y = (int)(px / (unsigned)W), xx = (int)(px - (unsigned)y * (unsigned)W);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = k0 + e;
      if (k < 27 * CIN) {
        const int tap = k / CIN, c = k - tap * CIN;
        const int kt = tap / 9, r9 = tap - kt * 9;
        const int ky = r9 / 3, kx = r9 - ky * 3;
        int ts = t0 + (int)tl + kt - 2;          // <= t0 + Tc - 1 <= T - 1 (the launcher checks t0 + Tc <= T)
        ts = ts < 0 ? 0 : ts;                    // the first frame replicated in front of the clip
        const int ys = y + ky - 1, xs = xx + kx - 1;
        if (ys >= 0 && ys < H && xs >= 0 && xs < W)
          o[e] = x[(((unsigned long long)(b * (unsigned)CIN + (unsigned)c) * (unsigned)T + (unsigned)ts) * (unsigned)H + (unsigned)ys) *
                       (unsigned)W + (unsigned)xs];
      }
    }
  }
  *(half8_t*)(out + (unsigned long long)row * ldo + k0) = o;
}

extern "C" int lkgd_cogvae_pixel_taps(const void* x, void* out, int32_t ldo, int32_t B, int32_t Cin, int32_t T, int32_t H, int32_t W,
                                      int32_t t0, int32_t Tc, lkgd_stream_t stream) {
  if (!x || !out) return LKGD_E_NULL;
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || Tc <= 0 || Cin < 1 || Cin > 4) return LKGD_E_SHAPE;
  if (t0 < 0 || (long long)t0 + Tc > T || ldo < 128) return LKGD_E_SHAPE;
  const long long rows = (long long)B * Tc * H * W;
  if (rows >= (1LL << 31) || (long long)H * W >= (1LL << 31)) return LKGD_E_SHAPE;
  if (!aligned16(out) || ldo % 8 || ((uintptr_t)x & 1u)) return LKGD_E_ALIGN;
  const dim3 grid((unsigned)((rows * 16 + 255) / 256)), block(256);
  const half_t* xs = (const half_t*)x;
  half_t* o = (half_t*)out;
  const hipStream_t s = (hipStream_t)stream;
  switch (Cin) {
    case 1: hipLaunchKernelGGL(pixel_taps_kernel<1>, grid, block, 0, s, xs, o, ldo, (unsigned)rows, T, H, W, t0, Tc); break;
    case 2: hipLaunchKernelGGL(pixel_taps_kernel<2>, grid, block, 0, s, xs, o, ldo, (unsigned)rows, T, H, W, t0, Tc); break;
    case 3: hipLaunchKernelGGL(pixel_taps_kernel<3>, grid, block, 0, s, xs, o, ldo, (unsigned)rows, T, H, W, t0, Tc); break;
    default: hipLaunchKernelGGL(pixel_taps_kernel<4>, grid, block, 0, s, xs, o, ldo, (unsigned)rows, T, H, W, t0, Tc); break;
  }
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// ---- lkgd_cogvae_time_pool -----------------------------------------------------------------------------------------------------------
// One thread = 8 channels (16 bytes) of one output row; consecutive threads walk a row's channels, then the next row: whole rows per
// wave instruction on both reads and on the write.
__global__ __launch_bounds__(256) void time_pool_kernel(const half_t* __restrict__ in, int ldi, half_t* __restrict__ out, int ldo,
                                                        unsigned orows, int T, int To, unsigned HW, int C) {
  const unsigned C8 = (unsigned)C >> 3;
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  const unsigned row = (unsigned)(i / C8);
  if (row >= orows) return;
  const unsigned c = ((unsigned)(i - (unsigned long long)row * C8)) << 3;
  const unsigned ToHW = (unsigned)To * HW;
  const unsigned b = row / ToHW, r = row - b * ToHW;
  const unsigned j = r / HW, s = r - j * HW;
  const unsigned odd = (unsigned)T & 1u;
  const unsigned long long base = (unsigned long long)b * (unsigned)T * HW + s;          // (b, frame 0, s)
  half8_t o;
  if (odd && j == 0) {
    o = *(const half8_t*)(in + base * ldi + c);
  } else {
    const unsigned ta = 2u * j - odd;             // j >= 1 when odd: ta >= 1; ta + 1 <= T - 1
    const half8_t a = *(const half8_t*)(in + (base + (unsigned long long)ta * HW) * ldi + c);
    const half8_t d = *(const half8_t*)(in + (base + (unsigned long long)(ta + 1u) * HW) * ldi + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)(((float)a[e] + (float)d[e]) * 0.5f);
  }
  *(half8_t*)(out + (unsigned long long)row * ldo + c) = o;
}

extern "C" int lkgd_cogvae_time_pool(const void* in, int32_t ldi, void* out, int32_t ldo, int32_t B, int32_t T, int64_t HW, int32_t C,
                                     lkgd_stream_t stream) {
  if (!in || !out) return LKGD_E_NULL;
  if (B <= 0 || T <= 0 || HW <= 0 || C <= 0 || C % 8 || ldi < C || ldo < C) return LKGD_E_SHAPE;
  if (HW >= (1LL << 31) || (long long)B * T * HW >= (1LL << 31)) return LKGD_E_SHAPE;
  const int To = (T & 1) ? 1 + (T - 1) / 2 : T / 2;
  const long long irows = (long long)B * T * HW, orows = (long long)B * To * HW;
  {  // the last byte either tensor holds: the row ranges must not meet
    const uintptr_t i0 = (uintptr_t)in, i1 = i0 + (uintptr_t)(((irows - 1) * ldi + C) * 2);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(((orows - 1) * ldo + C) * 2);
    if (i0 < o1 && o0 < i1) return LKGD_E_SHAPE;
  }
  if (!aligned16(in) || !aligned16(out) || ldi % 8 || ldo % 8) return LKGD_E_ALIGN;
  const long long total = orows * (C / 8);
  hipLaunchKernelGGL(time_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const half_t*)in, ldi,
                     (half_t*)out, ldo, (unsigned)orows, T, To, (unsigned)HW, C);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// ---- lkgd_cogvae_posterior -----------------------------------------------------------------------------------------------------------
// Rows to planes: thread = 8 channels of one moment row (16 bytes of the mean columns, 16 of the log-variance columns); blockIdx.y picks
// the 8 channels, adjacent lanes hold adjacent rows - the 2-byte accesses of a wave to one (b, c) plane of noise / mean / sample are
// 128 contiguous bytes.
__global__ __launch_bounds__(256) void posterior_kernel(const half_t* __restrict__ mom, int ldm, const half_t* __restrict__ noise,
                                                        half_t* __restrict__ mean, half_t* __restrict__ sample, float scale,
                                                        unsigned rows, unsigned THW, int lc) {
  const unsigned row = blockIdx.x * 256u + threadIdx.x;
  if (row >= rows) return;
  const unsigned c0 = blockIdx.y * 8u;
  const unsigned b = row / THW, r = row - b * THW;
  const half8_t m = *(const half8_t*)(mom + (unsigned long long)row * ldm + c0);
  const unsigned long long o = ((unsigned long long)b * (unsigned)lc + c0) * THW + r;          // (b, c0, r); a channel further = + THW
  if (noise == nullptr) {
#pragma unroll
    for (int e = 0; e < 8; ++e) mean[o + (unsigned long long)e * THW] = m[e];
    return;
  }
  const half8_t lv = *(const half8_t*)(mom + (unsigned long long)row * ldm + lc + c0);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned long long at = o + (unsigned long long)e * THW;
    const float l = fminf(fmaxf((float)lv[e], -30.0f), 20.0f);
    const float sd = __expf(0.5f * l);
    mean[at] = m[e];
    sample[at] = (half_t)(scale * ((float)m[e] + sd * (float)noise[at]));
  }
}

extern "C" int lkgd_cogvae_posterior(const void* mom, int32_t ldm, const void* noise, void* mean, void* sample, float scale, int32_t B,
                                     int32_t lc, int32_t T, int32_t h, int32_t w, lkgd_stream_t stream) {
  if (!mom || !mean || (noise && !sample)) return LKGD_E_NULL;
  if (B <= 0 || T <= 0 || h <= 0 || w <= 0 || lc <= 0 || lc % 8 || ldm < 2 * lc || !isfinite(scale)) return LKGD_E_SHAPE;
  const long long thw = (long long)T * h * w;
  if (thw >= (1LL << 31) || (long long)B * thw * lc >= (1LL << 31)) return LKGD_E_SHAPE;
  if (!aligned16(mom) || ldm % 8 || ((uintptr_t)mean & 1u) || ((uintptr_t)noise & 1u) || ((uintptr_t)sample & 1u)) return LKGD_E_ALIGN;
  const long long rows = (long long)B * thw;
  hipLaunchKernelGGL(posterior_kernel, dim3((unsigned)((rows + 255) / 256), (unsigned)(lc / 8)), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)mom, ldm, (const half_t*)noise, (half_t*)mean, (half_t*)sample, scale, (unsigned)rows, (unsigned)thw, lc);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
