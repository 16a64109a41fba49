// Frames out and image in of the CogVideoX image-to-video pipeline (include/lkgd_hip_video.h): planar fp16 clip -> interleaved uint8 /
// fp32 frames or frame-major fp16, and interleaved uint8 images -> planar fp16 in [-1, 1].  Memory-bound, no LDS, no reuse: every byte
// is moved once.  A launch is wide (a thread owns 8 pixels, 16-byte accesses to the planes) or narrow (one pixel) as a whole; the host
// decides.
#include "common.h"

#include "../../include/lkgd_hip_video.h"

// two fp16 roundings and fp32 steps exactly as written: nothing here may become an fma
#pragma clang fp contract(off)

typedef unsigned int uint2_t __attribute__((ext_vector_type(2)));

// (images / 2 + 0.5).clamp(0, 1) on a half tensor; NaN passes through both comparisons
__device__ __forceinline__ half_t denorm1(half_t v) {
  const half_t a = (half_t)((float)v / 2.0f);
  const half_t b = (half_t)((float)a + 0.5f);
  return b < (half_t)0.0f ? (half_t)0.0f : (b > (half_t)1.0f ? (half_t)1.0f : b);
}
// (images * 255).round().astype(uint8) on the fp32 of d in [0, 1]; NaN -> 0
__device__ __forceinline__ unsigned quant1(half_t d) {
  const float f = (float)d;
  return f == f ? (unsigned)rintf(f * 255.0f) : 0u;
}

// ---- lkgd_video_postprocess, interleaved modes -----------------------------------------------------------------------------------------
// wide: thread i = 8 consecutive pixels of one batch entry (per = L / 8 chunks each); narrow: thread i = one pixel (per = L)
template <int C_, int MODE, bool WIDE>
__global__ __launch_bounds__(256) void video_interleave_kernel(const half_t* __restrict__ x, void* __restrict__ out,
                                                               unsigned long long items, unsigned long long per, unsigned long long L) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (i >= items) return;
  const unsigned long long b = i / per;
  const unsigned long long px = (i - b * per) * (WIDE ? 8u : 1u);      // first pixel inside the batch entry
  const half_t* src = x + b * C_ * L + px;                               // plane c lies c * L further
  const unsigned long long o = (b * L + px) * C_;                        // first output element
  if (WIDE) {
    half_t d[8 * C_];                                                    // pixel-major: d[e * C_ + c]
#pragma unroll
    for (int c = 0; c < C_; ++c) {
      const half8_t v = *(const half8_t*)(src + c * L);
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e * C_ + c] = denorm1(v[e]);
    }
    if (MODE == LKGD_VIDEO_U8) {
      uint2_t* dst = (uint2_t*)((unsigned char*)out + o);                // 8 * C_ bytes, 8 bytes aligned
#pragma unroll
      for (int k = 0; k < C_; ++k) {
        uint2_t w;
        w.x = quant1(d[8 * k + 0]) | quant1(d[8 * k + 1]) << 8 | quant1(d[8 * k + 2]) << 16 | quant1(d[8 * k + 3]) << 24;
        w.y = quant1(d[8 * k + 4]) | quant1(d[8 * k + 5]) << 8 | quant1(d[8 * k + 6]) << 16 | quant1(d[8 * k + 7]) << 24;
        dst[k] = w;
      }
    } else {
      float4_t* dst = (float4_t*)((float*)out + o);                      // 8 * C_ floats, 16 bytes aligned
#pragma unroll
      for (int k = 0; k < 2 * C_; ++k) {
        float4_t w;
        w.x = (float)d[4 * k + 0];
        w.y = (float)d[4 * k + 1];
        w.z = (float)d[4 * k + 2];
        w.w = (float)d[4 * k + 3];
        dst[k] = w;
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < C_; ++c) {
      const half_t d = denorm1(src[c * L]);
      if (MODE == LKGD_VIDEO_U8) ((unsigned char*)out)[o + c] = (unsigned char)quant1(d);
      else ((float*)out)[o + c] = (float)d;
    }
  }
}

// ---- lkgd_video_postprocess, mode F16 ----------------------------------------------------------------------------------------------
// [B, C, T, HW] -> [B, T, C, HW]; wide: thread i = 8 consecutive values of one plane (per = HW / 8), narrow: one value (per = HW)
template <bool WIDE>
__global__ __launch_bounds__(256) void video_planes_kernel(const half_t* __restrict__ x, half_t* __restrict__ out, unsigned long long items,
                                                           unsigned long long per, unsigned long long HW, unsigned C_, unsigned T) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (i >= items) return;
  const unsigned long long plane = i / per;                              // (b * C + c) * T + t
  const unsigned long long s = (i - plane * per) * (WIDE ? 8u : 1u);
  const unsigned long long bc = plane / T;
  const unsigned long long t = plane - bc * T;
  const unsigned long long b = bc / C_;
  const unsigned long long c = bc - b * C_;
  const half_t* src = x + plane * HW + s;
  half_t* dst = out + ((b * T + t) * C_ + c) * HW + s;
  if (WIDE) {
    half8_t v = *(const half8_t*)src;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = denorm1(v[e]);
    *(half8_t*)dst = v;
  } else {
    *dst = denorm1(*src);
  }
}

template <int C_, int MODE>
static void launch_interleave(const void* x, void* out, unsigned long long B, unsigned long long L, bool wide, hipStream_t st) {
  const unsigned long long per = wide ? L / 8 : L, items = B * per;
  const dim3 grid((unsigned)((items + 255) / 256)), block(256);
  if (wide) hipLaunchKernelGGL((video_interleave_kernel<C_, MODE, true>), grid, block, 0, st, (const half_t*)x, out, items, per, L);
  else hipLaunchKernelGGL((video_interleave_kernel<C_, MODE, false>), grid, block, 0, st, (const half_t*)x, out, items, per, L);
}

template <int MODE>
static void launch_interleave_c(int C_, const void* x, void* out, unsigned long long B, unsigned long long L, bool wide, hipStream_t st) {
  switch (C_) {
    case 1: launch_interleave<1, MODE>(x, out, B, L, wide, st); break;
    case 2: launch_interleave<2, MODE>(x, out, B, L, wide, st); break;
    case 3: launch_interleave<3, MODE>(x, out, B, L, wide, st); break;
    default: launch_interleave<4, MODE>(x, out, B, L, wide, st); break;
  }
}

extern "C" int lkgd_video_postprocess(const void* x, void* out, int32_t mode, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                                      lkgd_stream_t stream) {
  if (!x || !out) return LKGD_E_NULL;
  if (B <= 0 || C <= 0 || C > 4 || T <= 0 || H <= 0 || W <= 0) return LKGD_E_SHAPE;
  const unsigned long long HW = (unsigned long long)H * W, L = HW * T;
  if (L >= (1ULL << 38) || (unsigned long long)B * C >= (1ULL << 38) / L) return LKGD_E_SHAPE;
  if (mode != LKGD_VIDEO_U8 && mode != LKGD_VIDEO_F32 && mode != LKGD_VIDEO_F16) return LKGD_E_MODE;
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  if ((xa & 1u) || (mode == LKGD_VIDEO_F32 && (oa & 3u)) || (mode == LKGD_VIDEO_F16 && (oa & 1u))) return LKGD_E_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (mode == LKGD_VIDEO_F16) {
    const bool wide = HW % 8 == 0 && aligned16(x) && aligned16(out);
    const unsigned long long per = wide ? HW / 8 : HW, items = (unsigned long long)B * C * T * per;
    const dim3 grid((unsigned)((items + 255) / 256)), block(256);
    if (wide) hipLaunchKernelGGL(video_planes_kernel<true>, grid, block, 0, st, (const half_t*)x, (half_t*)out, items, per, HW, (unsigned)C, (unsigned)T);
    else hipLaunchKernelGGL(video_planes_kernel<false>, grid, block, 0, st, (const half_t*)x, (half_t*)out, items, per, HW, (unsigned)C, (unsigned)T);
  } else if (mode == LKGD_VIDEO_U8) {
    launch_interleave_c<LKGD_VIDEO_U8>(C, x, out, (unsigned long long)B, L, L % 8 == 0 && aligned16(x) && (oa & 7u) == 0, st);
  } else {
    launch_interleave_c<LKGD_VIDEO_F32>(C, x, out, (unsigned long long)B, L, L % 8 == 0 && aligned16(x) && aligned16(out), st);
  }
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// ---- lkgd_image_preprocess -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ half_t norm1(unsigned u) { return (half_t)(__fdiv_rn((float)u, 255.0f) * 2.0f - 1.0f); }

// wide: thread i = 8 consecutive pixels of one image (per = HW / 8), narrow: one pixel (per = HW)
template <int C_, bool WIDE>
__global__ __launch_bounds__(256) void image_planes_kernel(const unsigned char* __restrict__ u, half_t* __restrict__ out,
                                                           unsigned long long items, unsigned long long per, unsigned long long HW) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (i >= items) return;
  const unsigned long long n = i / per;
  const unsigned long long px = (i - n * per) * (WIDE ? 8u : 1u);
  const unsigned char* src = u + (n * HW + px) * C_;
  half_t* dst = out + n * C_ * HW + px;                                  // plane c lies c * HW further
  if (WIDE) {
    unsigned w[2 * C_];                                                  // 8 * C_ bytes, 8 bytes aligned
#pragma unroll
    for (int k = 0; k < C_; ++k) {
      const uint2_t q = ((const uint2_t*)src)[k];
      w[2 * k] = q.x;
      w[2 * k + 1] = q.y;
    }
#pragma unroll
    for (int c = 0; c < C_; ++c) {
      half8_t v;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int byte = e * C_ + c;
        v[e] = norm1((w[byte >> 2] >> ((byte & 3) * 8)) & 0xffu);
      }
      *(half8_t*)(dst + c * HW) = v;
    }
  } else {
#pragma unroll
    for (int c = 0; c < C_; ++c) dst[c * HW] = norm1(src[c]);
  }
}

template <int C_>
static void launch_image(const void* u, void* out, unsigned long long N, unsigned long long HW, bool wide, hipStream_t st) {
  const unsigned long long per = wide ? HW / 8 : HW, items = N * per;
  const dim3 grid((unsigned)((items + 255) / 256)), block(256);
  if (wide) hipLaunchKernelGGL((image_planes_kernel<C_, true>), grid, block, 0, st, (const unsigned char*)u, (half_t*)out, items, per, HW);
  else hipLaunchKernelGGL((image_planes_kernel<C_, false>), grid, block, 0, st, (const unsigned char*)u, (half_t*)out, items, per, HW);
}

extern "C" int lkgd_image_preprocess(const void* u, void* out, int32_t N, int32_t H, int32_t W, int32_t C, lkgd_stream_t stream) {
  if (!u || !out) return LKGD_E_NULL;
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C > 4) return LKGD_E_SHAPE;
  const unsigned long long HW = (unsigned long long)H * W;
  if ((unsigned long long)N * C >= (1ULL << 38) / HW) return LKGD_E_SHAPE;
  if ((uintptr_t)out & 1u) return LKGD_E_ALIGN;
  const bool wide = HW % 8 == 0 && ((uintptr_t)u & 7u) == 0 && aligned16(out);
  hipStream_t st = (hipStream_t)stream;
  switch (C) {
    case 1: launch_image<1>(u, out, (unsigned long long)N, HW, wide, st); break;
    case 2: launch_image<2>(u, out, (unsigned long long)N, HW, wide, st); break;
    case 3: launch_image<3>(u, out, (unsigned long long)N, HW, wide, st); break;
    default: launch_image<4>(u, out, (unsigned long long)N, HW, wide, st); break;
  }
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
