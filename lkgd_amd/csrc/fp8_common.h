// The quantisation statement Q of include/lkgd_hip_fp8.h, shared by the FP8 quantisers (quant_fp8.hip).  Plain integer and
// fp32 arithmetic, no convert instruction: the rounding and the clamp are spelled out, so the bytes do not depend on a
// hardware overflow mode, and the same text compiles for the host.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LKGD_HD __host__ __device__ __forceinline__
#else
#define LKGD_HD static inline
#endif

#define LKGD_E4M3_MAX 448.0f

// fp32 v with |v| <= 448 -> OCP e4m3fn byte, round to nearest even.  Normal results (|v| >= 2^-6) round the fp32 mantissa
// to 3 bits in the integer domain (a carry walks into the exponent, 448 = 0x7E is the largest input so 0x7F is never
// produced); below that the value is a multiple of the subnormal step 2^-9: rint(|v| * 512) in 0..8, where 8 is the
// encoding of 2^-6 itself.
LKGD_HD uint32_t lkgd_e4m3_rne(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  const uint32_t sign = (u >> 24) & 0x80u;
  const uint32_t a = u & 0x7fffffffu;
  uint32_t q;
  if (a >= 0x3c800000u) {                                   // 2^-6
    q = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3);
  } else {
    float av;
    memcpy(&av, &a, 4);
    q = (uint32_t)(int)__builtin_rintf(av * 512.0f);
  }
  return sign | q;
}

// (inv, scale) of a row with maximum magnitude amax: 448 / amax and amax / 448, both correctly rounded; a zero row has scale 1
LKGD_HD void lkgd_q_scales(float amax, float* inv, float* scale) {
  if (amax == 0.0f) {
    *inv = 1.0f;
    *scale = 1.0f;
    return;
  }
#if defined(__HIP_DEVICE_COMPILE__)
  *inv = __fdiv_rn(LKGD_E4M3_MAX, amax);
  *scale = __fdiv_rn(amax, LKGD_E4M3_MAX);
#else
  *inv = LKGD_E4M3_MAX / amax;
  *scale = amax / LKGD_E4M3_MAX;
#endif
}

// one element: the product is ONE fp32 rounding (no contraction into a neighbour), the clamp explicit and before the conversion
LKGD_HD uint32_t lkgd_q_elem(float x, float inv) {
#if defined(__HIP_DEVICE_COMPILE__)
  float p = __fmul_rn(x, inv);
#else
  volatile float pv = x * inv;
  float p = pv;
#endif
  p = p > LKGD_E4M3_MAX ? LKGD_E4M3_MAX : p;
  p = p < -LKGD_E4M3_MAX ? -LKGD_E4M3_MAX : p;
  return lkgd_e4m3_rne(p);
}
