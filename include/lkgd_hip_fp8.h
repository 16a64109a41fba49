/*
 * lkgd_hip_fp8.h - the opt-in FP8 (OCP e4m3fn) form of the six linears of a CogVideoX DiT block (q, k, v, out, ff.0, ff.2): dynamic
 * per-row quantisers for the activations and a GEMM on the block-scaled matrix instruction of gfx950.  Same library, conventions,
 * return codes and footprint contract as lkgd_hip.h: raw pointers plus a stream, ONE launch each, no allocation, no host sync,
 * writes only inside the output windows, reads outside a logical window never influence a result.
 *
 * Format: OCP e4m3fn (bias 7, largest finite value 448 = 0x7E, NaN = 0x7F / 0xFF, no infinity) - NOT the e4m3fnuz of gfx942.
 *
 * ---- the quantisation statement Q(x) of one row x (fp16 values, taken as fp32) ---------------------------------------------------
 *   amax  = max |x|
 *   amax == 0:  scale = 1, every byte a zero (of the element's sign)
 *   else        inv = 448.0f / amax, scale = amax / 448.0f      both correctly rounded fp32 divisions
 *   q     = RNE_e4m3fn(clamp(x * inv, -448, 448))               the product is ONE fp32 rounding; the clamp is explicit and comes
 *                                                               before the conversion (no reliance on a convert's overflow mode)
 * so decode(q) * scale approximates x, a non-zero row always reaches |q| = 448, and no NaN byte is ever produced from finite input.
 * Weights use the same statement per OUTPUT CHANNEL, once at pack time on the host (lkgd_amd/fp8.py quantize_weight).
 *
 * ---- lkgd_quant_rows_fp8 ---------------------------------------------------------------------------------------------------------
 *   x      fp16 [T, K], row stride ldx >= K (elements)
 *   q      bytes [T, K], row stride ldq >= K (bytes)
 *   scale  fp32 [T]
 * Q per row.  K % 8 == 0, K <= 12288.
 *
 * ---- lkgd_gelu_tanh_quant_fp8 ----------------------------------------------------------------------------------------------------
 * Same arguments.  Equals lkgd_gelu_tanh followed by lkgd_quant_rows_fp8 EXACTLY: lkgd_gelu_tanh's arithmetic, the rounding to fp16 it
 * stores, then Q.  The fusion saves a round trip through memory, not a rounding point.
 *
 * ---- lkgd_layernorm_quant_fp8 ----------------------------------------------------------------------------------------------------
 * The arguments of lkgd_hip.h's lkgd_layernorm without its row-bias group, the output replaced by (q, ldq, scale):
 *   x fp16 [T, C] with ldx; gamma, beta fp32 [C] (both, or both NULL: no affine); eps; q bytes [T, C] with ldq; scale fp32 [T].
 * Equals lkgd_layernorm followed by lkgd_quant_rows_fp8 EXACTLY: the row arithmetic of lkgd_layernorm in its element
 * and shuffle order, the rounding to fp16, then Q.  C % 8 == 0, C <= 3072 (lkgd_layernorm's range).
 *
 * The three quantisers: LKGD_E_NULL for a null x / q / scale (or exactly one of gamma, beta); LKGD_E_SHAPE for T <= 0, a width out
 * of range or not a multiple of 8, ldx or ldq below the width; LKGD_E_ALIGN unless x, q (and gamma, beta) are 16 bytes aligned,
 * ldx % 8 == 0 and ldq % 16 == 0 (the rows are what lkgd_gemm_fp8 takes).
 *
 * ---- lkgd_gemm_fp8 ---------------------------------------------------------------------------------------------------------------
 *   a        e4m3fn bytes [M, K], row stride lda (bytes)         a_scale  fp32 [M]
 *   w        e4m3fn bytes [N, K], row stride ldw: K contiguous, the orientation of a Linear's own weight
 *   w_scale  fp32 [N]                                            bias     fp32 [N] or NULL
 *   out      fp16 [M, N], row stride ldc (elements)
 *   out[m, n] = fp16( (sum_k a[m, k] * w[n, k]) * a_scale[m] * w_scale[n] + bias[n] )
 * The products are exact and the sum is accumulated in fp32 by the matrix instruction (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 on
 * both sides, every block scale 2^0); the epilogue is fp32: (sum * a_scale[m]) * w_scale[n] + bias[n], the last two as one fused
 * multiply-add, then ONE rounding to fp16.
 * M >= 1 of any value: the rows of a and a_scale past M - 1 are never read, the rows of out past M - 1 never written.
 * Errors: LKGD_E_NULL for a null a / a_scale / w / w_scale / out; LKGD_E_SHAPE unless M, N, K > 0, N % 128 == 0, K % 128 == 0 (every
 * DiT width: 1920, 3072, 4 D, the tests' 128), lda, ldw >= K, ldc >= N; LKGD_E_ALIGN unless a, w, out, w_scale and bias are 16 bytes
 * aligned, lda % 16 == 0, ldw % 16 == 0 and ldc % 8 == 0.
 */
#ifndef LKGD_HIP_FP8_H
#define LKGD_HIP_FP8_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_quant_rows_fp8(const void* x, int32_t ldx, void* q, int32_t ldq, float* scale, int64_t T, int32_t K, lkgd_stream_t stream);

int lkgd_gelu_tanh_quant_fp8(const void* x, int32_t ldx, void* q, int32_t ldq, float* scale, int64_t T, int32_t K,
                             lkgd_stream_t stream);

int lkgd_layernorm_quant_fp8(const void* x, int32_t ldx, int64_t T, int32_t C, const float* gamma, const float* beta, float eps,
                             void* q, int32_t ldq, float* scale, lkgd_stream_t stream);

int lkgd_gemm_fp8(const void* a, int32_t lda, const float* a_scale, const void* w, int32_t ldw, const float* w_scale,
                  const float* bias, void* out, int32_t ldc, int32_t M, int32_t N, int32_t K, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
