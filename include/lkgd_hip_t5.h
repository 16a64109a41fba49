/*
 * lkgd_hip_t5.h - the operators of the T5 text encoder in front of the CogVideoX loop (lkgd_amd/t5.py; transformers' T5EncoderModel
 * [EXT], called by pipeline_cogvideox_image2video.py:262 as `self.text_encoder(text_input_ids)[0]`): the token embedding lookup, the
 * RMS norm over an fp32 residual stream, dense attention with an additive relative-position bias, the gated tanh-GELU and the fp32
 * residual add.  Same library, conventions, return codes and footprint contract as lkgd_hip.h: raw pointers plus a stream, ONE launch
 * each, no allocation, no host sync, writes only inside the output windows, reads outside a logical window never influence a result.
 * The linears between them are lkgd_gemm_f16.
 *
 * ---- lkgd_t5_embed_rows ----------------------------------------------------------------------------------------------------------
 *   ids    int64 [T]
 *   table  fp16 [V, D], row stride ldt >= D (elements)
 *   out    fp32 [T, D], row stride ldo >= D
 *   out[t, :] = float(table[ids[t], :])                                                    (nn.Embedding; exact)
 * The caller validates the ids; the kernel clamps an id into [0, V) all the same, so no launch reads outside the table.
 * LKGD_E_NULL for a null ids / table / out; LKGD_E_SHAPE for T <= 0, V <= 0, D <= 0, D % 8 != 0, ldt < D or ldo < D; LKGD_E_ALIGN
 * unless table and out are 16 bytes aligned, ids 8 bytes, ldt % 8 == 0 and ldo % 4 == 0.
 *
 * ---- lkgd_t5_rmsnorm -------------------------------------------------------------------------------------------------------------
 *   x       fp32 [T, C], row stride ldx >= C          weight  fp32 [C]
 *   out     fp16 [T, C], row stride ldo >= C
 *   out[t, c] = fp16( weight[c] * (x[t, c] * rsqrt(mean_c(x[t, :]^2) + eps)) )            (T5LayerNorm: no mean, no bias)
 * fp32 throughout, one rounding.  The sum of squares is taken in a fixed order (per thread, per wave, across the four waves).
 * LKGD_E_NULL for a null x / weight / out; LKGD_E_SHAPE for T <= 0, C <= 0, C % 8 != 0, C > 4096, ldx < C or ldo < C; LKGD_E_ALIGN
 * unless x, weight and out are 16 bytes aligned, ldx % 4 == 0 and ldo % 8 == 0.
 *
 * ---- lkgd_attn_dense_relbias -----------------------------------------------------------------------------------------------------
 * The lkgd_attn_dense of lkgd_hip.h section 16 with a relative-position bias: for query row i and key row j of one (batch entry, head h)
 *   score[i, j] = scale * (q_i . k_j) + relbias[h, j - i + S - 1],    out_i = softmax_j(score[i, :]) . v
 *   relbias  fp32 [heads, 2S - 1], contiguous: entry d + S - 1 of a row is the bias at key position minus query position d
 * Operand layout, alignment rule and arithmetic are lkgd_attn_dense's: q, k, v, out are token rows [nbatch * S, heads * head_dim] with
 * row strides (column windows of one [T, 3 * inner] buffer are valid operands); q / k / v 16 bytes aligned with ld % 8 == 0, out 4
 * bytes with ldo % 2 == 0; head_dim % 8 == 0, head_dim <= 128; K and V of one head, the four waves' probability and query rows AND
 * the head's 2S - 1 table entries must fit 160 KB of LDS (LKGD_E_SHAPE otherwise).  relbias: non-null (LKGD_E_NULL), 4 bytes aligned
 * (LKGD_E_ALIGN).  With an all-zero table the outputs equal lkgd_attn_dense's bit for bit: one kernel source, the bias a compile-time
 * switch (lkgd_amd/csrc/attn_dense.h).  T5 calls it with scale = 1: its attention does not divide by sqrt(head_dim).
 *
 * ---- lkgd_t5_gated_gelu ----------------------------------------------------------------------------------------------------------
 *   h    fp16 [T, 2F], row stride ldh >= 2F: columns [0, F) the wi_0 half, [F, 2F) the wi_1 half
 *   out  fp16 [T, F], row stride ldo >= F
 *   out[t, f] = fp16( gelu_tanh(h[t, f]) * h[t, F + f] ),   gelu_tanh(x) = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))
 * fp32 arithmetic, one rounding (T5DenseGatedActDense with transformers' `gelu_new`).  out must not overlap h.
 * LKGD_E_NULL for a null h / out; LKGD_E_SHAPE for T <= 0, F <= 0, F % 8 != 0, ldh < 2F or ldo < F; LKGD_E_ALIGN unless h and out are
 * 16 bytes aligned, ldh % 8 == 0 and ldo % 8 == 0.
 *
 * ---- lkgd_t5_residual_add --------------------------------------------------------------------------------------------------------
 *   x  fp32 [T, C], row stride ldx >= C, updated in place          y  fp16 [T, C], row stride ldy >= C
 *   x[t, c] += s * float(y[t, c])                                   (exact products for a power-of-two s)
 * The residual stream of the encoder stays fp32; s undoes the accumulator scale of the GEMM that produced y (lkgd_gemm_desc.s_acc).
 * LKGD_E_NULL for a null x / y; LKGD_E_SHAPE for T <= 0, C <= 0, C % 8 != 0, ldx < C or ldy < C; LKGD_E_ALIGN unless x and y are 16
 * bytes aligned, ldx % 4 == 0 and ldy % 8 == 0.
 */
#ifndef LKGD_HIP_T5_H
#define LKGD_HIP_T5_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_t5_embed_rows(const int64_t* ids, const void* table, int32_t ldt, int32_t V, int32_t D, float* out, int32_t ldo, int64_t T,
                       lkgd_stream_t stream);

int lkgd_t5_rmsnorm(const float* x, int32_t ldx, int64_t T, int32_t C, const float* weight, float eps, void* out, int32_t ldo,
                    lkgd_stream_t stream);

int lkgd_attn_dense_relbias(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* out, int32_t ldo,
                            int32_t nbatch, int32_t S, int32_t heads, int32_t head_dim, const float* relbias, float scale,
                            lkgd_stream_t stream);

int lkgd_t5_gated_gelu(const void* h, int32_t ldh, int64_t T, int32_t F, void* out, int32_t ldo, lkgd_stream_t stream);

int lkgd_t5_residual_add(float* x, int32_t ldx, const void* y, int32_t ldy, int64_t T, int32_t C, float s, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
