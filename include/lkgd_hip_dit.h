/*
 * lkgd_hip_dit.h - attention glue of the rotary CogVideoX DiT (CogVideoX-5B-I2V; CogVideo-main/finetune/models/cogvideox_i2v/
 * cogvideox_transformer_3d.py with use_rotary_positional_embeddings, the model every launcher of that port trains).  Same
 * library, conventions, return codes and footprint contract as lkgd_hip.h.
 *
 * lkgd_qk_norm_rope: the per-head LayerNorm of the queries and keys (attn.norm_q / attn.norm_k) and the rotary embedding of
 * their video rows (diffusers' CogVideoXAttnProcessor2_0 -> apply_rotary_emb, use_real_unbind_dim = -1), q and k in ONE launch,
 * in place.  As the reference writes it a layer costs two norms plus several fp32 round trips of both tensors; here every
 * element of q and k is read once and written once.
 *
 *   q, k   fp16 token matrices [rows, heads * 64] with row strides ldq, ldk (column windows of a wider buffer are fine);
 *          head h = columns [64 h, 64 h + 64).
 *   row r  belongs to batch entry r / rows_per_batch; it is a TEXT row when r % rows_per_batch < split, else the video row at
 *          position r % rows_per_batch - split.
 *   cos_t, sin_t   fp32 [rows_per_batch - split, 64] with row stride ldt: one table row per video position, shared by every
 *          head, by q and k, and by every batch entry.  Both NULL: norm only.
 *
 * Arithmetic and rounding points (the reference's):
 *   1. LayerNorm over the head's 64 channels - fp32 statistics, eps, fp32 affine, ROUNDED TO FP16.  The arithmetic is the
 *      arithmetic lkgd_layernorm performs on a 64-channel row (4 lanes x 2 vectors per row, same element and shuffle order,
 *      rsqrtf): norm-only mode is bit for bit lkgd_layernorm on the [rows * heads, 64] view.
 *   2. video rows only, on the fp16-rounded x, in fp32:  y[2i]   = x[2i]   * cos[2i]   - x[2i+1] * sin[2i]
 *                                                        y[2i+1] = x[2i+1] * cos[2i+1] + x[2i]   * sin[2i+1]
 *      two products and one sum, each rounded (no contraction), the result rounded to fp16.
 *   3. text rows: the norm only.
 *
 * Errors: LKGD_E_NULL for q, k or a gamma / beta, and when exactly one of cos_t / sin_t is NULL; LKGD_E_SHAPE for rows,
 * heads, rows_per_batch <= 0, rows % rows_per_batch, split outside [0, rows_per_batch], ld < heads * 64, ldt < 64;
 * LKGD_E_ALIGN for ld % 8, ldt % 4 or a pointer that is not 16 bytes aligned.  One launch, no allocation, no host sync, no LDS.
 */
#ifndef LKGD_HIP_DIT_H
#define LKGD_HIP_DIT_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_qk_norm_rope(void* q, int32_t ldq, void* k, int32_t ldk, int64_t rows, int32_t heads, const float* gamma_q,
                      const float* beta_q, const float* gamma_k, const float* beta_k, float eps, const float* cos_t,
                      const float* sin_t, int32_t ldt, int32_t rows_per_batch, int32_t split, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
