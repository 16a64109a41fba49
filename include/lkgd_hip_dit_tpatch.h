/*
 * lkgd_hip_dit_tpatch.h - the sampling-loop glue of lkgd_hip_dit_loop.h for the CogVideoX 1.5 architecture, whose patches span
 * p_t = 2 latent frames (cogvideox_transformer_3d.py:242, 326-331, 619-630; the padded frame count of
 * pipeline_cogvideox_image2video.py:382-384, 781-786).  Same library, conventions, return codes and footprint contract as
 * lkgd_hip.h and lkgd_hip_dit_loop.h: raw pointers plus a stream, no allocation, no host sync, writes only inside the output
 * windows, reads outside a logical window never influence a result.
 *
 * ---- lkgd_dit_patch_rows_t: latents (+ image latents) -> the 1.5 patch embedding's A rows ------------------------------------------
 *   latents        [B, F, C, H, W], fp16 or fp32 (latents_is_f32; rounded to fp16), element aligned.  F % p_t == 0.
 *   image_latents  fp16 [B, F, C, H, W], or NULL.
 *   rows_out       fp16 [B * (F/p_t) * (H/p) * (W/p), ldp]; row (b, ft, y, x), column ((c * p_t + pt) * p + py) * p + px holds
 *                  channel c of the 2C concatenated channels (latents first; C channels when image_latents is NULL) at frame
 *                  ft p_t + pt, pixel (y p + py, x p + px): bit for bit torch.cat([latents.half(), image_latents], 2) through
 *                    .permute(0, 1, 3, 4, 2).reshape(B, F/p_t, p_t, H/p, p, W/p, p, 2C).permute(0, 1, 3, 5, 7, 2, 4, 6)
 *                    .flatten(4, 7).flatten(1, 3)
 *                  - the reshape of diffusers' CogVideoXPatchEmbed for patch_size_t, whose Linear weight is [D, (c, pt, py, px)].
 *                  COLUMN ORDER: (c, pt, py, px), channel slowest.  It is restated from the published diffusers source (not in the
 *                  reference tree: PARITY UNPINNED); the in-tree un-patchify (:626-630) uses the same order for proj_out's columns.
 * One copy serves both CFG entries: the caller points both patch-embedding GEMMs at it.
 *
 * ---- lkgd_dit_cfg_ddim_step_t: CFG combine + DDIM update, in place on the latents -------------------------------------------------
 *   noise_rows  fp16 [cfg * B * Tv, ldn >= C p_t p p], Tv = (F/p_t) (H/p) (W/p), in the column order above (proj_out's output
 *               before the un-patchify of cogvideox_transformer_3d.py:626-630), the unconditional entries first.
 *   latents     [B, F, C, H, W] fp16 or fp32, read and written in place.
 * Per element in fp32, each statement's operations rounded one by one (no contraction) - the statements and rounding points of
 * lkgd_dit_cfg_ddim_step:
 *   n  = u + guidance * (c - u)        (n = u when cfg == 1)
 *   x0 = sqrt_alpha * x - sqrt_beta * n
 *   x' = a * x + b * x0                rounded to fp16 when the latents are fp16
 *
 * Both calls: LKGD_E_NULL for a null latents / rows pointer; LKGD_E_SHAPE unless B, F, C, H, W > 0, p == 2, p_t == 2,
 * F % p_t == 0, H % p == W % p == 0, (C p p) % 8 == 0, ld >= the row width, ld % 8 == 0, cfg in {1, 2}; LKGD_E_ALIGN unless the
 * rows are 16 bytes aligned.
 */
#ifndef LKGD_HIP_DIT_TPATCH_H
#define LKGD_HIP_DIT_TPATCH_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_dit_patch_rows_t(const void* latents, int32_t latents_is_f32, const void* image_latents, int32_t B, int32_t F, int32_t C,
                          int32_t H, int32_t W, int32_t p, int32_t p_t, void* rows_out, int32_t ldp, lkgd_stream_t stream);

int lkgd_dit_cfg_ddim_step_t(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, int32_t B, int32_t F,
                             int32_t C, int32_t H, int32_t W, int32_t p, int32_t p_t, int32_t cfg, float guidance, float a,
                             float b, float sqrt_alpha, float sqrt_beta, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
