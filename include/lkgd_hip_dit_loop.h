/*
 * lkgd_hip_dit_loop.h - what the CogVideoX sampling loop (CogVideo-main/.../pipeline_cogvideox_image2video.py:829-885) executes
 * around the DiT forward, and LKGD's latent-knowledge fuse of the text tokens (cogvideox_transformer_3d.py:519-582).  Same
 * library, conventions, return codes and footprint contract as lkgd_hip.h: raw pointers plus a stream, no allocation, no host
 * sync, writes only inside the output windows, reads outside a logical window never influence a result.
 *
 * ---- lkgd_lk_fuse_tokens: the DiT form of lkgd_hip.h section 18 (the SVD fuse), one launch --------------------------------------
 *   e    fp32 [B * L, 4096] with row stride lde >= 4096; row r belongs to batch entry r / L.
 *   d, f fp32 [Bd, 1000] (domain / flow logits), Bd = 1 (broadcast over the batch) or B.
 *   w    18 fp32 operands in the order of lkgd_lk_fuse with the DiT's shapes, matrices (in, out) row-major, Hamilton matrices
 *        expanded on the host:  lconv [256][16], dconv [256][4], fconv [256][4], texts [256], fuse [1024][512], bias [512],
 *        texts_fft_mag [129], texts_fft_pha [129], fft_mag [512][256], bias [256], fft_pha [512][256], bias [256],
 *        fft_mag0 (4 weights + bias) [5], fft_pha0 [5], sf[0] [1024][512], bias [512], sf[2] [512][4096], bias [4096].
 *   out  fp16 [B * L, 4096] with row stride ldo >= 4096.
 * Arithmetic: fp32 throughout, ONE rounding to fp16 at the store.  Linear interpolation 1000 -> 1024 (align_corners = False), the
 * three grouped 1x1 convolutions, the quaternion linear on low | low_d | low_f | texts, the direct 256-point real DFT of each,
 * abs / angle, the two quaternion linears on bins 0..127, the two Linear(4, 1) on bin 128, the 257-bin inverse DFT to 512 samples,
 * Linear(1024, 512), LeakyReLU(0.1), Linear(512, 4096).  The two real bins (DC, Nyquist) have an imaginary part of exactly +0: a
 * negative one has phase +pi, as torch.angle(torch.fft.rfft(x)) has on the host.
 * A row's result does not depend on its company: the accumulation order of every sum is fixed per row, so row r of a [B, L] call
 * has the bits of the same row computed alone (B = L = 1) and of the call with Bd == B and expanded d / f rows.
 * Errors: LKGD_E_NULL for any null pointer (an entry of w included); LKGD_E_SHAPE for B, L <= 0, Bd not in {1, B}, lde or
 * ldo < 4096, more than 2^31 - 1 rows; LKGD_E_ALIGN unless e, out and w[0], w[16], w[17] (lconv, sf[2] and its bias) are 16 bytes
 * aligned, lde % 4 == 0 and ldo % 8 == 0 (they move in 16-byte pieces).
 *
 * ---- lkgd_dit_patch_rows: latents (+ image latents) -> the patch-embedding GEMM's A rows -----------------------------------------
 *   latents        [B, F, C, H, W], fp16 or fp32 (latents_is_f32; rounded to fp16), element aligned.
 *   image_latents  fp16 [B, F, C, H, W], or NULL.
 *   rows_out       fp16 [B * F * (H/p) * (W/p), ldp]; row (b, f, y, x), column (c * p + py) * p + px holds channel c of the
 *                  2C concatenated channels (latents first; C channels when image_latents is NULL) at pixel (y p + py, x p + px):
 *                  bit for bit torch.cat([latents.half(), image_latents], 2) through the reshape / permute of the patch embedding.
 * One copy serves both CFG entries: the caller points both patch-embedding GEMMs at it.
 *
 * ---- lkgd_dit_cfg_ddim_step: CFG combine + DDIM update, in place on the latents ---------------------------------------------------
 *   noise_rows  fp16 [cfg * B * Tv, ldn >= C p p], Tv = F (H/p) (W/p), in the column order above (proj_out's output before the
 *               un-patchify), the unconditional entries first.
 *   latents     [B, F, C, H, W] fp16 or fp32, read and written in place.
 * Per element in fp32, each statement's operations rounded one by one (no contraction):
 *   n  = u + guidance * (c - u)        (n = u when cfg == 1)
 *   x0 = sqrt_alpha * x - sqrt_beta * n
 *   x' = a * x + b * x0                rounded to fp16 when the latents are fp16
 * - the rounding points of noise_pred.float(), the three CFG statements, CogVideoXDDIMScheduler.step and .to(float16).
 *
 * Both glue calls: LKGD_E_NULL for a null latents / rows pointer; LKGD_E_SHAPE unless B, F, C, H, W > 0, p == 2, H % p == W % p
 * == 0, (C p p) % 8 == 0, ld >= the row width, ld % 8 == 0, cfg in {1, 2}; LKGD_E_ALIGN unless the rows are 16 bytes aligned.
 */
#ifndef LKGD_HIP_DIT_LOOP_H
#define LKGD_HIP_DIT_LOOP_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_lk_fuse_tokens(const float* e, int32_t lde, const float* d, const float* f, int32_t B, int32_t L, int32_t Bd,
                        const float* const* w, void* out, int32_t ldo, lkgd_stream_t stream);

int lkgd_dit_patch_rows(const void* latents, int32_t latents_is_f32, const void* image_latents, int32_t B, int32_t F, int32_t C,
                        int32_t H, int32_t W, int32_t p, void* rows_out, int32_t ldp, lkgd_stream_t stream);

int lkgd_dit_cfg_ddim_step(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, int32_t B, int32_t F,
                           int32_t C, int32_t H, int32_t W, int32_t p, int32_t cfg, float guidance, float a, float b,
                           float sqrt_alpha, float sqrt_beta, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
