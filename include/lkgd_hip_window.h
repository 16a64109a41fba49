/*
 * lkgd_hip_window.h - loop glue of the long-video smoothing pipeline (pipeline/pipeline_stable_video_diffusion_smooth.py, driven
 * by run_models/run_inference_svd_smooth.py).  Same library, conventions, return codes and footprint contract as lkgd_hip.h.
 *
 * That pipeline denoises a video of T frames in frame WINDOWS: every Euler step cuts the frames into contiguous windows
 * (get_chunks, :526-533) and runs the UNet per window on a batch of four, [window, window reversed in time] x [uncond, cond]
 * (:549-577); only the forward clip's CFG result is kept (:579-591) and one Euler step is taken over all T frames (:594).  As
 * the reference writes it a window costs a gather, a flip, four cats, a repeat, a scale, a scatter and its share of a full-tensor
 * step; here it costs the two launches below, and neither the gathered batch, the repeated image latents, the unconditional
 * zeros nor `noise_pred` ever exists.
 *
 * The window is frames f0 .. f0+L-1 of `latents` [T,4,H,W] (fp16 or fp32; the reference's batch is 1).  UNet batch entry
 * e = 2*k + d: k = CFG half (uncond first when cfg == 2), d = 0 the forward clip, d = 1 the reversed clip.
 *
 * lkgd_window_prepare_input: tokens_out [2*cfg*L*H*W, 8] fp16, row (e, j, p):
 *     channels 0-3 = latents[f0 + (d ? L-1-j : j)] / sqrt(sigma^2+1)      (:551, :565-566; scale_model_input, rounded to fp16)
 *     channels 4-7 = 0 in the uncond half, else image_latents[d ? f0+L-1 : f0] for every j      (:554-559, :568)
 *   image_latents [T,4,H,W] fp16: ONE conditional latent per input frame (the window's first / last frame conditions the
 *   forward / reversed clip).  tokens_out 16 bytes aligned (ld = 8 by definition); latents: element aligned.
 *
 * lkgd_window_cfg_euler_step: noise_tokens [2*cfg*L*H*W, 4] fp16 (the UNet's output for the batch above).  Reads entry 0, and
 *   entry 2 when cfg == 2 - the forward clip - forms uncond + guidance[j]*(cond - uncond), j < L, and takes the Euler step in
 *   place on frames f0 .. f0+L-1 of `latents`, with lkgd_cfg_euler_step's fp16 rounding points (:579-591, scheduler.step
 *   :594).  Nothing outside those frames is read or written: the step is pointwise per frame, so stepping window by window
 *   equals the reference's assemble-then-step.  guidance: device fp32 [L] (torch.linspace(min, max, L), :581), may be NULL when
 *   cfg == 1.  noise_tokens 8 bytes aligned (ld = 4 by definition); latents: element aligned.
 *
 * Errors: LKGD_E_NULL; LKGD_E_SHAPE for T, H, W, L <= 0, f0 < 0, f0 + L > T, cfg not 1 / 2, sigma <= 0; LKGD_E_MODE for
 * prediction_type; LKGD_E_ALIGN for the token buffers.  One launch each, no allocation, no host sync.
 */
#ifndef LKGD_HIP_WINDOW_H
#define LKGD_HIP_WINDOW_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_window_prepare_input(const void* latents, int32_t latents_is_f32, const void* image_latents, int32_t T, int32_t f0,
                              int32_t L, int32_t H, int32_t W, int32_t cfg, float sigma, void* tokens_out,
                              lkgd_stream_t stream);
int lkgd_window_cfg_euler_step(const void* noise_tokens, void* latents, int32_t latents_is_f32, const float* guidance,
                               int32_t T, int32_t f0, int32_t L, int32_t H, int32_t W, int32_t cfg, float sigma,
                               float sigma_next, int32_t prediction_type /*0 eps, 1 v*/, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
