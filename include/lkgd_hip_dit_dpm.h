/*
 * lkgd_hip_dit_dpm.h - the step of the CogVideoX sampling loop's OTHER scheduler branch (CogVideo-main/.../
 * pipeline_cogvideox_image2video.py:832-883, ``CogVideoXDPMScheduler``: DPM-Solver++ SDE, 2M), for 2-D patches and for the temporal
 * patches of the 1.5 models.  Same library, conventions, return codes and footprint contract as lkgd_hip.h and lkgd_hip_dit_loop.h:
 * raw pointers plus a stream, no allocation, no host sync, writes only inside the output windows, reads outside a logical window
 * never influence a result.
 *
 * ---- lkgd_dit_cfg_dpm_step / lkgd_dit_cfg_dpm_step_t: CFG combine + DPM-Solver++ update, in place on the latents ----------------
 *   noise_rows  fp16 [cfg * B * Tv, ldn], proj_out's token rows exactly as the DDIM step of lkgd_hip_dit_loop.h takes them: Tv = F
 *               (H/p) (W/p), ldn >= C p p, column (c, py, px); _t, as the DDIM step of lkgd_hip_dit_tpatch.h: Tv = (F/p_t) (H/p)
 *               (W/p), ldn >= C p_t p p, column (c, pt, py, px).  The unconditional entries first.
 *   latents     [B, F, C, H, W] fp16 or fp32 (latents_is_f32), read and written in place.
 *   x0_state    fp32 [B, F, C, H, W]: the scheduler's ``old_pred_original_sample``.  READ only when order == 2 (the previous step's
 *               x0), ALWAYS written with this step's x0.  One thread reads and then writes its own elements: in place is safe.
 *   eps         [B, F, C, H, W] in the latents' dtype: the step's noise.  May be NULL only when mn == 0; with mn == 0 it is never
 *               read, even when given.
 *   order       1 or 2; the scalars are CogVideoXDPMScheduler.coefficients(t, t_back) (lkgd_amd/cogvideox.py), fp64 on the host,
 *               rounded to fp32 here.
 * Per element in fp32, each statement's operations rounded one by one (no contraction), sums evaluated left to right:
 *   n  = u + guidance * (c - u)                       (n = u when cfg == 1)
 *   x0 = sqrt_alpha * x - sqrt_beta * n               v-prediction; stored to x0_state
 *   order 1:  x' = m1 * x - m2 * x0 + mn * eps
 *   order 2:  d  = m3 * x0 - m4 * x0_old
 *             x' = m1 * x - m2 * d  + mn * eps
 *   x' is rounded to fp16 when the latents are fp16; with mn == 0 the noise term is not evaluated at all (x' = m1 * x - m2 * ..).
 * - the rounding points of noise_pred.float(), the three CFG statements, CogVideoXDPMScheduler.step on .float() operands and
 * .to(float16).
 *
 * Errors: LKGD_E_NULL for a null noise_rows, latents or x0_state, and for a null eps with mn != 0; LKGD_E_SHAPE unless B, F, C, H,
 * W > 0, p == 2, H % p == W % p == 0, (C p p) % 8 == 0, ldn >= the row width, ldn % 8 == 0 (_t: and p_t == 2, F % p_t == 0), cfg in
 * {1, 2}, order in {1, 2}; LKGD_E_ALIGN unless the rows are 16 bytes and x0_state 4 bytes aligned.
 */
#ifndef LKGD_HIP_DIT_DPM_H
#define LKGD_HIP_DIT_DPM_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_dit_cfg_dpm_step(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, void* x0_state,
                          const void* eps, int32_t B, int32_t F, int32_t C, int32_t H, int32_t W, int32_t p, int32_t cfg,
                          int32_t order, float guidance, float sqrt_alpha, float sqrt_beta, float m1, float m2, float m3, float m4,
                          float mn, lkgd_stream_t stream);

int lkgd_dit_cfg_dpm_step_t(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, void* x0_state,
                            const void* eps, int32_t B, int32_t F, int32_t C, int32_t H, int32_t W, int32_t p, int32_t p_t,
                            int32_t cfg, int32_t order, float guidance, float sqrt_alpha, float sqrt_beta, float m1, float m2,
                            float m3, float m4, float mn, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
