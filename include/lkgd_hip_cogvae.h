/*
 * lkgd_hip_cogvae.h - the latent-modulated norm of the CogVideoX 3-D causal VAE decoder (lkgd_amd/cogvideox_vae.py;
 * AutoencoderKLCogVideoX [EXT diffusers autoencoder_kl_cogvideox.py, PARITY UNPINNED: diffusers is un-vendored and the reference tree
 * only imports the class], reached from pipeline_cogvideox_image2video.py:430-435 `decode_latents`).  Same library, conventions, return
 * codes and footprint contract as lkgd_hip.h: raw pointers plus a stream, ONE launch, no allocation, no host sync, writes only inside
 * the output window, reads outside a logical window never influence a result.  The decoder's convolutions are lkgd_gemm_f16
 * (LKGD_A_CCONV3, LKGD_A_CONV3X3, plain).
 *
 * ---- lkgd_spatial_norm3d ---------------------------------------------------------------------------------------------------------
 * CogVideoXSpatialNorm3D:  norm_layer(f) * conv_y(zq') + conv_b(zq'),  zq' = the latent zq resized to f's (T, H, W) by nearest
 * interpolation (first frame apart when T is odd and above one), norm_layer = GroupNorm(32, C), conv_y / conv_b pointwise (1x1x1).
 * A pointwise convolution commutes with nearest upsampling, so the caller runs conv_y | conv_b ONCE on the latent grid (one plain GEMM,
 * N = 2C) and this kernel gathers its rows: the two C-channel full-resolution tensors of the diffusers form never exist.
 *   f      fp16 [B*T*H*W, C] token rows (b, t, Y, X), row stride ldf >= C
 *   stats  fp32 [B][32][2] = (mean, rstd) per (batch entry, group) over the entry's T*H*W rows (lkgd_groupnorm_stats /
 *          lkgd_groupnorm_stats_cols with rows_per_sample = T*H*W: the statistics span the frames of the chunk)
 *   gamma, beta  fp32 [C], the GroupNorm's affine
 *   yb     fp16 [B*Tz*h*w, 2C], row stride ldyb >= 2C: columns [0, C) = conv_y(zq), [C, 2C) = conv_b(zq) on the latent grid,
 *          h = H >> sh, w = W >> sh
 *   tmap   int32 [T]: latent frame of every frame of f (the host builds it; an entry outside [0, Tz) is clamped into it)
 *   out    fp16 rows of C channels, row stride ldo >= C: row r = (t*H + Y)*W + X of batch entry b goes to row b * out_batch_rows + r.
 *          out_batch_rows >= T*H*W - with `out` pointing behind the two context frames of a [B][T + 2][H*W] buffer and
 *          out_batch_rows = (T + 2)*H*W the rows land where the next LKGD_A_CCONV3 launch reads them, and no copy is needed
 *   out[b, r, c] = act( ((f - mean_g) * rstd_g * gamma_c + beta_c) * yb[src, c] + yb[src, C + c] ),
 *                  src = ((b*Tz + tmap[t])*h + (Y >> sh))*w + (X >> sh),  g = c / (C/32),  act = SiLU (act = 1) or identity (0)
 * fp32 arithmetic, one rounding.  Every thread moves 16 bytes of f and of out (8 channels of one row).  out must not overlap f.
 * LKGD_E_NULL for a null f / stats / gamma / beta / yb / tmap / out; LKGD_E_SHAPE for B, T, H, W, Tz <= 0, C <= 0 or C % 64 != 0,
 * sh outside [0, 3], H or W not a multiple of 1 << sh, ldf < C, ldo < C, ldyb < 2C, out_batch_rows < T*H*W, B*T*H*W or
 * B*out_batch_rows >= 2^31, act outside {0, 1}; LKGD_E_ALIGN unless f, yb and out are 16 bytes aligned with ldf, ldyb, ldo % 8 == 0,
 * gamma and beta 16 bytes, stats 8 bytes, tmap 4 bytes aligned.
 */
#ifndef LKGD_HIP_COGVAE_H
#define LKGD_HIP_COGVAE_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_spatial_norm3d(const void* f, int32_t ldf, const float* stats, const float* gamma, const float* beta, const void* yb,
                        int32_t ldyb, const int32_t* tmap, void* out, int32_t ldo, int64_t out_batch_rows, int32_t B, int32_t T,
                        int32_t H, int32_t W, int32_t C, int32_t Tz, int32_t sh, int32_t act, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
