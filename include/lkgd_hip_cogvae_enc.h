/*
 * lkgd_hip_cogvae_enc.h - the three operators the ENCODER of the CogVideoX 3-D causal VAE adds to the library
 * (lkgd_amd/cogvideox_vae.py; AutoencoderKLCogVideoX.encode [EXT diffusers autoencoder_kl_cogvideox.py, PARITY UNPINNED: diffusers is
 * un-vendored and the reference tree only imports the class], reached from pipeline_cogvideox_image2video.py:386-393 `prepare_latents`
 * and inference/cli_vae_demo.py:63).  Same library, conventions, return codes and footprint contract as lkgd_hip.h: raw pointers plus a
 * stream, ONE launch, no allocation, no host sync, writes only inside the output window, reads outside a logical window never
 * influence a result; fp32 arithmetic, one rounding.  The encoder's other launches are the GEMM of lkgd_hip.h section 1 - plain,
 * LKGD_A_CCONV3, LKGD_A_CONV3X3 with stride 2 and pad_off = 1 - and the GroupNorm statistics and apply passes of section 2.
 *
 * ---- lkgd_cogvae_pixel_taps ------------------------------------------------------------------------------------------------------
 * The A operand of conv_in, a causal 3x3x3 convolution over Cin <= 4 PIXEL channels: LKGD_A_CCONV3 needs Cin % 64 == 0, and padding
 * the pixels to 64 channels would make K = 1728 for 27*Cin <= 108 real taps.  This kernel writes the taps as rows of K = 128 instead;
 * one plain GEMM with K = 128, the weight repacked into the same k order, follows.
 *   x    fp16 [B, Cin, T, H, W], contiguous (the clip as the pipeline holds it)
 *   out  fp16 rows of 128 columns, row stride ldo >= 128: row ((b*Tc + tl)*H + y)*W + xx is output pixel (b, t0 + tl, y, xx), tl < Tc
 *   out[row, k] = x[b, c, max(t0 + tl + kt - 2, 0), y + ky - 1, xx + kx - 1]   for k = ((kt*3 + ky)*3 + kx)*Cin + c < 27*Cin,
 *                 zero where the pixel lies outside the image;  out[row, k] = 0 for 27*Cin <= k < 128.
 * The clamp at frame 0 is the replication of the first frame in front of the first chunk.  A later chunk (t0 >= 2) reads its two
 * context frames from the clip itself - for conv_in the clip IS the conv cache, so no cache and no context-prefixed buffer exist.
 * Every thread writes 16 bytes (8 columns of one row); the reads are 2-byte gathers from the planar clip (27*Cin per row, from L2).
 * LKGD_E_NULL for a null x / out; LKGD_E_SHAPE for B, T, H, W, Tc <= 0, Cin outside [1, 4], t0 < 0, t0 + Tc > T, ldo < 128,
 * B*Tc*H*W >= 2^31; LKGD_E_ALIGN unless out is 16 bytes aligned with ldo % 8 == 0 and x 2 bytes aligned.
 *
 * ---- lkgd_cogvae_time_pool -------------------------------------------------------------------------------------------------------
 * The `compress_time` half of CogVideoXDownsample3D (avg_pool1d(kernel 2, stride 2) along the frames, the FIRST frame apart when the
 * count is odd), on token rows; it runs before the stride-2 convolution, as in diffusers, and halves that convolution's rows.
 *   in   fp16 [B*T*HW, C] rows (b, t, s), row stride ldi >= C;   out  fp16 [B*To*HW, C] rows (b, j, s), row stride ldo >= C
 *   T even:  To = T/2,            out[b, j] = (in[b, 2j] + in[b, 2j+1]) / 2
 *   T odd:   To = 1 + (T-1)/2,    out[b, 0] = in[b, 0],  out[b, j] = (in[b, 2j-1] + in[b, 2j]) / 2 for j >= 1   (T = 1 stays 1)
 * The sum and the halving are fp32 (the halving is exact), one rounding to fp16.  Every thread moves 16 bytes (8 channels of one
 * output row).  `in` and `out` must not overlap.
 * LKGD_E_NULL for a null in / out; LKGD_E_SHAPE for B, T, HW, C <= 0, C % 8 != 0, ldi < C, ldo < C, B*T*HW >= 2^31, or overlapping
 * in / out row ranges; LKGD_E_ALIGN unless in and out are 16 bytes aligned with ldi, ldo % 8 == 0.
 *
 * ---- lkgd_cogvae_posterior -------------------------------------------------------------------------------------------------------
 * DiagonalGaussianDistribution of the moment rows conv_out leaves: the mean and, with a noise tensor, the scaled sample.
 *   mom     fp16 [B*T*h*w, >= 2*lc] rows (b, t, y, xx), row stride ldm >= 2*lc: columns [0, lc) the mean, [lc, 2*lc) the log-variance
 *   noise   fp16 [B, lc, T, h, w] contiguous, or NULL
 *   mean    fp16 [B, lc, T, h, w] contiguous:  mean[b, c, t, y, xx] = mom[row, c]
 *   sample  fp16 [B, lc, T, h, w] contiguous (read only when noise != NULL):
 *           sample = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise)
 * noise == NULL writes the mean only (`mode()`); `scale` folds the scaling factor `prepare_latents` multiplies by.  A thread reads
 * 16 bytes of the mean and of the log-variance columns of one row; adjacent lanes hold adjacent rows, so the 2-byte planar accesses
 * of a wave are contiguous.
 * LKGD_E_NULL for a null mom / mean, or noise without sample; LKGD_E_SHAPE for B, T, h, w <= 0, lc <= 0 or lc % 8 != 0,
 * ldm < 2*lc, B*T*h*w*lc >= 2^31, a scale that is not finite; LKGD_E_ALIGN unless mom is 16 bytes aligned with ldm % 8 == 0 and
 * noise, mean, sample 2 bytes aligned.
 */
#ifndef LKGD_HIP_COGVAE_ENC_H
#define LKGD_HIP_COGVAE_ENC_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_cogvae_pixel_taps(const void* x, void* out, int32_t ldo, int32_t B, int32_t Cin, int32_t T, int32_t H, int32_t W,
                           int32_t t0, int32_t Tc, lkgd_stream_t stream);

int lkgd_cogvae_time_pool(const void* in, int32_t ldi, void* out, int32_t ldo, int32_t B, int32_t T, int64_t HW, int32_t C,
                          lkgd_stream_t stream);

int lkgd_cogvae_posterior(const void* mom, int32_t ldm, const void* noise, void* mean, void* sample, float scale, int32_t B,
                          int32_t lc, int32_t T, int32_t h, int32_t w, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
