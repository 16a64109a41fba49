/*
 * lkgd_hip_video.h - frames in and frames out of the CogVideoX image-to-video pipeline (lkgd_amd/pipeline_cogvideox.py,
 * lkgd_amd/video_processor.py): the two calls of diffusers' VideoProcessor the reference's `__call__` makes either side of the model
 * [EXT diffusers video_processor.py / image_processor.py, PARITY UNPINNED: diffusers is un-vendored and the reference tree only imports
 * the class].  Same library, conventions, return codes and footprint contract as lkgd_hip.h: raw pointers plus a stream, ONE launch, no
 * allocation, no host sync, writes only inside `out`, reads only inside the input.  Every tensor is contiguous.  Both kernels are
 * memory-bound, use no LDS and move every byte once; indices are 64-bit; the source is compiled with floating-point contraction off.
 *
 * ---- lkgd_video_postprocess ------------------------------------------------------------------------------------------------------
 * `video_processor.postprocess_video(video, output_type)` (pipeline_cogvideox_image2video.py:909) on the decoded clip.
 *   x    fp16 [B, C, T, H, W], 1 <= C <= 4 (planes: what the VAE decoder leaves)
 *   d(v) = clamp(h(h(f(v) / 2) + 0.5), 0, 1)          h rounds to fp16 (nearest even), f widens to fp32: ATen's `(images / 2 +
 *                                                     0.5).clamp(0, 1)` on a half tensor, two roundings
 *   mode LKGD_VIDEO_U8  (0)  out uint8 [B, T, H, W, C] = (uint8) rint(f(d) * 255.0f)       output_type "pil": numpy_to_pil's
 *                            `(images * 255).round().astype("uint8")` on pt_to_numpy's fp32; an fp32 multiply, rint half-to-even
 *   mode LKGD_VIDEO_F32 (1)  out fp32  [B, T, H, W, C] = f(d)                               output_type "np"
 *   mode LKGD_VIDEO_F16 (2)  out fp16  [B, T, C, H, W] = d                                  output_type "pt"
 * NaN: d(NaN) = NaN (the clamp's comparisons are false for it, as torch.clamp propagates it); modes F32 and F16 store that NaN, mode
 * U8 stores 0.  -inf gives 0, +inf gives 1 / 255.
 * The interleaved modes are a 1-D problem: per batch entry, C planes of L = T*H*W values become L pixels of C values.  Wide path: a
 * thread owns 8 consecutive pixels - one 16-byte load from each plane, 8*C consecutive outputs (U8: 8-byte stores, F32: 16-byte
 * stores), so a wave writes one contiguous run.  It is taken when L % 8 == 0 (then every plane starts 16 bytes aligned), x is 16
 * bytes aligned and out is 8 (U8) / 16 (F32) bytes aligned.  Otherwise the whole launch takes the narrow path: a thread owns one
 * pixel, C 2-byte loads and C stores.  The choice is made once per launch, on the host: no launch mixes the paths, there is no tail.
 * Mode F16 permutes planes of H*W values; its wide path (a thread owns 8 consecutive values of one plane) needs H*W % 8 == 0 and both
 * pointers 16 bytes aligned, its narrow path owns one value.
 * LKGD_E_NULL for a null x / out; LKGD_E_SHAPE for B, C, T, H, W <= 0, C > 4 or B*C*T*H*W >= 2^38; LKGD_E_MODE for a mode outside
 * 0 .. 2; LKGD_E_ALIGN unless x is 2 bytes aligned and out aligned to its element.
 *
 * ---- lkgd_image_preprocess -------------------------------------------------------------------------------------------------------
 * `video_processor.preprocess(image, height, width)` (:788) behind PIL's own resize: pil_to_numpy -> numpy_to_pt -> normalize, and
 * the `.to(dtype=prompt_embeds.dtype)` that follows it at :789.
 *   u    uint8 [N, H, W, C], 1 <= C <= 4 (np.asarray of the resized PIL images, stacked)
 *   out  fp16  [N, C, H, W] = h((f(u) / 255.0f) * 2.0f - 1.0f)     the division correctly rounded (IEEE), each step in fp32
 * Wide path (H*W % 8 == 0, u 8 bytes and out 16 bytes aligned): a thread owns 8 consecutive pixels - 8*C consecutive bytes in, one
 * 16-byte store to each plane.  Otherwise one pixel per thread.
 * LKGD_E_NULL for a null u / out; LKGD_E_SHAPE for N, H, W, C <= 0, C > 4 or N*C*H*W >= 2^38; LKGD_E_ALIGN unless out is 2 bytes aligned.
 */
#ifndef LKGD_HIP_VIDEO_H
#define LKGD_HIP_VIDEO_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LKGD_VIDEO_U8 = 0, LKGD_VIDEO_F32 = 1, LKGD_VIDEO_F16 = 2 };

int lkgd_video_postprocess(const void* x, void* out, int32_t mode, int32_t B, int32_t C, int32_t T, int32_t H, int32_t W,
                           lkgd_stream_t stream);

int lkgd_image_preprocess(const void* u, void* out, int32_t N, int32_t H, int32_t W, int32_t C, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
