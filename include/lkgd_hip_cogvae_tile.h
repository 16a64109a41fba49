/*
 * lkgd_hip_cogvae_tile.h - the seam operator the TILED encode and decode of the CogVideoX 3-D causal VAE add to the library
 * (lkgd_amd/cogvideox_vae.py; AutoencoderKLCogVideoX.tiled_decode / tiled_encode [EXT diffusers autoencoder_kl_cogvideox.py, PARITY
 * UNPINNED: diffusers is un-vendored and the reference tree only imports the class], switched on by `vae.enable_tiling()` at
 * inference/cli_demo.py:151-152 and finetune/trainer.py:156-159).  Same library, conventions, return codes and footprint contract as
 * lkgd_hip.h: raw pointers plus a stream, ONE launch, no allocation, no host sync, writes only inside `tile` and the crop window of
 * `out`, reads outside a logical window never influence a result.
 *
 * One kernel in two layouts.  A tile of the output (frames for the decode, moment rows for the encode) was computed alone; its first
 * rows are cross-faded with the last rows of the tile above it, its first columns with the last columns of the tile to its left, and
 * the part of it that no later tile covers is placed in the output.  diffusers does this with one `mul, mul, add, copy` quartet per
 * blended row or column and a `cat` per tile row (about 2 700 strided launches for one 480 x 720 decode); here it is one launch per
 * tile.  Per element (y, x) of the tile, every plane p alike:
 *
 *   ey = up   ? min(Yu, Yt, e_y) : 0          ex = left ? min(Xl, Xt, e_x) : 0
 *   v  = (y < ey) ? h( h( f(up[Yu - ey + y, x]) * f32(1 - y/ey) ) + h( f(tile[y, x]) * f32(y/ey) ) ) : tile[y, x]
 *   r  = (x < ex) ? h( h( f(left[y, Xl - ex + x]) * f32(1 - x/ex) ) + h( f(v) * f32(x/ex) ) )        : v
 *   tile[y, x] = r                                      (in place: the tile becomes its blended form, which ITS neighbours read)
 *   if (y < c_y && x < c_x)  out[y0 + y, x0 + x] = r
 *
 * h rounds to fp16 (nearest even), f widens to fp32.  1 - y/ey and y/ey are evaluated in DOUBLE and then narrowed to fp32 - what
 * ATen does with the Python scalars of `a * (1 - y / e) + b * (y / e)` against a half tensor - and each product is rounded to fp16
 * before the fp32 sum, which is rounded once more: the result equals torch's fp16 statements bit for bit (the source is compiled with
 * floating-point contraction off).  The vertical blend comes first, the horizontal blend acts on its result; both apply in the
 * corner.  `up` and `left` are the neighbours' ALREADY BLENDED tiles, whole and uncropped, so tiles are assembled in row-major order.
 *
 * ---- lkgd_cogvae_tile_blend_planar -----------------------------------------------------------------------------------------------
 * The decode's layout: P = B*C*T contiguous planes.
 *   tile  fp16 [P, Yt, Xt] contiguous, read and written
 *   up    fp16 [P, Yu, Xt] contiguous, or NULL (first tile row);   left  fp16 [P, Yt, Xl] contiguous, or NULL (first tile column)
 *   out   fp16 [P, Y, X]   contiguous; the window [y0, y0 + min(c_y, Yt)) x [x0, x0 + min(c_x, Xt)) of every plane is written
 * Memory-bound, no LDS: a thread owns 8 consecutive x of one row.  It moves them with 16-byte accesses where the operand allows:
 * `tile` and `up` when Xt % 8 == 0 and both are 16 bytes aligned; `left` when also Xl % 8 == 0 and ex % 8 == 0; `out` when also
 * X % 8 == 0, x0 % 8 == 0 and min(c_x, Xt) % 8 == 0 (the real geometries - 360 | 288 | 72 and 680 | 544 | 136 wide, and the 80 | 64 |
 * 16 of the tests - take this path everywhere).  An operand that fails its condition is moved with 2-byte accesses, the others keep
 * theirs; a last column chunk of fewer than 8 elements (Xt % 8 != 0) is always 2-byte.
 * LKGD_E_NULL for a null tile / out; LKGD_E_SHAPE for P, Yt, Xt, Y, X <= 0, Yu <= 0 with up, Xl <= 0 with left, e_y, e_x, c_y, c_x,
 * y0, x0 < 0, a crop window that leaves out (y0 + min(c_y, Yt) > Y or x0 + min(c_x, Xt) > X), P * Yt * ceil(Xt / 8) >= 2^38, or
 * `tile` overlapping up / left / out; LKGD_E_ALIGN unless every pointer is 2 bytes aligned.
 *
 * ---- lkgd_cogvae_tile_blend_rows -------------------------------------------------------------------------------------------------
 * The encode's layout: channels-last token rows, P = B*T images of rows (y, x), C channels each (the 2*16 moments of conv_out).
 *   tile  fp16 rows [P*Yt*Xt, C], row stride ldt >= C: row (p*Yt + y)*Xt + x, read and written
 *   up    fp16 rows [P*Yu*Xt, C], row stride ldu, or NULL;   left  fp16 rows [P*Yt*Xl, C], row stride ldl, or NULL
 *   out   fp16 rows [P*Y*X, C],   row stride ldo: row (p*Y + y0 + y)*X + x0 + x is written for y < min(c_y, Yt), x < min(c_x, Xt)
 * A thread owns 8 channels (16 bytes) of one row; consecutive threads walk a row's channels, then the next row.
 * LKGD_E_NULL for a null tile / out; LKGD_E_SHAPE as above and for C <= 0, C % 8 != 0, a row stride below C, P * Yt * Xt * C / 8
 * >= 2^38; LKGD_E_ALIGN unless every pointer is 16 bytes aligned and every row stride a multiple of 8.
 */
#ifndef LKGD_HIP_COGVAE_TILE_H
#define LKGD_HIP_COGVAE_TILE_H

#include "lkgd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lkgd_cogvae_tile_blend_planar(void* tile, const void* up, const void* left, void* out, int64_t P, int32_t Yt, int32_t Xt,
                                  int32_t Yu, int32_t Xl, int32_t Y, int32_t X, int32_t y0, int32_t x0, int32_t e_y, int32_t e_x,
                                  int32_t c_y, int32_t c_x, lkgd_stream_t stream);

int lkgd_cogvae_tile_blend_rows(void* tile, int32_t ldt, const void* up, int32_t ldu, const void* left, int32_t ldl, void* out,
                                int32_t ldo, int64_t P, int32_t C, int32_t Yt, int32_t Xt, int32_t Yu, int32_t Xl, int32_t Y, int32_t X,
                                int32_t y0, int32_t x0, int32_t e_y, int32_t e_x, int32_t c_y, int32_t c_x, lkgd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
