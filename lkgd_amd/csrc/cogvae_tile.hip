// The seam operator of the tiled CogVideoX VAE (include/lkgd_hip_cogvae_tile.h): cross-fade a tile's first rows / columns with the
// last rows / columns of its upper / left neighbour, in place, and place the tile's crop in the output - one launch per tile, planes
// (decode) or channels-last rows (encode).  Memory-bound, no LDS, no reuse: every byte is moved once.
#include "common.h"

#include "../../include/lkgd_hip_cogvae_tile.h"

// each product is rounded to fp16 before the sum (torch's `a * s + b * t` on half tensors): nothing here may become an fma
#pragma clang fp contract(off)

// the pair of fp32 weights of blend step i of e: the Python doubles 1 - i/e and i/e, narrowed
struct blend_w { float a, b; };
__device__ __forceinline__ blend_w blend_weights(int i, int e) {
  const double q = (double)i / (double)e;
  blend_w w;
  w.a = (float)(1.0 - q);
  w.b = (float)q;
  return w;
}
__device__ __forceinline__ half_t blend1(half_t nb, half_t own, blend_w w) {
  const half_t pa = (half_t)((float)nb * w.a);
  const half_t pb = (half_t)((float)own * w.b);
  return (half_t)((float)pa + (float)pb);
}

// ---- lkgd_cogvae_tile_blend_planar ---------------------------------------------------------------------------------------------------
// One thread = 8 consecutive x of one row of one plane; consecutive threads walk the row, then the next row: a wave's 16-byte accesses
// to tile / up / out are contiguous runs.  vt / vl / vo (wave-uniform) say which operand takes 16-byte accesses.
__global__ __launch_bounds__(256) void tile_blend_planar_kernel(half_t* __restrict__ tile, const half_t* __restrict__ up,
                                                                const half_t* __restrict__ left, half_t* __restrict__ out,
                                                                unsigned long long chunks, int X8, int Yt, int Xt, int Yu, int Xl, int Y,
                                                                int X, int y0, int x0, int ey, int ex, int cy, int cx, int vt, int vl,
                                                                int vo) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (i >= chunks) return;
  const unsigned long long row = i / (unsigned)X8;
  const int xc = (int)(i - row * (unsigned)X8) << 3;
  const unsigned long long p = row / (unsigned)Yt;
  const int y = (int)(row - p * (unsigned)Yt);
  const int n = Xt - xc < 8 ? Xt - xc : 8;
  half_t* trow = tile + row * (unsigned)Xt + xc;
  half8_t v;
  if (vt) {
    v = *(const half8_t*)trow;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = e < n ? trow[e] : (half_t)0.0f;
  }
  if (y < ey) {                                                     // ey = 0 without an upper neighbour
    const half_t* urow = up + (p * (unsigned)Yu + (unsigned)(Yu - ey + y)) * (unsigned)Xt + xc;
    half8_t u;
    if (vt) {
      u = *(const half8_t*)urow;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) u[e] = e < n ? urow[e] : (half_t)0.0f;
    }
    const blend_w w = blend_weights(y, ey);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = blend1(u[e], v[e], w);
  }
  if (xc < ex) {                                                    // ex = 0 without a left neighbour
    const half_t* lrow = left + (p * (unsigned)Yt + (unsigned)y) * (unsigned)Xl + (Xl - ex + xc);
    if (vl) {                                                       // ex % 8 == 0: the whole chunk lies inside the blend
      const half8_t l = *(const half8_t*)lrow;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = blend1(l[e], v[e], blend_weights(xc + e, ex));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < n && xc + e < ex) v[e] = blend1(lrow[e], v[e], blend_weights(xc + e, ex));
    }
  }
  if (vt) {
    *(half8_t*)trow = v;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < n) trow[e] = v[e];
  }
  if (y < cy && xc < cx) {
    half_t* orow = out + (p * (unsigned)Y + (unsigned)(y0 + y)) * (unsigned)X + (x0 + xc);
    if (vo) {                                                       // cx % 8 == 0 and Xt % 8 == 0: the whole chunk lies inside the crop
      *(half8_t*)orow = v;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < n && xc + e < cx) orow[e] = v[e];
    }
  }
}

static inline bool spans_meet(const void* a, unsigned long long abytes, const void* b, unsigned long long bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + bbytes && b0 < a0 + abytes;
}

extern "C" int lkgd_cogvae_tile_blend_planar(void* tile, const void* up, const void* left, void* out, int64_t P, int32_t Yt, int32_t Xt,
                                             int32_t Yu, int32_t Xl, int32_t Y, int32_t X, int32_t y0, int32_t x0, int32_t e_y,
                                             int32_t e_x, int32_t c_y, int32_t c_x, lkgd_stream_t stream) {
  if (!tile || !out) return LKGD_E_NULL;
  if (P <= 0 || Yt <= 0 || Xt <= 0 || Y <= 0 || X <= 0 || (up && Yu <= 0) || (left && Xl <= 0)) return LKGD_E_SHAPE;
  if (e_y < 0 || e_x < 0 || c_y < 0 || c_x < 0 || y0 < 0 || x0 < 0) return LKGD_E_SHAPE;
  const int cy = c_y < Yt ? c_y : Yt, cx = c_x < Xt ? c_x : Xt;
  if ((long long)y0 + cy > Y || (long long)x0 + cx > X) return LKGD_E_SHAPE;
  int ey = 0, ex = 0;
  if (up) { ey = e_y < Yt ? e_y : Yt; ey = ey < Yu ? ey : Yu; }
  if (left) { ex = e_x < Xt ? e_x : Xt; ex = ex < Xl ? ex : Xl; }
  const int X8 = (Xt + 7) / 8;
  if (P >= (1LL << 38) || (long long)P * Yt >= (1LL << 38) || (long long)P * Yt * X8 >= (1LL << 38)) return LKGD_E_SHAPE;
  if ((long long)P * Y >= (1LL << 40) / X || (up && (long long)P * Yu >= (1LL << 40) / Xt) || (left && (long long)P * Yt >= (1LL << 40) / Xl))
    return LKGD_E_SHAPE;
  const unsigned long long tb = (unsigned long long)P * Yt * Xt * 2;
  if (spans_meet(tile, tb, out, (unsigned long long)P * Y * X * 2)) return LKGD_E_SHAPE;
  if (up && spans_meet(tile, tb, up, (unsigned long long)P * Yu * Xt * 2)) return LKGD_E_SHAPE;
  if (left && spans_meet(tile, tb, left, (unsigned long long)P * Yt * Xl * 2)) return LKGD_E_SHAPE;
  if (((uintptr_t)tile | (uintptr_t)up | (uintptr_t)left | (uintptr_t)out) & 1u) return LKGD_E_ALIGN;
  const int vt = Xt % 8 == 0 && aligned16(tile) && (!up || aligned16(up));
  const int vl = vt && left && Xl % 8 == 0 && ex % 8 == 0 && aligned16(left);
  const int vo = vt && X % 8 == 0 && x0 % 8 == 0 && cx % 8 == 0 && aligned16(out);
  const unsigned long long chunks = (unsigned long long)P * Yt * X8;
  hipLaunchKernelGGL(tile_blend_planar_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (half_t*)tile,
                     (const half_t*)up, (const half_t*)left, (half_t*)out, chunks, X8, Yt, Xt, Yu, Xl, Y, X, y0, x0, ey, ex, cy, cx, vt,
                     vl, vo);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// ---- lkgd_cogvae_tile_blend_rows -----------------------------------------------------------------------------------------------------
// One thread = 8 channels (16 bytes) of one token row; consecutive threads walk a row's channels, then the next row.
__global__ __launch_bounds__(256) void tile_blend_rows_kernel(half_t* __restrict__ tile, int ldt, const half_t* __restrict__ up, int ldu,
                                                              const half_t* __restrict__ left, int ldl, half_t* __restrict__ out, int ldo,
                                                              unsigned long long chunks, int C8, int Yt, int Xt, int Yu, int Xl, int Y,
                                                              int X, int y0, int x0, int ey, int ex, int cy, int cx) {
  const unsigned long long i = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (i >= chunks) return;
  const unsigned long long row = i / (unsigned)C8;                   // (p*Yt + y)*Xt + x
  const int c = (int)(i - row * (unsigned)C8) << 3;
  const unsigned long long py = row / (unsigned)Xt;                  // p*Yt + y
  const int x = (int)(row - py * (unsigned)Xt);
  const unsigned long long p = py / (unsigned)Yt;
  const int y = (int)(py - p * (unsigned)Yt);
  half_t* tp = tile + row * (unsigned)ldt + c;
  half8_t v = *(const half8_t*)tp;
  if (y < ey) {
    const half8_t u = *(const half8_t*)(up + ((p * (unsigned)Yu + (unsigned)(Yu - ey + y)) * (unsigned)Xt + (unsigned)x) * (unsigned)ldu + c);
    const blend_w w = blend_weights(y, ey);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = blend1(u[e], v[e], w);
  }
  if (x < ex) {
    const half8_t l = *(const half8_t*)(left + (py * (unsigned)Xl + (unsigned)(Xl - ex + x)) * (unsigned)ldl + c);
    const blend_w w = blend_weights(x, ex);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = blend1(l[e], v[e], w);
  }
  *(half8_t*)tp = v;
  if (y < cy && x < cx)
    *(half8_t*)(out + ((p * (unsigned)Y + (unsigned)(y0 + y)) * (unsigned)X + (unsigned)(x0 + x)) * (unsigned)ldo + c) = v;
}

extern "C" int lkgd_cogvae_tile_blend_rows(void* tile, int32_t ldt, const void* up, int32_t ldu, const void* left, int32_t ldl, void* out,
                                           int32_t ldo, int64_t P, int32_t C, int32_t Yt, int32_t Xt, int32_t Yu, int32_t Xl, int32_t Y,
                                           int32_t X, int32_t y0, int32_t x0, int32_t e_y, int32_t e_x, int32_t c_y, int32_t c_x,
                                           lkgd_stream_t stream) {
  if (!tile || !out) return LKGD_E_NULL;
  if (P <= 0 || C <= 0 || C % 8 || Yt <= 0 || Xt <= 0 || Y <= 0 || X <= 0 || (up && Yu <= 0) || (left && Xl <= 0)) return LKGD_E_SHAPE;
  if (ldt < C || ldo < C || (up && ldu < C) || (left && ldl < C)) return LKGD_E_SHAPE;
  if (e_y < 0 || e_x < 0 || c_y < 0 || c_x < 0 || y0 < 0 || x0 < 0) return LKGD_E_SHAPE;
  const int cy = c_y < Yt ? c_y : Yt, cx = c_x < Xt ? c_x : Xt;
  if ((long long)y0 + cy > Y || (long long)x0 + cx > X) return LKGD_E_SHAPE;
  int ey = 0, ex = 0;
  if (up) { ey = e_y < Yt ? e_y : Yt; ey = ey < Yu ? ey : Yu; }
  if (left) { ex = e_x < Xt ? e_x : Xt; ex = ex < Xl ? ex : Xl; }
  const int C8 = C / 8;
  if (P >= (1LL << 38) || (long long)P * Yt >= (1LL << 38) || (long long)P * Yt * Xt >= (1LL << 38) / C8) return LKGD_E_SHAPE;
  if ((long long)P * Y >= (1LL << 38) / X || (up && (long long)P * Yu >= (1LL << 38) / Xt) || (left && (long long)P * Yt >= (1LL << 38) / Xl))
    return LKGD_E_SHAPE;
  const unsigned long long trows = (unsigned long long)P * Yt * Xt;
  const unsigned long long tb = ((trows - 1) * ldt + C) * 2;
  if (spans_meet(tile, tb, out, (((unsigned long long)P * Y * X - 1) * ldo + C) * 2)) return LKGD_E_SHAPE;
  if (up && spans_meet(tile, tb, up, (((unsigned long long)P * Yu * Xt - 1) * ldu + C) * 2)) return LKGD_E_SHAPE;
  if (left && spans_meet(tile, tb, left, (((unsigned long long)P * Yt * Xl - 1) * ldl + C) * 2)) return LKGD_E_SHAPE;
  if (!aligned16(tile) || !aligned16(out) || (up && !aligned16(up)) || (left && !aligned16(left))) return LKGD_E_ALIGN;
  if (ldt % 8 || ldo % 8 || (up && ldu % 8) || (left && ldl % 8)) return LKGD_E_ALIGN;
  const unsigned long long chunks = trows * C8;
  hipLaunchKernelGGL(tile_blend_rows_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (half_t*)tile, ldt,
                     (const half_t*)up, ldu, (const half_t*)left, ldl, (half_t*)out, ldo, chunks, C8, Yt, Xt, Yu, Xl, Y, X, y0, x0, ey, ex,
                     cy, cx);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
