// Loop glue of the CogVideoX DiT sampling loop (include/lkgd_hip_dit_loop.h; pipeline_cogvideox_image2video.py:829-885): the
// patch rows of the embedding GEMM straight from the latents and the image latents, and CFG combine + DDIM update straight from
// proj_out's token rows into the latents.  Both HBM/latency-bound.  A token row holds p x p = 4 pixels of every channel, channel
// major: one thread moves one 16-byte piece of a row = 2 channels x (py, px).  Lanes run along x, so the px pairs of neighbouring
// patches are one contiguous run of a latent plane's line; the grid rule is prepare_input_kernel's (elementwise.hip).
// The temporal-patch pair (include/lkgd_hip_dit_tpatch.h, CogVideoX 1.5: p_t = 2) is the same two kernels instantiated with T3: a
// piece is then ONE channel x (pt, py, px), its four 2-element runs two frames x two lines apart instead of two channels x two lines.
// The DPM-Solver++ step (include/lkgd_hip_dit_dpm.h) is the step kernel once more with the other scheduler's statements after the
// shared CFG combine and x0: it also reads the noise and reads / writes the fp32 x0 state at the latents' own element offsets.
#include <type_traits>

#include "common.h"
#include "../../include/lkgd_hip_dit_loop.h"
#include "../../include/lkgd_hip_dit_tpatch.h"
#include "../../include/lkgd_hip_dit_dpm.h"

static unsigned dit_grid_for(long long work_items, int per_block) {
  long long g = (work_items + per_block - 1) / per_block;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// piece i -> (x, q, y, bf): x fastest, then the piece q of the row, then the patch line y, then b * F + f
struct dit_piece { int x, q, y; long long bf; };
__device__ __forceinline__ dit_piece dit_piece_of(long long i, int w, int h, int pieces) {
  dit_piece d;
  d.x = (int)(i % w);
  const long long t1 = i / w;
  d.q = (int)(t1 % pieces);
  const long long t2 = t1 / pieces;
  d.y = (int)(t2 % h);
  d.bf = t2 / h;
  return d;
}

// where a piece's 2 x 2 runs of (px, px + 1) start in [.., C, H, W] planes, and the stride between its two outer runs.  2-D patches
// (T3 = false): piece q = the channels 2q, 2q + 1 of frame bf, runs (cc, py).  Temporal patches (T3 = true, p_t = 2): piece q = channel
// q of the frames 2 bf, 2 bf + 1, runs (pt, py) - column ((c p_t + pt) p + py) p + px of a row
template <bool T3>
__device__ __forceinline__ long long dit_piece_planes(long long bf, int c, int C, long long HW, long long& outer) {
  outer = T3 ? C * HW : HW;
  return ((T3 ? 2 * bf : bf) * C + c) * HW;
}

template <typename T>
__device__ __forceinline__ void dit_gather(const T* __restrict__ src0, long long outer, int W, half8_t& o) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      const T* src = src0 + a * outer + (long long)py * W;
      o[a * 4 + py * 2] = (half_t)src[0];
      o[a * 4 + py * 2 + 1] = (half_t)src[1];
    }
}

// ---- torch.cat([latents.half(), image_latents], 2) -> patch rows [B F h w, (c, py, px)] (T3: [B F/2 h w, (c, pt, py, px)], bf = b F/2 +
// ft); C2 = channels of a row (C or 2 C)
template <typename LT, bool T3>
__global__ __launch_bounds__(256) void dit_patch_rows_kernel(const LT* __restrict__ latents, const half_t* __restrict__ image_latents,
                                                             int C, int C2, int H, int W, long long total,
                                                             half_t* __restrict__ out, int ldp) {
  const int h = H / 2, w = W / 2, pieces = T3 ? C2 : C2 / 2;
  const long long HW = (long long)H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const dit_piece d = dit_piece_of(i, w, h, pieces);
    const int c0 = T3 ? d.q : 2 * d.q;    // 2-D: C is even, a piece never straddles the two tensors
    const long long at = (long long)2 * d.y * W + 2 * d.x;
    long long outer;
    half8_t o;
    if (c0 < C) dit_gather(latents + dit_piece_planes<T3>(d.bf, c0, C, HW, outer) + at, outer, W, o);
    else dit_gather(image_latents + dit_piece_planes<T3>(d.bf, c0 - C, C, HW, outer) + at, outer, W, o);
    *(half8_t*)(out + ((d.bf * h + d.y) * w + d.x) * ldp + d.q * 8) = o;
  }
}

// ---- one element of a step: the reference's fp32 statements, each operation rounded (ATen runs them as separate kernels).  The CFG
// combine and the v-prediction x0 are the same statements in both schedulers' steps
__device__ __forceinline__ float cfg_combine(float g, int cfg, float u, float c) {
#pragma clang fp contract(off)
  float n = u;
  if (cfg == 2) {
    const float diff = c - u;
    const float gd = g * diff;
    n = u + gd;
  }
  return n;
}
__device__ __forceinline__ float vpred_x0(float sa, float sb, float x, float n) {
#pragma clang fp contract(off)
  const float sx = sa * x;
  const float sn = sb * n;
  return sx - sn;
}

struct ddim_t { float g, a, b, sa, sb; };
__device__ __forceinline__ float ddim_advance(const ddim_t& k, int cfg, float u, float c, float x) {
#pragma clang fp contract(off)
  const float x0 = vpred_x0(k.sa, k.sb, x, cfg_combine(k.g, cfg, u, c));
  const float ax = k.a * x;
  const float bx = k.b * x0;
  return ax + bx;
}

// DPM-Solver++ (SDE, 2M; include/lkgd_hip_dit_dpm.h): ``x0_old`` is the previous step's x0 (used when order == 2), ``x0_out`` this
// step's; ``noisy`` false (mn == 0): the noise term is no statement at all
struct dpm_t { float g, sa, sb, m1, m2, m3, m4, mn; };
__device__ __forceinline__ float dpm_advance(const dpm_t& k, int cfg, int order, bool noisy, float u, float c, float x, float eps,
                                             float x0_old, float& x0_out) {
#pragma clang fp contract(off)
  const float x0 = vpred_x0(k.sa, k.sb, x, cfg_combine(k.g, cfg, u, c));
  x0_out = x0;
  float d = x0;
  if (order == 2) {
    const float d3 = k.m3 * x0;
    const float d4 = k.m4 * x0_old;
    d = d3 - d4;
  }
  const float ax = k.m1 * x;
  const float bd = k.m2 * d;
  float r = ax - bd;
  if (noisy) {
    const float ne = k.mn * eps;
    r = r + ne;
  }
  return r;
}

template <typename LT, bool T3>
__global__ __launch_bounds__(256) void dit_cfg_ddim_kernel(const half_t* __restrict__ noise, int ldn, LT* __restrict__ latents,
                                                           int C, int H, int W, int cfg, long long cond_rows, ddim_t k,
                                                           long long total) {
  const int h = H / 2, w = W / 2, pieces = T3 ? C : C / 2;
  const long long HW = (long long)H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const dit_piece d = dit_piece_of(i, w, h, pieces);
    const long long row = (d.bf * h + d.y) * w + d.x;
    const half8_t u = *(const half8_t*)(noise + row * ldn + d.q * 8);
    half8_t c = u;
    if (cfg == 2) c = *(const half8_t*)(noise + (row + cond_rows) * ldn + d.q * 8);
    long long outer;
    LT* at = latents + dit_piece_planes<T3>(d.bf, T3 ? d.q : 2 * d.q, C, HW, outer) + (long long)2 * d.y * W + 2 * d.x;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      LT* px = at + (e >> 2) * outer + (long long)((e >> 1) & 1) * W + (e & 1);
      *px = (LT)ddim_advance(k, cfg, (float)u[e], (float)c[e], (float)*px);
    }
  }
}

// eps == nullptr <=> mn == 0 (the host passes it so): the noise term is then no statement at all.  A thread reads x0_state's elements
// of its piece (order == 2 only) before it writes them, and no other thread touches them
template <typename LT, bool T3>
__global__ __launch_bounds__(256) void dit_cfg_dpm_kernel(const half_t* __restrict__ noise, int ldn, LT* __restrict__ latents,
                                                          float* __restrict__ x0_state, const LT* __restrict__ eps, int C, int H, int W,
                                                          int cfg, int order, long long cond_rows, dpm_t k, long long total) {
  const int h = H / 2, w = W / 2, pieces = T3 ? C : C / 2;
  const long long HW = (long long)H * W;
  const bool noisy = eps != nullptr;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const dit_piece d = dit_piece_of(i, w, h, pieces);
    const long long row = (d.bf * h + d.y) * w + d.x;
    const half8_t u = *(const half8_t*)(noise + row * ldn + d.q * 8);
    half8_t c = u;
    if (cfg == 2) c = *(const half8_t*)(noise + (row + cond_rows) * ldn + d.q * 8);
    long long outer;
    const long long at = dit_piece_planes<T3>(d.bf, T3 ? d.q : 2 * d.q, C, HW, outer) + (long long)2 * d.y * W + 2 * d.x;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const long long o = at + (e >> 2) * outer + (long long)((e >> 1) & 1) * W + (e & 1);
      const float old = order == 2 ? x0_state[o] : 0.f;
      const float ep = noisy ? (float)eps[o] : 0.f;
      float x0;
      latents[o] = (LT)dpm_advance(k, cfg, order, noisy, (float)u[e], (float)c[e], (float)latents[o], ep, old, x0);
      x0_state[o] = x0;
    }
  }
}

// T3: the temporal-patch pair (include/lkgd_hip_dit_tpatch.h): a row spans p_t = 2 latent frames, a 16-byte piece is one channel's
// (pt, py, px).  ``width`` = the elements of a row, refused before anything narrows it to int32
template <bool T3>
static int dit_shape_ok(int32_t B, int32_t F, int32_t C, int32_t H, int32_t W, int32_t p, int32_t p_t, long long width, int32_t ld) {
  if (width > 0x7fffffffll || (T3 && (p_t != 2 || F <= 0 || F % p_t))) return 0;
  if (B <= 0 || F <= 0 || C <= 0 || H <= 0 || W <= 0 || p != 2) return 0;
  if (H % p || W % p || (C * p * p) % 8) return 0;
  return ld >= width && ld % 8 == 0;
}
template <typename Launch>
static int dit_launch_typed(int32_t is_f32, Launch&& launch) {
  if (is_f32) launch((float*)nullptr);
  else launch((half_t*)nullptr);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

template <bool T3>
static int dit_patch_rows_host(const void* latents, int32_t latents_is_f32, const void* image_latents, int32_t B, int32_t F, int32_t C,
                               int32_t H, int32_t W, int32_t p, int32_t p_t, void* rows_out, int32_t ldp, lkgd_stream_t stream) {
  if (!latents || !rows_out) return LKGD_E_NULL;
  const long long C2 = image_latents ? 2ll * C : C;
  if (!dit_shape_ok<T3>(B, F, C, H, W, p, p_t, C2 * (T3 ? 8 : 4), ldp)) return LKGD_E_SHAPE;
  if (!aligned16(rows_out)) return LKGD_E_ALIGN;
  const long long total = (long long)B * (T3 ? F / 2 : F) * (H / 2) * (W / 2) * (T3 ? C2 : C2 / 2);
  return dit_launch_typed(latents_is_f32, [&](auto* tag) {
    using LT = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL((dit_patch_rows_kernel<LT, T3>), dim3(dit_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const LT*)latents, (const half_t*)image_latents, C, (int)C2, H, W, total, (half_t*)rows_out, ldp);
  });
}

template <bool T3>
static int dit_cfg_ddim_host(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, int32_t B, int32_t F,
                             int32_t C, int32_t H, int32_t W, int32_t p, int32_t p_t, int32_t cfg, float guidance, float a, float b,
                             float sqrt_alpha, float sqrt_beta, lkgd_stream_t stream) {
  if (!noise_rows || !latents) return LKGD_E_NULL;
  if (!dit_shape_ok<T3>(B, F, C, H, W, p, p_t, (T3 ? 8ll : 4ll) * C, ldn) || (cfg != 1 && cfg != 2)) return LKGD_E_SHAPE;
  if (!aligned16(noise_rows)) return LKGD_E_ALIGN;
  const long long rows = (long long)B * (T3 ? F / 2 : F) * (H / 2) * (W / 2);
  const long long total = rows * (T3 ? C : C / 2);
  const ddim_t k = {guidance, a, b, sqrt_alpha, sqrt_beta};
  return dit_launch_typed(latents_is_f32, [&](auto* tag) {
    using LT = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL((dit_cfg_ddim_kernel<LT, T3>), dim3(dit_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)noise_rows, ldn, (LT*)latents, C, H, W, cfg, rows, k, total);
  });
}

template <bool T3>
static int dit_cfg_dpm_host(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, void* x0_state, const void* eps,
                            int32_t B, int32_t F, int32_t C, int32_t H, int32_t W, int32_t p, int32_t p_t, int32_t cfg, int32_t order,
                            const dpm_t& k, lkgd_stream_t stream) {
  if (!noise_rows || !latents || !x0_state || (!eps && k.mn != 0.f)) return LKGD_E_NULL;
  if (!dit_shape_ok<T3>(B, F, C, H, W, p, p_t, (T3 ? 8ll : 4ll) * C, ldn) || (cfg != 1 && cfg != 2) || (order != 1 && order != 2))
    return LKGD_E_SHAPE;
  if (!aligned16(noise_rows) || ((uintptr_t)x0_state & 3)) return LKGD_E_ALIGN;
  const long long rows = (long long)B * (T3 ? F / 2 : F) * (H / 2) * (W / 2);
  const long long total = rows * (T3 ? C : C / 2);
  const void* noise_term = k.mn != 0.f ? eps : nullptr;      // mn == 0: eps is never read, even when given
  return dit_launch_typed(latents_is_f32, [&](auto* tag) {
    using LT = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL((dit_cfg_dpm_kernel<LT, T3>), dim3(dit_grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)noise_rows, ldn, (LT*)latents, (float*)x0_state, (const LT*)noise_term, C, H, W, cfg, order, rows,
                       k, total);
  });
}

extern "C" int lkgd_dit_patch_rows(const void* latents, int32_t latents_is_f32, const void* image_latents, int32_t B, int32_t F,
                                   int32_t C, int32_t H, int32_t W, int32_t p, void* rows_out, int32_t ldp, lkgd_stream_t stream) {
  return dit_patch_rows_host<false>(latents, latents_is_f32, image_latents, B, F, C, H, W, p, 0, rows_out, ldp, stream);
}

extern "C" int lkgd_dit_cfg_ddim_step(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, int32_t B,
                                      int32_t F, int32_t C, int32_t H, int32_t W, int32_t p, int32_t cfg, float guidance, float a,
                                      float b, float sqrt_alpha, float sqrt_beta, lkgd_stream_t stream) {
  return dit_cfg_ddim_host<false>(noise_rows, ldn, latents, latents_is_f32, B, F, C, H, W, p, 0, cfg, guidance, a, b, sqrt_alpha,
                                  sqrt_beta, stream);
}

extern "C" int lkgd_dit_patch_rows_t(const void* latents, int32_t latents_is_f32, const void* image_latents, int32_t B, int32_t F,
                                     int32_t C, int32_t H, int32_t W, int32_t p, int32_t p_t, void* rows_out, int32_t ldp,
                                     lkgd_stream_t stream) {
  return dit_patch_rows_host<true>(latents, latents_is_f32, image_latents, B, F, C, H, W, p, p_t, rows_out, ldp, stream);
}

extern "C" int lkgd_dit_cfg_ddim_step_t(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, int32_t B,
                                        int32_t F, int32_t C, int32_t H, int32_t W, int32_t p, int32_t p_t, int32_t cfg,
                                        float guidance, float a, float b, float sqrt_alpha, float sqrt_beta, lkgd_stream_t stream) {
  return dit_cfg_ddim_host<true>(noise_rows, ldn, latents, latents_is_f32, B, F, C, H, W, p, p_t, cfg, guidance, a, b, sqrt_alpha,
                                 sqrt_beta, stream);
}

extern "C" int lkgd_dit_cfg_dpm_step(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, void* x0_state,
                                     const void* eps, int32_t B, int32_t F, int32_t C, int32_t H, int32_t W, int32_t p, int32_t cfg,
                                     int32_t order, float guidance, float sqrt_alpha, float sqrt_beta, float m1, float m2, float m3,
                                     float m4, float mn, lkgd_stream_t stream) {
  return dit_cfg_dpm_host<false>(noise_rows, ldn, latents, latents_is_f32, x0_state, eps, B, F, C, H, W, p, 0, cfg, order,
                                 dpm_t{guidance, sqrt_alpha, sqrt_beta, m1, m2, m3, m4, mn}, stream);
}

extern "C" int lkgd_dit_cfg_dpm_step_t(const void* noise_rows, int32_t ldn, void* latents, int32_t latents_is_f32, void* x0_state,
                                       const void* eps, int32_t B, int32_t F, int32_t C, int32_t H, int32_t W, int32_t p, int32_t p_t,
                                       int32_t cfg, int32_t order, float guidance, float sqrt_alpha, float sqrt_beta, float m1, float m2,
                                       float m3, float m4, float mn, lkgd_stream_t stream) {
  return dit_cfg_dpm_host<true>(noise_rows, ldn, latents, latents_is_f32, x0_state, eps, B, F, C, H, W, p, p_t, cfg, order,
                                dpm_t{guidance, sqrt_alpha, sqrt_beta, m1, m2, m3, m4, mn}, stream);
}
