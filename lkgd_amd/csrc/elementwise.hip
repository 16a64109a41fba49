// Loop glue and small elementwise kernels (include/lkgd_hip.h sections 6, 7; include/lkgd_hip_window.h).  All HBM/latency-bound.
// Every kernel that takes an Euler step does it through ONE core (euler_setup / euler_x0 / euler_advance), and the plain and the
// windowed CFG + Euler entry points launch ONE step kernel (cfg_euler_kernel).
#include <type_traits>

#include "common.h"
#include "../../include/lkgd_hip_window.h"

// ---- CFG duplicate + scale_model_input + channel concat, NCHW planes -> channels-last tokens [.., 8]
// reference: pipeline_stable_video_diffusion_trans.py:549-553, scheduler scale_model_input :284-285
template <typename LT>
__global__ __launch_bounds__(256) void prepare_input_kernel(const LT* __restrict__ latents,
                                                            const half_t* __restrict__ image_latents, int B, int F,
                                                            int HW, int cfg, float inv_scale,
                                                            half_t* __restrict__ out) {
  const long long total = (long long)cfg * B * F * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long nf = i / HW;          // cb*F + f
    const int f = (int)(nf % F);
    const int cb = (int)(nf / F);
    const int b = cb % B;                 // torch.cat([latents] * 2): uncond copies first, then cond copies
    half8_t o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float x = (float)latents[(((long long)b * F + f) * 4 + c) * HW + p];
      o[c] = (half_t)(x * inv_scale);
      o[4 + c] = image_latents[(((long long)cb * F + f) * 4 + c) * HW + p];
    }
    *(half8_t*)(out + i * 8) = o;
  }
}

// ---- per-frame CFG  uncond + g[f] * (cond - uncond)  of one token row, on fp16 values as the reference's fp16 tensors form it
// (pipeline :578-592): the difference, the product and the sum are each rounded to fp16.  Contraction is off here: fused into
// one fp16 multiply-add the product would skip its rounding, and one fp16 ulp of the noise is sigma / 1024 in an epsilon-
// prediction x0 - more than an fp16 ulp of the latents at the high-noise steps.
__device__ __forceinline__ half4_t cfg_combine(const half_t* __restrict__ noise, long long i, long long cond_off, int cfg,
                                               const float* __restrict__ guidance, int f) {
#pragma clang fp contract(off)
  half4_t u = *(const half4_t*)(noise + i * 4);
  if (cfg != 2) return u;
  half4_t c = *(const half4_t*)(noise + (i + cond_off) * 4);
  const half_t g = (half_t)guidance[f];
  half4_t n;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    half_t d = (half_t)((float)c[e] - (float)u[e]);
    half_t gd = (half_t)((float)g * (float)d);
    n[e] = (half_t)((float)u[e] + (float)gd);
  }
  return n;
}

// ---- the Euler core (scheduler.step :481-520).  fp16 rounding points follow the reference's tensor dtypes: model_output *
// c_out (or * sigma) stays fp16 (a 0-dim fp32 scalar does not promote), everything after the upcast of `sample` is fp32.
// `sigma_hat` is sigma itself everywhere but in the standalone scheduler's churn step.
struct euler_t { float c_out, c_skip, sigma_hat, dt; };
__device__ __forceinline__ euler_t euler_setup(float sigma, float sigma_hat, float sigma_next) {
  euler_t e;
  e.c_out = -sigma / sqrtf(sigma * sigma + 1.0f);
  e.c_skip = sigma * sigma + 1.0f;
  e.sigma_hat = sigma_hat;
  e.dt = sigma_next - sigma_hat;
  return e;
}
__device__ __forceinline__ float euler_x0(const euler_t& e, int vpred, half_t n, float x) {
  if (vpred) return (float)(half_t)((float)n * e.c_out) + x / e.c_skip;
  return x - (float)(half_t)((float)n * e.sigma_hat);
}
__device__ __forceinline__ float euler_advance(const euler_t& e, float x, float x0) {
  const float deriv = (x - x0) / e.sigma_hat;
  return x + deriv * e.dt;
}

// ---- per-frame CFG + Euler step (pipeline :578-592): CFG arithmetic on fp16 tensors (cfg_combine), then the core.  `cond_off`:
// token rows from an unconditional row to its conditional one - B*F*HW for the whole batch; 2*L*HW for a window of the smoothing
// pipeline, which is this kernel with B = 1, F = L and `latents` advanced to the window's first frame.
template <typename LT>
__global__ __launch_bounds__(256) void cfg_euler_kernel(const half_t* __restrict__ noise, LT* __restrict__ latents,
                                                        const float* __restrict__ guidance, int B, int F, int HW,
                                                        int cfg, long long cond_off, float sigma, float sigma_next,
                                                        int vpred) {
  const long long total = (long long)B * F * HW;
  const euler_t e = euler_setup(sigma, sigma, sigma_next);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long bf = i / HW;
    const int f = (int)(bf % F);
    const int b = (int)(bf / F);
    const half4_t n = cfg_combine(noise, i, cond_off, cfg, guidance, f);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const long long li = (((long long)b * F + f) * 4 + c) * HW + p;
      const float x = (float)latents[li];
      latents[li] = (LT)euler_advance(e, x, euler_x0(e, vpred, n[c], x));
    }
  }
}

// ---- direct-fusion Euler step of the trans-ControlNet pipeline (pipeline_stable_video_diffusion_trans_controlnet.py
// :637-667): per-frame CFG (cfg_combine) and x0 of every clip as cfg_euler_kernel forms them, then the forward clip b and the
// frame-reversed backward clip b+P are blended through their x0 with weight[f] = linspace(1, 0, F)[f] (fp32), and both
// clips take the Euler step from the blend (clip b+P at frame F-1-f from xb[b, f]).  One thread owns element (b, f, ., p)
// and its mirror (b+P, F-1-f, ., p): it reads both latents before it writes either, so the in-place update is race-free.
template <typename LT>
__global__ __launch_bounds__(256) void cfg_fusion_euler_kernel(const half_t* __restrict__ noise,
                                                               LT* __restrict__ latents,
                                                               const float* __restrict__ guidance,
                                                               const float* __restrict__ weight, int B, int F, int HW,
                                                               int cfg, float sigma, float sigma_next, int vpred) {
  const int P = B / 2;
  const long long total = (long long)B * F * HW;         // token rows of one CFG half
  const long long pairs = (long long)P * F * HW;         // threads: one per (b < P, f, p)
  const euler_t e = euler_setup(sigma, sigma, sigma_next);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long bf = i / HW;
    const int f = (int)(bf % F);
    const int b = (int)(bf / F);
    const int fm = F - 1 - f;
    const long long im = ((long long)(b + P) * F + fm) * HW + p;     // token row of the mirror element
    const half4_t na = cfg_combine(noise, i, total, cfg, guidance, f);
    const half4_t nm = cfg_combine(noise, im, total, cfg, guidance, fm);
    const float w = weight[f];
    const float wc = 1.0f - w;
    const long long la = ((long long)b * F + f) * 4 * HW + p;
    const long long lm = ((long long)(b + P) * F + fm) * 4 * HW + p;
    float xa[4], xm[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      xa[c] = (float)latents[la + (long long)c * HW];
      xm[c] = (float)latents[lm + (long long)c * HW];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float xb = euler_x0(e, vpred, na[c], xa[c]) * w + euler_x0(e, vpred, nm[c], xm[c]) * wc;
      latents[la + (long long)c * HW] = (LT)euler_advance(e, xa[c], xb);
      latents[lm + (long long)c * HW] = (LT)euler_advance(e, xm[c], xb);
    }
  }
}

// ---- layout converters at the UNet.forward API boundary
__global__ __launch_bounds__(256) void tokens_to_nchw_kernel(const half_t* __restrict__ tok, int ld, long long N,
                                                             int C, int HW, half_t* __restrict__ out) {
  const long long total = N * C * (long long)HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long nc = i / HW;
    const int c = (int)(nc % C);
    const long long n = nc / C;
    out[i] = tok[(n * HW + p) * ld + c];
  }
}
__global__ __launch_bounds__(256) void nchw_to_tokens_kernel(const half_t* __restrict__ in, long long N, int C, int HW,
                                                             half_t* __restrict__ tok, int ld) {
  const long long total = N * C * (long long)HW;
  // consecutive threads walk p (coalesced reads from the planes); writes are strided by ld (small C at this boundary)
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long nc = i / HW;
    const int c = (int)(nc % C);
    const long long n = nc / C;
    tok[(n * HW + p) * ld + c] = in[i];
  }
}

// ---- sinusoidal timestep embedding [cos | sin] (flip_sin_to_cos=True, shift 0): unet_..._controlnet.py:406,415
__global__ void timestep_embedding_kernel(const float* __restrict__ t, int n, int dim, half_t* __restrict__ out,
                                          int ldo) {
  const int half_dim = dim / 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n * half_dim; i += gridDim.x * blockDim.x) {
    const int r = i / half_dim, j = i - r * half_dim;
    const float freq = expf(-9.210340371976184f * (float)j / (float)half_dim);
    const float a = t[r] * freq;
    out[(long long)r * ldo + j] = (half_t)cosf(a);
    out[(long long)r * ldo + half_dim + j] = (half_t)sinf(a);
  }
}

__global__ __launch_bounds__(256) void silu_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long long n) {
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (long long)gridDim.x * 2048) {
    if (i + 8 <= n) {
      half8_t v = *(const half8_t*)(x + i), o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (half_t)silu_f((float)v[e]);
      *(half8_t*)(y + i) = o;
    } else {
      for (long long j = i; j < n; ++j) y[j] = (half_t)silu_f((float)x[j]);
    }
  }
}
__global__ __launch_bounds__(256) void add_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b,
                                                  half_t* __restrict__ y, long long n) {
  for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (long long)gridDim.x * 2048) {
    if (i + 8 <= n) {
      *(half8_t*)(y + i) = *(const half8_t*)(a + i) + *(const half8_t*)(b + i);
    } else {
      for (long long j = i; j < n; ++j) y[j] = a[j] + b[j];
    }
  }
}

// ---- standalone scheduler API kernels (scale_model_input :264-288 / step :418-528 on tensors of any shape)
__global__ __launch_bounds__(256) void scale_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long long n,
                                                    float s) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    y[i] = (half_t)((float)x[i] * s);
}
template <typename ST>
__global__ __launch_bounds__(256) void euler_kernel(const half_t* __restrict__ mo, const ST* __restrict__ sample,
                                                    const half_t* __restrict__ noise, half_t* __restrict__ prev, long long n,
                                                    float sigma, float sigma_hat, float s_noise, float churn, float sigma_next,
                                                    int vpred) {
  // sigma_hat = sigma * (gamma + 1); gamma > 0 ("churn", scheduling_euler_discrete_karras_fix.py:485-497) first adds
  // noise * s_noise * sqrt(sigma_hat^2 - sigma^2) to the sample, each product rounded to fp16 as the reference's tensors are
  const euler_t e = euler_setup(sigma, sigma_hat, sigma_next);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float x = (float)sample[i];
    if (noise) x += (float)(half_t)((float)(half_t)((float)noise[i] * s_noise) * churn);
    prev[i] = (half_t)euler_advance(e, x, euler_x0(e, vpred, mo[i], x));
  }
}

static unsigned grid_for(long long work_items, int per_block) {
  long long g = (work_items + per_block - 1) / per_block;
  if (g > 256 * 16) g = 256 * 16;
  if (g < 1) g = 1;
  return (unsigned)g;
}

// ---- shared by the loop-glue entry points.  The order of the checks is part of the ABI: null, guidance for cfg 2, shape, mode,
// alignment.
static int batch_shape_ok(int32_t B, int32_t F, int32_t H, int32_t W, int32_t cfg) {
  return B > 0 && F > 0 && H > 0 && W > 0 && (cfg == 1 || cfg == 2);
}
static int window_shape_ok(int32_t T, int32_t f0, int32_t L, int32_t H, int32_t W, int32_t cfg, float sigma) {
  return T > 0 && H > 0 && W > 0 && L > 0 && f0 >= 0 && (long long)f0 + L <= T && (cfg == 1 || cfg == 2) && sigma > 0.f;
}
static int prepare_check(const void* latents, const void* image_latents, const void* tokens_out, int shape_ok) {
  if (!latents || !image_latents || !tokens_out) return LKGD_E_NULL;
  if (!shape_ok) return LKGD_E_SHAPE;
  return aligned16(tokens_out) ? LKGD_OK : LKGD_E_ALIGN;
}
static int step_check(const void* noise_tokens, const void* latents, const float* guidance, int32_t cfg, int shape_ok,
                      int32_t prediction_type) {
  if (!noise_tokens || !latents) return LKGD_E_NULL;
  if (cfg == 2 && !guidance) return LKGD_E_NULL;
  if (!shape_ok) return LKGD_E_SHAPE;
  if (prediction_type != 0 && prediction_type != 1) return LKGD_E_MODE;
  return ((uintptr_t)noise_tokens & 7) ? LKGD_E_ALIGN : LKGD_OK;
}
// launch(tag) with a float* or half_t* tag: the one place an entry point spells its launch, for both latent dtypes
template <typename Launch>
static int launch_typed(int32_t is_f32, Launch&& launch) {
  if (is_f32) launch((float*)nullptr);
  else launch((half_t*)nullptr);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_prepare_unet_input(const void* latents, int32_t latents_is_f32, const void* image_latents,
                                       int32_t B, int32_t F, int32_t H, int32_t W, int32_t cfg, float sigma,
                                       void* tokens_out, lkgd_stream_t stream) {
  if (int rc = prepare_check(latents, image_latents, tokens_out, batch_shape_ok(B, F, H, W, cfg))) return rc;
  const float inv = 1.0f / sqrtf(sigma * sigma + 1.0f);
  const long long total = (long long)cfg * B * F * H * W;
  return launch_typed(latents_is_f32, [&](auto* tag) {
    using LT = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(prepare_input_kernel<LT>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const LT*)latents, (const half_t*)image_latents, B, F, H * W, cfg, inv, (half_t*)tokens_out);
  });
}

// the plain step and the window step: `latents` + first_elem is frame 0 of the B x F frames to step, one thread per (b, f, pixel)
static int cfg_euler_launch(const void* noise_tokens, void* latents, int32_t latents_is_f32, const float* guidance,
                            long long first_elem, int32_t B, int32_t F, int32_t HW, int32_t cfg, long long cond_off,
                            int shape_ok, float sigma, float sigma_next, int32_t prediction_type, lkgd_stream_t stream) {
  if (int rc = step_check(noise_tokens, latents, guidance, cfg, shape_ok, prediction_type)) return rc;
  const long long total = (long long)B * F * HW;
  return launch_typed(latents_is_f32, [&](auto* tag) {
    using LT = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(cfg_euler_kernel<LT>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)noise_tokens, (LT*)latents + first_elem, guidance, B, F, HW, cfg, cond_off, sigma,
                       sigma_next, prediction_type);
  });
}

extern "C" int lkgd_cfg_euler_step(const void* noise_tokens, void* latents, int32_t latents_is_f32,
                                   const float* guidance, int32_t B, int32_t F, int32_t H, int32_t W, int32_t cfg,
                                   float sigma, float sigma_next, int32_t prediction_type, lkgd_stream_t stream) {
  return cfg_euler_launch(noise_tokens, latents, latents_is_f32, guidance, 0, B, F, H * W, cfg, (long long)B * F * H * W,
                          batch_shape_ok(B, F, H, W, cfg) && sigma > 0.f, sigma, sigma_next, prediction_type, stream);
}

extern "C" int lkgd_cfg_fusion_euler_step(const void* noise_tokens, void* latents, int32_t latents_is_f32,
                                          const float* guidance, const float* weight, int32_t B, int32_t F, int32_t H,
                                          int32_t W, int32_t cfg, float sigma, float sigma_next,
                                          int32_t prediction_type, lkgd_stream_t stream) {
  if (!weight) return LKGD_E_NULL;
  if (int rc = step_check(noise_tokens, latents, guidance, cfg, batch_shape_ok(B, F, H, W, cfg) && !(B & 1) && sigma > 0.f,
                          prediction_type))
    return rc;
  const long long pairs = (long long)(B / 2) * F * H * W;
  return launch_typed(latents_is_f32, [&](auto* tag) {
    using LT = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(cfg_fusion_euler_kernel<LT>, dim3(grid_for(pairs, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)noise_tokens, (LT*)latents, guidance, weight, B, F, H * W, cfg, sigma, sigma_next,
                       prediction_type);
  });
}

// ---- windowed loop glue of the long-video smoothing pipeline (include/lkgd_hip_window.h; pipeline_stable_video_diffusion_
// smooth.py:545-594).  A window is frames f0 .. f0+L-1 of latents [T,4,H,W]; the UNet batch is entry e = 2*k + d, k = CFG half,
// d = 0 the window, d = 1 the window reversed in time.  The gather is a kernel of its own (frame flip, zero unconditional half),
// with the rounding points, 16-byte token rows, plane-coalesced reads and grid rule of prepare_input_kernel; the step is
// cfg_euler_kernel on the window's frames.
template <typename LT>
__global__ __launch_bounds__(256) void window_prepare_kernel(const LT* __restrict__ latents,
                                                             const half_t* __restrict__ image_latents, int f0, int L,
                                                             int HW, int cfg, float inv_scale,
                                                             half_t* __restrict__ out) {
  const long long total = 2ll * cfg * L * HW;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int p = (int)(i % HW);
    const long long ej = i / HW;          // e*L + j
    const int j = (int)(ej % L);
    const int e = (int)(ej / L);
    const int d = e & 1;
    const bool cond = (e >> 1) == cfg - 1;                // torch.cat([latents_chunk] * 2): the uncond entries come first
    const long long lf = f0 + (d ? L - 1 - j : j);        // latents_chunk.flip(dims=[1]) for the reversed clip (:551)
    const long long cf = d ? f0 + L - 1 : f0;             // first_frame_ids (:554): the clip's own first frame conditions it
    half8_t o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float x = (float)latents[(lf * 4 + c) * HW + p];
      o[c] = (half_t)(x * inv_scale);
      o[4 + c] = cond ? image_latents[(cf * 4 + c) * HW + p] : (half_t)0.0f;
    }
    *(half8_t*)(out + i * 8) = o;
  }
}

extern "C" int lkgd_window_prepare_input(const void* latents, int32_t latents_is_f32, const void* image_latents, int32_t T,
                                         int32_t f0, int32_t L, int32_t H, int32_t W, int32_t cfg, float sigma,
                                         void* tokens_out, lkgd_stream_t stream) {
  if (int rc = prepare_check(latents, image_latents, tokens_out, window_shape_ok(T, f0, L, H, W, cfg, sigma))) return rc;
  const float inv = 1.0f / sqrtf(sigma * sigma + 1.0f);
  const long long total = 2ll * cfg * L * H * W;
  return launch_typed(latents_is_f32, [&](auto* tag) {
    using LT = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(window_prepare_kernel<LT>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const LT*)latents, (const half_t*)image_latents, f0, L, H * W, cfg, inv, (half_t*)tokens_out);
  });
}

// the window's frames are a [1, L] clip that starts f0 frames into the latents; of the batch [fwd, rev] x [uncond, cond] only the
// forward clip steps: its unconditional rows are entry 0, its conditional rows entry 2
extern "C" int lkgd_window_cfg_euler_step(const void* noise_tokens, void* latents, int32_t latents_is_f32,
                                          const float* guidance, int32_t T, int32_t f0, int32_t L, int32_t H, int32_t W,
                                          int32_t cfg, float sigma, float sigma_next, int32_t prediction_type,
                                          lkgd_stream_t stream) {
  return cfg_euler_launch(noise_tokens, latents, latents_is_f32, guidance, (long long)f0 * 4 * H * W, 1, L, H * W, cfg,
                          2ll * L * H * W, window_shape_ok(T, f0, L, H, W, cfg, sigma), sigma, sigma_next, prediction_type,
                          stream);
}

// ---- rows of a frame shard regrouped by destination pixel shard (and back): the pack / unpack around the all-to-all that
// re-shards the temporal attention by pixels (lkgd_amd/dist.py::frames_to_pixels / pixels_to_frames).  Row (f, p) of the
// [fl, HW, C] slice sits in the send buffer at  fl * p0[r] + f * px[r] + (p - p0[r])  with r = the shard that owns pixel p.
typedef unsigned sr_vec_t __attribute__((ext_vector_type(4)));
struct shard_tab { int k; int px[16]; int p0[16]; };
template <bool PACK>
__global__ __launch_bounds__(256) void shard_rows_kernel(const sr_vec_t* __restrict__ src, sr_vec_t* __restrict__ dst, int fl, int HW,
                                                         int c8, shard_tab tab) {
  const long long n = (long long)fl * HW * c8;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long row = i / c8;
    const int v = (int)(i - row * c8);
    const int f = (int)(row / HW), p = (int)(row - (long long)f * HW);
    int r = 0;
    while (r + 1 < tab.k && p >= tab.p0[r + 1]) ++r;
    const long long prow = (long long)fl * tab.p0[r] + (long long)f * tab.px[r] + (p - tab.p0[r]);
    if (PACK) dst[prow * c8 + v] = src[i];
    else dst[i] = src[prow * c8 + v];
  }
}

extern "C" int lkgd_shard_rows(const void* src, void* dst, int32_t fl, int32_t HW, int32_t C, int32_t k, const int32_t* px,
                               int32_t pack, lkgd_stream_t stream) {
  if (!src || !dst || !px) return LKGD_E_NULL;
  if (fl <= 0 || HW <= 0 || C <= 0 || C % 8 || k <= 0 || k > 16) return LKGD_E_SHAPE;
  if (!aligned16(src) || !aligned16(dst)) return LKGD_E_ALIGN;
  shard_tab tab;
  tab.k = k;
  int o = 0;
  for (int r = 0; r < k; ++r) {
    if (px[r] <= 0) return LKGD_E_SHAPE;
    tab.px[r] = px[r];
    tab.p0[r] = o;
    o += px[r];
  }
  if (o != HW) return LKGD_E_SHAPE;
  const long long n = (long long)fl * HW * (C / 8);
  const dim3 gr(grid_for(n, 256)), bl(256);
  if (pack) hipLaunchKernelGGL(shard_rows_kernel<true>, gr, bl, 0, (hipStream_t)stream, (const sr_vec_t*)src, (sr_vec_t*)dst, fl, HW, C / 8, tab);
  else hipLaunchKernelGGL(shard_rows_kernel<false>, gr, bl, 0, (hipStream_t)stream, (const sr_vec_t*)src, (sr_vec_t*)dst, fl, HW, C / 8, tab);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_tokens_to_nchw(const void* tokens, int32_t ld, int64_t N, int32_t C, int32_t HW, void* out,
                                   lkgd_stream_t stream) {
  if (!tokens || !out) return LKGD_E_NULL;
  if (N <= 0 || C <= 0 || HW <= 0 || ld < C) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(tokens_to_nchw_kernel, dim3(grid_for(N * C * (long long)HW, 256)), dim3(256), 0,
                     (hipStream_t)stream, (const half_t*)tokens, ld, (long long)N, C, HW, (half_t*)out);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_nchw_to_tokens(const void* nchw, int64_t N, int32_t C, int32_t HW, void* tokens, int32_t ld,
                                   lkgd_stream_t stream) {
  if (!nchw || !tokens) return LKGD_E_NULL;
  if (N <= 0 || C <= 0 || HW <= 0 || ld < C) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(nchw_to_tokens_kernel, dim3(grid_for(N * C * (long long)HW, 256)), dim3(256), 0,
                     (hipStream_t)stream, (const half_t*)nchw, (long long)N, C, HW, (half_t*)tokens, ld);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_timestep_embedding(const float* t, int32_t n, int32_t dim, void* out, int32_t ldo,
                                       lkgd_stream_t stream) {
  if (!t || !out) return LKGD_E_NULL;
  if (n <= 0 || dim <= 0 || dim % 2 || ldo < dim) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3(grid_for((long long)n * dim / 2, 256)), dim3(256), 0,
                     (hipStream_t)stream, t, n, dim, (half_t*)out, ldo);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_silu(const void* x, void* y, int64_t n, lkgd_stream_t stream) {
  if (!x || !y) return LKGD_E_NULL;
  if (n <= 0) return LKGD_E_SHAPE;
  if (!aligned16(x) || !aligned16(y)) return LKGD_E_ALIGN;
  hipLaunchKernelGGL(silu_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, (hipStream_t)stream, (const half_t*)x,
                     (half_t*)y, (long long)n);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_add(const void* a, const void* b, void* y, int64_t n, lkgd_stream_t stream) {
  if (!a || !b || !y) return LKGD_E_NULL;
  if (n <= 0) return LKGD_E_SHAPE;
  if (!aligned16(a) || !aligned16(b) || !aligned16(y)) return LKGD_E_ALIGN;
  hipLaunchKernelGGL(add_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, (hipStream_t)stream, (const half_t*)a,
                     (const half_t*)b, (half_t*)y, (long long)n);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

extern "C" int lkgd_scale(const void* x, void* y, int64_t n, float s, lkgd_stream_t stream) {
  if (!x || !y) return LKGD_E_NULL;
  if (n <= 0) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, (const half_t*)x,
                     (half_t*)y, (long long)n, s);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

static int euler_launch(const void* model_output, const void* sample, int32_t sample_is_f32, const void* noise, void* prev,
                        int64_t n, float sigma, float sigma_hat, float s_noise, float churn, float sigma_next,
                        int32_t prediction_type, lkgd_stream_t stream) {
  if (!model_output || !sample || !prev) return LKGD_E_NULL;
  if (n <= 0 || !(sigma > 0.f) || !(sigma_hat >= sigma)) return LKGD_E_SHAPE;
  if (prediction_type != 0 && prediction_type != 1) return LKGD_E_MODE;
  return launch_typed(sample_is_f32, [&](auto* tag) {
    using ST = std::remove_pointer_t<decltype(tag)>;
    hipLaunchKernelGGL(euler_kernel<ST>, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)model_output, (const ST*)sample, (const half_t*)noise, (half_t*)prev, (long long)n,
                       sigma, sigma_hat, s_noise, churn, sigma_next, prediction_type);
  });
}

extern "C" int lkgd_euler_step(const void* model_output, const void* sample, int32_t sample_is_f32, void* prev,
                               int64_t n, float sigma, float sigma_next, int32_t prediction_type,
                               lkgd_stream_t stream) {
  return euler_launch(model_output, sample, sample_is_f32, nullptr, prev, n, sigma, sigma, 0.f, 0.f, sigma_next,
                      prediction_type, stream);
}

extern "C" int lkgd_euler_step_churn(const void* model_output, const void* sample, int32_t sample_is_f32, const void* noise,
                                     void* prev, int64_t n, float sigma, float sigma_hat, float s_noise, float churn,
                                     float sigma_next, int32_t prediction_type, lkgd_stream_t stream) {
  if (!noise) return LKGD_E_NULL;
  return euler_launch(model_output, sample, sample_is_f32, noise, prev, n, sigma, sigma_hat, s_noise, churn, sigma_next,
                      prediction_type, stream);
}

extern "C" const char* lkgd_version(void) { return "lkgd_hip 1 gfx950"; }

// ---------------------------------------------------------------------------------------------------------------
// DiT glue (include/lkgd_hip.h section 14; CogVideoX blocks)
//   lkgd_gelu_tanh : y = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))   F.gelu(approximate="tanh"), fp16 in / out, in place ok
//   lkgd_gated_add : out[r, :] = res[r, :] + gate[g(r), :] * x[r, :],  g(r) = (r / rows_per_batch) * 2 + ((r % rows_per_batch) >= split)
//                    the adaLN-zero residual of the two token streams (text rows first, then video rows) of every batch entry
__global__ void gelu_tanh_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long long n8) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const half8_t v = *(const half8_t*)(x + i * 8);
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float f = (float)v[e];
    const float u = 0.7978845608028654f * (f + 0.044715f * f * f * f);
    // tanh(u) = 1 - 2 / (exp(2u) + 1); exp2-based, saturates cleanly for |u| large
    const float t = 1.0f - 2.0f / (__builtin_amdgcn_exp2f(u * 2.885390081777927f) + 1.0f);
    o[e] = (half_t)(0.5f * f * (1.0f + t));
  }
  *(half8_t*)(y + i * 8) = o;
}

extern "C" int lkgd_gelu_tanh(const void* x, void* y, int64_t n, lkgd_stream_t stream) {
  if (!x || !y) return LKGD_E_NULL;
  if (n <= 0 || n % 8) return LKGD_E_SHAPE;
  if (!aligned16(x) || !aligned16(y)) return LKGD_E_ALIGN;
  const long long n8 = n / 8, nblk = (n8 + 255) / 256;
  if (nblk > 0x7fffffffLL) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(gelu_tanh_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (half_t*)y, n8);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

__global__ void gated_add_kernel(const half_t* __restrict__ x, int ldx, const float* __restrict__ gate, const half_t* __restrict__ res,
                                 int ldr, half_t* __restrict__ out, int ldo, long long rows, int C8, int rows_per_batch, int split) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * C8) return;
  const long long r = i / C8;
  const int cv = (int)(i - r * C8);
  const long long b = r / rows_per_batch;
  const int g = (int)(b * 2 + ((r - b * rows_per_batch) >= split ? 1 : 0));
  const half8_t xv = *(const half8_t*)(x + r * ldx + cv * 8), rv = *(const half8_t*)(res + r * ldr + cv * 8);
  const float4_t g0 = *(const float4_t*)(gate + ((long long)g * C8 + cv) * 8), g1 = *(const float4_t*)(gate + ((long long)g * C8 + cv) * 8 + 4);
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)rv[e] + (e < 4 ? g0[e & 3] : g1[e & 3]) * (float)xv[e]);
  *(half8_t*)(out + r * ldo + cv * 8) = o;
}

extern "C" int lkgd_gated_add(const void* x, int32_t ldx, const float* gate, const void* res, int32_t ldr, void* out, int32_t ldo,
                              int64_t rows, int32_t C, int32_t rows_per_batch, int32_t split, lkgd_stream_t stream) {
  if (!x || !gate || !res || !out) return LKGD_E_NULL;
  if (rows <= 0 || C <= 0 || C % 8 || rows_per_batch <= 0 || rows % rows_per_batch || split < 0 || split > rows_per_batch)
    return LKGD_E_SHAPE;
  if (ldx % 8 || ldr % 8 || ldo % 8 || !aligned16(x) || !aligned16(res) || !aligned16(out) || !aligned16(gate)) return LKGD_E_ALIGN;
  const long long total = rows * (C / 8), nblk = (total + 255) / 256;
  if (nblk > 0x7fffffffLL) return LKGD_E_SHAPE;
  hipLaunchKernelGGL(gated_add_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, ldx, gate,
                     (const half_t*)res, ldr, (half_t*)out, ldo, (long long)rows, C / 8, rows_per_batch, split);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
