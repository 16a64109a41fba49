// LKGD latent-knowledge fuse (include/lkgd_hip.h section 18): the block the reference recomputes in every UNet forward
// (models/unet_spatio_temporal_condition.py:536-595) - grouped 1x1 convolutions of the CLIP embedding and of the domain / flow
// logits (interpolated 1000 -> 1024), a quaternion linear on their concatenation, a 256-point real DFT of each, quaternion
// linears on magnitudes and phases, a 257-bin inverse DFT (512 real samples), and the two-layer `fuse_sf` MLP whose output
// REPLACES the CLIP embedding.  ~1.3 M multiply-adds on [B, 1024] vectors, input-invariant over the Euler steps: it runs once
// per clip, one workgroup per batch entry, fp32 throughout (the reference's FFT has no half path either), everything between
// the input vectors and the output row in LDS.  Latency, not a roofline: ~35 us, of which ~25 are the 2-MB weight read of the
// first quaternion linear by ONE workgroup.
#include "common.h"
#include "../../include/lkgd_hip_dit_loop.h"

struct lk_params {
  const float *e, *d, *f;            // [B, 1024], [Bd, 1000], [Bd, 1000] (Bd = 1: broadcast, reference :544-546)
  int B, Bd;
  const float *wl, *wd, *wf;         // Conv1d(1024 -> 256, k = 1, groups = 256): [256][4]
  const float* ctx;                  // [256]
  const float *w_fuse, *b_fuse;      // Hamilton matrix [1024][512] (in, out), [512]
  const float *cmag, *cpha;          // learned spectrum context [129]
  const float *w_mag, *b_mag, *w_pha, *b_pha;   // [512][256] (in, out), [256]
  const float *l0m, *l0p;            // Linear(4 -> 1) on the last bin: 4 weights + bias
  const float *sf0_w, *sf0_b, *sf2_w, *sf2_b;   // [1024][256] (in, out), [256]; [256][1024] (in, out), [1024]
  half_t* out;                       // [B, ldo]
  int ldo;
};

#define LK_NT 256
#define LK_PI 3.14159265358979323846f

// y[o] = b[o] + sum_i x[i] * W[i][o], W row-major (in, out): consecutive threads read consecutive columns
template <int PER>
__device__ __forceinline__ void lk_matvec(const float* __restrict__ W, const float* __restrict__ b, const float* x, int nin,
                                          int nout, float* y, int t) {
  float acc[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) acc[u] = 0.f;
  for (int i = 0; i < nin; ++i) {
    const float xi = x[i];
#pragma unroll
    for (int u = 0; u < PER; ++u) acc[u] = fmaf(xi, W[(long long)i * nout + t + u * LK_NT], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) y[t + u * LK_NT] = acc[u] + b[t + u * LK_NT];
}

__global__ __launch_bounds__(LK_NT) void lk_fuse_kernel(const lk_params p) {
  __shared__ float s_in[3][1024];        // e, interp(d), interp(f)
  __shared__ float s_cat[1024];          // low | low_d | low_f | ctx, later spatial | freq
  __shared__ float s_tw[512][2];         // cos, sin of 2 pi j / 512
  __shared__ float s_sp[3][129][2];      // spectra (re, im)
  __shared__ float s_mp[2][512];         // magnitudes | phases of bins 0..127 (4 x 128 each)
  __shared__ float s_mag[256], s_pha[256];
  __shared__ float s_spec[257][2];
  __shared__ float s_h[256];
  __shared__ float s_last[2][4];         // bin 128: magnitudes, phases
  const int t = threadIdx.x, b = blockIdx.x;
  const int bd = p.Bd == 1 ? 0 : b;
  for (int i = t; i < 1024; i += LK_NT) {
    s_in[0][i] = p.e[(long long)b * 1024 + i];
    // F.interpolate(size = 1024, mode = "linear", align_corners = False) of a 1000-sample row (reference :537,:540)
    float src = ((float)i + 0.5f) * (1000.0f / 1024.0f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    const int i0 = (int)src, i1 = i0 + 1 < 1000 ? i0 + 1 : 999;
    const float w1 = src - (float)i0, w0 = 1.0f - w1;
    s_in[1][i] = w0 * p.d[(long long)bd * 1000 + i0] + w1 * p.d[(long long)bd * 1000 + i1];
    s_in[2][i] = w0 * p.f[(long long)bd * 1000 + i0] + w1 * p.f[(long long)bd * 1000 + i1];
  }
  for (int j = t; j < 512; j += LK_NT) {
    float sn, cs;
    sincospif((float)j * (1.0f / 256.0f), &sn, &cs);      // 2 pi j / 512
    s_tw[j][0] = cs; s_tw[j][1] = sn;
  }
  __syncthreads();
  {   // grouped 1x1 convolutions: output channel c = 4-tap weighted sum of inputs 4c .. 4c+3 (thread = channel)
    const float* ws[3] = {p.wl, p.wd, p.wf};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) a += s_in[s][4 * t + k] * ws[s][4 * t + k];
      s_cat[s * 256 + t] = a;
    }
    s_cat[768 + t] = p.ctx[t];
  }
  __syncthreads();
  // 256-point real DFT of low / low_d / low_f, bins 0..128: X[k] = sum_n x[n] (cos - i sin)(2 pi k n / 256)
  for (int q = t; q < 3 * 129; q += LK_NT) {
    const int s = q / 129, k = q - s * 129;
    float re = 0.f, im = 0.f;
    for (int n = 0; n < 256; ++n) {
      const int j = ((k * n) & 255) * 2;             // table of 512 entries: angle 2 pi (kn mod 256) / 256
      const float x = s_cat[s * 256 + n];
      re = fmaf(x, s_tw[j][0], re);
      im = fmaf(-x, s_tw[j][1], im);
    }
    s_sp[s][k][0] = re; s_sp[s][k][1] = im;
  }
  __syncthreads();
  // spatial = quaternion_linear(cat) (the Hamilton matrix is expanded on the host): 1024 -> 512
  float spatial[2];
  {
    float acc[2] = {0.f, 0.f};
    for (int i = 0; i < 1024; ++i) {
      const float xi = s_cat[i];
      acc[0] = fmaf(xi, p.w_fuse[(long long)i * 512 + t], acc[0]);
      acc[1] = fmaf(xi, p.w_fuse[(long long)i * 512 + t + LK_NT], acc[1]);
    }
    spatial[0] = acc[0] + p.b_fuse[t]; spatial[1] = acc[1] + p.b_fuse[t + LK_NT];
  }
  // magnitudes / phases: bins 0..127 -> [4 x 128], bin 128 apart (reference :555-577).  Sign convention of the two REAL bins
  // (DC, Nyquist): the direct DFT above accumulates sin(0) / sin(pi k) terms that are exactly +0, so im = +0 and a negative real
  // part has phase +pi - what torch.angle(torch.fft.rfft(x)) returns on the host as well (tests/test_oracle_golden.py pins it;
  // an FFT library that produced -0 there would give -pi, 2 pi w away through pha0 / the pha quaternion linear)
  for (int q = t; q < 4 * 129; q += LK_NT) {
    const int s = q / 129, k = q - s * 129;
    float m, ph;
    if (s < 3) {
      const float re = s_sp[s][k][0], im = s_sp[s][k][1];
      m = hypotf(re, im);
      ph = atan2f(im, re);
    } else {
      m = p.cmag[k]; ph = p.cpha[k];
    }
    if (k < 128) { s_mp[0][s * 128 + k] = m; s_mp[1][s * 128 + k] = ph; }
    else { s_last[0][s] = m; s_last[1][s] = ph; }
  }
  __syncthreads();
  lk_matvec<1>(p.w_mag, p.b_mag, s_mp[0], 512, 256, s_mag, t);
  lk_matvec<1>(p.w_pha, p.b_pha, s_mp[1], 512, 256, s_pha, t);
  __syncthreads();
  {
    float sn, cs;
    sincosf(s_pha[t], &sn, &cs);
    s_spec[t][0] = s_mag[t] * cs; s_spec[t][1] = s_mag[t] * sn;
    if (t == 0) {
      float m0 = p.l0m[4], p0 = p.l0p[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) { m0 = fmaf(s_last[0][s], p.l0m[s], m0); p0 = fmaf(s_last[1][s], p.l0p[s], p0); }
      sincosf(p0, &sn, &cs);
      s_spec[256][0] = m0 * cs; s_spec[256][1] = m0 * sn;
    }
  }
  __syncthreads();
  // inverse real DFT of 257 bins -> 512 samples (the imaginary parts of bins 0 and 256 do not enter, as in irfft)
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int n = t + u * LK_NT;
    float a = s_spec[0][0] + ((n & 1) ? -s_spec[256][0] : s_spec[256][0]);
    float acc = 0.f;
    for (int k = 1; k < 256; ++k) {
      const int j = (k * n) & 511;
      acc = fmaf(s_spec[k][0], s_tw[j][0], acc);
      acc = fmaf(-s_spec[k][1], s_tw[j][1], acc);
    }
    s_cat[512 + n] = (a + 2.0f * acc) * (1.0f / 512.0f);
  }
  s_cat[t] = spatial[0]; s_cat[t + LK_NT] = spatial[1];
  __syncthreads();
  // fuse_sf: Linear(1024 -> 256), LeakyReLU(0.1), Linear(256 -> 1024)
  {
    float acc = 0.f;
    for (int i = 0; i < 1024; ++i) acc = fmaf(s_cat[i], p.sf0_w[(long long)i * 256 + t], acc);
    acc += p.sf0_b[t];
    s_h[t] = acc > 0.f ? acc : 0.1f * acc;
  }
  __syncthreads();
  {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < 256; ++i) {
      const float hi = s_h[i];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = fmaf(hi, p.sf2_w[(long long)i * 1024 + t + u * LK_NT], acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) p.out[(long long)b * p.ldo + t + u * LK_NT] = (half_t)(acc[u] + p.sf2_b[t + u * LK_NT]);
  }
}

extern "C" int lkgd_lk_fuse(const float* e, const float* d, const float* f, int32_t B, int32_t Bd, const float* const* w,
                            void* out, int32_t ldo, lkgd_stream_t stream) {
  if (!e || !d || !f || !w || !out) return LKGD_E_NULL;
  if (B <= 0 || B > 65535 || (Bd != 1 && Bd != B) || ldo < 1024) return LKGD_E_SHAPE;
  for (int i = 0; i < 18; ++i)
    if (!w[i]) return LKGD_E_NULL;
  lk_params p;
  p.e = e; p.d = d; p.f = f; p.B = B; p.Bd = Bd;
  p.wl = w[0]; p.wd = w[1]; p.wf = w[2]; p.ctx = w[3]; p.w_fuse = w[4]; p.b_fuse = w[5]; p.cmag = w[6]; p.cpha = w[7];
  p.w_mag = w[8]; p.b_mag = w[9]; p.w_pha = w[10]; p.b_pha = w[11]; p.l0m = w[12]; p.l0p = w[13];
  p.sf0_w = w[14]; p.sf0_b = w[15]; p.sf2_w = w[16]; p.sf2_b = w[17];
  p.out = (half_t*)out; p.ldo = ldo;
  hipLaunchKernelGGL(lk_fuse_kernel, dim3((unsigned)B), dim3(LK_NT), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}

// ---- the DiT form (include/lkgd_hip_dit_loop.h; cogvideox_transformer_3d.py:519-582): the same block on the TEXT tokens - 226 rows
// per batch entry, a 16-tap grouped conv from 4096 channels, fuse_sf 1024 -> 512 -> 4096.  Only `low` (and what follows from it)
// differs from row to row; low_d, low_f, texts, their spectra, magnitudes, phases and bin-128 terms are the batch entry's.  Their
// shares of the three quaternion linears (rows 256..1023 of w_fuse, rows 128..511 of w_mag / w_pha) and of the two Linear(4, 1)
// are summed ONCE per workgroup; a workgroup owns LKT_R rows of one batch entry, so every weight element it loads (10.75 MB of
// fp32 per pass: w_fuse rows 0..255, w_mag / w_pha rows 0..127, sf[0], sf[2]) feeds LKT_R accumulators.  Row inputs sit in LDS
// as [k][row] so that one ds_read_b128 pair broadcasts the LKT_R operands of a weight; `e` is read straight from global memory
// (16 taps = four 16-byte pieces per output channel).  Every sum is one fmaf chain in index order that starts at zero, row share
// and invariant share apart, joined as (row + invariant) + bias: a row's bits do not depend on LKT_R, on the rows next to it or
// on Bd.  LDS: one 32-KB region holds the phase-1 data (low, spectra), then magnitudes / phases, then spatial | freq; a 16-KB
// region the magnitude / phase inputs, then the spectrum, then the hidden layer.
#define LKT_NT 512
#define LKT_R 8

struct lkt_params {
  const float *e, *d, *f;            // [B * L, lde], [Bd, 1000], [Bd, 1000]
  int lde, L, Bd, nblk;              // nblk = workgroups per batch entry
  const float *wl, *wd, *wf;         // [256][16], [256][4], [256][4]
  const float* ctx;                  // [256]
  const float *w_fuse, *b_fuse;      // [1024][512], [512]
  const float *cmag, *cpha;          // [129]
  const float *w_mag, *b_mag, *w_pha, *b_pha;   // [512][256], [256]
  const float *l0m, *l0p;            // 4 weights + bias
  const float *sf0_w, *sf0_b, *sf2_w, *sf2_b;   // [1024][512], [512]; [512][4096], [4096]
  half_t* out;                       // [B * L, ldo]
  int ldo;
};

// acc[r] += x[r] * w for the LKT_R rows of one LDS operand group [.][LKT_R]
__device__ __forceinline__ void lkt_fma_rows(const float* xr, float w, float (&acc)[LKT_R]) {
  const float4_t x0 = *(const float4_t*)xr, x1 = *(const float4_t*)(xr + 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) { acc[r] = fmaf(x0[r], w, acc[r]); acc[4 + r] = fmaf(x1[r], w, acc[4 + r]); }
}

__global__ __launch_bounds__(LKT_NT) void lk_fuse_tokens_kernel(const lkt_params p) {
  static_assert(LKT_R == 8 && LKT_NT == 512, "the LDS carve and the thread maps below are written for 8 rows x 512 threads");
  __shared__ __attribute__((aligned(16))) float s_u[LKT_R * 1024];
  __shared__ __attribute__((aligned(16))) float s_b[257 * LKT_R * 2];
  __shared__ float s_tw[512][2];          // cos, sin of 2 pi j / 512
  __shared__ float s_lastr[2][LKT_R];     // bin 128 of the rows: magnitudes, phases
  __shared__ float s_inv0[2];             // bias + the invariant terms of fft_mag0 / fft_pha0
  // phase 1 views
  float* const cat_inv = s_u;             // low_d | low_f | texts                    [768]
  float* const lowT = s_u + 768;          // low                                       [256][R]
  float* const sp = s_u + 768 + 256 * LKT_R;   // spectra of the rows, of low_d, low_f [(R + 2)][129][2]
  float* const mpT = s_b;                 // rows: magnitudes | phases of bins 0..127  [2][128][R]
  float* const mpi = s_b + 2 * 128 * LKT_R;    // low_d | low_f | texts, the same      [2][384]
  float* const lasti = mpi + 2 * 384;     // bin 128 of low_d, low_f, texts            [2][3]
  const int t = threadIdx.x;
  const int b = blockIdx.x / p.nblk;
  const int r0 = (blockIdx.x - b * p.nblk) * LKT_R;
  const int bd = p.Bd == 1 ? 0 : b;
  {
    float sn, cs;
    sincospif((float)t * (1.0f / 256.0f), &sn, &cs);
    s_tw[t][0] = cs; s_tw[t][1] = sn;
  }
  {   // low_d (threads 0..255) and low_f (256..511): 4 taps of the interpolated logits per channel
    const int s = t >> 8, c = t & 255;
    const float* src = (s ? p.f : p.d) + (long long)bd * 1000;
    const float* wt = s ? p.wf : p.wd;
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // F.interpolate(size = 1024, mode = "linear", align_corners = False) of a 1000-sample row, as lk_fuse_kernel
      const int i = 4 * c + k;
      float pos = ((float)i + 0.5f) * (1000.0f / 1024.0f) - 0.5f;
      pos = pos < 0.f ? 0.f : pos;
      const int i0 = (int)pos, i1 = i0 + 1 < 1000 ? i0 + 1 : 999;
      const float w1 = pos - (float)i0, w0 = 1.0f - w1;
      a = fmaf(w0 * src[i0] + w1 * src[i1], wt[i], a);
    }
    cat_inv[t] = a;
    if (t < 256) cat_inv[512 + t] = p.ctx[t];
  }
#pragma unroll
  for (int u = 0; u < LKT_R * 256 / LKT_NT; ++u) {   // low: 16 taps of the row's 4096 channels, straight from global memory
    const int q = t + u * LKT_NT, r = q >> 8, c = q & 255;
    const int row = r0 + r < p.L ? r0 + r : p.L - 1;        // a ragged tail recomputes the last row and stores nothing
    const float4_t* ep = (const float4_t*)(p.e + ((long long)b * p.L + row) * p.lde + 16 * c);
    const float4_t* wp = (const float4_t*)(p.wl + 16 * c);
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4_t ev = ep[k], wv = wp[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) a = fmaf(ev[j], wv[j], a);
    }
    lowT[c * LKT_R + r] = a;
  }
  __syncthreads();
  // 256-point real DFT, bins 0..128, of the rows' low and of low_d, low_f (lk_fuse_kernel's loop and table)
  for (int q = t; q < (LKT_R + 2) * 129; q += LKT_NT) {
    const int s = q / 129, k = q - s * 129;
    const float* x = s < LKT_R ? lowT + s : cat_inv + (s - LKT_R) * 256;
    const int xs = s < LKT_R ? LKT_R : 1;
    float re = 0.f, im = 0.f;
    for (int n = 0; n < 256; ++n) {
      const int j = ((k * n) & 255) * 2;
      const float v = x[n * xs];
      re = fmaf(v, s_tw[j][0], re);
      im = fmaf(-v, s_tw[j][1], im);
    }
    sp[q * 2] = re; sp[q * 2 + 1] = im;
  }
  // spatial = quaternion_linear(low | low_d | low_f | texts): thread = output column
  float spatial[LKT_R];
  {
    float acc[LKT_R];
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) acc[r] = 0.f;
#pragma unroll 8
    for (int i = 0; i < 256; ++i) lkt_fma_rows(lowT + i * LKT_R, p.w_fuse[(long long)i * 512 + t], acc);
    float inv = 0.f;
#pragma unroll 8
    for (int i = 0; i < 768; ++i) inv = fmaf(cat_inv[i], p.w_fuse[(long long)(256 + i) * 512 + t], inv);
    const float bias = p.b_fuse[t];
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) spatial[r] = (acc[r] + inv) + bias;
  }
  __syncthreads();
  // magnitudes / phases (sign convention of the two real bins: see lk_fuse_kernel - im is exactly +0 there)
  for (int q = t; q < (LKT_R + 2) * 129; q += LKT_NT) {
    const int s = q / 129, k = q - s * 129;
    const float re = sp[q * 2], im = sp[q * 2 + 1];
    const float m = hypotf(re, im), ph = atan2f(im, re);
    if (s < LKT_R) {
      if (k < 128) { mpT[k * LKT_R + s] = m; mpT[(128 + k) * LKT_R + s] = ph; }
      else { s_lastr[0][s] = m; s_lastr[1][s] = ph; }
    } else {
      const int j = s - LKT_R;
      if (k < 128) { mpi[j * 128 + k] = m; mpi[384 + j * 128 + k] = ph; }
      else { lasti[j] = m; lasti[3 + j] = ph; }
    }
  }
  if (t < 129) {
    if (t < 128) { mpi[256 + t] = p.cmag[t]; mpi[384 + 256 + t] = p.cpha[t]; }
    else { lasti[2] = p.cmag[128]; lasti[5] = p.cpha[128]; }
  }
  __syncthreads();
  {   // the two quaternion linears on bins 0..127: threads 0..255 a magnitude column, 256..511 a phase column
    const int which = t >> 8, col = t & 255;
    const float* Wm = which ? p.w_pha : p.w_mag;
    float acc[LKT_R];
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) acc[r] = 0.f;
#pragma unroll 8
    for (int i = 0; i < 128; ++i) lkt_fma_rows(mpT + (which * 128 + i) * LKT_R, Wm[i * 256 + col], acc);
    float inv = 0.f;
#pragma unroll 8
    for (int i = 0; i < 384; ++i) inv = fmaf(mpi[which * 384 + i], Wm[(128 + i) * 256 + col], inv);
    const float bias = (which ? p.b_pha : p.b_mag)[col];
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) s_u[(which * LKT_R + r) * 256 + col] = (acc[r] + inv) + bias;   // phase-1 data is dead
    if (col == 0) {   // Linear(4, 1) on bin 128: bias and the three invariant inputs
      const float* l0 = which ? p.l0p : p.l0m;
      float v = l0[4];
#pragma unroll
      for (int j = 0; j < 3; ++j) v = fmaf(lasti[which * 3 + j], l0[1 + j], v);
      s_inv0[which] = v;
    }
  }
  __syncthreads();
  float* const specT = s_b;               // [257][R][2]
#pragma unroll
  for (int u = 0; u < LKT_R * 256 / LKT_NT; ++u) {
    const int q = t + u * LKT_NT, r = q >> 8, k = q & 255;
    float sn, cs;
    sincosf(s_u[(LKT_R + r) * 256 + k], &sn, &cs);
    const float m = s_u[r * 256 + k];
    specT[(k * LKT_R + r) * 2] = m * cs; specT[(k * LKT_R + r) * 2 + 1] = m * sn;
  }
  if (t < LKT_R) {
    const float m0 = fmaf(s_lastr[0][t], p.l0m[0], s_inv0[0]), p0 = fmaf(s_lastr[1][t], p.l0p[0], s_inv0[1]);
    float sn, cs;
    sincosf(p0, &sn, &cs);
    specT[(256 * LKT_R + t) * 2] = m0 * cs; specT[(256 * LKT_R + t) * 2 + 1] = m0 * sn;
  }
  __syncthreads();
  float* const xT = s_u;                  // spatial | freq, [1024][R]
  {   // inverse real DFT of 257 bins -> 512 samples: thread = sample, the twiddle of (k, n) shared by the rows
    const int n = t;
    float acc[LKT_R];
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) acc[r] = 0.f;
    for (int k = 1; k < 256; ++k) {
      const int j = (k * n) & 511;
      const float cs = s_tw[j][0], sn = s_tw[j][1];
      const float* sk = specT + k * LKT_R * 2;
#pragma unroll
      for (int r = 0; r < LKT_R; ++r) {
        acc[r] = fmaf(sk[2 * r], cs, acc[r]);
        acc[r] = fmaf(-sk[2 * r + 1], sn, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) {
      const float ny = specT[(256 * LKT_R + r) * 2];
      const float a = specT[r * 2] + ((n & 1) ? -ny : ny);
      xT[(512 + n) * LKT_R + r] = (a + 2.0f * acc[r]) * (1.0f / 512.0f);
      xT[t * LKT_R + r] = spatial[r];
    }
  }
  __syncthreads();
  float* const hT = s_b;                  // [512][R]
  {   // fuse_sf[0]: Linear(1024 -> 512) + LeakyReLU(0.1), thread = output column
    float acc[LKT_R];
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) acc[r] = 0.f;
#pragma unroll 8
    for (int i = 0; i < 1024; ++i) lkt_fma_rows(xT + i * LKT_R, p.sf0_w[(long long)i * 512 + t], acc);
    const float bias = p.sf0_b[t];
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) {
      const float v = acc[r] + bias;
      hT[t * LKT_R + r] = v > 0.f ? v : 0.1f * v;
    }
  }
  __syncthreads();
  {   // fuse_sf[2]: Linear(512 -> 4096), thread = 8 consecutive output columns (two 16-byte weight pieces, one 16-byte store per row)
    float acc[LKT_R][8];
#pragma unroll
    for (int r = 0; r < LKT_R; ++r)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[r][c] = 0.f;
    const float* wcol = p.sf2_w + 8 * t;
#pragma unroll 2
    for (int i = 0; i < 512; ++i) {
      const float4_t w0 = *(const float4_t*)(wcol + (long long)i * 4096), w1 = *(const float4_t*)(wcol + (long long)i * 4096 + 4);
      const float4_t h0 = *(const float4_t*)(hT + i * LKT_R), h1 = *(const float4_t*)(hT + i * LKT_R + 4);
#pragma unroll
      for (int r = 0; r < LKT_R; ++r) {
        const float hv = r < 4 ? h0[r & 3] : h1[r & 3];
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc[r][c] = fmaf(hv, w0[c], acc[r][c]); acc[r][4 + c] = fmaf(hv, w1[c], acc[r][4 + c]); }
      }
    }
    const float4_t b0 = *(const float4_t*)(p.sf2_b + 8 * t), b1 = *(const float4_t*)(p.sf2_b + 8 * t + 4);
#pragma unroll
    for (int r = 0; r < LKT_R; ++r) {
      if (r0 + r >= p.L) break;
      half8_t o;
#pragma unroll
      for (int c = 0; c < 4; ++c) { o[c] = (half_t)(acc[r][c] + b0[c]); o[4 + c] = (half_t)(acc[r][4 + c] + b1[c]); }
      *(half8_t*)(p.out + ((long long)b * p.L + r0 + r) * p.ldo + 8 * t) = o;
    }
  }
}

extern "C" int lkgd_lk_fuse_tokens(const float* e, int32_t lde, const float* d, const float* f, int32_t B, int32_t L, int32_t Bd,
                                   const float* const* w, void* out, int32_t ldo, lkgd_stream_t stream) {
  if (!e || !d || !f || !w || !out) return LKGD_E_NULL;
  for (int i = 0; i < 18; ++i)
    if (!w[i]) return LKGD_E_NULL;
  if (B <= 0 || L <= 0 || (Bd != 1 && Bd != B) || lde < 4096 || ldo < 4096) return LKGD_E_SHAPE;
  const long long nblk = ((long long)L + LKT_R - 1) / LKT_R;
  if ((long long)B * L > 0x7fffffffll || (long long)B * nblk > 0x7fffffffll) return LKGD_E_SHAPE;
  if (!aligned16(e) || !aligned16(out) || (lde & 3) || (ldo & 7)) return LKGD_E_ALIGN;
  // the operands read in 16-byte pieces: lconv, sf[2] and its bias
  for (int i : {0, 16, 17})
    if (!aligned16(w[i])) return LKGD_E_ALIGN;
  lkt_params p;
  p.e = e; p.d = d; p.f = f; p.lde = lde; p.L = L; p.Bd = Bd; p.nblk = (int)nblk;
  p.wl = w[0]; p.wd = w[1]; p.wf = w[2]; p.ctx = w[3]; p.w_fuse = w[4]; p.b_fuse = w[5]; p.cmag = w[6]; p.cpha = w[7];
  p.w_mag = w[8]; p.b_mag = w[9]; p.w_pha = w[10]; p.b_pha = w[11]; p.l0m = w[12]; p.l0p = w[13];
  p.sf0_w = w[14]; p.sf0_b = w[15]; p.sf2_w = w[16]; p.sf2_b = w[17];
  p.out = (half_t*)out; p.ldo = ldo;
  hipLaunchKernelGGL(lk_fuse_tokens_kernel, dim3((unsigned)(B * nblk)), dim3(LKT_NT), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? LKGD_OK : LKGD_E_LAUNCH;
}
