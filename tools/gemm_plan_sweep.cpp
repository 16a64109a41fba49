// Walks a grid of descriptors through lkgd_gemm_plan on the host alone and prints a checksum of every answer: the planner
// (lkgd_amd/csrc/gemm_plan.cpp) is pure arithmetic, so it runs under the sanitizers without a device, and two revisions of its
// rules agree on the grid exactly when their checksums are equal.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/gemm_plan_sweep.cpp -o tools/gemm_plan_sweep
//   tools/gemm_plan_sweep          (exit 0; one line: calls, plans, checksum)
//
// Grid: M x N x K x every A mode x each epilogue source (bias, row bias, two residuals) on and off x geglu x cus x with and
// without a workspace.  For the convolution modes the grid's K is the channel count Cin (K = 9 | 3 | 27 x Cin; the 8-channel
// mode has its one K = 128) and the image / frame geometry is the largest of a few that divides M.  Pointers are fake aligned
// addresses: with cus != 0 the planner dereferences none.
#include <cstdint>
#include <cstdio>

#include "../lkgd_amd/csrc/gemm_plan.cpp"

// no device here: the sweep never asks with cus = 0
int lkgd_gemm::gemm_device_cus(int*) { return LKGD_E_LAUNCH; }

static const int MS[] = {1, 31, 128, 257, 4032, 16128, 258048, (1 << 24) - 1, 1 << 24};
static const int NS[] = {4, 8, 128, 160, 256, 320, 324, 1280, 3840};
static const int KS[] = {64, 320, 704, 3840};
static const int CUS[] = {8, 64, 256, 304};
static const int GEGLU[] = {0, 32, 80};
static const int MODES[] = {LKGD_A_PLAIN, LKGD_A_CONV3X3, LKGD_A_TCONV3, LKGD_A_CONV3X3_C8, LKGD_A_CCONV3};

static void* fake(int i) { return (void*)(uintptr_t)((uintptr_t)(i + 1) << 24); }

// the largest w of 32, 16 ... 1 whose square (times f) divides M
static int side(int M, int f) {
  for (int w = 32; w > 1; w >>= 1)
    if (M % (f * w * w) == 0) return w;
  return 1;
}

static lkgd_gemm_desc make(int M, int N, int k, int mode, int src, int geglu, bool ws) {
  lkgd_gemm_desc d = {};
  d.a0 = fake(0); d.w = fake(1); d.out = fake(2); d.zeros = fake(3);
  d.M = M; d.N = N; d.mode = mode;
  d.ldc = N; d.s_acc = 1.f; d.geglu = geglu;
  if (src & 1) d.bias = (const float*)fake(4);
  if (src & 2) { d.rowbias = fake(5); d.ldrb = N; d.rb_d1 = 1; d.rb_d2 = 1; d.rb_md = 1; }
  if (src & 4) { d.res1 = fake(6); d.ldr1 = N; d.r1 = 1.f; }
  if (src & 8) { d.res2 = fake(7); d.ldr2 = N; d.r2 = 1.f; }
  if (ws) { d.workspace = fake(8); d.workspace_bytes = 1LL << 30; }
  const int f = M % 2 ? 1 : 2;                   // frames per batch entry of the two temporal modes
  switch (mode) {
    case LKGD_A_PLAIN: d.K = k; d.lda0 = k; d.csplit = k; break;
    case LKGD_A_CONV3X3:
      d.Cin = k; d.K = 9 * k; d.lda0 = k; d.csplit = k; d.stride = 1;
      d.Hout = d.Wout = d.Hin = d.Win = side(M, 1);
      break;
    case LKGD_A_TCONV3:
      d.Cin = k; d.K = 3 * k; d.lda0 = k; d.csplit = k;
      d.F = d.Floc = f; d.HW = M / f;
      break;
    case LKGD_A_CONV3X3_C8:
      d.Cin = 8; d.K = 128; d.lda0 = 8; d.csplit = 8; d.stride = 1;
      d.Hout = d.Wout = d.Hin = d.Win = side(M, 1);
      break;
    case LKGD_A_CCONV3:
      d.Cin = k; d.K = 27 * k; d.lda0 = k; d.csplit = k; d.stride = 1;
      d.Floc = f; d.F = f + 2;
      d.Hout = d.Wout = d.Hin = d.Win = side(M, f);
      break;
  }
  return d;
}

int main() {
  uint64_t sum = 1469598103934665603ull;         // FNV-1a over every answer
  auto mix = [&](int v) { sum = (sum ^ (uint32_t)v) * 1099511628211ull; };
  long calls = 0, plans = 0;
  for (int M : MS) for (int N : NS) for (int k : KS) for (int mode : MODES)
    for (int src = 0; src < 16; ++src) for (int geglu : GEGLU) for (int ws = 0; ws < 2; ++ws) {
      const lkgd_gemm_desc d = make(M, N, k, mode, src, geglu, ws != 0);
      for (int cus : CUS) {
        lkgd_gemm_plan_info p = {};
        const int rc = lkgd_gemm_plan(&d, cus, &p);
        ++calls;
        mix(rc);
        if (rc != LKGD_OK) continue;
        ++plans;
        if (p.program < LKGD_GEMM_TILE128 || p.program > LKGD_GEMM_MID || p.k_slices < 1 || p.tile_m <= 0 || p.tile_n <= 0) return 1;
        mix(p.program); mix(p.k_slices); mix(p.tile_m); mix(p.tile_n); mix(p.colstats_block); mix(p.lds_out);
      }
    }
  printf("%ld calls, %ld plans, checksum %016llx\n", calls, plans, (unsigned long long)sum);
  return 0;
}
