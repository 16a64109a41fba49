// Device helpers shared by the files that host a generated main loop (tools/gen_*_asm.py -> *.inc): access to the
// accumulation registers the loop leaves its state in, the half-wave exchange, compile-time unrolling and SGPR pointer
// halves.  Everything here is __forceinline__: it leaves no symbol and no instruction of its own in the device code.
// A new loop host includes this header; it does not copy from it (KERNELS.md, "Hosts of a generated statement").
#pragma once
#include <utility>

#include "common.h"

// one accumulation register, by compile-time index: as raw bits, as a float, and written from raw bits
template <int REG>
__device__ __forceinline__ unsigned agpr_read() {
  unsigned v;
  asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(v) : "i"(REG));
  return v;
}
// (its own statement, not a bit cast of agpr_read: attn_spatial_pipe.hip's register allocation differs with the cast)
template <int REG>
__device__ __forceinline__ float agpr_readf() {
  float v;
  asm volatile("v_accvgpr_read_b32 %0, a[%1]" : "=v"(v) : "i"(REG));
  return v;
}
template <int REG>
__device__ __forceinline__ void agpr_write(unsigned v) {
  asm volatile("v_accvgpr_write_b32 a[%1], %0" : : "v"(v), "i"(REG));
}
// one 4-register accumulator fragment a[BASE .. BASE+3] (the host says how its fragments map to BASE)
template <int BASE>
__device__ __forceinline__ float4_t agpr_read4() {
  float a, b, c, d;
  asm volatile("v_accvgpr_read_b32 %0, a[%4]\n\tv_accvgpr_read_b32 %1, a[%4+1]\n\t"
               "v_accvgpr_read_b32 %2, a[%4+2]\n\tv_accvgpr_read_b32 %3, a[%4+3]"
               : "=v"(a), "=v"(b), "=v"(c), "=v"(d)
               : "i"(BASE));
  return (float4_t){a, b, c, d};
}

// v_permlane32_swap_b32: lanes 32..63 of `a` <-> lanes 0..31 of `b`.  Through the builtin, not inline asm: the instruction has
// wait-state requirements after a VALU write of its operands that only the compiler's hazard recogniser sees
__device__ __forceinline__ void swap32(unsigned& a, unsigned& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r[0];
  b = r[1];
}

// compile-time unrolling: f(IC<0>{}), f(IC<1>{}), ... - the index is a type, so it can name a register
template <int V> struct IC { static constexpr int value = V; };
template <class F, int... Is> __device__ __forceinline__ void static_for(F&& f, IC<Is>...) { (f(IC<Is>{}), ...); }
template <class F, int... Is> __device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, Is...>) { (f(IC<Is>{}), ...); }
template <int N, class F> __device__ __forceinline__ void for_n(F&& f) { static_for(f, std::make_integer_sequence<int, N>{}); }

// a wave-uniform 64-bit address as the two SGPR halves an asm statement takes ("s" operands)
struct sgpr_ptr_t { unsigned lo, hi; };
__device__ __forceinline__ sgpr_ptr_t sgpr_ptr(unsigned long long p) {
  return {(unsigned)__builtin_amdgcn_readfirstlane((unsigned)p), (unsigned)__builtin_amdgcn_readfirstlane((unsigned)(p >> 32))};
}
