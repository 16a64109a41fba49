// 16-byte pointer alignment: what the kernels' 16-byte loads and the GEMM planner's applicability rules both ask.  No HIP here.
#pragma once
#include <stdint.h>

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
