// fe_util.h — the device helpers of k_forward_fx's tile arithmetic, one definition
// for every kernel that owes its bits (the fx family through fx_tile.h, kernels_fi.hip and, through
// fe_stream.h, kernels_fe.hip and kernels_fs.hip): the row-sum MFMA, the digit
// combine, the lane transpose and the pin of a wave-uniform float.
#pragma once
#include "kernel_util.h"

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

// 64 sum_k A[.][k] of one chunk's digit operands, added to acc: the start of the raw-byte
// (fourth cumulative) accumulator, field 3 being stored as code - 1
__device__ __forceinline__ v4i rowsum64_acc(v4i A, v4i acc) {
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(A, v4i{0x40404040, 0x40404040, 0x40404040, 0x40404040}, acc, 0, 0, 0);
}
__device__ __forceinline__ float comb4(v4i d) {  // sum_d D_d 2^(-7 d)
  return (float)d[0] + (float)d[1] * 0x1p-7f + (float)d[2] * 0x1p-14f + (float)d[3] * 0x1p-21f;
}
__device__ __forceinline__ void swap32(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b),
                                                  false, false);
  a = __builtin_bit_cast(float, (unsigned)r[0]);
  b = __builtin_bit_cast(float, (unsigned)r[1]);
}
__device__ __forceinline__ void swap16(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b),
                                                  false, false);
  a = __builtin_bit_cast(float, (unsigned)r[0]);
  b = __builtin_bit_cast(float, (unsigned)r[1]);
}
__device__ __forceinline__ float sgpr_f(float v) {  // a wave-uniform value, pinned to a scalar register
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
