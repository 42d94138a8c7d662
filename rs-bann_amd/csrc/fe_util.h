// fe_util.h — device helpers shared by the multi-model passes over the fx tile
// images (kernels_fe.hip: forward rows; kernels_fs.hip: branch statistics): the
// row-sum MFMA, the digit combine and the lane transpose of k_forward_fx.
#pragma once
#include "kernel_util.h"

typedef unsigned int v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v4i fe_rowsum64_acc(v4i A, v4i acc) {
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(A, v4i{0x40404040, 0x40404040, 0x40404040, 0x40404040}, acc, 0, 0, 0);
}
__device__ __forceinline__ float fe_comb4(v4i d) {  // sum_d D_d 2^(-7 d)
  return (float)d[0] + (float)d[1] * 0x1p-7f + (float)d[2] * 0x1p-14f + (float)d[3] * 0x1p-21f;
}
__device__ __forceinline__ void fe_swap32(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b),
                                                  false, false);
  a = __builtin_bit_cast(float, (unsigned)r[0]);
  b = __builtin_bit_cast(float, (unsigned)r[1]);
}
__device__ __forceinline__ void fe_swap16(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b),
                                                  false, false);
  a = __builtin_bit_cast(float, (unsigned)r[0]);
  b = __builtin_bit_cast(float, (unsigned)r[1]);
}
