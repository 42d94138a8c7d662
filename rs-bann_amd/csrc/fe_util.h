// fe_util.h — the device helpers of k_forward_fx's tile arithmetic, one definition
// for every kernel that owes its bits (the fx family through fx_tile.h, kernels_fi.hip and, through
// fe_stream.h, kernels_fe.hip and kernels_fs.hip): the row-sum MFMA, the digit
// combine, the lane transpose and the pin of a wave-uniform float.
#pragma once
#include "fx_combine.h"
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
// Z0 of one tile from the cumulative forward's four fragments (fx_tile.h; facc[3] started at the
// rowsum64_acc sum), before the lane transpose: lane (column g, slot i) gets z_q of individual
// 4 i + q.  zk: fx_zk of the column's scale, zbias: its first-layer bias (c0), both the lane's.  Digit
// pairs, field differences on the pairs, one fma per value: fx_combine.h, at most 8 chunks.
__device__ __forceinline__ float fx_zk(float scale) { return scale * 0x1p-7f; }  // once per branch: pairs are in units of digit 1
__device__ __forceinline__ void fx_z0_cum(const v4i (&facc)[4], float zk, float zbias, float& z0, float& z1,
                                          float& z2, float& z3) {
  const int32_t c[4][4] = {{facc[0][0], facc[0][1], facc[0][2], facc[0][3]},
                           {facc[1][0], facc[1][1], facc[1][2], facc[1][3]},
                           {facc[2][0], facc[2][1], facc[2][2], facc[2][3]},
                           {facc[3][0], facc[3][1], facc[3][2], facc[3][3]}};
  int32_t hi[4], lo[4];
  fxc_field_pairs(c, hi, lo);
  z0 = fxc_z0(hi[0], lo[0], 1.f, zk, zbias);  // field q weighs 4^q
  z1 = fxc_z0(hi[1], lo[1], 0.25f, zk, zbias);
  z2 = fxc_z0(hi[2], lo[2], 0.0625f, zk, zbias);
  z3 = fxc_z0(hi[3], lo[3], 0.015625f, zk, zbias);
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
