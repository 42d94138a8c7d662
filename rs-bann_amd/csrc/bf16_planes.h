// bf16_planes.h — an f32 value as three bf16 planes and the transposing LDS read of bf16 fragments,
// shared by the kernels that run f32-accurate GEMMs on v_mfma_f32_16x16x32_bf16: the gx masked and hidden
// layers (kernels_gx_b3.hip, kernels_gx.hip, the pre-split weights of kernels_gx_head.hip) and the
// wide fused kernel (kernels_wx.hip, which splits four values at a time with its own split3x4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// x = hi + mid + lo exactly, by truncation: hi = the top 8 significant bits, mid
// the next 8 of the (exact) remainder, lo the last 8 (representable as is): two
// ANDs and two subtractions, no conversions; each plane is the high half of an
// f32 word
__device__ __forceinline__ void split3(float x, __bf16& hi, __bf16& mi, __bf16& lo) {
  const uint32_t hb = __float_as_uint(x) & 0xFFFF0000u;
  const float r = x - __uint_as_float(hb);  // exact
  const uint32_t mb = __float_as_uint(r) & 0xFFFF0000u;
  const uint32_t lb = __float_as_uint(r - __uint_as_float(mb));  // exact, <= 8 significant bits
  hi = __builtin_bit_cast(__bf16, (uint16_t)(hb >> 16));
  mi = __builtin_bit_cast(__bf16, (uint16_t)(mb >> 16));
  lo = __builtin_bit_cast(__bf16, (uint16_t)(lb >> 16));
}

typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;
// 16-lane-group transposing read (two ds_read_b64_tr_b16): lane 4q + p of a group gives the LDS address
// of row q, columns 4p .. 4p+3 of a 4 x 16 block of bf16; lane i receives column i, row q in element q.
// Two of them stacked (rows 0..3 at p0, 4..7 at p1) = one 8-deep bf16 MFMA fragment along the rows.
__device__ __forceinline__ bf16x8 tr16_pair(const void* p0, const void* p1) {
  const v4s a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(p0));
  const v4s b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(p1));
  typedef short v8s __attribute__((ext_vector_type(8)));
  const v8s r = v8s{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, r);
}
