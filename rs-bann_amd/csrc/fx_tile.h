// fx_tile.h — the 2-bit genotype tile image of the fx family and the device helpers that more
// than one of its kernels uses: k_fused_grad_fx (kernels_fx.hip), k_forward_fx
// (kernels_fx_fwd.hip), k_forward_gsum (kernels_fx_gsum.hip), k_fused_grad_fxl
// (kernels_fxl.hip) and k_fused_grad_fxh (kernels_fxh.hip).  The counted vector-memory wait
// they share with the multi-model passes is vm_wait (kernel_util.h).
//
// Genotype tile image (HBM == LDS, 16 B per marker row, "u2t" layout):
//   row j (marker) = 16 quads Q; quad Q = individuals 4Q .. 4Q+3 as 2-bit
//   codes at bits 2p (p = individual - 4Q).  Rows are stored in 16-row windows
//   w = j >> 4 at position P = ((j & 15) + 8 (w & 1)) & 15, and the two 8-byte
//   halves of a row at position P >= 8 are swapped (bank-conflict-free reads).
//   * forward B operand (K = 64 markers, N = 16 individuals): two
//     ds_read_b64_tr_b8 per chunk give lane (g, i) the quad-i byte of the 16
//     markers of window 4c + g; (x >> 2q) & 0x03030303 is the i8 operand of
//     individual 4i + q ("fragment" q).
//   * backward B operand (K = 64 individuals, N = 16 markers): one ds_read_b32
//     gives lane (r, n) quads 4r .. 4r+3 of marker 16u + n; (w >> 2p) &
//     0x03030303 holds individuals 16r + 4b + p (byte b), K slot 16r + 4p + b.
//     Fields p = 1, 2 are used in place (w & 0x0C0C0C0C = 4 x code, w &
//     0x30303030 = 16 x code); the delta0 digits of those individuals are taken
//     at a 4^p smaller scale, so the MFMA sum is unchanged.  The delta0 digit
//     operand A is written in the same K order.
#pragma once
#include "fe_util.h"

#define FX_WAVES 4        // waves per workgroup (one work item, tiles interleaved)
#define FX_SLOT 8192      // one tile image at <= 8 chunks (512 markers x 16 B)
constexpr int FXL_PD = 8;  // fxl, fxh: the backward reads its genotype windows this many windows ahead

// Field 3 of every fx / fxl / fxh tile image is stored as code - 1 (k_pack_tiles, PackJob::f3m1):
// read as a signed int8, a genotype byte is then f0 + 4 f1 + 16 f2 + 64 (f3 - 1) (codes <= 2, so
// the 2-bit field holds -1 .. 1).  The forward takes CUMULATIVE fragments -- x & 0x03, x & 0x0F,
// x & 0x3F and the raw byte: 3 ANDs per dword instead of 5 -- and recovers the in-place fields
// exactly in int32 once per tile: F1 = C1 - C0, F2 = C2 - C1, F3 = C3 - C2 with C3 started at
// 64 sum_k A (the W0-digit row sums over the wave's chunks, rowsum64_acc), so F_q = 4^q S_q.  With
// at most 8 chunks the four digits of a fragment are first combined in pairs in int32, the
// differences are taken on the pairs and Z0 comes out of one fma per pair of pairs with the bias as
// its addend (fx_z0_cum, fe_util.h; the arithmetic and its bounds: fx_combine.h); the wide items
// of fxl / fxh take the differences per digit (fx_fwd_fields) and the four-digit combine (comb4).
// The backward keeps field 3 in place too (x & 0xC0 = 64 (f3 - 1):
// one AND instead of a shift and an AND), with the delta0 digits of K-group 3 pre-divided by 64;
// the -1 comes back as 64 sum_(i in group 3) digit_i, one MFMA per tile against FX_ONES3, added
// to every marker's digit sums at the end.

#define FX_ONES3 (v4i{0, 0, 0, 0x40404040})  // 64 in every K slot of field 3 (the backward's group 3)

// one chunk of the forward: the four cumulative fragments of a quad-byte operand
__device__ __forceinline__ void fx_fwd_chunk(v4i A, v4u X, v4i (&facc)[4]) {
  facc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, (v4i)(X & 0x03030303u), facc[0], 0, 0, 0);
  facc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, (v4i)(X & 0x0F0F0F0Fu), facc[1], 0, 0, 0);
  facc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, (v4i)(X & 0x3F3F3F3Fu), facc[2], 0, 0, 0);
  facc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, (v4i)X, facc[3], 0, 0, 0);
}
// cumulative sums -> in-place fields F_q = 4^q S_q (facc[3] started at the rowsum64_acc sum), digit by
// digit: fxl and fxh, whose items are wider than the pair combine's 8 chunks
__device__ __forceinline__ void fx_fwd_fields(v4i (&facc)[4]) {
  facc[3] -= facc[2];
  facc[2] -= facc[1];
  facc[1] -= facc[0];
}
// the backward's fragments of one window dword: every field in place (x 1, 4, 16, and
// 64 (f3 - 1)); the delta0 digits of K-group p carry 4^-p (p = 3: 64^-1)
__device__ __forceinline__ v4i fx_bwd_unpack(uint32_t wv) {
  return v4i{(int)(wv & 0x03030303u), (int)(wv & 0x0C0C0C0Cu), (int)(wv & 0x30303030u), (int)(wv & 0xC0C0C0C0u)};
}

// delta0 digits: V = rint(x 2^e), |V| < 2^27, as four signed 8-bit digits
// V = d0 + d1 2^8 + d2 2^16 + d3 2^24 (byte d = digit d, d0..d2 in [-128, 127],
// d3 in [-8, 8]): offsetting the three low bytes by 128 and flipping their top
// bits is the whole recoding, 2 VALU
__device__ __forceinline__ uint32_t digits4_fx(float x, int e) {
  const int V = (int)__builtin_rintf(__builtin_amdgcn_ldexpf(x, e));
  return ((uint32_t)V + 0x00808080u) ^ 0x00808080u;
}

// value(G) of digit sums G (digit d weighs 2^(8 d)), rounded once: the digit sums
// grow past 2^24 over an item's tiles (in-place fields weigh up to 48), where a
// per-digit float conversion would round each one
__device__ __forceinline__ float comb4_exact(v4i G) {
  const int64_t N = (int64_t)G[0] + ((int64_t)G[1] << 8) + ((int64_t)G[2] << 16) + ((int64_t)G[3] << 24);
  return (float)N;
}
// the same for two digit-sum vectors (a window's sums and the item's K-group-3 correction)
__device__ __forceinline__ float comb4_exact2(v4i G, v4i H) {
  const int64_t N = (int64_t)G[0] + ((int64_t)G[1] << 8) + ((int64_t)G[2] << 16) + ((int64_t)G[3] << 24) +
                    (int64_t)H[0] + ((int64_t)H[1] << 8) + ((int64_t)H[2] << 16) + ((int64_t)H[3] << 24);
  return (float)N;
}

// value(G) * 2^-sh for digit sums G, sh >= 0: form N in int64 (|G_d| < 2^31),
// shift it, and re-split into 8-bit digits (exact up to the dropped low bits, < 1
// of the new unit).  Branch- and loop-free so the accumulators are updated in place.
__device__ __forceinline__ v4i shr_digits(v4i G, int sh) {
  const int64_t N = (int64_t)G[0] + ((int64_t)G[1] << 8) + ((int64_t)G[2] << 16) + ((int64_t)G[3] << 24);
  const int64_t M = N >> (sh < 63 ? sh : 63);
  return v4i{(int)(M & 255), (int)((M >> 8) & 255), (int)((M >> 16) & 255), (int)(M >> 24)};
}
