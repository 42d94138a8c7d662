// fx_combine.h — Z0 from the forward's digit sums: the one definition of how the four digit sums of
// a first-layer input become a float, for every kernel that computes an fx-shaped branch's Z0
// (k_fused_grad_fx, k_forward_fx, k_forward_gsum, fe_head of k_forward_fe / k_stats_fe, and
// k_forward_fi).  Plain C++ with no HIP call: tests/fx_combine_check.cpp includes it on the host.
//
// A W0 / sigma entry is four signed digits in base 2^7, most significant first (the digit image,
// kernels_update.hip: |digit 0| <= 127, the others <= 64), so a column's sum over markers is
// D0 + D1 2^-7 + D2 2^-14 + D3 2^-21 with int32 digit sums D_d.  The digit sums are combined in
// PAIRS in int32 first,
//     hi = D0 2^7 + D1        lo = D2 2^7 + D3        value = (hi + lo 2^-14) 2^-7,
// each pair converts to float once, and one fma joins them: 2 + 2 + 1 vector instructions per
// value instead of the 4 conversions + 3 multiply-adds of the per-digit combine (comb4, fe_util.h),
// and the field differences of the cumulative forward (fx_tile.h) are taken on 2 registers per
// fragment instead of 4.
//
// Bounds, for an item of at most FXC_MAX_CHUNKS chunks.  A field of the forward is a 2-bit value
// (<= 3; a genotype code <= FXC_CODE_MAX) in place, x 4^q for fragment q <= 3, summed over at most
// 512 markers against one digit.  So a field's pair is 4^q P with
//     |P| <= FXC_PAIR_UNIT x (field value) x 512,   FXC_PAIR_UNIT = 127 x 2^7 + 64:
//   * int32: 64 x FXC_PAIR_UNIT x 3 x 512 < 2^31 whatever the 2-bit fields hold (FXC_PAIR_MAX).  The
//     cumulative sums' own pairs may wrap; their differences are taken in wrapping (unsigned)
//     arithmetic, so only the field's pair has to fit.
//   * float: with genotype codes (<= 2) |P| <= FXC_PAIR_UNIT x 2 x 512 < 2^24, and 4^q P converts
//     exactly.  The only roundings of Z0 are then the two fmas' (value, then value x scale + bias):
//     the value is the correctly rounded exact sum, where the per-digit combine rounded three times.
// Neither holds for the wide items of fxl / fxh (up to 32 chunks): they keep the four-digit combine.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FXC_HD __host__ __device__ inline
#else
#define FXC_HD inline
#endif

constexpr int FXC_DIGIT0_MAX = 127;    // |digit 0| of a W0 / sigma entry (the column scale: max / s <= 127)
constexpr int FXC_DIGIT_MAX = 64;      // |digit 1 .. 3| (the remainder of a rint, x 128)
constexpr int FXC_FIELD_MAX = 3;       // a 2-bit field
constexpr int FXC_CODE_MAX = 2;        // a genotype code (field 3 is stored as code - 1 and comes back as code)
constexpr int FXC_CHUNK_MARKERS = 64;  // markers per chunk (one MFMA's K)
constexpr int FXC_MAX_CHUNKS = 8;      // chunks of an item that takes the pair combine (512 markers)

constexpr int64_t FXC_PAIR_UNIT = (int64_t)FXC_DIGIT0_MAX * 128 + FXC_DIGIT_MAX;
// the largest |digit sum| and |pair| of a field in place (fragment 3: x 64), any 2-bit field values
constexpr int64_t FXC_SUM_MAX = (int64_t)64 * FXC_DIGIT0_MAX * FXC_FIELD_MAX * FXC_CHUNK_MARKERS * FXC_MAX_CHUNKS;
constexpr int64_t FXC_PAIR_MAX = (int64_t)64 * FXC_PAIR_UNIT * FXC_FIELD_MAX * FXC_CHUNK_MARKERS * FXC_MAX_CHUNKS;
// the largest |pair| / 4^q with genotype codes
constexpr int64_t FXC_PAIR_EXACT_MAX = FXC_PAIR_UNIT * FXC_CODE_MAX * FXC_CHUNK_MARKERS * FXC_MAX_CHUNKS;
static_assert(FXC_MAX_CHUNKS <= 8 && FXC_PAIR_MAX < ((int64_t)1 << 31),
              "a digit pair of an item with this many chunks no longer fits int32: keep the four-digit combine");
static_assert(FXC_PAIR_EXACT_MAX < ((int64_t)1 << 24),
              "a digit pair of an item with this many chunks no longer converts to float exactly");

// two neighbouring digit sums as one int32: a 2^7 + b (v_lshl_add_u32)
FXC_HD int32_t fxc_pair(int32_t a, int32_t b) { return (int32_t)(((uint32_t)a << 7) + (uint32_t)b); }
// the difference of two pairs (or digit sums): wrap in the operands cancels when the result fits
FXC_HD int32_t fxc_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
// the value of a pair of pairs in units of digit 1 (2^-7): hi + lo 2^-14
FXC_HD float fxc_value(int32_t hi, int32_t lo) { return fmaf((float)lo, 0x1p-14f, (float)hi); }
// the first-layer input of one individual and column: (value x w) x k + bias, the last two in one
// fma.  w: the exact power of two that undoes the field's weight (4^-q for fragment q of the
// cumulative forward; 1 folds away), applied to the value so that the kernels keep ONE scale
// register per lane instead of four; k: the column's scale x 2^-7; bias: its first-layer bias.
FXC_HD float fxc_z0(int32_t hi, int32_t lo, float w, float k, float bias) {
  return fmaf(fxc_value(hi, lo) * w, k, bias);
}

// The four fragments of the cumulative forward (C_q: digit sums of x & 0x03, x & 0x0F, x & 0x3F and
// the raw byte, four digits each): the pairs of the in-place fields F_q = C_q - C_(q-1) = 4^q S_q,
// differences taken on the pairs.  hi[q], lo[q] equal the pairs of F_q's own digits.
FXC_HD void fxc_field_pairs(const int32_t (&c)[4][4], int32_t (&hi)[4], int32_t (&lo)[4]) {
  int32_t ch[4], cl[4];
  for (int q = 0; q < 4; ++q) {
    ch[q] = fxc_pair(c[q][0], c[q][1]);
    cl[q] = fxc_pair(c[q][2], c[q][3]);
  }
  hi[0] = ch[0];
  lo[0] = cl[0];
  for (int q = 1; q < 4; ++q) {
    hi[q] = fxc_sub(ch[q], ch[q - 1]);
    lo[q] = fxc_sub(cl[q], cl[q - 1]);
  }
}
