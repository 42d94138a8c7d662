// fx_combine_check.cpp — host check of the digit-pair combine (rs-bann_amd/csrc/fx_combine.h), the
// arithmetic that turns the forward's int32 digit sums into Z0 in every fx-shaped kernel.  Built and
// run by tests/test_fx_combine_cpu.py with -fsanitize=address,undefined; no GPU, no HIP.
//
// A fragment set is what the forward's MFMAs leave: for each digit d the cumulative sums C_q[d] of
// digit x (operand byte & mask_q) over the markers.  Field q of the byte sits in place, so the field
// sums are F_q = C_q - C_(q-1) = 4^q S_q with S_q[d] = sum digit_d x (2-bit field value).
//
// Case 1: random sets drawn at the header's bound for genotype codes: |digit 0| <= 127, the other
//         digits <= 64, field values <= 2, 512 markers, i.e. |S_q[d]| <= digit x 2 x 512; a tenth of
//         the draws at the bound itself.
// Case 1b (integers only): the same with field values up to 3, whatever a 2-bit field can hold: the
//         int32 bound FXC_PAIR_MAX.  (Above codes a pair no longer converts exactly, and a value
//         whose hi and lo parts cancel is then not within an ulp: measured here on unstructured
//         draws at 3/2 x 2^22 per digit sum, 65 of 12 million values were off by more.)
// Case 2: the extreme tiles: every digit at +-(127, 64, 64, 64) in all 16 sign patterns, every
//         marker's operand byte 0x7F (every cumulative fragment at its maximum: 3, 15, 63, 127),
//         0x80 (the raw byte's minimum, -128) and 0x6A (every genotype code 2), 512 markers, the raw
//         fragment on top of its 64 x row-sum start.
// For each: the pair-combined field integers equal an int64 reference exactly, and the float value
// is within 1 ulp of the exact int64 value converted once.  The value of a field that weighs 4^q,
// taken back by w = 4^-q, has the bits of the x 16 form k_forward_fi computes.  The largest |hi| and
// |lo| seen are printed and must be below 2^31.
#include <inttypes.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "fx_combine.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng_next() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
static int64_t rng_sym(int64_t bound) {  // uniform in [-bound, bound]
  return (int64_t)(rng_next() % (uint64_t)(2 * bound + 1)) - bound;
}

static int64_t max_hi = 0, max_lo = 0;
static long long n_checked = 0;
static int failures = 0;

static int64_t abs64(int64_t v) { return v < 0 ? -v : v; }
static uint32_t fbits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
static float ulp_of(float x) {
  const float a = fabsf(x);
  return nextafterf(a, INFINITY) - a;
}

#define CHECK(cond, ...)              \
  do {                                \
    if (!(cond)) {                    \
      if (failures < 10) {            \
        fprintf(stderr, "FAIL: ");    \
        fprintf(stderr, __VA_ARGS__); \
        fprintf(stderr, "\n");        \
      }                               \
      ++failures;                     \
    }                                 \
  } while (0)

// F[q][d]: the true field digit sums.  The cumulative fragments are their running sums, held in
// int32 as the MFMA accumulators hold them.
static void check_fields(const int64_t (&F)[4][4], bool check_float) {
  int32_t c[4][4];
  int64_t run[4] = {0, 0, 0, 0};
  for (int q = 0; q < 4; ++q)
    for (int d = 0; d < 4; ++d) {
      run[d] += F[q][d];
      c[q][d] = (int32_t)(uint32_t)(uint64_t)run[d];  // two's complement, as the accumulator wraps
    }
  int32_t hi[4], lo[4];
  fxc_field_pairs(c, hi, lo);
  for (int q = 0; q < 4; ++q) {
    const int64_t H = F[q][0] * 128 + F[q][1], L = F[q][2] * 128 + F[q][3];
    if (abs64(H) > max_hi) max_hi = abs64(H);
    if (abs64(L) > max_lo) max_lo = abs64(L);
    CHECK(H == (int64_t)hi[q] && L == (int64_t)lo[q], "pairs q=%d: hi %d (want %" PRId64 "), lo %d (want %" PRId64 ")",
          q, hi[q], H, lo[q], L);
    if (!check_float) continue;
    // the exact value in units of digit 3 (2^-21), converted once, against the pair combine
    const int64_t N = H * 16384 + L;  // |N| < 2^45
    const float ref = (float)N * 0x1p-14f, got = fxc_value(hi[q], lo[q]);
    CHECK(fabsf(got - ref) <= ulp_of(ref), "value q=%d: got %a, exact once-rounded %a (N = %" PRId64 ")", q, got, ref, N);
  }
  ++n_checked;
}

// the bits two kernels must share: a field that weighs 4^q, taken back by w = 4^-q, against the same
// digit sums x 16 scaled by k / 16 (k_forward_fi's form)
static void check_weight_invariance(const int64_t (&S)[4], float k, float bias) {
  const float w[4] = {1.f, 0.25f, 0.0625f, 0.015625f};
  int32_t s16[4];
  for (int d = 0; d < 4; ++d) s16[d] = (int32_t)(16 * S[d]);
  const float zi = fxc_z0(fxc_pair(s16[0], s16[1]), fxc_pair(s16[2], s16[3]), 1.f, k * 0.0625f, bias);
  for (int q = 0; q < 4; ++q) {
    int32_t f[4];
    for (int d = 0; d < 4; ++d) f[d] = (int32_t)(S[d] * ((int64_t)1 << (2 * q)));
    const float zq = fxc_z0(fxc_pair(f[0], f[1]), fxc_pair(f[2], f[3]), w[q], k, bias);
    CHECK(fbits(zq) == fbits(zi), "weight q=%d: %a vs x16 form %a", q, zq, zi);
  }
}

int main() {
  const int64_t markers = (int64_t)FXC_CHUNK_MARKERS * FXC_MAX_CHUNKS;
  const int64_t dmax[4] = {FXC_DIGIT0_MAX, FXC_DIGIT_MAX, FXC_DIGIT_MAX, FXC_DIGIT_MAX};
  // ---- case 1, 1b ----
  const long long NR = 3000000;
  for (long long i = 0; i < NR; ++i) {
    const int fmax = (i & 3) == 3 ? FXC_FIELD_MAX : FXC_CODE_MAX;  // every fourth set: case 1b
    int64_t F[4][4], S0[4];
    for (int q = 0; q < 4; ++q)
      for (int d = 0; d < 4; ++d) {
        const uint64_t r = rng_next();
        const int64_t smax = dmax[d] * fmax * markers;
        const int64_t s = (r % 10 == 0) ? ((r & 16) ? smax : -smax) : rng_sym(smax);
        F[q][d] = s * ((int64_t)1 << (2 * q));
        if (q == 0) S0[d] = s;
      }
    check_fields(F, fmax == FXC_CODE_MAX);
    if ((i & 7) == 0) {
      const float k = ldexpf(1.f + (float)(rng_next() % 1000) / 1000.f, (int)(rng_next() % 24) - 20);
      const float bias = (float)rng_sym(1000) / 256.f;
      check_weight_invariance(S0, k, bias);
    }
  }
  // ---- case 2 ----
  const int tiles[3] = {0x7F, 0x80, 0x6A};
  for (int t = 0; t < 3; ++t)
    for (int signs = 0; signs < 16; ++signs) {
      const int x = tiles[t];
      const int64_t bytes[4] = {x & 0x03, x & 0x0F, x & 0x3F, (int64_t)(int8_t)(uint8_t)x};
      int64_t F[4][4], prev[4] = {0, 0, 0, 0};
      for (int q = 0; q < 4; ++q)
        for (int d = 0; d < 4; ++d) {
          const int64_t a = (signs >> d & 1) ? -dmax[d] : dmax[d];
          // cumulative fragment q: digit x byte over every marker; the raw byte's starts at 64 x the row sum
          const int64_t cq = a * markers * (bytes[q] + (q == 3 ? 64 : 0));
          F[q][d] = cq - prev[d];
          CHECK(abs64(F[q][d]) <= FXC_SUM_MAX, "case 2: field sum %" PRId64 " above the header's bound", F[q][d]);
          prev[d] = cq;
        }
      check_fields(F, true);
    }
  printf("checked %lld fragment sets\n", n_checked);
  printf("max |hi| = %" PRId64 ", max |lo| = %" PRId64 " (bound %" PRId64 ", 2^31 = %" PRId64 ")\n", max_hi, max_lo,
         (int64_t)FXC_PAIR_MAX, (int64_t)1 << 31);
  CHECK(max_hi < ((int64_t)1 << 31) && max_lo < ((int64_t)1 << 31), "a pair left int32");
  CHECK(max_hi <= FXC_PAIR_MAX && max_lo <= FXC_PAIR_MAX, "a pair above the header's bound");
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
