// init_draw_check.cpp — csrc/init_draw.h as a plain host compiler builds it (tests/test_net_init_cpu.py
// compiles and runs this program):
//   - the normal draw: 200 000 draws of one stream, mean within 5 / sqrt(N) of 0 and variance within
//     5 sqrt(2 / N) of 1 (five standard errors), every draw finite and never 0, the same counters the
//     same bits, another stream or seed another sequence;
//   - the exact-count selection: for m = 1, 64, 65, 700 and e = 0, 1, m - 1, m the number of kept
//     markers equals e, and for 0 < e < m two seeds keep different sets (m = 1 has no such e).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "init_draw.h"

static std::vector<char> keep_exact(uint64_t seed, int32_t branch, int32_t m, int32_t e) {
  std::vector<uint32_t> key(m);
  for (int32_t j = 0; j < m; ++j) key[j] = init_select_key(seed, branch, j);
  std::vector<char> keep(m);
  for (int32_t j = 0; j < m; ++j) {
    int32_t rank = 0;
    for (int32_t i = 0; i < m; ++i) rank += init_key_before(key[i], i, key[j], j) ? 1 : 0;
    keep[j] = rank < e;
  }
  return keep;
}

int main() {
  int bad = 0;
  const int64_t N = 200000;
  const uint64_t stream = INIT_STREAM_THETA | 3u;
  double s = 0.0, q = 0.0;
  int64_t differ = 0, differ_seed = 0;
  for (int64_t i = 0; i < N; ++i) {
    const double z = init_normal(1234, stream, (uint64_t)i);
    if (!std::isfinite(z) || z == 0.0) ++bad;
    if (z != init_normal(1234, stream, (uint64_t)i)) ++bad;
    differ += z != init_normal(1234, INIT_STREAM_THETA | 4u, (uint64_t)i);
    differ_seed += z != init_normal(1235, stream, (uint64_t)i);
    s += z;
    q += z * z;
  }
  const double mean = s / N, var = (q - N * mean * mean) / (N - 1);
  std::printf("normal: N %lld mean %.6f var %.6f\n", (long long)N, mean, var);
  if (std::fabs(mean) > 5.0 / std::sqrt((double)N)) ++bad;
  if (std::fabs(var - 1.0) > 5.0 * std::sqrt(2.0 / N)) ++bad;
  if (differ < N - 10 || differ_seed < N - 10) ++bad;
  // the tails of the inverse distribution function against erfc
  for (const double p : {1e-9, 1e-4, 0.3, 0.5, 0.9, 1.0 - 1e-7}) {
    const double back = 0.5 * std::erfc(-init_ppnd(p) / std::sqrt(2.0));
    if (std::fabs(back - p) > 1e-12 * (p < 0.5 ? p : 1.0) + 1e-16) {
      std::printf("ppnd(%g) reads back %g\n", p, back);
      ++bad;
    }
  }
  for (const int32_t m : {1, 64, 65, 700}) {
    for (const int32_t e : {0, 1, m - 1, m}) {
      const std::vector<char> a = keep_exact(11, 2, m, e), b = keep_exact(12, 2, m, e);
      int32_t ca = 0, cb = 0;
      bool same = true;
      for (int32_t j = 0; j < m; ++j) {
        ca += a[j];
        cb += b[j];
        same = same && a[j] == b[j];
      }
      if (ca != e || cb != e) {
        std::printf("m %d e %d: kept %d / %d\n", m, e, ca, cb);
        ++bad;
      }
      if (e > 0 && e < m && same) {
        std::printf("m %d e %d: two seeds keep the same set\n", m, e);
        ++bad;
      }
    }
  }
  if (bad) {
    std::printf("FAILED %d\n", bad);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
