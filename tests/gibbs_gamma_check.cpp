// Stand-alone host check of csrc/gibbs_gamma.h (built and run by tests/test_gibbs_cpu.py): the
// Gamma sampler of the device Gibbs step, compiled by the host C++ compiler.  For the shape
// classes the Gibbs step meets (0.501: width-1 layers through the shape < 1 boost; 1.0; 2.001;
// 250.001; 1000.001) N = 200 000 variates at scale 1 from fixed seeds: the sample mean within
// 5 sqrt(a / N) of a and the sample variance within 5 sqrt((2 a^2 + 6 a) / N) of a -- five standard
// errors from the Gamma's exact second and fourth central moments (mu_2 = a, mu_4 = 3 a^2 + 6 a, so
// Var(s^2) ~ (mu_4 - mu_2^2) / N) -- every draw finite and > 0, and the same counters give the same bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gibbs_gamma.h"

int main() {
  const double shapes[] = {0.501, 1.0, 2.001, 250.001, 1000.001};
  const int N = 200000;
  int bad = 0;
  for (int si = 0; si < 5; ++si) {
    const double a = shapes[si];
    const uint64_t seed = 0x5EEDull + 977ull * (uint64_t)si;
    std::vector<float> v(N);
    int64_t attempts = 0;
    for (int i = 0; i < N; ++i) {
      const uint64_t stream = gibbs_stream(i >> 9, i & 511);
      int32_t k = 0;
      const double g = gibbs_gamma_std(a, seed, stream, &k);
      attempts += k;
      v[i] = gibbs_gamma_f32(a, 1.0, seed, stream);
      if (v[i] != (float)g) {
        std::printf("shape %g draw %d: the f32 draw is not the rounded f64 draw\n", a, i);
        ++bad;
      }
      if (!std::isfinite(v[i]) || !(v[i] > 0.f)) {
        std::printf("shape %g draw %d: %g is not finite and positive\n", a, i, (double)v[i]);
        ++bad;
      }
      if (k < 1 || k >= GIBBS_GAMMA_MAX_ATTEMPTS) {
        std::printf("shape %g draw %d: %d attempts\n", a, i, k);
        ++bad;
      }
    }
    double mean = 0.0;
    for (float x : v) mean += x;
    mean /= N;
    double var = 0.0;
    for (float x : v) var += (x - mean) * (x - mean);
    var /= (N - 1);
    const double tm = 5.0 * std::sqrt(a / N), tv = 5.0 * std::sqrt((2.0 * a * a + 6.0 * a) / N);
    std::printf("shape %.3f mean %.6f (|err| %.3g <= %.3g) var %.6f (|err| %.3g <= %.3g) attempts/draw %.3f\n", a, mean,
                std::fabs(mean - a), tm, var, std::fabs(var - a), tv, (double)attempts / N);
    if (!(std::fabs(mean - a) <= tm) || !(std::fabs(var - a) <= tv)) ++bad;
    // the same counters, the same bits; another seed or stream, another draw somewhere
    int same = 0, other_seed = 0, other_stream = 0;
    for (int i = 0; i < 4096; ++i) {
      const uint64_t stream = gibbs_stream(i >> 9, i & 511);
      const float w = gibbs_gamma_f32(a, 1.0, seed, stream);
      same += std::memcmp(&w, &v[i], sizeof(float)) == 0;
      const float s2 = gibbs_gamma_f32(a, 1.0, seed + 1, stream);
      other_seed += std::memcmp(&s2, &v[i], sizeof(float)) != 0;
      const float t2 = gibbs_gamma_f32(a, 1.0, seed, gibbs_stream((i >> 9) + 1000, i & 511));
      other_stream += std::memcmp(&t2, &v[i], sizeof(float)) != 0;
    }
    if (same != 4096 || other_seed < 4000 || other_stream < 4000) {
      std::printf("shape %g: repeat %d / 4096 equal, other seed %d, other stream %d differ\n", a, same, other_seed,
                  other_stream);
      ++bad;
    }
  }
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
