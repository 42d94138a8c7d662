// gibbs_gamma.h — the Gamma sampler of the device Gibbs step (kernels_gibbs.hip), host and
// device: Marsaglia-Tsang (2000) in f64 on the Philox counters of rng.h.  A draw is a pure
// function of (seed, stream, shape): every rejection attempt takes the next counter of the
// stream, so the result does not depend on the launch geometry or on any other draw.  Plain
// host compilers can include it (g++ -I <rocm>/include -D__HIP_PLATFORM_AMD__;
// tests/gibbs_gamma_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "rng.h"

// attempts per draw: one fails with probability < 0.26 (the polar normal's pi / 4 times the
// squeeze's >= 0.95), so the cap is never reached in practice; it bounds the device loop
#define GIBBS_GAMMA_MAX_ATTEMPTS 256

// stream of a precision draw: (branch index in the context, index in precision_vec)
__host__ __device__ inline uint64_t gibbs_stream(int32_t branch, int32_t q) {
  return ((uint64_t)(uint32_t)branch << 32) | (uint64_t)(uint32_t)q;
}

// uniform strictly inside (0, 1), 32-bit resolution
__host__ __device__ inline double gibbs_u01(uint32_t x) { return ((double)x + 0.5) * (1.0 / 4294967296.0); }

// Gamma(shape, 1), shape > 0.  One Philox block per attempt: x, y -> a standard normal by the
// polar method (no trigonometric function), z -> the acceptance uniform, w -> the uniform of the
// shape < 1 boost (Gamma(a) = Gamma(a + 1) U^(1/a)), taken from the accepting attempt.
// attempts_out (nullable): the counters consumed.
__host__ __device__ inline double gibbs_gamma_std(double shape, uint64_t seed, uint64_t stream,
                                                  int32_t* attempts_out) {
  const bool boost = shape < 1.0;
  const double a = boost ? shape + 1.0 : shape;
  const double d = a - 1.0 / 3.0;
  const double c = 1.0 / sqrt(9.0 * d);
  double g = d;  // the cap's fallback (the mode region); unreachable in practice
  int32_t k = 0;
  for (; k < GIBBS_GAMMA_MAX_ATTEMPTS; ++k) {
    const u32x4 r = philox_bits(seed, stream, (uint64_t)k);
    const double p = 2.0 * gibbs_u01(r.x) - 1.0, q = 2.0 * gibbs_u01(r.y) - 1.0;
    const double s = p * p + q * q;
    if (s >= 1.0 || s <= 0.0) continue;
    const double x = p * sqrt(-2.0 * log(s) / s);
    double v = 1.0 + c * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    const double u = gibbs_u01(r.z);
    const double x2 = x * x;
    if (u < 1.0 - 0.0331 * x2 * x2 || log(u) < 0.5 * x2 + d * (1.0 - v + log(v))) {
      g = d * v;
      if (boost) g *= exp(log(gibbs_u01(r.w)) / shape);
      ++k;
      break;
    }
  }
  if (attempts_out) *attempts_out = k;
  return g;
}

// one precision: Gamma(shape, scale) rounded to f32 once, as the host path's (float)draw_gamma
__host__ __device__ inline float gibbs_gamma_f32(double shape, double scale, uint64_t seed, uint64_t stream) {
  return (float)(gibbs_gamma_std(shape, seed, stream, nullptr) * scale);
}
