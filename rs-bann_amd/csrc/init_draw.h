// init_draw.h — the draws of the device model initialisation (kernels_init.hip), host and
// device: standard normals and marker-selection keys on the Philox counters of rng.h.  A draw
// is a pure function of (seed, stream, index): nothing depends on the launch geometry or on
// any other draw.  Plain host compilers can include it (g++ -I <rocm>/include
// -D__HIP_PLATFORM_AMD__; tests/init_draw_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "rng.h"

// Streams.  Bit 63 is set, which no other stream of the library has: the momentum and
// Metropolis streams are small constants plus a branch index (kernels_update.hip), the Gibbs
// streams (branch << 32 | entry) with branch < 2^31 (gibbs_gamma.h), the synthetic cohort's
// (marker << 8 | attempt) and a constant below 2^48 (kernels_data.hip).
#define INIT_STREAM_THETA 0xB100000000000000ull   // | branch: the parameters, counter = entry / 4
#define INIT_STREAM_SELECT 0xB200000000000000ull  // | branch: the marker keys, counter = marker
#define INIT_STREAM_NOISE 0xB300000000000000ull   // the phenotype noise, counter = individual / 4
#define INIT_STREAM_EFFECT 0xB400000000000000ull  // the linear model's effects (kernels_lin.hip), counter = entry / 4
#define INIT_STREAM_INCLUDE 0xB500000000000000ull // its inclusion keys, counter = entry

__host__ __device__ inline uint32_t init_word(const u32x4& r, uint32_t k) {
  return k == 0 ? r.x : (k == 1 ? r.y : (k == 2 ? r.z : r.w));
}

// Inverse of the standard normal distribution function: Wichura's AS 241 (Appl. Statist. 37,
// 1988), routine PPND16, relative accuracy about 1e-16.  p strictly inside (0, 1).
__host__ __device__ inline double init_ppnd(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    const double num =
        (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
             4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
          1.3314166789178437745e+2) * r + 3.387132872796366608);
    const double den =
        (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
             2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
          4.2313330701600911252e+1) * r + 1.0);
    return q * num / den;
  }
  double r = sqrt(-log(q < 0.0 ? p : 1.0 - p));
  double v;
  if (r <= 5.0) {
    r -= 1.6;
    const double num =
        (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
             1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.76949722146069140550) * r +
          4.63033784615654529590) * r + 1.42343711074968357734);
    const double den =
        (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
             1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940) * r +
          2.05319162663775882187) * r + 1.0);
    v = num / den;
  } else {
    r -= 5.0;
    const double num =
        (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
             2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580) * r +
          5.46378491116411436990) * r + 6.65790464350110377720);
    const double den =
        (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
             7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
          5.99832206555887937690e-1) * r + 1.0);
    v = num / den;
  }
  return q < 0.0 ? -v : v;
}

// standard normal number idx of a stream: word idx % 4 of the Philox block at counter idx / 4,
// as a uniform strictly inside (0, 1) at 32-bit resolution (never 1/2: the draw is never 0),
// through the inverse distribution function.  |z| <= 6.3.
__host__ __device__ inline double init_normal(uint64_t seed, uint64_t stream, uint64_t idx) {
  const u32x4 r = philox_bits(seed, stream, idx >> 2);
  return init_ppnd(((double)init_word(r, (uint32_t)(idx & 3)) + 0.5) * (1.0 / 4294967296.0));
}

// selection key of marker j of a branch: word x of the block at counter j
__host__ __device__ inline uint32_t init_select_key(uint64_t seed, int32_t branch, int32_t j) {
  return philox_bits(seed, INIT_STREAM_SELECT | (uint64_t)(uint32_t)branch, (uint64_t)j).x;
}

// inclusion key of entry t of a linear model (the concatenated entry list, not per branch): word x
// of the block at counter t
__host__ __device__ inline uint32_t init_include_key(uint64_t seed, uint64_t t) {
  return philox_bits(seed, INIT_STREAM_INCLUDE, t).x;
}

// exact-count selection: marker j is kept iff fewer than e of the branch's markers come before
// it in the order of (key, index).  Integer arithmetic only.
__host__ __device__ inline bool init_key_before(uint32_t ki, int32_t i, uint32_t kj, int32_t j) {
  return ki < kj || (ki == kj && i < j);
}

// proportion rule: kept iff u01(key) < p
__host__ __device__ inline bool init_keep_proportion(uint32_t key, float p) { return u01(key) < p; }
