// kernels_lin.hip — linear scores of the resident cohort, the linear-model simulator's effect draws
// and its phenotypes.
//
// Restates LinearModel::predict (linear_model.rs:121-134) for K effect vectors at once,
// LinearModelBuilder::with_random_effects (linear_model.rs:46-91) with the counter-based draws of
// init_draw.h, and the tail of simulate_y_linear (rs-bann.rs:578-606).  The score reads the 2-bit
// variant-major image (kernels_data.hip header) directly: no branches, no tile images, no finalize.
//
//   k_lin_weights  w[k][t] = effects[k][t] / sigma[markers[t]] (0 where sigma = 0), per entry t
//   k_lin_offset   c_k = - sum_t w[k][t] mu[markers[t]] in f64: per block of 4 096 entries strided partials and
//                  the fixed LDS tree, then k_lin_offset_fold over the blocks (k_sim_partial / k_sim_fold's shape)
//   k_lin_score    grid (chunk of entries, stripe of individuals): a thread owns one dword of a row
//                  (16 individuals), a workgroup LIN_THREADS dwords (1 KiB of every row it reads); the
//                  chunk's weights and marker indices pass through LDS in tiles of LIN_TILE entries;
//                  16 f32 accumulators per column, KC <= LIN_KP columns per pass; one partial row per
//                  (chunk, column) into the scratch [chunk][KC][npad]
//   k_lin_fold     out[k][i] = (float)(sum over chunks ascending of (double)partial + c_k)
//
// An accumulator adds its chunk's entries in file order with one fused multiply-add each, whatever
// KC is and whichever column of the pass it serves: a column's bits depend on its effects, the cohort
// and the chunk length alone.  An overlapped marker's row is read once per entry.  No atomics.
//
//   k_lin_hist / k_lin_scan   radix select of the e-th (key, index) pair: four 16-bit digits of
//                             key << 32 | index, one histogram pass each (integer atomics)
//   k_lin_count / k_lin_draw  the inclusion count, then sd = sqrtf(h / m_incl) and the effects
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ctx_internal.h"
#include "init_draw.h"

#define LIN_THREADS 256
#define LIN_KP 4        // columns per genotype pass
#define LIN_TILE 256    // entries staged in LDS at a time
#define LIN_ROWS 8      // row loads in flight per thread
#define LIN_CHUNK 2048  // default entries per chunk: the f32 terms one accumulator sums
#define LIN_BINS 65536  // one 16-bit digit
#define LIN_OFF_BLOCK 4096  // entries per workgroup of the offset's first stage

typedef float lin_f2 __attribute__((ext_vector_type(2)));

struct LinSel {
  unsigned long long prefix;  // the digits found so far of the e-th (key << 32 | index)
  unsigned long long remain;  // its 1-based rank among the pairs that share the prefix
  unsigned long long count;   // kept entries (m_incl)
};

namespace {

__device__ double lin_block_fold(double s, double* sh) {
  const int t = threadIdx.x;
  sh[t] = s;
  __syncthreads();
  for (int o = LIN_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(LIN_THREADS) void k_lin_weights(const float* __restrict__ effects,
                                                              const int32_t* __restrict__ markers,
                                                              const float* __restrict__ sigma, int64_t E,
                                                              float* __restrict__ w) {
  const int64_t t = (int64_t)blockIdx.x * LIN_THREADS + threadIdx.x;
  if (t >= E) return;
  const float sg = sigma[markers[t]];
  const int64_t o = (int64_t)blockIdx.y * E + t;
  w[o] = sg > 0.f ? effects[o] / sg : 0.f;
}

// grid (block of LIN_OFF_BLOCK entries, column): part[column][block] = sum of w mu over the block's entries,
// strided partials and the fixed tree, as k_sim_partial
__global__ __launch_bounds__(LIN_THREADS) void k_lin_offset(const float* __restrict__ w,
                                                             const int32_t* __restrict__ markers,
                                                             const float* __restrict__ mu, int64_t E,
                                                             double* __restrict__ part) {
  __shared__ double sh[LIN_THREADS];
  const float* wk = w + (int64_t)blockIdx.y * E;
  const int64_t t0 = (int64_t)blockIdx.x * LIN_OFF_BLOCK, t1 = t0 + LIN_OFF_BLOCK < E ? t0 + LIN_OFF_BLOCK : E;
  double s = 0.0;
  for (int64_t t = t0 + threadIdx.x; t < t1; t += LIN_THREADS) s += (double)wk[t] * (double)mu[markers[t]];
  s = lin_block_fold(s, sh);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// one workgroup per column: c = - sum of the column's block partials, as k_sim_fold
__global__ __launch_bounds__(LIN_THREADS) void k_lin_offset_fold(const double* __restrict__ part, int32_t nblk,
                                                                  double* __restrict__ c) {
  __shared__ double sh[LIN_THREADS];
  const double* pk = part + (int64_t)blockIdx.x * nblk;
  double s = 0.0;
  for (int32_t b = threadIdx.x; b < nblk; b += LIN_THREADS) s += pk[b];
  s = lin_block_fold(s, sh);
  if (threadIdx.x == 0) c[blockIdx.x] = -s;
}

template <int KC>
__global__ __launch_bounds__(LIN_THREADS) void k_lin_score(const uint8_t* __restrict__ raw, int64_t rowb,
                                                            const int32_t* __restrict__ markers,
                                                            const float* __restrict__ w, int64_t E, int64_t chunk,
                                                            int64_t npad, float* __restrict__ part) {
  __shared__ float ws[LIN_TILE][LIN_KP];
  __shared__ int32_t ms[LIN_TILE];
  const int tid = threadIdx.x;
  const int64_t d = (int64_t)blockIdx.y * LIN_THREADS + tid;  // the thread's dword of every row
  const bool live = d < rowb / 4;                              // rowb is a multiple of 16
  const int64_t t0 = (int64_t)blockIdx.x * chunk, t1 = t0 + chunk < E ? t0 + chunk : E;
  const uint8_t* col = raw + 4 * d;
  lin_f2 acc[KC][8];
#pragma unroll
  for (int k = 0; k < KC; ++k)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[k][q] = lin_f2{0.f, 0.f};
  for (int64_t tt = t0; tt < t1; tt += LIN_TILE) {
    const int cnt = (int)(t1 - tt < LIN_TILE ? t1 - tt : LIN_TILE);
    __syncthreads();
    if (tid < cnt) {
      ms[tid] = markers[tt + tid];
#pragma unroll
      for (int k = 0; k < KC; ++k) ws[tid][k] = w[(int64_t)k * E + tt + tid];
    }
    __syncthreads();
    if (!live) continue;
    // one row of the thread's dword into every column's accumulators; rows are added in file order
    auto add_row = [&](uint32_t v, int i) {
      // individual p = 4 b + k sits in byte b of (v >> 2 k) & 0x03030303: four masks, then one byte-to-float
      // conversion per genotype.  The empty asm keeps the compiler from folding mask and byte select back
      // into one shift-and-mask pair per genotype.
      uint32_t mk[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        mk[k] = (v >> (2 * k)) & 0x03030303u;
        asm("" : "+v"(mk[k]));
      }
      lin_f2 g[8];
#pragma unroll
      for (int q = 0; q < 8; ++q)
        g[q] = lin_f2{(float)((mk[(2 * q) & 3] >> (8 * ((2 * q) >> 2))) & 0xffu),
                      (float)((mk[(2 * q + 1) & 3] >> (8 * ((2 * q + 1) >> 2))) & 0xffu)};
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const float wk = ws[i][k];
        const lin_f2 w2 = lin_f2{wk, wk};
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[k][q] = __builtin_elementwise_fma(w2, g[q], acc[k][q]);
      }
    };
    // groups of LIN_ROWS rows, double-buffered: the next group's loads are in flight while this one is added
    int i = 0;
    uint32_t nxt[LIN_ROWS];
    if (cnt >= LIN_ROWS) {
#pragma unroll
      for (int u = 0; u < LIN_ROWS; ++u) nxt[u] = *reinterpret_cast<const uint32_t*>(col + (int64_t)ms[u] * rowb);
    }
    for (; i + LIN_ROWS <= cnt; i += LIN_ROWS) {
      uint32_t v[LIN_ROWS];
#pragma unroll
      for (int u = 0; u < LIN_ROWS; ++u) v[u] = nxt[u];
      if (i + 2 * LIN_ROWS <= cnt) {
#pragma unroll
        for (int u = 0; u < LIN_ROWS; ++u)
          nxt[u] = *reinterpret_cast<const uint32_t*>(col + (int64_t)ms[i + LIN_ROWS + u] * rowb);
      }
      __builtin_amdgcn_sched_barrier(0);  // the loads stay in front of the arithmetic
#pragma unroll
      for (int u = 0; u < LIN_ROWS; ++u) add_row(v[u], i + u);
    }
    for (; i < cnt; ++i) add_row(*reinterpret_cast<const uint32_t*>(col + (int64_t)ms[i] * rowb), i);
  }
  if (!live) return;
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    float4* dst = reinterpret_cast<float4*>(part + ((int64_t)blockIdx.x * KC + k) * npad + 16 * d);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      dst[q] = make_float4(acc[k][2 * q].x, acc[k][2 * q].y, acc[k][2 * q + 1].x, acc[k][2 * q + 1].y);
  }
}

// grid (individuals, column of the pass)
__global__ __launch_bounds__(LIN_THREADS) void k_lin_fold(const float* __restrict__ part, int32_t nchunk, int32_t kc,
                                                           int64_t npad, int64_t n, const double* __restrict__ c,
                                                           float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * LIN_THREADS + threadIdx.x;
  const int k = blockIdx.y;
  if (i >= n) return;
  double s = 0.0;
  for (int32_t ch = 0; ch < nchunk; ++ch) s += (double)part[((int64_t)ch * kc + k) * npad + i];
  out[(int64_t)k * n + i] = (float)(s + c[k]);
}

// ---- effects ----

__device__ inline unsigned long long lin_pair(uint64_t seed, int64_t t) {
  return ((unsigned long long)init_include_key(seed, (uint64_t)t) << 32) | (unsigned long long)(uint32_t)t;
}

// mode 0: every entry; 1: the pairs up to the selected one; 2: u01(key) < p
__device__ inline bool lin_keep(int mode, uint64_t seed, int64_t t, unsigned long long last, float p) {
  if (mode == 0) return true;
  if (mode == 1) return lin_pair(seed, t) <= last;
  return init_keep_proportion(init_include_key(seed, (uint64_t)t), p);
}

// digit 3 - pass of the pairs whose higher digits equal sel->prefix
__global__ __launch_bounds__(LIN_THREADS) void k_lin_hist(int64_t E, uint64_t seed, int pass,
                                                           const LinSel* __restrict__ sel,
                                                           uint32_t* __restrict__ hist) {
  const unsigned long long prefix = sel->prefix;
  for (int64_t t = (int64_t)blockIdx.x * LIN_THREADS + threadIdx.x; t < E; t += (int64_t)gridDim.x * LIN_THREADS) {
    const unsigned long long c = lin_pair(seed, t);
    if (pass == 0 || (c >> (16 * (4 - pass))) == prefix) atomicAdd(&hist[(c >> (16 * (3 - pass))) & 0xFFFFull], 1u);
  }
}

// one workgroup: the bin that holds rank sel->remain, appended to the prefix; the histogram back to zero
__global__ __launch_bounds__(LIN_THREADS) void k_lin_scan(LinSel* __restrict__ sel, uint32_t* __restrict__ hist) {
  __shared__ unsigned long long seg[LIN_THREADS];
  const int t = threadIdx.x;
  const int per = LIN_BINS / LIN_THREADS;
  unsigned long long s = 0;
  for (int b = 0; b < per; ++b) s += hist[t * per + b];
  seg[t] = s;
  __syncthreads();
  if (t == 0) {
    const unsigned long long rem = sel->remain;
    unsigned long long cum = 0;
    int sg = 0;
    while (sg < LIN_THREADS - 1 && cum + seg[sg] < rem) cum += seg[sg++];
    int b = sg * per;
    while (b < sg * per + per - 1 && cum + hist[b] < rem) cum += hist[b++];
    sel->prefix = (sel->prefix << 16) | (unsigned long long)b;
    sel->remain = rem - cum;
  }
  __syncthreads();
  for (int b = 0; b < per; ++b) hist[t * per + b] = 0u;
}

__global__ __launch_bounds__(LIN_THREADS) void k_lin_count(int64_t E, uint64_t seed, int mode, float p,
                                                            LinSel* __restrict__ sel) {
  __shared__ unsigned long long red[LIN_THREADS / 64];
  const unsigned long long last = sel->prefix;
  unsigned long long c = 0;
  for (int64_t t = (int64_t)blockIdx.x * LIN_THREADS + threadIdx.x; t < E; t += (int64_t)gridDim.x * LIN_THREADS)
    c += lin_keep(mode, seed, t, last, p) ? 1ull : 0ull;
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
    for (int k = 0; k < LIN_THREADS / 64; ++k) s += red[k];
    if (s) atomicAdd(&sel->count, s);
  }
}

__global__ __launch_bounds__(LIN_THREADS) void k_lin_draw(int64_t E, uint64_t seed, int mode, float p, float h,
                                                           const LinSel* __restrict__ sel, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * LIN_THREADS + threadIdx.x;
  if (t >= E) return;
  const unsigned long long m = sel->count;
  const float sd = m ? sqrtf(h / (float)m) : 0.f;
  out[t] = lin_keep(mode, seed, t, sel->prefix, p) ? sd * (float)init_normal(seed, INIT_STREAM_EFFECT, (uint64_t)t) : 0.f;
}

// the device buffers of one call, freed at its end
struct LinBuf {
  int32_t* markers = nullptr;
  float* eff = nullptr;
  float* w = nullptr;
  double* c = nullptr;
  double* cpart = nullptr;  // [K][blocks of LIN_OFF_BLOCK entries]
  float* part = nullptr;
  float* out = nullptr;  // [K][n]
  float* y = nullptr;    // simulate_y: [K][n]
  double* sums = nullptr;
  double* mpart = nullptr;
  LinSel* sel = nullptr;
  uint32_t* hist = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~LinBuf() {
    dfree(markers);
    dfree(eff);
    dfree(w);
    dfree(c);
    dfree(cpart);
    dfree(part);
    dfree(out);
    dfree(y);
    dfree(sums);
    dfree(mpart);
    dfree(sel);
    dfree(hist);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

int lin_check(bann_ctx* ctx, int32_t num_groups, const int64_t* offsets, const int32_t* markers, const float* effects,
              int32_t K, int64_t* E_out) {
  if (!ctx->d_g)
    return fail(ctx, BANN_E_STATE,
                ctx->finalized ? "the cohort image was freed at bann_finalize (free_raw): the linear score reads it"
                               : "no genotypes loaded");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  if (K < 1 || K > 65535) return fail(ctx, BANN_E_ARG, "K must be in [1, 65535]");
  if (num_groups < 1 || !offsets || !markers || !effects) return fail(ctx, BANN_E_ARG, "null or empty grouping, or null effects");
  if (offsets[0] != 0) return fail(ctx, BANN_E_ARG, "offsets[0] must be 0");
  for (int32_t g = 0; g < num_groups; ++g)
    if (offsets[g + 1] < offsets[g]) return fail(ctx, BANN_E_ARG, "offsets must not decrease");
  const int64_t E = offsets[num_groups];
  if (E < 1) return fail(ctx, BANN_E_ARG, "the grouping has no entry");
  for (int64_t t = 0; t < E; ++t)
    if (markers[t] < 0 || markers[t] >= ctx->M)
      return fail(ctx, BANN_E_ARG, "marker index " + std::to_string(markers[t]) + " outside the cohort");
  *E_out = E;
  return BANN_OK;
}

template <int KC>
void lin_launch_pass(bann_ctx* ctx, const LinBuf& b, int64_t E, int64_t chunk, int32_t nchunk, int32_t stripes,
                     int64_t npad, int32_t k0) {
  hipLaunchKernelGGL(k_lin_score<KC>, dim3((unsigned)nchunk, (unsigned)stripes), dim3(LIN_THREADS), 0, ctx->stream,
                     ctx->d_g, ctx->rowb, b.markers, b.w + (int64_t)k0 * E, E, chunk, npad, b.part);
}

// every launch of the score, no host wait: b.out[k][i] on the device, events around the launches
int lin_score_launch(bann_ctx* ctx, LinBuf& b, const int32_t* markers, const float* effects, int64_t E, int32_t K) {
  CK(hipSetDevice(ctx->device));
  const int64_t n = ctx->n, npad = ctx->rowb * 4;
  const int64_t chunk = ctx->lin_chunk > 0 ? ctx->lin_chunk : LIN_CHUNK;
  const int64_t nchunk = (E + chunk - 1) / chunk;
  const int64_t stripes = (ctx->rowb / 4 + LIN_THREADS - 1) / LIN_THREADS;
  if (nchunk > 0x7fffffff || stripes > 65535) return fail(ctx, BANN_E_SHAPE, "too many chunks or stripes for one grid");
  const int32_t kp = std::min<int32_t>(K, LIN_KP);
  CK(dalloc(&b.markers, E));
  CK(dalloc(&b.eff, (int64_t)K * E));
  CK(dalloc(&b.w, (int64_t)K * E));
  CK(dalloc(&b.c, K));
  const int64_t oblk = (E + LIN_OFF_BLOCK - 1) / LIN_OFF_BLOCK;
  CK(dalloc(&b.cpart, (int64_t)K * oblk));
  CK(dalloc(&b.part, nchunk * kp * npad));
  CK(dalloc(&b.out, (int64_t)K * n));
  CK(hipEventCreate(&b.ev0));
  CK(hipEventCreate(&b.ev1));
  hipStream_t s = ctx->stream;
  CK(hipMemcpyAsync(b.markers, markers, (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice, s));
  CK(hipMemcpyAsync(b.eff, effects, (size_t)K * E * sizeof(float), hipMemcpyHostToDevice, s));
  CK(hipEventRecord(b.ev0, s));
  const dim3 blk(LIN_THREADS);
  hipLaunchKernelGGL(k_lin_weights, dim3((unsigned)((E + LIN_THREADS - 1) / LIN_THREADS), (unsigned)K), blk, 0, s, b.eff,
                     b.markers, ctx->d_sigma, E, b.w);
  hipLaunchKernelGGL(k_lin_offset, dim3((unsigned)oblk, (unsigned)K), blk, 0, s, b.w, b.markers, ctx->d_mu, E, b.cpart);
  hipLaunchKernelGGL(k_lin_offset_fold, dim3((unsigned)K), blk, 0, s, b.cpart, (int32_t)oblk, b.c);
  for (int32_t k0 = 0; k0 < K; k0 += LIN_KP) {
    const int32_t kc = std::min<int32_t>(LIN_KP, K - k0);
    switch (kc) {
      case 1: lin_launch_pass<1>(ctx, b, E, chunk, (int32_t)nchunk, (int32_t)stripes, npad, k0); break;
      case 2: lin_launch_pass<2>(ctx, b, E, chunk, (int32_t)nchunk, (int32_t)stripes, npad, k0); break;
      case 3: lin_launch_pass<3>(ctx, b, E, chunk, (int32_t)nchunk, (int32_t)stripes, npad, k0); break;
      default: lin_launch_pass<4>(ctx, b, E, chunk, (int32_t)nchunk, (int32_t)stripes, npad, k0); break;
    }
    hipLaunchKernelGGL(k_lin_fold, dim3((unsigned)((n + LIN_THREADS - 1) / LIN_THREADS), (unsigned)kc), blk, 0, s, b.part,
                       (int32_t)nchunk, kc, npad, n, b.c + k0, b.out + (int64_t)k0 * n);
  }
  CK(hipEventRecord(b.ev1, s));
  CK(hipGetLastError());
  return BANN_OK;
}

int lin_timing_resolve(bann_ctx* ctx, const LinBuf& b) {
  float t = 0.f;
  CK(hipEventElapsedTime(&t, b.ev0, b.ev1));
  ctx->lin_ms = t;
  return BANN_OK;
}

}  // namespace

extern "C" int bann_genotypes_linear_score(bann_ctx* ctx, int32_t num_groups, const int64_t* offsets,
                                           const int32_t* markers, const float* effects, int32_t K, float* out) {
  if (!ctx) return BANN_E_ARG;
  int64_t E = 0;
  if (int rc = lin_check(ctx, num_groups, offsets, markers, effects, K, &E)) return rc;
  if (!out) return fail(ctx, BANN_E_ARG, "out is null");
  ctx->lin_ms = 0.0;
  LinBuf b;
  if (int rc = lin_score_launch(ctx, b, markers, effects, E, K)) return rc;
  CK(hipMemcpyAsync(out, b.out, (size_t)K * ctx->n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return lin_timing_resolve(ctx, b);
}

extern "C" int bann_genotypes_linear_chunk(bann_ctx* ctx, int64_t entries_per_chunk) {
  if (!ctx) return BANN_E_ARG;
  if (entries_per_chunk < 0) return fail(ctx, BANN_E_ARG, "entries_per_chunk must not be negative (0: the default)");
  ctx->lin_chunk = entries_per_chunk;
  return BANN_OK;
}

extern "C" int bann_genotypes_linear_timing(const bann_ctx* ctx, double* kernel_ms) {
  if (!ctx || !kernel_ms) return BANN_E_ARG;
  *kernel_ms = ctx->lin_ms;
  return BANN_OK;
}

extern "C" int bann_linear_effects(bann_ctx* ctx, int64_t E, float heritability, int64_t num_effective,
                                   float proportion_effective, uint64_t seed, float* effects_out, int64_t* m_incl) {
  if (!ctx) return BANN_E_ARG;
  if (!effects_out) return fail(ctx, BANN_E_ARG, "effects_out is null");
  if (E < 1 || E > 0xffffffffll) return fail(ctx, BANN_E_ARG, "E must be in [1, 2^32)");
  if (!(heritability > 0.f && heritability <= 1.f)) return fail(ctx, BANN_E_ARG, "heritability must be in (0, 1]");
  const int mode = num_effective >= 0 ? 1 : (proportion_effective >= 0.f ? 2 : 0);
  if (mode == 1 && num_effective > E)
    return fail(ctx, BANN_E_ARG, "num_effective " + std::to_string(num_effective) + " exceeds the " + std::to_string(E) + " entries");
  if (mode == 1 && num_effective == 0) return fail(ctx, BANN_E_ARG, "no effective marker");
  CK(hipSetDevice(ctx->device));
  LinBuf b;
  CK(dalloc(&b.sel, 1));
  CK(dalloc(&b.out, E));
  hipStream_t s = ctx->stream;
  const LinSel init{0ull, mode == 1 ? (unsigned long long)num_effective : 0ull, 0ull};
  CK(hipMemcpyAsync(b.sel, &init, sizeof(init), hipMemcpyHostToDevice, s));
  const int64_t eb = (E + LIN_THREADS - 1) / LIN_THREADS;
  const dim3 blk(LIN_THREADS), strided((unsigned)std::min<int64_t>(eb, 4096));
  if (mode == 1) {
    CK(dalloc(&b.hist, LIN_BINS));
    CK(hipMemsetAsync(b.hist, 0, LIN_BINS * sizeof(uint32_t), s));
    for (int pass = 0; pass < 4; ++pass) {
      hipLaunchKernelGGL(k_lin_hist, strided, blk, 0, s, E, seed, pass, b.sel, b.hist);
      hipLaunchKernelGGL(k_lin_scan, dim3(1), blk, 0, s, b.sel, b.hist);
    }
  }
  hipLaunchKernelGGL(k_lin_count, strided, blk, 0, s, E, seed, mode, proportion_effective, b.sel);
  hipLaunchKernelGGL(k_lin_draw, dim3((unsigned)eb), blk, 0, s, E, seed, mode, proportion_effective, heritability, b.sel,
                     b.out);
  CK(hipGetLastError());
  LinSel fin{};
  CK(hipMemcpyAsync(effects_out, b.out, (size_t)E * sizeof(float), hipMemcpyDeviceToHost, s));
  CK(hipMemcpyAsync(&fin, b.sel, sizeof(fin), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  if (m_incl) *m_incl = (int64_t)fin.count;
  if (fin.count == 0) return fail(ctx, BANN_E_ARG, "no effective marker");
  return BANN_OK;
}

extern "C" int bann_linear_simulate_y(bann_ctx* ctx, int32_t num_groups, const int64_t* offsets, const int32_t* markers,
                                      const float* effects, int32_t K, float heritability, const uint64_t* seeds,
                                      float* y_out, float* g_out, double* stats) {
  if (!ctx) return BANN_E_ARG;
  int64_t E = 0;
  if (int rc = lin_check(ctx, num_groups, offsets, markers, effects, K, &E)) return rc;
  if (!seeds || !y_out || !stats) return fail(ctx, BANN_E_ARG, "null seeds or output");
  if (!(heritability > 0.f && heritability <= 1.f))
    return fail(ctx, BANN_E_ARG, "heritability must be in (0, 1] (0: the noise variance is infinite)");
  const int64_t n = ctx->n;
  if (n < 2) return fail(ctx, BANN_E_SHAPE, "a sample variance needs at least two individuals");
  ctx->lin_ms = 0.0;
  LinBuf b;
  CK(hipSetDevice(ctx->device));
  CK(dalloc(&b.y, (int64_t)K * n));
  CK(dalloc(&b.sums, (int64_t)K * 5));  // per column [0..1] g, [2..3] y, [4] rv, as simulate_y_device
  CK(dalloc(&b.mpart, sim_moment_blocks(n)));
  if (int rc = lin_score_launch(ctx, b, markers, effects, E, K)) return rc;
  hipStream_t s = ctx->stream;
  CK(hipMemsetAsync(b.sums, 0, (size_t)K * 5 * sizeof(double), s));
  CK(hipMemcpyAsync(b.y, b.out, (size_t)K * n * sizeof(float), hipMemcpyDeviceToDevice, s));
  const bool noise = heritability != 1.f;
  for (int32_t k = 0; k < K; ++k) {
    float* yk = b.y + (int64_t)k * n;
    double* sk = b.sums + 5 * (int64_t)k;
    sim_launch_moments(b.out + (int64_t)k * n, n, b.mpart, sk, s);
    if (noise) sim_launch_noise(yk, n, 1.0 / (double)heritability - 1.0, sk + 1, seeds[k], sk + 4, s);
    sim_launch_moments(yk, n, b.mpart, sk + 2, s);
  }
  CK(hipGetLastError());
  CK(hipMemcpyAsync(y_out, b.y, (size_t)K * n * sizeof(float), hipMemcpyDeviceToHost, s));
  if (g_out) CK(hipMemcpyAsync(g_out, b.out, (size_t)K * n * sizeof(float), hipMemcpyDeviceToHost, s));
  CK(hipMemcpyAsync(stats, b.sums, (size_t)K * 5 * sizeof(double), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  return lin_timing_resolve(ctx, b);
}
