// kernels_init.hip — starting a model on the device: the initial BranchCfgs of every listed branch
// (bann_init_branches) and the phenotypes of rs-bann simulate-y (simulate_y_device).
//
// Restates BranchCfgBuilder::build / build_base / build_ard (branch_cfg_builder.rs:155-398), the
// joint output-layer precision of BlockNetCfg::build_net (architectures.rs:175-185) and the noise
// and moments of simulate-y (rs-bann.rs:466-501).  One launch sequence serves every listed branch,
// grid over (chunk, listed branch):
//
//   k_init_theta   the parameter draws (init_draw.h) and the proportion rule's zeros
//   k_init_select  exact-count selection: rank of (key_j, j) counted over LDS tiles of keys
//   k_init_stats   the precision vectors and the two output-weight statistics per branch
//   k_init_joint   network level: the sums over the listed branches and the joint output precision
//   k_init_expand  lam / lamld / step bases / eprec from the precision vectors (prec_expand.h)
//
// then launch_fused_const as bann_branch_set_params runs it.  Sums are f64 sums of f32 terms in a
// fixed order: an ARD row over k ascending by one thread; whole-layer, bias, output-weight and
// cohort sums as strided partial sums folded by a fixed tree.  No floating-point atomics; no value
// depends on the grid or on which other branches are listed.  The init kernels read no genotypes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "ctx_internal.h"
#include "init_draw.h"
#include "prec_expand.h"

#define INIT_THREADS 256
#define SIM_CHUNK 4096  // individuals per workgroup of the moment passes

struct InitDev {
  int32_t mode;
  float sd;  // modes 1 and 2: the standard deviation of every draw
  int32_t num_effective;
  float proportion;  // < 0: every marker kept
  int32_t has_fixed;
  float fixed;
};

namespace {

// every thread of the workgroup calls it: thread t takes t, t + INIT_THREADS, ...; the partials fold
// pairwise (stride 128, 64, ... 1).  mu is subtracted first (the second pass of a variance).
template <bool ABS>
__device__ double block_sum(const float* __restrict__ v, int64_t cnt, double mu, double* sh) {
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t i = t; i < cnt; i += INIT_THREADS) {
    const double w = (double)v[i] - mu;
    s += ABS ? fabs(w) : w * w;
  }
  sh[t] = s;
  __syncthreads();
  for (int o = INIT_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__device__ double block_fold(double s, double* sh) {
  const int t = threadIdx.x;
  sh[t] = s;
  __syncthreads();
  for (int o = INIT_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(INIT_THREADS) void k_init_theta(const BranchDev* __restrict__ br,
                                                              const int32_t* __restrict__ list, InitDev ic,
                                                              uint64_t seed, float* __restrict__ theta) {
  const int b = list[blockIdx.y];
  const BranchDev& d = br[b];
  const int p = blockIdx.x * INIT_THREADS + threadIdx.x;
  if (p >= d.P) return;
  const bool weight = p < d.boff[0];
  float v;
  if (ic.mode == 0 && !weight) {
    v = 0.f;
  } else {
    const float sd = ic.mode == 0 ? sqrtf(1.f / (float)d.m) : ic.sd;
    v = sd * (float)init_normal(seed, INIT_STREAM_THETA | (uint64_t)(uint32_t)b, (uint64_t)p);
  }
  // the proportion rule (the exact count, which takes precedence, is k_init_select's)
  if (ic.num_effective < 0 && ic.proportion >= 0.f && p < d.m * d.widths[0] &&
      !init_keep_proportion(init_select_key(seed, b, p % d.m), ic.proportion))
    v = 0.f;
  theta[d.p_off + p] = v;
}

// marker j = blockIdx.x * INIT_THREADS + t: its rank among the branch's (key, index) pairs, counted
// over tiles of INIT_THREADS keys staged in LDS; rank >= e removes the marker
__global__ __launch_bounds__(INIT_THREADS) void k_init_select(const BranchDev* __restrict__ br,
                                                               const int32_t* __restrict__ list, int32_t e,
                                                               uint64_t seed, float* __restrict__ theta) {
  __shared__ uint32_t keys[INIT_THREADS];
  const int b = list[blockIdx.y];
  const BranchDev& d = br[b];
  const int m = d.m, t = threadIdx.x;
  if ((int)blockIdx.x * INIT_THREADS >= m) return;  // the whole workgroup: no marker of this branch here
  const int j = blockIdx.x * INIT_THREADS + t;
  const uint32_t kj = j < m ? init_select_key(seed, b, j) : 0u;
  int32_t rank = 0;
  for (int i0 = 0; i0 < m; i0 += INIT_THREADS) {
    keys[t] = i0 + t < m ? init_select_key(seed, b, i0 + t) : 0u;
    __syncthreads();
    const int cnt = min(INIT_THREADS, m - i0);
    for (int i = 0; i < cnt; ++i) rank += init_key_before(keys[i], i0 + i, kj, j) ? 1 : 0;
    __syncthreads();
  }
  if (j < m && rank >= e) {
    float* W0 = theta + d.p_off;
    for (int k = 0; k < d.widths[0]; ++k) W0[(int64_t)k * m + j] = 0.f;
  }
}

// one workgroup per listed branch: its precision vector into prec[q_off ...] and, at stat[2 b], the
// sum of squares and summary_stat_fn (ridge: squares, lasso: absolute values) of its output weights
__global__ __launch_bounds__(INIT_THREADS) void k_init_stats(const BranchDev* __restrict__ br,
                                                              const float* __restrict__ theta,
                                                              const int32_t* __restrict__ list, InitDev ic,
                                                              float* __restrict__ prec, double* __restrict__ stat) {
  __shared__ double sh[INIT_THREADS];
  const int b = list[blockIdx.x];
  const BranchDev& d = br[b];
  const float* th = theta + d.p_off;
  float* pq = prec + d.q_off;
  const int L = d.L, t = threadIdx.x;
  const bool ard = d.prior == BANN_RIDGE_ARD || d.prior == BANN_LASSO_ARD;
  const bool lasso = d.prior == BANN_LASSO_ARD || d.prior == BANN_LASSO_BASE;
  for (int l = 0; l < L; ++l) {
    const int in = d.win[l], out = d.widths[l];
    const float* W = th + d.woff[l];
    if (ard && l < L - 1) {
      for (int j = t; j < in; j += INIT_THREADS) {  // one precision per input node (row of W_l)
        double s = 0.0;
        for (int k = 0; k < out; ++k) {
          const double w = (double)W[(int64_t)k * in + j];
          s += w * w;
        }
        pq[d.qoff[l] + j] = (float)((double)out / s);  // s == 0: +inf
      }
    } else {
      const double s = block_sum<false>(W, (int64_t)in * out, 0.0, sh);
      if (t == 0) {
        if (l == L - 1) stat[2 * b] = s;
        pq[d.qoff[l]] = ard ? 1.f : (float)((double)in * (double)out / s);
      }
    }
    if (l < L - 1) {
      const double sb = block_sum<false>(th + d.boff[l], out, 0.0, sh);
      if (t == 0) pq[d.qbias + l] = (float)((double)out / sb);
    }
  }
  const double sa = lasso ? block_sum<true>(th + d.woff[L - 1], d.win[L - 1], 0.0, sh) : 0.0;
  if (t == 0) {
    if (lasso) stat[2 * b + 1] = sa;
    else stat[2 * b + 1] = stat[2 * b];
    pq[d.nq - 1] = 2.f;
  }
  if (ic.has_fixed) {
    __syncthreads();
    for (int q = t; q < d.nq; q += INIT_THREADS) pq[q] = ic.fixed;
  }
}

// one workgroup: the two statistics summed over the listed branches (list order, strided partials,
// the fixed tree) into stat_sum[0..1]; unless a fixed precision holds, nb / sum of squares, rounded
// once, into every listed branch's output-layer entry
__global__ __launch_bounds__(INIT_THREADS) void k_init_joint(const BranchDev* __restrict__ br,
                                                              const int32_t* __restrict__ list, int32_t nb,
                                                              int32_t has_fixed, const double* __restrict__ stat,
                                                              double* __restrict__ stat_sum,
                                                              float* __restrict__ prec) {
  __shared__ double sh[INIT_THREADS];
  const int t = threadIdx.x;
  double s2 = 0.0, sr = 0.0;
  for (int i = t; i < nb; i += INIT_THREADS) {
    s2 += stat[2 * list[i]];
    sr += stat[2 * list[i] + 1];
  }
  s2 = block_fold(s2, sh);
  sr = block_fold(sr, sh);
  if (t == 0) {
    stat_sum[0] = s2;
    stat_sum[1] = sr;
  }
  if (has_fixed) return;
  const float op = (float)((double)nb / s2);
  for (int i = t; i < nb; i += INIT_THREADS) {
    const BranchDev& d = br[list[i]];
    prec[d.q_off + d.qoff[d.L - 1]] = op;
  }
}

__global__ __launch_bounds__(INIT_THREADS) void k_init_expand(const BranchDev* __restrict__ br,
                                                               const int32_t* __restrict__ list,
                                                               const int32_t* __restrict__ pidx,
                                                               const float* __restrict__ prec,
                                                               float* __restrict__ lam, float* __restrict__ lamld,
                                                               double* __restrict__ sbase, float* __restrict__ ep) {
  const int b = list[blockIdx.x];
  const BranchDev& d = br[b];
  const float* pq = prec + d.q_off;
  if (threadIdx.x == 0) ep[b] = pq[d.nq - 1];
  expand_branch_precisions(d, pq, pidx, lam, lamld, sbase, threadIdx.x, INIT_THREADS);
}

// ---- phenotypes ----

// part[blockIdx.x] = sum over the workgroup's SIM_CHUNK entries of (x - mu)^pw, pw = 1 or 2, with
// mu = mu_sum[0] / n (mu_sum null: 0): the first or second pass of the two-pass moments
__global__ __launch_bounds__(INIT_THREADS) void k_sim_partial(const float* __restrict__ x, int64_t n, int pw,
                                                               const double* __restrict__ mu_sum,
                                                               double* __restrict__ part) {
  __shared__ double sh[INIT_THREADS];
  const double mu = mu_sum ? mu_sum[0] / (double)n : 0.0;
  const int64_t i0 = (int64_t)blockIdx.x * SIM_CHUNK, i1 = i0 + SIM_CHUNK < n ? i0 + SIM_CHUNK : n;
  double s = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += INIT_THREADS) {
    const double w = (double)x[i] - mu;
    s += pw == 1 ? w : w * w;
  }
  s = block_fold(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// one workgroup: *out = sum of part[0 .. nblk)
__global__ __launch_bounds__(INIT_THREADS) void k_sim_fold(const double* __restrict__ part, int32_t nblk,
                                                            double* __restrict__ out) {
  __shared__ double sh[INIT_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblk; i += INIT_THREADS) s += part[i];
  s = block_fold(s, sh);
  if (threadIdx.x == 0) *out = s;
}

// y_i = g_i + (float)(sqrt(rv) z_i), rv = ss[0] / (n - 1) (1 / h - 1) with ss[0] the centred sum of
// squares of g; rv also to *rv_out
__global__ __launch_bounds__(INIT_THREADS) void k_sim_noise(float* __restrict__ y, int64_t n, double inv_h_m1,
                                                             const double* __restrict__ ss, uint64_t seed,
                                                             double* __restrict__ rv_out) {
  const int64_t i = (int64_t)blockIdx.x * INIT_THREADS + threadIdx.x;
  const double rv = ss[0] / (double)(n - 1) * inv_h_m1;
  if (i == 0) *rv_out = rv;
  if (i < n) y[i] += (float)(sqrt(rv) * init_normal(seed, INIT_STREAM_NOISE, (uint64_t)i));
}

int init_buffers(bann_ctx* ctx) {
  if (ctx->d_init_prec) return BANN_OK;
  const int64_t nb = (int64_t)ctx->br.size();
  CK(dalloc(&ctx->d_init_prec, ctx->total_q));
  CK(dalloc(&ctx->d_init_stat, 2 * nb + 2));
  CK(dalloc(&ctx->d_init_list, nb));
  return BANN_OK;
}

bool is_ard(int32_t prior) { return prior == BANN_RIDGE_ARD || prior == BANN_LASSO_ARD; }

// every check of bann_init_branches; ic = the configuration as the kernels take it
int init_check(bann_ctx* ctx, const int32_t* branches, int32_t nb, const bann_init_cfg* cfg, InitDev& ic) {
  if (!ctx) return BANN_E_ARG;
  if (!ctx->finalized) return fail(ctx, BANN_E_STATE, "not finalized");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  if (!branches || nb <= 0 || !cfg) return fail(ctx, BANN_E_ARG, "null or empty branch list, or null configuration");
  const int32_t nbr = (int32_t)ctx->br.size();
  if (nb > nbr) return fail(ctx, BANN_E_ARG, "branch list longer than the branch set");
  ic = InitDev{cfg->mode, 0.f, cfg->num_effective < 0 ? -1 : cfg->num_effective, -1.f, cfg->has_fixed_precision ? 1 : 0,
               cfg->fixed_precision};
  if (cfg->mode == 1) {
    if (!(cfg->variance > 0.f)) return fail(ctx, BANN_E_ARG, "mode 1: the variance must be positive");
    ic.sd = sqrtf(cfg->variance);
  } else if (cfg->mode == 2) {
    const float pr = cfg->gamma_shape * cfg->gamma_scale;  // the Gamma mean, in f32 as the reference forms it
    if (!(pr > 0.f)) return fail(ctx, BANN_E_ARG, "mode 2: shape * scale must be positive");
    ic.sd = sqrtf(1.f / pr);
  } else if (cfg->mode != 0) {
    return fail(ctx, BANN_E_ARG, "unknown initialisation mode");
  }
  if (cfg->proportion_effective >= 0.f && cfg->proportion_effective < 1.f) ic.proportion = cfg->proportion_effective;
  if (ic.has_fixed && !(cfg->fixed_precision > 0.f)) return fail(ctx, BANN_E_ARG, "the fixed precision must be positive");
  std::vector<char> seen(nbr, 0);
  for (int32_t i = 0; i < nb; ++i) {
    const int32_t b = branches[i];
    if (!check_branch(ctx, b)) return fail(ctx, BANN_E_ARG, "branch out of range");
    if (seen[b]) return fail(ctx, BANN_E_ARG, "duplicate branch in list");
    seen[b] = 1;
    const BranchHost& h = ctx->br[b];
    if (ic.num_effective > h.m)
      return fail(ctx, BANN_E_ARG, "num_effective " + std::to_string(ic.num_effective) + " exceeds the " +
                                       std::to_string(h.m) + " markers of branch " + std::to_string(b));
    if (ic.has_fixed && is_ard(h.prior))
      return fail(ctx, BANN_E_ARG, "ARD branch " + std::to_string(b) +
                                       ": fixed precisions are for base priors (branch_cfg_builder.rs:331)");
  }
  return BANN_OK;
}

// the launch sequence; joint: the network-level output precision and sums (k_init_joint)
int init_run(bann_ctx* ctx, const int32_t* branches, int32_t nb, const InitDev& ic, uint64_t seed, bool joint,
             double* reg_sum_out) {
  int rc = init_buffers(ctx);
  if (rc) return rc;
  int32_t max_p = 1, max_m = 1;
  for (int32_t i = 0; i < nb; ++i) {
    max_p = std::max(max_p, ctx->br[branches[i]].P);
    max_m = std::max(max_m, ctx->br[branches[i]].m);
  }
  hipStream_t s = ctx->stream;
  CK(hipMemcpyAsync(ctx->d_init_list, branches, nb * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const dim3 blk(INIT_THREADS);
  hipLaunchKernelGGL(k_init_theta, dim3((unsigned)((max_p + INIT_THREADS - 1) / INIT_THREADS), (unsigned)nb), blk, 0, s,
                     ctx->d_br, ctx->d_init_list, ic, seed, ctx->d_theta);
  if (ic.num_effective >= 0)
    hipLaunchKernelGGL(k_init_select, dim3((unsigned)((max_m + INIT_THREADS - 1) / INIT_THREADS), (unsigned)nb), blk, 0,
                       s, ctx->d_br, ctx->d_init_list, ic.num_effective, seed, ctx->d_theta);
  hipLaunchKernelGGL(k_init_stats, dim3((unsigned)nb), blk, 0, s, ctx->d_br, ctx->d_theta, ctx->d_init_list, ic,
                     ctx->d_init_prec, ctx->d_init_stat);
  double* stat_sum = ctx->d_init_stat + 2 * (int64_t)ctx->br.size();
  if (joint)
    hipLaunchKernelGGL(k_init_joint, dim3(1), blk, 0, s, ctx->d_br, ctx->d_init_list, nb, ic.has_fixed,
                       ctx->d_init_stat, stat_sum, ctx->d_init_prec);
  hipLaunchKernelGGL(k_init_expand, dim3((unsigned)nb), blk, 0, s, ctx->d_br, ctx->d_init_list, ctx->d_pidx,
                     ctx->d_init_prec, ctx->d_lam, ctx->d_lamld, ctx->d_stepbase, ctx->d_eprec);
  launch_fused_const(ctx->st, ctx->d_init_list, nb, s);  // the W0 digit image and FusedConst, as set_params
  CK(hipGetLastError());
  // the host mirrors of the listed branches from the compact device copy: one copy, one wait
  std::vector<float> pr(ctx->total_q);
  double sums[2] = {0.0, 0.0};
  CK(hipMemcpyAsync(pr.data(), ctx->d_init_prec, ctx->total_q * sizeof(float), hipMemcpyDeviceToHost, s));
  if (joint) CK(hipMemcpyAsync(sums, stat_sum, sizeof(sums), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  for (int32_t i = 0; i < nb; ++i) {
    BranchHost& h = ctx->br[branches[i]];
    h.prec.assign(pr.begin() + h.dev.q_off, pr.begin() + h.dev.q_off + h.dev.nq);
    ctx->pred_ok[branches[i]] = 0;
  }
  if (reg_sum_out) *reg_sum_out = sums[1];
  return BANN_OK;
}

int64_t sim_blocks(int64_t n) { return (n + SIM_CHUNK - 1) / SIM_CHUNK; }

// sums[0] = sum x, sums[1] = sum (x - mean)^2 on the device, no host wait
void launch_moments(bann_ctx* ctx, const float* x, double* sums) {
  sim_launch_moments(x, ctx->n, ctx->d_sim_part, sums, ctx->stream);
}

}  // namespace

void init_release(bann_ctx* ctx) {  // init_buffers' and simulate-y's partials
  dfree_all(ctx->d_init_prec, ctx->d_init_stat, ctx->d_init_list, ctx->d_sim_part);
}

int64_t sim_moment_blocks(int64_t n) { return sim_blocks(n); }

void sim_launch_moments(const float* x, int64_t n, double* part, double* sums, hipStream_t s) {
  const int32_t nblk = (int32_t)sim_blocks(n);
  const dim3 blk(INIT_THREADS);
  hipLaunchKernelGGL(k_sim_partial, dim3((unsigned)nblk), blk, 0, s, x, n, 1, (const double*)nullptr, part);
  hipLaunchKernelGGL(k_sim_fold, dim3(1), blk, 0, s, part, nblk, sums);
  hipLaunchKernelGGL(k_sim_partial, dim3((unsigned)nblk), blk, 0, s, x, n, 2, sums, part);
  hipLaunchKernelGGL(k_sim_fold, dim3(1), blk, 0, s, part, nblk, sums + 1);
}

void sim_launch_noise(float* y, int64_t n, double inv_h_m1, const double* ss, uint64_t seed, double* rv_out,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_sim_noise, dim3((unsigned)((n + INIT_THREADS - 1) / INIT_THREADS)), dim3(INIT_THREADS), 0, s, y, n,
                     inv_h_m1, ss, seed, rv_out);
}

extern "C" int bann_init_branches(bann_ctx* ctx, const int32_t* branches, int32_t nb, const bann_init_cfg* cfg,
                                  uint64_t seed) {
  InitDev ic;
  const int rc = init_check(ctx, branches, nb, cfg, ic);
  if (rc) return rc;
  return init_run(ctx, branches, nb, ic, seed, false, nullptr);
}

int init_branches_net(bann_ctx* ctx, const bann_init_cfg* cfg, uint64_t seed, double* reg_sum_out) {
  if (!ctx) return BANN_E_ARG;
  std::vector<int32_t> all(ctx->br.size());
  for (size_t b = 0; b < all.size(); ++b) all[b] = (int32_t)b;
  InitDev ic;
  const int rc = init_check(ctx, all.data(), (int32_t)all.size(), cfg, ic);
  if (rc) return rc;
  return init_run(ctx, all.data(), (int32_t)all.size(), ic, seed, true, reg_sum_out);
}

int simulate_y_device(bann_ctx* ctx, float bias, float heritability, uint64_t seed, float* y_out, float stats_out[3]) {
  if (!ctx || !y_out || !stats_out) return fail(ctx, BANN_E_ARG, "null context or output");
  if (!ctx->finalized) return fail(ctx, BANN_E_STATE, "not finalized");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  if (!(heritability > 0.f && heritability <= 1.f))
    return fail(ctx, BANN_E_ARG, "heritability must be in (0, 1] (0: the noise variance is infinite)");
  const int64_t n = ctx->n;
  if (n < 2) return fail(ctx, BANN_E_SHAPE, "a sample variance needs at least two individuals");
  if (!ctx->d_sim_part) CK(dalloc(&ctx->d_sim_part, sim_blocks(n) + 5));
  // the branch rows as bann_predict_many forms them, then Net::predict's sum (launch_models_sum)
  const int32_t nb = (int32_t)ctx->br.size();
  std::vector<int32_t> all(nb);
  for (int32_t b = 0; b < nb; ++b) all[b] = b;
  Plan p;
  int rc = build_plan(ctx, all.data(), nb, p, false);
  if (rc) return rc;
  rc = run_forward(ctx, p);
  if (rc) return rc;
  float* y = ctx->d_delta;  // n floats of scratch outside a session (bann_residual_init stages through it too)
  FeModels mm{};
  mm.nk = 1;
  mm.pred[0] = ctx->d_pred;
  mm.bias[0] = bias;
  launch_models_sum(mm, nb, n, y, ctx->stream);
  double* sums = ctx->d_sim_part + sim_blocks(n);  // [0..1] g, [2..3] y, [4] rv
  const bool noise = heritability != 1.f;
  if (noise) {
    launch_moments(ctx, y, sums);
    sim_launch_noise(y, n, 1.0 / (double)heritability - 1.0, sums + 1, seed, sums + 4, ctx->stream);
  }
  launch_moments(ctx, y, sums + 2);
  CK(hipGetLastError());
  double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  CK(hipMemcpyAsync(y_out, y, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(h, sums, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  stats_out[0] = (float)(h[2] / (double)n);
  stats_out[1] = (float)(h[3] / (double)(n - 1));
  stats_out[2] = noise ? (float)h[4] : 0.f;
  return BANN_OK;
}
