// kernels_gibbs.hip — the Gibbs step of the network driver on the device: every listed branch's
// local precisions (all of precision_vec but the output-layer and the error precision) redrawn
// from their Gamma posteriors given the current parameters, and everything
// bann_branch_set_precisions derives from a precision vector rewritten in the same launch.
//
// Restates sample_prior_precisions (ridge_ard.rs:271-301, lasso_ard.rs:271-298, the whole-layer
// draws of ridge_base.rs / lasso_base.rs) over the posteriors of gibbs_steps.rs:25-57, 76-129.
// In the sequential sweep these draws sit inside a per-branch dependency chain; given theta all
// branches' draws are independent, so here they are one launch: one workgroup per listed branch.
//
//   k_gibbs_stats  f64 (shape, scale) of every local precision and the output-weight statistic
//   k_gibbs_draw   the draws (gibbs_gamma.h), the two global precisions, lam / lamld, the
//                  Izmailov step bases, eprec[b] and a compact copy of the precision vectors
//
// Sums are f64 sums of f32 entries in a fixed order: an ARD row over k ascending by one thread;
// whole-layer, bias and output-weight sums as GIBBS_THREADS strided partial sums folded by a
// fixed tree.  No floating-point atomics; nothing depends on the grid or on the other listed
// branches.  The kernels read no genotypes.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx_internal.h"
#include "gibbs_gamma.h"
#include "prec_expand.h"

#define GIBBS_THREADS 256

struct GibbsHyper {
  double k[2], s[2];  // (shape, scale): [0] dense layers l < L-2, [1] the summary layer l = L-2
};

namespace {

// sum over cnt entries of v^2 (lasso: |v|): thread t takes t, t + GIBBS_THREADS, ...; the
// partials fold pairwise (stride 128, 64, ... 1).  Every thread of the workgroup calls it.
__device__ double block_stat(const float* __restrict__ v, int cnt, bool lasso, double* sh) {
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < cnt; i += GIBBS_THREADS) {
    const double w = (double)v[i];
    s += lasso ? fabs(w) : w * w;
  }
  sh[t] = s;
  __syncthreads();
  for (int o = GIBBS_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__device__ inline void ridge_post(double k, double s, double sum_sq, double num, double& shape, double& scale) {
  shape = k + num / 2.0;
  scale = 2.0 * s / (2.0 + s * sum_sq);
}
__device__ inline void lasso_post(double k, double s, double sum_abs, double num, double& shape, double& scale) {
  shape = k + num;
  scale = s / (1.0 + s * sum_abs);
}

__global__ __launch_bounds__(GIBBS_THREADS) void k_gibbs_stats(const BranchDev* __restrict__ br,
                                                                const float* __restrict__ theta,
                                                                const int32_t* __restrict__ list, GibbsHyper hp,
                                                                double* __restrict__ shape, double* __restrict__ scale,
                                                                double* __restrict__ out_stat) {
  __shared__ double sh[GIBBS_THREADS];
  const int b = list[blockIdx.x];
  const BranchDev& d = br[b];
  const float* th = theta + d.p_off;
  double* sp = shape + d.q_off;
  double* sc = scale + d.q_off;
  const int L = d.L, t = threadIdx.x;
  const bool ard = d.prior == BANN_RIDGE_ARD || d.prior == BANN_LASSO_ARD;
  const bool lasso = d.prior == BANN_LASSO_ARD || d.prior == BANN_LASSO_BASE;
  for (int l = 0; l < L - 1; ++l) {
    const int h = l == L - 2 ? 1 : 0;
    const double kl = hp.k[h], sl = hp.s[h];
    const int in = d.win[l], out = d.widths[l];
    const float* W = th + d.woff[l];
    if (ard) {
      for (int j = t; j < in; j += GIBBS_THREADS) {  // one precision per input node (row of W_l)
        double s = 0.0;
        for (int k = 0; k < out; ++k) {
          const double w = (double)W[(int64_t)k * in + j];
          s += lasso ? fabs(w) : w * w;
        }
        double a, c;
        if (lasso) {
          a = (double)out + kl;
          c = sl / (1.0 + sl * s);
        } else {
          a = (double)out / 2.0 + kl;
          c = 2.0 * sl / (2.0 + sl * s);
        }
        sp[d.qoff[l] + j] = a;
        sc[d.qoff[l] + j] = c;
      }
    } else {
      const double s = block_stat(W, in * out, lasso, sh);
      if (t == 0) {
        double a, c;
        if (lasso)
          lasso_post(kl, sl, s, (double)in * out, a, c);
        else
          ridge_post(kl, sl, s, (double)in * out, a, c);
        sp[d.qoff[l]] = a;
        sc[d.qoff[l]] = c;
      }
    }
    const double sb = block_stat(th + d.boff[l], out, false, sh);  // biases: always ridge
    if (t == 0) {
      double a, c;
      ridge_post(kl, sl, sb, (double)out, a, c);
      sp[d.qbias + l] = a;
      sc[d.qbias + l] = c;
    }
  }
  // summary_stat_fn of the output weights (ridge_ard.rs:39-41, lasso_ard.rs:45-47)
  const double so = block_stat(th + d.woff[L - 1], d.win[L - 1], lasso, sh);
  if (t == 0) {
    out_stat[b] = so;
    sp[d.qoff[L - 1]] = sc[d.qoff[L - 1]] = 0.0;  // the output-layer and error entries: not local
    sp[d.nq - 1] = sc[d.nq - 1] = 0.0;
  }
}

// one draw, kept out of line: inlined into k_gibbs_draw's loop the f64 log / exp / sqrt constants of
// the sampler stay live in scalar registers across the whole kernel and some of them spill
__device__ __noinline__ float draw_precision(double shape, double scale, uint64_t seed, uint64_t stream) {
  return gibbs_gamma_f32(shape, scale, seed, stream);
}

__global__ __launch_bounds__(GIBBS_THREADS) void k_gibbs_draw(
    const BranchDev* __restrict__ br, const int32_t* __restrict__ list, const double* __restrict__ shape,
    const double* __restrict__ scale, float oprec, float eprec, uint64_t seed, const int32_t* __restrict__ pidx,
    float* __restrict__ prec, float* __restrict__ lam, float* __restrict__ lamld, double* __restrict__ sbase,
    float* __restrict__ ep) {
  const int b = list[blockIdx.x];
  const BranchDev& d = br[b];
  const int t = threadIdx.x;
  float* pq = prec + d.q_off;
  const int qout = d.qoff[d.L - 1], qerr = d.nq - 1;
  for (int q = t; q < d.nq; q += GIBBS_THREADS) {
    float v;
    if (q == qout)
      v = oprec;
    else if (q == qerr)
      v = eprec;
    else
      v = draw_precision(shape[d.q_off + q], scale[d.q_off + q], seed, gibbs_stream(b, q));
    pq[q] = v;
  }
  if (t == 0) ep[b] = eprec;
  __syncthreads();  // the workgroup's own global writes are visible to it
  expand_branch_precisions(d, pq, pidx, lam, lamld, sbase, t, GIBBS_THREADS);
}

// the Gibbs scratch of a context, allocated at the first call: (shape, scale) and the compact
// precision copy over total_q, the output statistics and the list over the branches
int gibbs_buffers(bann_ctx* ctx) {
  if (ctx->d_gb_shape) return BANN_OK;
  const int64_t nb = (int64_t)ctx->br.size();
  CK(dalloc(&ctx->d_gb_shape, ctx->total_q));
  CK(dalloc(&ctx->d_gb_scale, ctx->total_q));
  CK(dalloc(&ctx->d_gb_prec, ctx->total_q));
  CK(dalloc(&ctx->d_gb_out, nb));
  CK(dalloc(&ctx->d_gb_list, nb));
  return BANN_OK;
}

int gibbs_check(bann_ctx* ctx, const int32_t* branches, int32_t nb, const float* hyper) {
  if (!ctx) return BANN_E_ARG;
  if (!ctx->finalized) return fail(ctx, BANN_E_STATE, "not finalized");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  if (!branches || nb <= 0 || !hyper) return fail(ctx, BANN_E_ARG, "null or empty branch list, or null hyper");
  const int32_t nbr = (int32_t)ctx->br.size();
  if (nb > nbr) return fail(ctx, BANN_E_ARG, "branch list longer than the branch set");
  std::vector<char> seen(nbr, 0);
  for (int32_t i = 0; i < nb; ++i) {
    if (!check_branch(ctx, branches[i])) return fail(ctx, BANN_E_ARG, "branch out of range");
    if (seen[branches[i]]) return fail(ctx, BANN_E_ARG, "duplicate branch in list");
    seen[branches[i]] = 1;
    if (ctx->br[branches[i]].prior == BANN_STD_NORMAL)
      return fail(ctx, BANN_E_ARG, "std_normal branches have no precisions to sample (std_normal_branch.rs:119-131)");
  }
  return BANN_OK;
}

// the list upload and the stats launch (no host wait)
int gibbs_stats(bann_ctx* ctx, const int32_t* branches, int32_t nb, const float* hyper) {
  int rc = gibbs_buffers(ctx);
  if (rc) return rc;
  CK(hipMemcpyAsync(ctx->d_gb_list, branches, nb * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  GibbsHyper hp;
  hp.k[0] = hyper[0], hp.s[0] = hyper[1], hp.k[1] = hyper[2], hp.s[1] = hyper[3];
  hipLaunchKernelGGL(k_gibbs_stats, dim3((unsigned)nb), dim3(GIBBS_THREADS), 0, ctx->stream, ctx->d_br, ctx->d_theta,
                     ctx->d_gb_list, hp, ctx->d_gb_shape, ctx->d_gb_scale, ctx->d_gb_out);
  CK(hipGetLastError());
  return BANN_OK;
}

}  // namespace

void gibbs_release(bann_ctx* ctx) {  // gibbs_buffers'
  dfree_all(ctx->d_gb_shape, ctx->d_gb_scale, ctx->d_gb_prec, ctx->d_gb_out, ctx->d_gb_list);
}

extern "C" int bann_gibbs_posterior(bann_ctx* ctx, const int32_t* branches, int32_t nb, const float* hyper,
                                    double* shape_out, double* scale_out, double* out_stat_out) {
  int rc = gibbs_check(ctx, branches, nb, hyper);
  if (rc) return rc;
  if (!shape_out && !scale_out && !out_stat_out) return fail(ctx, BANN_E_ARG, "no output requested");
  rc = gibbs_stats(ctx, branches, nb, hyper);
  if (rc) return rc;
  // the branches' slices are contiguous runs of the device arrays: one copy per output for the
  // whole set, then the listed slices in list order
  std::vector<double> sh, sc, os;
  if (shape_out) {
    sh.resize(ctx->total_q);
    CK(hipMemcpyAsync(sh.data(), ctx->d_gb_shape, ctx->total_q * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (scale_out) {
    sc.resize(ctx->total_q);
    CK(hipMemcpyAsync(sc.data(), ctx->d_gb_scale, ctx->total_q * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (out_stat_out) {
    os.resize(ctx->br.size());
    CK(hipMemcpyAsync(os.data(), ctx->d_gb_out, os.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  CK(hipStreamSynchronize(ctx->stream));
  int64_t o = 0;
  for (int32_t i = 0; i < nb; ++i) {
    const BranchDev& d = ctx->br[branches[i]].dev;
    if (shape_out) std::memcpy(shape_out + o, sh.data() + d.q_off, d.nq * sizeof(double));
    if (scale_out) std::memcpy(scale_out + o, sc.data() + d.q_off, d.nq * sizeof(double));
    if (out_stat_out) out_stat_out[i] = os[branches[i]];
    o += d.nq;
  }
  return BANN_OK;
}

extern "C" int bann_gibbs_sample_precisions(bann_ctx* ctx, const int32_t* branches, int32_t nb, const float* hyper,
                                            float output_precision, float error_precision, uint64_t seed) {
  int rc = gibbs_check(ctx, branches, nb, hyper);
  if (rc) return rc;
  rc = gibbs_stats(ctx, branches, nb, hyper);
  if (rc) return rc;
  hipLaunchKernelGGL(k_gibbs_draw, dim3((unsigned)nb), dim3(GIBBS_THREADS), 0, ctx->stream, ctx->d_br, ctx->d_gb_list,
                     ctx->d_gb_shape, ctx->d_gb_scale, output_precision, error_precision, seed, ctx->d_pidx,
                     ctx->d_gb_prec, ctx->d_lam, ctx->d_lamld, ctx->d_stepbase, ctx->d_eprec);
  CK(hipGetLastError());
  // the host mirrors of the listed branches from the compact device copy: one copy, one wait
  std::vector<float> pr(ctx->total_q);
  CK(hipMemcpyAsync(pr.data(), ctx->d_gb_prec, ctx->total_q * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  for (int32_t i = 0; i < nb; ++i) {
    BranchHost& h = ctx->br[branches[i]];
    h.prec.assign(pr.begin() + h.dev.q_off, pr.begin() + h.dev.q_off + h.dev.nq);
  }
  return BANN_OK;
}

extern "C" int bann_get_params_all(bann_ctx* ctx, float* out) {
  if (!ctx || !out) return fail(ctx, BANN_E_ARG, "null context or output");
  if (!ctx->finalized) return fail(ctx, BANN_E_STATE, "not finalized");
  CK(hipMemcpyAsync(out, ctx->d_theta, ctx->total_p * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}
