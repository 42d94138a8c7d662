// bann_eval.hip — the per-branch BranchSampler math of include/bann.h at the current state,
// outside a trajectory: predictions, rss, the log-density gradients (one branch, several,
// joint), forward_feed, effect sizes, log density and -H.
#include <math.h>

#include <algorithm>
#include <vector>

#include "ctx_internal.h"

// gradient and rss of the listed branches at the current parameters: one packed gradient
// launch and the MODE_GRAD update that folds its partials
static int eval_branches(bann_ctx* ctx, const int32_t* branches, int32_t nb) {
  Plan p;
  int rc = build_plan(ctx, branches, nb, p, false);
  if (rc) return rc;
  rc = run_grad(ctx, p, 0);
  if (rc) return rc;
  run_update(ctx, p, MODE_GRAD, 0);
  CK(hipGetLastError());
  return BANN_OK;
}

extern "C" int bann_predict(bann_ctx* ctx, int32_t b, float* pred_out) {
  if (!check_branch(ctx, b) || !pred_out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  int rc = ensure_predictions(ctx, &b, 1);
  if (rc) return rc;
  CK(hipMemcpyAsync(pred_out, ctx->d_pred + (int64_t)b * ctx->n, ctx->n * sizeof(float), hipMemcpyDeviceToHost,
                    ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_predict_many(bann_ctx* ctx, const int32_t* branches, int32_t nb, float* pred_out) {
  if (!ctx || !branches || nb <= 0 || !pred_out) return fail(ctx, BANN_E_ARG, "bad branch list or null output");
  if (!ctx->finalized) return fail(ctx, BANN_E_STATE, "call bann_finalize first");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  Plan p;
  int rc = build_plan(ctx, branches, nb, p, false);
  if (rc) return rc;
  rc = run_forward(ctx, p);  // one packed forward launch per kernel group
  if (rc) return rc;
  for (int32_t i = 0; i < nb; ++i)
    CK(hipMemcpyAsync(pred_out + (int64_t)i * ctx->n, ctx->d_pred + (int64_t)branches[i] * ctx->n,
                      ctx->n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_rss(bann_ctx* ctx, int32_t b, double* rss_out) {
  if (!check_branch(ctx, b) || !rss_out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  int rc = eval_branches(ctx, &b, 1);
  if (rc) return rc;
  CK(hipMemcpyAsync(rss_out, ctx->d_rss + b, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_log_density_gradient(bann_ctx* ctx, int32_t b, float* grad_out, double* rss_out) {
  if (!check_branch(ctx, b) || !grad_out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  int rc = eval_branches(ctx, &b, 1);
  if (rc) return rc;
  const BranchHost& h = ctx->br[b];
  CK(hipMemcpyAsync(grad_out, ctx->d_grad + h.dev.p_off, h.P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (rss_out) CK(hipMemcpyAsync(rss_out, ctx->d_rss + b, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

// Net::gradient (net.rs:520-527): the log-density gradients of several branches
// against their current targets from one packed gradient launch
extern "C" int bann_log_density_gradient_many(bann_ctx* ctx, const int32_t* branches, int32_t nb, float* grad_out,
                                              double* rss_out) {
  if (!ctx || !branches || nb <= 0 || !grad_out) return fail(ctx, BANN_E_ARG, "bad branch list or null output");
  if (!ctx->finalized) return fail(ctx, BANN_E_STATE, "call bann_finalize first");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  for (int i = 0; i < nb; ++i)
    if (!check_branch(ctx, branches[i])) return fail(ctx, BANN_E_ARG, "bad branch");
  const int rc = eval_branches(ctx, branches, nb);  // build_plan refuses a duplicate before any launch
  if (rc) return rc;
  int64_t off = 0;
  for (int i = 0; i < nb; ++i) {
    const BranchHost& h = ctx->br[branches[i]];
    CK(hipMemcpyAsync(grad_out + off, ctx->d_grad + h.dev.p_off, h.P * sizeof(float), hipMemcpyDeviceToHost,
                      ctx->stream));
    if (rss_out) CK(hipMemcpyAsync(rss_out + i, ctx->d_rss + branches[i], sizeof(double), hipMemcpyDeviceToHost,
                                   ctx->stream));
    off += h.P;
  }
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

// log_density_gradient_joint (branch_sampler.rs:406-422) at the branch's current
// parameters and precisions: [params | precisions], the joint log density
// (log_density_joint 292-305) and the rss; k_update_joint in MODE_GRAD
extern "C" int bann_log_density_gradient_joint(bann_ctx* ctx, int32_t b, const float* hyper, float* grad_out,
                                               double* rss_out, double* log_density_out) {
  if (!check_branch(ctx, b) || !hyper || !grad_out) return fail(ctx, BANN_E_ARG, "bad branch or null pointer");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  const BranchHost& h = ctx->br[b];
  if (h.prior == BANN_STD_NORMAL)
    return fail(ctx, BANN_E_ARG, "std_normal has no joint density (std_normal_branch.rs:119-131)");
  if (h.dev.nq > BANN_JOINT_MAXQ) return fail(ctx, BANN_E_SHAPE, "too many precisions for the joint update");
  for (int k = 0; k < 6; ++k) ctx->st.hyper[k] = hyper[k];
  const float ows[2] = {h.ows_reg_sum, h.ows_num >= 0.f ? h.ows_num : (float)h.widths[h.L - 2]};
  CK(hipMemcpyAsync(ctx->d_phi + h.dev.q_off, h.prec.data(), h.dev.nq * sizeof(float), hipMemcpyHostToDevice,
                    ctx->stream));
  CK(hipMemcpyAsync(ctx->d_ows + 2 * b, ows, 2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  Plan p;
  int rc = build_plan(ctx, &b, 1, p, false);
  if (rc) return rc;
  rc = run_grad(ctx, p, 0);
  if (rc) return rc;
  launch_update_joint(ctx->st, p.d_all, 1, MODE_GRAD, 0, ctx->stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(grad_out, ctx->d_grad + h.dev.p_off, h.P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(grad_out + h.P, ctx->d_gphi + h.dev.q_off, h.dev.nq * sizeof(float), hipMemcpyDeviceToHost,
                    ctx->stream));
  double r[2] = {0.0, 0.0};
  CK(hipMemcpyAsync(&r[0], ctx->d_rss + b, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipMemcpyAsync(&r[1], ctx->d_ld + b, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  if (rss_out) *rss_out = r[0];
  if (log_density_out) *log_density_out = r[1];
  return BANN_OK;
}

// forward_feed (branch_sampler.rs:743-782) with every layer kept, for
// Net::activations (net.rs:509-518): kernels_feed.hip, scratch per call
extern "C" int bann_forward_feed(bann_ctx* ctx, int32_t b, float* pre_out, float* act_out) {
  if (!check_branch(ctx, b) || !act_out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  const BranchHost& h = ctx->br[b];
  int64_t wa = 0, wp = 0;
  for (int l = 0; l < h.L; ++l) {
    wa += h.widths[l];
    if (l < h.L - 1) wp += h.widths[l];
  }
  const int64_t n = ctx->n;
  float *d_act = nullptr, *d_pre = nullptr;
  CK(dalloc(&d_act, wa * n));
  if (pre_out && dalloc(&d_pre, wp * n) != hipSuccess) {
    dfree(d_act);
    return fail(ctx, BANN_E_OOM, "forward_feed scratch");
  }
  launch_forward_feed(ctx->st, b, h.dev, d_pre, d_act, ctx->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(act_out, d_act, wa * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && pre_out)
    e = hipMemcpyAsync(pre_out, d_pre, wp * n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  dfree(d_act);
  dfree(d_pre);
  CK(e);
  return BANN_OK;
}

EffectScratch::~EffectScratch() {
  for (void* p : {(void*)pre, (void*)act, (void*)ea, (void*)eb, (void*)full, (void*)pop, (void*)s}) dfree(p);
}

hipError_t EffectScratch::alloc(const bann_ctx* ctx, const int32_t* branches, int32_t nb, bool want_full) {
  int64_t wp = 1, wa = 1, we = 1, wm = 1, w0 = 1;
  for (int32_t i = 0; i < nb; ++i) {
    const BranchHost& h = ctx->br[branches[i]];
    int64_t p = 0, a = 0;
    for (int l = 0; l < h.L; ++l) {
      a += h.widths[l];
      if (l < h.L - 1) p += h.widths[l];
      if (l >= 1) we = std::max<int64_t>(we, h.dev.win[l]);
    }
    wp = std::max(wp, p);
    wa = std::max(wa, a);
    wm = std::max<int64_t>(wm, h.m);
    w0 = std::max<int64_t>(w0, h.widths[0]);
  }
  const int64_t n = ctx->n;
  hipError_t e = dalloc(&pre, wp * n);
  if (e == hipSuccess) e = dalloc(&act, wa * n);
  if (e == hipSuccess) e = dalloc(&ea, we * n);
  if (e == hipSuccess) e = dalloc(&eb, we * n);
  if (e == hipSuccess) e = want_full ? dalloc(&full, wm * n) : dalloc(&pop, wm);
  if (e == hipSuccess) e = dalloc(&s, w0);
  return e;
}

// BranchSampler::effect_sizes (branch_sampler.rs:784-811): forward_feed + the
// output-seeded backward chain (kernels_feed.hip), the n x m matrix to the host
extern "C" int bann_effect_sizes(bann_ctx* ctx, int32_t b, float* out) {
  if (!check_branch(ctx, b) || !out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  const BranchHost& h = ctx->br[b];
  EffectScratch sc;
  if (sc.alloc(ctx, &b, 1, true) != hipSuccess) return fail(ctx, BANN_E_OOM, "effect_sizes scratch");
  launch_forward_feed(ctx->st, b, h.dev, sc.pre, sc.act, ctx->stream);
  launch_effect_sizes(ctx->st, b, h.dev, sc.pre, sc.act, sc.ea, sc.eb, sc.full, nullptr, nullptr, ctx->stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(out, sc.full, (int64_t)h.m * ctx->n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

// Net::population_effect_sizes' per-branch column means (net.rs:529-543)
extern "C" int bann_population_effect_sizes(bann_ctx* ctx, const int32_t* branches, int32_t nb, float* out) {
  if (!ctx || !branches || nb <= 0 || !out) return fail(ctx, BANN_E_ARG, "null pointer or empty branch list");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  for (int32_t i = 0; i < nb; ++i)
    if (!check_branch(ctx, branches[i])) return fail(ctx, BANN_E_ARG, "bad branch index");
  EffectScratch sc;
  if (sc.alloc(ctx, branches, nb, false) != hipSuccess) return fail(ctx, BANN_E_OOM, "population_effect_sizes scratch");
  int64_t at = 0;
  for (int32_t i = 0; i < nb; ++i) {
    const BranchHost& h = ctx->br[branches[i]];
    launch_forward_feed(ctx->st, branches[i], h.dev, sc.pre, sc.act, ctx->stream);
    launch_effect_sizes(ctx->st, branches[i], h.dev, sc.pre, sc.act, sc.ea, sc.eb, nullptr, sc.s, sc.pop,
                        ctx->stream);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(out + at, sc.pop, (int64_t)h.m * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    at += h.m;
  }
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

// host evaluation of log_density at the current parameters (branch_sampler.rs:72-78)
static int host_log_density(bann_ctx* ctx, int32_t b, double rss, double* out) {
  const BranchHost& h = ctx->br[b];
  std::vector<float> th(h.P), lam, lamld;
  CK(hipMemcpyAsync(th.data(), ctx->d_theta + h.dev.p_off, h.P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  float ep = 1.f;
  expand_precisions(h, lam, lamld, ep);
  const bool lasso = (h.prior == BANN_LASSO_ARD || h.prior == BANN_LASSO_BASE);
  double ld = 0.0;
  for (int i = 0; i < h.P; ++i)
    ld -= lasso ? (double)lamld[i] * fabs((double)th[i]) : 0.5 * (double)lamld[i] * (double)th[i] * (double)th[i];
  *out = ld - (double)ep * rss / 2.0;
  return BANN_OK;
}

extern "C" int bann_log_density(bann_ctx* ctx, int32_t b, double rss, double* out) {
  if (!check_branch(ctx, b) || !out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  return host_log_density(ctx, b, rss, out);
}

extern "C" int bann_neg_hamiltonian(bann_ctx* ctx, int32_t b, const float* momentum, double* out) {
  if (!check_branch(ctx, b) || !momentum || !out) return fail(ctx, BANN_E_ARG, "bad branch or null pointer");
  double rss = 0.0;
  int rc = bann_rss(ctx, b, &rss);
  if (rc) return rc;
  double ld = 0.0;
  rc = host_log_density(ctx, b, rss, &ld);
  if (rc) return rc;
  double k = 0.0;
  for (int64_t i = 0; i < ctx->br[b].P; ++i) k += (double)momentum[i] * (double)momentum[i];
  *out = ld - 0.5 * k;
  return BANN_OK;
}
