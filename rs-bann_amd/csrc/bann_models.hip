// bann_models.hip — the model-slot bank of include/bann.h (bann_models_*) and the chain-level
// branch statistics over it (bann_models_branch_stats).
#include <algorithm>
#include <string>
#include <vector>

#include "ctx_internal.h"

// ---------------------------------------------------------------------------
// Model slots: a bank of parameter sets beside the live one, for predicting a chain of
// saved models from one genotype pass (rs-bann predict, rs-bann.rs:276-312).  A slot owns
// its theta, its W0 / sigma digit image and its fused constants; every slot kernel runs on
// a DevState copy whose theta / dig / fc point at the slot and whose prediction rows point
// at the pass scratch, so the live state (theta, dig, fc, pred, pred0, pred_ok, targets,
// momenta, step sizes) is never written.  The partial-gradient slabs, rss partials and the
// gx scratch, which every evaluation rewrites, serve the non-fx paths as scratch.
// ---------------------------------------------------------------------------
void models_release(bann_ctx* ctx) {
  dfree_all(ctx->d_ms_theta, ctx->d_ms_dig, ctx->d_ms_fc, ctx->d_ms_rows, ctx->d_ms_yhat, ctx->d_ms_mom);
  ctx->ms_cap = 0;
  ctx->ms_bias.clear();
  ctx->ms_set.clear();
  dfree_all(ctx->d_bs_y, ctx->d_bs_part, ctx->d_bs_rss, ctx->d_bs_pop, ctx->d_bs_mom, ctx->d_bs_jobs);
  ctx->bs_part_cap = ctx->bs_rss_cap = ctx->bs_pop_cap = ctx->bs_mom_cap = ctx->bs_jobs_cap = 0;
}

static DevState slot_state(const bann_ctx* ctx, int32_t k) {
  DevState s = ctx->st;
  s.theta = ctx->d_ms_theta + (int64_t)k * ctx->total_p;
  s.dig = ctx->d_ms_dig + (int64_t)k * ctx->ms_dig_bytes;
  s.fc = ctx->d_ms_fc + (int64_t)k * (int64_t)ctx->br.size();
  s.pred = ctx->d_ms_rows;
  return s;
}

static int models_ready(bann_ctx* ctx) {
  if (!ctx) return BANN_E_ARG;
  if (!ctx->finalized) return fail(ctx, BANN_E_STATE, "call bann_finalize first");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  return BANN_OK;
}

extern "C" int bann_models_pass_width(void) { return BANN_FE_KM; }

extern "C" int bann_models_capacity(const bann_ctx* ctx) { return ctx ? ctx->ms_cap : 0; }

extern "C" int bann_models_reserve(bann_ctx* ctx, int32_t num_models) {
  int rc = models_ready(ctx);
  if (rc) return rc;
  if (num_models < 0) return fail(ctx, BANN_E_ARG, "negative model count");
  CK(hipStreamSynchronize(ctx->stream));
  models_release(ctx);
  if (num_models == 0) return BANN_OK;
  const int64_t nb = (int64_t)ctx->br.size(), K = num_models;
  int64_t dig_bytes = 0;  // the digit image as plan_layout sizes it
  for (const BranchHost& h : ctx->br)
    if (h.dev.fused != PATH_GX)
      dig_bytes = std::max(dig_bytes, h.dev.dig_off + (int64_t)h.dev.nchunks * 1024 * (h.dev.fused == PATH_WX ? 8 : 1));
  ctx->ms_dig_bytes = (dig_bytes + 15) / 16 * 16;
  auto alloc_all = [&]() -> hipError_t {
    hipError_t e;
    if ((e = dalloc(&ctx->d_ms_theta, K * ctx->total_p)) != hipSuccess) return e;
    if ((e = dalloc(&ctx->d_ms_dig, K * ctx->ms_dig_bytes)) != hipSuccess) return e;
    if ((e = dalloc(&ctx->d_ms_fc, K * nb)) != hipSuccess) return e;
    if ((e = dalloc(&ctx->d_ms_rows, (int64_t)BANN_FE_KM * nb * ctx->n)) != hipSuccess) return e;
    if ((e = dalloc(&ctx->d_ms_yhat, K * ctx->n)) != hipSuccess) return e;
    if ((e = dalloc(&ctx->d_ms_mom, 2 * ctx->n)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(ctx->d_ms_theta, 0, (size_t)std::max<int64_t>(K * ctx->total_p, 1) * sizeof(float),
                            ctx->stream)) != hipSuccess)
      return e;
    // the padding rows of a digit image stay zero, as in the live image (alloc_branch_state)
    if ((e = hipMemsetAsync(ctx->d_ms_dig, 0, (size_t)std::max<int64_t>(K * ctx->ms_dig_bytes, 1), ctx->stream)) !=
        hipSuccess)
      return e;
    if ((e = hipMemsetAsync(ctx->d_ms_fc, 0, (size_t)(K * nb) * sizeof(FusedConst), ctx->stream)) != hipSuccess) return e;
    return hipStreamSynchronize(ctx->stream);
  };
  const hipError_t e = alloc_all();
  if (e != hipSuccess) {
    models_release(ctx);
    return fail(ctx, e == hipErrorOutOfMemory ? BANN_E_OOM : BANN_E_HIP,
                std::string("bann_models_reserve: ") + hipGetErrorString(e));
  }
  ctx->ms_cap = num_models;
  ctx->ms_bias.assign((size_t)K, 0.f);
  ctx->ms_set.assign((size_t)(K * nb), 0);
  return BANN_OK;
}

extern "C" int bann_models_set_params(bann_ctx* ctx, int32_t k, int32_t b, const float* param_vec) {
  int rc = models_ready(ctx);
  if (rc) return rc;
  if (k < 0 || k >= ctx->ms_cap) return fail(ctx, BANN_E_ARG, "model slot out of range");
  if (!check_branch(ctx, b) || !param_vec) return fail(ctx, BANN_E_ARG, "bad branch or null params");
  const BranchHost& h = ctx->br[b];
  const DevState s = slot_state(ctx, k);
  CK(hipMemcpyAsync(s.theta + h.dev.p_off, param_vec, h.P * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  int32_t bb = b;
  CK(hipMemcpyAsync(ctx->d_list_scr, &bb, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  launch_fused_const(s, ctx->d_list_scr, 1, ctx->stream);  // the slot's digits and constants: the live path's bits
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->stream));
  ctx->ms_set[(size_t)k * ctx->br.size() + b] = 1;
  return BANN_OK;
}

extern "C" int bann_models_set_bias(bann_ctx* ctx, int32_t k, float bias) {
  int rc = models_ready(ctx);
  if (rc) return rc;
  if (k < 0 || k >= ctx->ms_cap) return fail(ctx, BANN_E_ARG, "model slot out of range");
  ctx->ms_bias[k] = bias;
  return BANN_OK;
}

// the rows of slots k0 .. k0 + nk (nk <= BANN_FE_KM) for the plan's branches into the pass
// scratch ([model][branch][n]): fx groups through the multi-model forward, every other path
// per model through its own forward launches on the slot state
static int models_pass(bann_ctx* ctx, const Plan& p, int32_t k0, int32_t nk, FeModels& mm) {
  const int64_t nb = (int64_t)ctx->br.size();
  DevState sj[BANN_FE_KM];
  mm = FeModels{};
  mm.nk = nk;
  for (int j = 0; j < nk; ++j) {
    sj[j] = slot_state(ctx, k0 + j);
    sj[j].pred = ctx->d_ms_rows + (int64_t)j * nb * ctx->n;
    mm.theta[j] = sj[j].theta;
    mm.dig[j] = sj[j].dig;
    mm.fc[j] = sj[j].fc;
    mm.pred[j] = sj[j].pred;
    mm.bias[j] = ctx->ms_bias[k0 + j];
  }
  for (const auto& g : p.groups) {
    if (g.kind == PATH_FX) {
      launch_forward_fe(ctx->st, mm, g.d_items, (int32_t)g.items.size(), g.L, g.act, ctx->stream);
    } else {
      for (int j = 0; j < nk; ++j) launch_group_grad(ctx, sj[j], g, 1, -1, 0, nullptr, nullptr);
    }
  }
  if (!p.gxg.empty())
    for (int j = 0; j < nk; ++j) launch_gx_phases(ctx, sj[j], p, true);
  CK(hipGetLastError());
  return BANN_OK;
}

extern "C" int bann_models_predict(bann_ctx* ctx, int32_t k0, int32_t nk, float* y_hat_out, float* mean_out,
                                   float* var_out) {
  int rc = models_ready(ctx);
  if (rc) return rc;
  if (!y_hat_out) return fail(ctx, BANN_E_ARG, "null output");
  if (k0 < 0 || nk <= 0 || (int64_t)k0 + nk > ctx->ms_cap) return fail(ctx, BANN_E_ARG, "model slots out of range");
  const int32_t nb = (int32_t)ctx->br.size();
  for (int32_t k = k0; k < k0 + nk; ++k)
    for (int32_t b = 0; b < nb; ++b)
      if (!ctx->ms_set[(size_t)k * nb + b])
        return fail(ctx, BANN_E_STATE, "model slot " + std::to_string(k) + ": branch " + std::to_string(b) +
                                           " has no parameters");
  std::vector<int32_t> all(nb);
  for (int32_t b = 0; b < nb; ++b) all[b] = b;
  Plan p;
  rc = build_plan(ctx, all.data(), nb, p, false);
  if (rc) return rc;
  for (int32_t j0 = 0; j0 < nk; j0 += BANN_FE_KM) {
    FeModels mm;
    rc = models_pass(ctx, p, k0 + j0, std::min<int32_t>(BANN_FE_KM, nk - j0), mm);
    if (rc) return rc;
    launch_models_sum(mm, nb, ctx->n, ctx->d_ms_yhat + (int64_t)j0 * ctx->n, ctx->stream);
  }
  if (mean_out || var_out)
    launch_models_moments(ctx->d_ms_yhat, nk, ctx->n, mean_out ? ctx->d_ms_mom : nullptr,
                          var_out ? ctx->d_ms_mom + ctx->n : nullptr, ctx->stream);
  CK(hipGetLastError());
  CK(hipMemcpyAsync(y_hat_out, ctx->d_ms_yhat, (size_t)nk * ctx->n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (mean_out) CK(hipMemcpyAsync(mean_out, ctx->d_ms_mom, ctx->n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (var_out)
    CK(hipMemcpyAsync(var_out, ctx->d_ms_mom + ctx->n, ctx->n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_models_branch_predictions(bann_ctx* ctx, int32_t k, const int32_t* branches, int32_t nb,
                                              float* pred_out) {
  int rc = models_ready(ctx);
  if (rc) return rc;
  if (!branches || nb <= 0 || !pred_out) return fail(ctx, BANN_E_ARG, "bad branch list or null output");
  if (k < 0 || k >= ctx->ms_cap) return fail(ctx, BANN_E_ARG, "model slot out of range");
  for (int32_t i = 0; i < nb; ++i) {
    if (!check_branch(ctx, branches[i])) return fail(ctx, BANN_E_ARG, "branch out of range");
    if (!ctx->ms_set[(size_t)k * ctx->br.size() + branches[i]])
      return fail(ctx, BANN_E_STATE, "model slot " + std::to_string(k) + ": branch " + std::to_string(branches[i]) +
                                         " has no parameters");
  }
  Plan p;
  rc = build_plan(ctx, branches, nb, p, false);
  if (rc) return rc;
  FeModels mm;
  rc = models_pass(ctx, p, k, 1, mm);
  if (rc) return rc;
  for (int32_t i = 0; i < nb; ++i)
    CK(hipMemcpyAsync(pred_out + (int64_t)i * ctx->n, mm.pred[0] + (int64_t)branches[i] * ctx->n, ctx->n * sizeof(float),
                      hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

// ---------------------------------------------------------------------------
// Chain-level branch statistics (rs-bann branch-r2, rs-bann.rs:128-166, and
// population-effect-sizes, 314-372): per model slot and listed branch the rss of f_b
// against y and the branch's population effect sizes.  fx branches: k_stats_fe
// (kernels_fs.hip) streams each tile once per BANN_FS_KM models and leaves five doubles
// per (model, work item); k_stats_fold turns them into the results.  Every other kernel
// path goes model by model on the slot's DevState copy: its forward launch into the pass
// scratch rows and a row reduction for the rss, forward_feed + the effect-size chain
// (kernels_feed.hip) for the population effect sizes.  The live state is never written.
// ---------------------------------------------------------------------------
extern "C" int bann_models_stats_pass_width(void) { return BANN_FS_KM; }

// a scratch buffer of at least `need` elements (the old contents are not kept)
template <typename T>
static hipError_t stats_grow(T** p, int64_t* cap, int64_t need) {
  if (*p && *cap >= need) return hipSuccess;
  dfree(*p);
  *cap = 0;
  const hipError_t e = dalloc(p, need);
  if (e == hipSuccess) *cap = std::max<int64_t>(need, 1);
  return e;
}

// kernel_ms (nullable): the HIP-event time of the call's k_stats_fe launches, every pass and fx group
static int models_branch_stats(bann_ctx* ctx, int32_t k0, int32_t nk, const int32_t* branches, int32_t nb,
                               const float* y, double* rss_out, float* pop_out, float* pop_mean_out,
                               float* pop_var_out, float* kernel_ms) {
  int rc = models_ready(ctx);
  if (rc) return rc;
  if (!branches || nb <= 0) return fail(ctx, BANN_E_ARG, "null or empty branch list");
  if ((y == nullptr) != (rss_out == nullptr)) return fail(ctx, BANN_E_ARG, "y and rss_out go together");
  const bool want_pop = pop_out || pop_mean_out || pop_var_out;
  if (!rss_out && !want_pop) return fail(ctx, BANN_E_ARG, "no output requested");
  if (k0 < 0 || nk <= 0 || (int64_t)k0 + nk > ctx->ms_cap) return fail(ctx, BANN_E_ARG, "model slots out of range");
  const int32_t nbr = (int32_t)ctx->br.size();
  if (nb > nbr) return fail(ctx, BANN_E_ARG, "branch list longer than the branch set");
  std::vector<char> seen(nbr, 0);
  for (int32_t i = 0; i < nb; ++i) {
    if (!check_branch(ctx, branches[i])) return fail(ctx, BANN_E_ARG, "branch out of range");
    if (seen[branches[i]]) return fail(ctx, BANN_E_ARG, "duplicate branch in list");
    seen[branches[i]] = 1;
  }
  for (int32_t k = k0; k < k0 + nk; ++k)
    for (int32_t i = 0; i < nb; ++i)
      if (!ctx->ms_set[(size_t)k * nbr + branches[i]])
        return fail(ctx, BANN_E_STATE, "model slot " + std::to_string(k) + ": branch " + std::to_string(branches[i]) +
                                           " has no parameters");
  Plan p;
  rc = build_plan(ctx, branches, nb, p, false);
  if (rc) return rc;
  const int64_t n = ctx->n;
  // the fx groups' work items in launch order: the index space of the records
  std::vector<int64_t> gbase(p.groups.size(), 0);
  int64_t nitems = 0;
  for (size_t gi = 0; gi < p.groups.size(); ++gi)
    if (p.groups[gi].kind == PATH_FX) {
      gbase[gi] = nitems;
      nitems += (int64_t)p.groups[gi].items.size();
    }
  std::vector<int64_t> pop_off(nb);
  int64_t summ = 0;
  std::vector<FsFoldJob> jobs;
  std::vector<int32_t> others;  // list positions of the branches of the other kernel paths
  for (int32_t i = 0; i < nb; ++i) {
    const BranchHost& h = ctx->br[branches[i]];
    pop_off[i] = summ;
    summ += h.m;
    if (h.dev.fused != PATH_FX) {
      others.push_back(i);
      continue;
    }
    FsFoldJob jb{branches[i], i, 0, 0, pop_off[i]};
    for (size_t gi = 0; gi < p.groups.size() && jb.item_count == 0; ++gi) {
      const LaunchGroup& g = p.groups[gi];
      if (g.kind != PATH_FX) continue;
      for (size_t q = 0; q < g.items.size(); ++q)  // a branch's items are consecutive (plan_fused_groups)
        if (g.items[q].branch == branches[i]) {
          if (jb.item_count == 0) jb.item_begin = (int32_t)(gbase[gi] + (int64_t)q);
          ++jb.item_count;
        }
    }
    jobs.push_back(jb);
  }
  const int64_t model_stride = nitems * 5;
  hipError_t e = hipSuccess;
  if (y && !ctx->d_bs_y) e = dalloc(&ctx->d_bs_y, n);
  if (e == hipSuccess) e = stats_grow(&ctx->d_bs_part, &ctx->bs_part_cap, (int64_t)nk * model_stride);
  if (e == hipSuccess) e = stats_grow(&ctx->d_bs_rss, &ctx->bs_rss_cap, (int64_t)nk * nb);
  if (e == hipSuccess && want_pop) e = stats_grow(&ctx->d_bs_pop, &ctx->bs_pop_cap, (int64_t)nk * summ);
  if (e == hipSuccess && (pop_mean_out || pop_var_out)) e = stats_grow(&ctx->d_bs_mom, &ctx->bs_mom_cap, 2 * summ);
  if (e == hipSuccess) e = stats_grow(&ctx->d_bs_jobs, &ctx->bs_jobs_cap, (int64_t)jobs.size());
  if (e != hipSuccess)
    return fail(ctx, e == hipErrorOutOfMemory ? BANN_E_OOM : BANN_E_HIP,
                std::string("bann_models_branch_stats: ") + hipGetErrorString(e));
  const float* dy = nullptr;
  if (y) {
    CK(hipMemcpyAsync(ctx->d_bs_y, y, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    dy = ctx->d_bs_y;
  }
  double* d_rss = rss_out ? ctx->d_bs_rss : nullptr;
  float* d_pop = want_pop ? ctx->d_bs_pop : nullptr;
  struct EventPair {  // around the k_stats_fe launches, when the caller wants their time
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } ev;
  if (kernel_ms) *kernel_ms = 0.f;
  if (!jobs.empty()) {
    CK(hipMemcpyAsync(ctx->d_bs_jobs, jobs.data(), jobs.size() * sizeof(FsFoldJob), hipMemcpyHostToDevice, ctx->stream));
    if (kernel_ms) {
      CK(hipEventCreate(&ev.a));
      CK(hipEventCreate(&ev.b));
      CK(hipEventRecord(ev.a, ctx->stream));
    }
    for (int32_t j0 = 0; j0 < nk; j0 += BANN_FS_KM) {
      FsModels mm{};
      mm.nk = std::min<int32_t>(BANN_FS_KM, nk - j0);
      for (int j = 0; j < mm.nk; ++j) {
        const DevState sj = slot_state(ctx, k0 + j0 + j);
        mm.theta[j] = sj.theta;
        mm.dig[j] = sj.dig;
        mm.fc[j] = sj.fc;
      }
      for (size_t gi = 0; gi < p.groups.size(); ++gi) {
        const LaunchGroup& g = p.groups[gi];
        if (g.kind != PATH_FX) continue;
        launch_stats_fe(ctx->st, mm, g.d_items, (int32_t)g.items.size(), g.L, g.act, dy,
                        ctx->d_bs_part + (int64_t)j0 * model_stride + gbase[gi] * 5, model_stride, ctx->stream);
      }
    }
    if (kernel_ms) CK(hipEventRecord(ev.b, ctx->stream));
    launch_stats_fold(ctx->st, ctx->d_ms_theta + (int64_t)k0 * ctx->total_p, ctx->total_p, nk, ctx->d_bs_jobs,
                      (int32_t)jobs.size(), ctx->d_bs_part, model_stride, d_rss, nb, d_pop, summ, ctx->stream);
    CK(hipGetLastError());
  }
  EffectScratch sc;  // outlives its launches: the stream is drained before every return below
  if (!others.empty()) {
    std::vector<int32_t> ob;
    for (int32_t i : others) ob.push_back(branches[i]);
    if (want_pop && sc.alloc(ctx, ob.data(), (int32_t)ob.size(), false) != hipSuccess) {
      (void)hipStreamSynchronize(ctx->stream);
      return fail(ctx, BANN_E_OOM, "bann_models_branch_stats: effect-size scratch");
    }
    for (int32_t j = 0; j < nk; ++j) {
      const DevState sj = slot_state(ctx, k0 + j);  // prediction rows: the pass scratch
      if (d_rss) {
        for (const auto& g : p.groups)
          if (g.kind != PATH_FX) launch_group_grad(ctx, sj, g, 1, -1, 0, nullptr, nullptr);
        if (!p.gxg.empty()) launch_gx_phases(ctx, sj, p, true);
        for (int32_t i : others)
          launch_row_rss(sj.pred + ctx->br[branches[i]].dev.y_off, dy, n, d_rss + (int64_t)j * nb + i, ctx->stream);
      }
      if (d_pop)
        for (int32_t i : others) {
          const BranchHost& h = ctx->br[branches[i]];
          launch_forward_feed(sj, branches[i], h.dev, sc.pre, sc.act, ctx->stream);
          launch_effect_sizes(sj, branches[i], h.dev, sc.pre, sc.act, sc.ea, sc.eb, nullptr, sc.s,
                              d_pop + (int64_t)j * summ + pop_off[i], ctx->stream);
        }
    }
  }
  hipError_t le = hipGetLastError();
  if (le == hipSuccess && (pop_mean_out || pop_var_out))
    launch_models_moments(d_pop, nk, summ, pop_mean_out ? ctx->d_bs_mom : nullptr,
                          pop_var_out ? ctx->d_bs_mom + summ : nullptr, ctx->stream);
  if (le == hipSuccess) le = hipGetLastError();
  if (le == hipSuccess) le = hipStreamSynchronize(ctx->stream);  // nothing is written to an output before this
  if (le != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);
    return fail(ctx, BANN_E_HIP, std::string("bann_models_branch_stats: ") + hipGetErrorString(le));
  }
  if (ev.b) CK(hipEventElapsedTime(kernel_ms, ev.a, ev.b));
  if (rss_out) CK(hipMemcpy(rss_out, ctx->d_bs_rss, (size_t)nk * nb * sizeof(double), hipMemcpyDeviceToHost));
  if (pop_out) CK(hipMemcpy(pop_out, ctx->d_bs_pop, (size_t)nk * summ * sizeof(float), hipMemcpyDeviceToHost));
  if (pop_mean_out) CK(hipMemcpy(pop_mean_out, ctx->d_bs_mom, (size_t)summ * sizeof(float), hipMemcpyDeviceToHost));
  if (pop_var_out) CK(hipMemcpy(pop_var_out, ctx->d_bs_mom + summ, (size_t)summ * sizeof(float), hipMemcpyDeviceToHost));
  return BANN_OK;
}

extern "C" int bann_models_branch_stats(bann_ctx* ctx, int32_t k0, int32_t nk, const int32_t* branches, int32_t nb,
                                        const float* y, double* rss_out, float* pop_out, float* pop_mean_out,
                                        float* pop_var_out) {
  return models_branch_stats(ctx, k0, nk, branches, nb, y, rss_out, pop_out, pop_mean_out, pop_var_out, nullptr);
}

extern "C" int bann_models_branch_stats_timed(bann_ctx* ctx, int32_t k0, int32_t nk, const int32_t* branches,
                                              int32_t nb, const float* y, double* rss_out, float* pop_out,
                                              float* stats_kernel_ms) {
  if (!stats_kernel_ms) return fail(ctx, BANN_E_ARG, "null timing output");
  return models_branch_stats(ctx, k0, nk, branches, nb, y, rss_out, pop_out, nullptr, nullptr, stats_kernel_ms);
}
