// bann_branch.hip — the branch registry of include/bann.h and the state bann_finalize builds
// from it: bann_branch_add, bann_finalize and its stages (plan_layout of finalize_layout.h
// decides, the stages here allocate, pack and upload), the precision-derived device arrays
// (expand_precisions, step_bases, upload_precisions), parameters / precisions / targets set
// and get.
//
// Host-side counterpart of the reference's B::from_cfg / to_cfg (branch_struct.rs:12-29,
// branch_sampler.rs:155-171).
#include <math.h>
#include <stdio.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx_internal.h"

extern "C" int bann_branch_add(bann_ctx* ctx, const int32_t* snp_idx, int32_t m, const int32_t* layer_widths,
                               int32_t num_layers, int32_t activation, int32_t prior) {
  if (!ctx || !snp_idx || !layer_widths) return BANN_E_ARG;
  if (ctx->finalized) return fail(ctx, BANN_E_STATE, "branch set is fixed after bann_finalize");
  if (m <= 0) return fail(ctx, BANN_E_SHAPE, "a branch needs at least one marker");
  if (num_layers < 2 || num_layers > BANN_MAXL)
    return fail(ctx, BANN_E_SHAPE, "num_layers must be in [2, 8] (summary + output at least)");
  if (layer_widths[num_layers - 1] != 1) return fail(ctx, BANN_E_SHAPE, "output layer width must be 1");
  if (activation < 0 || activation > 4) return fail(ctx, BANN_E_ARG, "unknown activation");
  if (prior < 0 || prior > 4) return fail(ctx, BANN_E_ARG, "unknown prior");
  for (int l = 0; l < num_layers; ++l)
    if (layer_widths[l] <= 0) return fail(ctx, BANN_E_SHAPE, "layer widths must be positive");
  for (int i = 0; i < m; ++i)
    if (snp_idx[i] < 0 || (ctx->M > 0 && snp_idx[i] >= ctx->M))
      return fail(ctx, BANN_E_SHAPE, "marker index out of range");
  ctx->br.push_back(make_branch(snp_idx, m, layer_widths, num_layers, activation, prior));
  return (int)ctx->br.size() - 1;
}

// expanded per-parameter precision multipliers and the error precision
void expand_precisions(const BranchHost& h, std::vector<float>& lam, std::vector<float>& lamld, float& eprec) {
  const BranchDev& d = h.dev;
  lam.assign(h.P, 0.f);
  lamld.assign(h.P, 0.f);
  const bool ard = (h.prior == BANN_RIDGE_ARD || h.prior == BANN_LASSO_ARD);
  int pi = 0;
  for (int l = 0; l < h.L; ++l) {
    const int wi = d.win[l], wo = d.widths[l];
    for (int k = 0; k < wo; ++k)
      for (int j = 0; j < wi; ++j) {
        float v;
        if (h.prior == BANN_STD_NORMAL)
          v = 1.f;
        else if (ard && l < h.L - 1)
          v = h.prec[pi + j];
        else
          v = h.prec[pi];
        lam[d.woff[l] + k * wi + j] = v;
        lamld[d.woff[l] + k * wi + j] = v;
      }
    pi += (ard && l < h.L - 1) ? wi : 1;
  }
  if (h.prior == BANN_STD_NORMAL)  // std_normal_branch.rs:149-158: l2 bias term in log_density only
    for (int l = 0; l < h.L - 1; ++l)
      for (int k = 0; k < d.widths[l]; ++k) lamld[d.boff[l] + k] = 1.f;
  eprec = h.prec.back();
}

// per-parameter Izmailov step base, so the device can form eps = base * c / L
// for any factor c and trajectory length L without a host round trip:
// ridge / bias terms pi / (2 sqrt(lam)), lasso 1 / (4 lam); negative = the
// factor c does not apply (std_normal weights and biases).  eps = base * c / L
// reproduces the reference's c * pi / (2 sqrt(lam) L) and c / (4 lam L).
static void step_bases(const BranchHost& h, std::vector<double>& out) {
  const BranchDev& d = h.dev;
  out.assign(h.P, 0.0);
  const bool ard = (h.prior == BANN_RIDGE_ARD || h.prior == BANN_LASSO_ARD);
  const bool lasso = (h.prior == BANN_LASSO_ARD || h.prior == BANN_LASSO_BASE);
  const bool stdn = h.prior == BANN_STD_NORMAL;
  const double PI = 3.14159265358979323846;
  int pi = 0;
  for (int l = 0; l < h.L; ++l) {
    const int wi = d.win[l], wo = d.widths[l];
    for (int k = 0; k < wo; ++k)
      for (int j = 0; j < wi; ++j) {
        const double lam = (ard && l < h.L - 1) ? h.prec[pi + j] : h.prec[pi];
        double e;
        if (stdn)
          e = -PI / (2.0 * sqrt(lam));
        else if (lasso)
          e = 1.0 / (4.0 * lam);
        else
          e = PI / (2.0 * sqrt(lam));
        out[d.woff[l] + k * wi + j] = e;
      }
    pi += (ard && l < h.L - 1) ? wi : 1;
  }
  for (int l = 0; l < h.L - 1; ++l) {
    const double lb = h.prec[pi + l];
    const double e = PI / (2.0 * sqrt(lb));
    for (int k = 0; k < d.widths[l]; ++k) out[d.boff[l] + k] = stdn ? -e : e;
  }
}

// ---------------------------------------------------------------------------
// finalize: plan_layout (finalize_layout.h) decides, the steps below allocate, pack and upload
// ---------------------------------------------------------------------------
// floats of one gx scratch group: BANN_GX_SCRATCH_MB, default a quarter of the free device
// memory, at least 8 and at most 64 GiB
static int64_t gx_scratch_budget(const EnvOptions& opt) {
  int64_t budget = 8192ll << 18;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0)
    budget = std::max<int64_t>(budget, std::min<int64_t>((int64_t)(fr / 4) / 4, 65536ll << 18));
  return opt.gx_scratch_mb > 0 ? opt.gx_scratch_mb << 18 : budget;
}

// the host arrays that bann_finalize's asynchronous copies read and the temporary device
// arrays of its pack launches: alive until its steps have synchronised
struct FinalizeStage {
  std::vector<int32_t> allidx;  // the branches' marker indices, concatenated
  std::vector<PackJob> jobs;
  std::vector<BranchDev> descs;
  std::vector<float> eprec;
  int32_t* d_idx = nullptr;
  PackJob* d_jobs = nullptr;
  PackJob* d_fijobs = nullptr;
};

// parameter -> precision index (within the branch), for the joint update
static std::vector<int32_t> precision_index(const std::vector<BranchHost>& br, int64_t total_p) {
  std::vector<int32_t> pidx(total_p);
  for (auto& h : br) {
    const BranchDev& d = h.dev;
    const bool ard = (h.prior == BANN_RIDGE_ARD || h.prior == BANN_LASSO_ARD);
    for (int l = 0; l < h.L; ++l)
      for (int k = 0; k < d.widths[l]; ++k)
        for (int j = 0; j < d.win[l]; ++j)
          pidx[d.p_off + d.woff[l] + (int64_t)k * d.win[l] + j] = d.qoff[l] + ((ard && l < h.L - 1) ? j : 0);
    for (int l = 0; l < h.L - 1; ++l)
      for (int k = 0; k < d.widths[l]; ++k) pidx[d.p_off + d.boff[l] + k] = d.qbias + l;
  }
  return pidx;
}

// the images, the parameter- and precision-sized arrays, the partial slabs and the n-vectors
static int alloc_branch_state(bann_ctx* ctx, const LayoutTotals& t) {
  const int64_t n = ctx->n, nb = (int64_t)ctx->br.size(), p_off = t.total_p;
  CK(dalloc(&ctx->d_xu2, t.tile_bytes));
  ctx->xi_bytes = t.fi_bytes;
  if (t.fi_bytes > 0) CK(dalloc(&ctx->d_xi, t.fi_bytes));
  CK(dalloc(&ctx->d_dig, t.dig_bytes));
  CK(hipMemsetAsync(ctx->d_dig, 0, (size_t)std::max<int64_t>(t.dig_bytes, 1), ctx->stream));
  CK(dalloc(&ctx->d_fc, nb));
  CK(hipMemsetAsync(ctx->d_fc, 0, nb * sizeof(FusedConst), ctx->stream));
  CK(dalloc(&ctx->d_mub, t.total_markers));
  CK(dalloc(&ctx->d_sigb, t.total_markers));
  float** pbufs[] = {&ctx->d_theta, &ctx->d_mom, &ctx->d_eps, &ctx->d_theta0, &ctx->d_lam, &ctx->d_lamld,
                     &ctx->d_grad};
  for (float** pb : pbufs) {
    CK(dalloc(pb, p_off));
    CK(hipMemsetAsync(*pb, 0, p_off * sizeof(float), ctx->stream));
  }
  CK(dalloc(&ctx->d_stepbase, p_off));
  for (float** qb : {&ctx->d_phi, &ctx->d_phi0, &ctx->d_mphi, &ctx->d_ephi, &ctx->d_gphi}) CK(dalloc(qb, t.total_q));
  CK(dalloc(&ctx->d_ows, 2 * nb));
  {
    const std::vector<int32_t> pidx = precision_index(ctx->br, p_off);
    CK(dalloc(&ctx->d_pidx, p_off));
    CK(hipMemcpy(ctx->d_pidx, pidx.data(), p_off * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  CK(dalloc(&ctx->d_part, t.part_total + t.solo_part_cap));
  CK(hipMemsetAsync(ctx->d_part, 0, t.part_total * sizeof(float), ctx->stream));
  CK(dalloc(&ctx->d_rss_part, nb * t.max_splits + t.solo_rss_cap));
  CK(hipMemsetAsync(ctx->d_rss_part, 0, nb * t.max_splits * sizeof(double), ctx->stream));
  CK(dalloc(&ctx->d_y, nb * n));
  CK(hipMemsetAsync(ctx->d_y, 0, nb * n * sizeof(float), ctx->stream));
  CK(dalloc(&ctx->d_pred, nb * n));
  CK(hipMemsetAsync(ctx->d_pred, 0, nb * n * sizeof(float), ctx->stream));
  CK(dalloc(&ctx->d_pred0, nb * n));
  CK(dalloc(&ctx->d_delta, n));
  CK(dalloc(&ctx->d_delta_part, residual_delta_scratch_floats(n)));
  return BANN_OK;
}

// the pinned host mirrors, the per-branch trajectory scalars and a per-call plan's scratch
static int alloc_driver_scratch(bann_ctx* ctx, const LayoutTotals& t) {
  const int64_t n = ctx->n, nb = (int64_t)ctx->br.size();
  CK(hipHostMalloc((void**)&ctx->h_status, nb * sizeof(int32_t), hipHostMallocDefault));
  {
    int64_t max_p = 1;
    for (const auto& h : ctx->br) max_p = std::max<int64_t>(max_p, h.P);
    CK(hipHostMalloc((void**)&ctx->h_par_stage, max_p * sizeof(float), hipHostMallocDefault));
  }
  CK(hipHostMalloc((void**)&ctx->h_delta, n * sizeof(float), hipHostMallocDefault));
  CK(hipMemsetAsync(ctx->d_pred0, 0, nb * n * sizeof(float), ctx->stream));
  CK(dalloc(&ctx->d_scr, t.scr_floats));
  CK(dalloc(&ctx->d_eprec, nb));
  CK(dalloc(&ctx->d_upd_cnt, nb));
  CK(hipMemsetAsync(ctx->d_upd_cnt, 0, nb * sizeof(int32_t), ctx->stream));
  CK(dalloc(&ctx->d_u, nb));
  CK(dalloc(&ctx->d_h0, nb));
  CK(dalloc(&ctx->d_ld, nb));
  CK(dalloc(&ctx->d_rss, nb));
  CK(dalloc(&ctx->d_status, nb));
  CK(dalloc(&ctx->d_uturn, nb));
  return plan_scratch_alloc(ctx, t);
}

// what bann_finalize and upload_precisions allocated.  The BANN_STAMPS sums (a diagnostic
// build's per-phase cycle counts of the fused kernel) are printed before they go.
void branch_release(bann_ctx* ctx) {
  if (ctx->d_dbg) {
    unsigned long long h[16] = {};
    (void)hipMemcpy(h, ctx->d_dbg, sizeof(h), hipMemcpyDeviceToHost);
    fprintf(stderr, "BANN_STAMPS tiles=%llu cycles/tile:", h[15]);
    for (int i = 0; i < 8; ++i) fprintf(stderr, " p%d=%.0f", i, h[15] ? (double)h[i] / (double)h[15] : 0.0);
    fprintf(stderr, "\n");
  }
  dfree_all(ctx->d_dbg, ctx->d_br, ctx->d_xu2, ctx->d_xi, ctx->d_dig, ctx->d_fc, ctx->d_mub, ctx->d_sigb, ctx->d_theta,
            ctx->d_mom, ctx->d_eps, ctx->d_theta0, ctx->d_lam, ctx->d_lamld, ctx->d_grad, ctx->d_stepbase, ctx->d_phi,
            ctx->d_phi0, ctx->d_mphi, ctx->d_ephi, ctx->d_gphi, ctx->d_ows, ctx->d_pidx, ctx->d_part, ctx->d_rss_part,
            ctx->d_y, ctx->d_pred, ctx->d_pred0, ctx->d_delta, ctx->d_delta_part, ctx->d_scr, ctx->d_eprec,
            ctx->d_upd_cnt, ctx->d_u, ctx->d_h0, ctx->d_ld, ctx->d_rss, ctx->d_status, ctx->d_uturn);
  // upload_precisions' stage: its last copy has read the pinned side
  if (ctx->prec_ev_pending && ctx->ev_prec) (void)hipEventSynchronize(ctx->ev_prec);
  ctx->prec_ev_pending = false;
  dfree_all(ctx->d_prec_stage);
  for (void* p : {(void*)ctx->h_status, (void*)ctx->h_par_stage, (void*)ctx->h_delta, (void*)ctx->h_prec_stage})
    if (p) (void)hipHostFree(p);
  ctx->h_status = nullptr;
  ctx->h_par_stage = ctx->h_delta = nullptr;
  ctx->h_prec_stage = nullptr;
  ctx->prec_stage_cap = 0;
  if (ctx->ev_prec) (void)hipEventDestroy(ctx->ev_prec);
  ctx->ev_prec = nullptr;
}

// every branch's tile image in ONE batched pack launch (no per-branch sync), the fi images
// in another, the marker statistics in one gather
static int pack_images(bann_ctx* ctx, const LayoutTotals& t, FinalizeStage& fs) {
  const int64_t ntile = (t.nfrag + BANN_TILE_FRAGS - 1) / BANN_TILE_FRAGS;
  fs.allidx.reserve(t.total_markers);
  for (auto& h : ctx->br) {
    const int32_t base = (int32_t)fs.allidx.size();
    fs.allidx.insert(fs.allidx.end(), h.snp_idx.begin(), h.snp_idx.end());
    for (int c = 0; c < h.dev.nchunks; ++c)
      fs.jobs.push_back(PackJob{h.dev.x_off + 1024ll * c, 1024ll * h.dev.nchunks, base + 64 * c,
                                std::min(64, h.m - 64 * c), tile_f3m1(h.dev.fused) ? 1 : 0});
  }
  CK(dalloc(&fs.d_idx, (int64_t)fs.allidx.size()));
  CK(dalloc(&fs.d_jobs, (int64_t)fs.jobs.size()));
  CK(hipMemcpyAsync(fs.d_idx, fs.allidx.data(), fs.allidx.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                    ctx->stream));
  CK(hipMemcpyAsync(fs.d_jobs, fs.jobs.data(), fs.jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice, ctx->stream));
  launch_pack_tiles(ctx->d_g, ctx->rowb, fs.d_jobs, (int32_t)fs.jobs.size(), fs.d_idx, ntile, ctx->d_xu2, ctx->stream);
  if (ctx->d_xi) {  // the fi images: one job per (branch, 256-marker segment)
    std::vector<PackJob> fj;
    int32_t base = 0;
    for (auto& h : ctx->br) {
      const int nseg = (h.dev.nchunks + 3) / 4;
      if (h.dev.xi_off >= 0)
        for (int sg = 0; sg < nseg; ++sg)
          fj.push_back(PackJob{h.dev.xi_off + 1024ll * sg, 1024ll * nseg, base + 256 * sg,
                               std::min(256, h.m - 256 * sg)});
      base += h.m;
    }
    CK(dalloc(&fs.d_fijobs, (int64_t)fj.size()));
    CK(hipMemcpyAsync(fs.d_fijobs, fj.data(), fj.size() * sizeof(PackJob), hipMemcpyHostToDevice, ctx->stream));
    launch_pack_fi(ctx->d_g, ctx->rowb, fs.d_fijobs, (int32_t)fj.size(), fs.d_idx, ntile, ctx->d_xi, ctx->stream);
    CK(hipStreamSynchronize(ctx->stream));  // fj goes out of scope
  }
  launch_gather_stats(ctx->d_mu, ctx->d_sigma, fs.d_idx, (int32_t)fs.allidx.size(), ctx->d_mub, ctx->d_sigb,
                      ctx->stream);
  CK(hipGetLastError());
  return BANN_OK;
}

// the precision-derived arrays in one copy each, then the branch descriptors; frees the pack
// launches' device arrays once the stream has drained
static int upload_derived(bann_ctx* ctx, const LayoutTotals& t, FinalizeStage& fs) {
  const int64_t nb = (int64_t)ctx->br.size(), p_off = t.total_p;
  std::vector<float> lam_all(p_off), lamld_all(p_off), lam, lamld;
  std::vector<double> sbase_all(p_off), sbase;
  fs.eprec.assign(nb, 1.f);
  for (size_t b = 0; b < ctx->br.size(); ++b) {
    BranchHost& h = ctx->br[b];
    fs.descs.push_back(h.dev);
    float ep = 1.f;
    expand_precisions(h, lam, lamld, ep);
    fs.eprec[b] = ep;
    step_bases(h, sbase);
    std::copy(lam.begin(), lam.end(), lam_all.begin() + h.dev.p_off);
    std::copy(lamld.begin(), lamld.end(), lamld_all.begin() + h.dev.p_off);
    std::copy(sbase.begin(), sbase.end(), sbase_all.begin() + h.dev.p_off);
  }
  CK(hipMemcpyAsync(ctx->d_lam, lam_all.data(), p_off * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(ctx->d_lamld, lamld_all.data(), p_off * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(ctx->d_stepbase, sbase_all.data(), p_off * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));  // host vectors go out of scope
  dfree(fs.d_idx);
  dfree(fs.d_jobs);
  dfree(fs.d_fijobs);
  CK(dalloc(&ctx->d_br, nb));
  CK(hipMemcpyAsync(ctx->d_br, fs.descs.data(), nb * sizeof(BranchDev), hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(ctx->d_eprec, fs.eprec.data(), nb * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  if (ctx->opt.stamps) {
    CK(hipMalloc((void**)&ctx->d_dbg, 16 * sizeof(unsigned long long)));
    CK(hipMemsetAsync(ctx->d_dbg, 0, 16 * sizeof(unsigned long long), ctx->stream));
  }
  return BANN_OK;
}

extern "C" int bann_finalize(bann_ctx* ctx, int32_t free_raw) {
  if (!ctx) return BANN_E_ARG;
  if (ctx->finalized) return fail(ctx, BANN_E_STATE, "already finalized");
  if (!ctx->d_g) return fail(ctx, BANN_E_STATE, "no genotypes uploaded");
  if (ctx->br.empty()) return fail(ctx, BANN_E_STATE, "no branches");
  CK(hipSetDevice(ctx->device));
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0)
    cus = 256;
  ctx->cus = cus;
  const LayoutTotals t =
      plan_layout(ctx->n, ctx->M, cus, gx_scratch_budget(ctx->opt), ctx->fused_enabled, ctx->opt, ctx->br);
  if (t.err) return fail(ctx, t.err, t.msg);
  if (ctx->has_code3)  // field 3 of an fx / fxl / fxh tile image holds code - 1 in two bits (fx_tile.h)
    for (const BranchHost& h : ctx->br)
      if (h.dev.fused == PATH_FX || h.dev.fused == PATH_FXL)
        return fail(ctx, BANN_E_ARG,
                    "the cohort holds the genotype value 3, which the fx / fxl kernels (widths <= 4, m <= 4096) "
                    "cannot represent: upload values 0..2, or turn the fused kernels off");
  ctx->nfrag = t.nfrag;
  ctx->max_splits = t.max_splits;
  ctx->solo_threshold = t.solo_threshold;
  ctx->solo_rss_cap = t.solo_rss_cap;
  ctx->solo_part_cap = t.solo_part_cap;
  ctx->part_total = t.part_total;
  ctx->packed_bytes = t.tile_bytes;
  ctx->total_p = t.total_p;
  ctx->total_q = t.total_q;
  ctx->gxpre_cap = t.gxpre_cap;
  ctx->items_cap = t.items_cap;
  ctx->plan_off_fold = t.plan_off_fold;
  ctx->plan_off_items = t.plan_off_items;
  ctx->plan_scr_bytes = t.plan_scr_bytes;
  FinalizeStage fs;  // outlives every asynchronous copy below
  int rc = alloc_branch_state(ctx, t);
  if (!rc) rc = alloc_driver_scratch(ctx, t);
  if (!rc) rc = pack_images(ctx, t, fs);
  if (!rc) rc = upload_derived(ctx, t, fs);
  if (rc) return rc;
  ctx->finalized = true;
  ctx->pred_ok.assign(ctx->br.size(), 0);
  rc = ensure_htrace(ctx, 1);
  if (rc) return rc;
  rc = net_buffers_init(ctx);  // the network sampler allocates nothing inside its trajectories
  if (rc) return rc;
  refresh_state(ctx);
  CK(hipStreamSynchronize(ctx->stream));
  if (free_raw) {
    dfree(ctx->d_g);
    dfree(ctx->d_pm);
    ctx->d_g = ctx->d_pm = nullptr;
  }
  return BANN_OK;
}

extern "C" int bann_branch_set_params(bann_ctx* ctx, int32_t b, const float* param_vec) {
  if (!check_branch(ctx, b) || !param_vec) return fail(ctx, BANN_E_ARG, "bad branch or null params");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  const BranchHost& h = ctx->br[b];
  CK(hipMemcpyAsync(ctx->d_theta + h.dev.p_off, param_vec, h.P * sizeof(float), hipMemcpyHostToDevice,
                    ctx->stream));
  int32_t bb = b;
  CK(hipMemcpyAsync(ctx->d_list_scr, &bb, sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  launch_fused_const(ctx->st, ctx->d_list_scr, 1, ctx->stream);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->stream));
  ctx->pred_ok[b] = 0;
  return BANN_OK;
}

extern "C" int bann_branch_get_params(bann_ctx* ctx, int32_t b, float* out) {
  if (!check_branch(ctx, b) || !out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  const BranchHost& h = ctx->br[b];
  CK(hipMemcpyAsync(out, ctx->d_theta + h.dev.p_off, h.P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

// device copies derived from the host precision vector h.prec: per-parameter
// prior multipliers, error precision, Izmailov step bases
// the staged arrays of upload_precisions -> their device homes (one launch)
__global__ void k_scatter_prec(const char* __restrict__ stage, int P, float* __restrict__ lam,
                               float* __restrict__ lamld, double* __restrict__ sbase, float* __restrict__ ep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const double* sb = reinterpret_cast<const double*>(stage);
  const float* l = reinterpret_cast<const float*>(stage + 8 * (size_t)P);
  if (i < P) {
    sbase[i] = sb[i];
    lam[i] = l[i];
    lamld[i] = l[P + i];
  }
  if (i == 0) *ep = l[2 * P];
}

// One branch's precision-derived device arrays (prior multipliers, error precision,
// Izmailov step bases): staged in pinned memory as [sbase (f64) | lam | lamld | ep], one
// H2D copy and one scatter launch, no host wait -- the sequential driver does this once
// per branch update (it was four copies and a stream synchronisation).  The staging
// buffer is reused after the previous upload's copy has completed (event).
int upload_precisions(bann_ctx* ctx, int32_t b) {
  const BranchHost& h = ctx->br[b];
  std::vector<float> lam, lamld;
  float ep = 1.f;
  expand_precisions(h, lam, lamld, ep);
  std::vector<double> sbase;
  step_bases(h, sbase);
  const size_t bytes = 16 * (size_t)h.P + 16;
  if (bytes > ctx->prec_stage_cap) {
    if (ctx->prec_ev_pending) CK(hipEventSynchronize(ctx->ev_prec));
    if (ctx->h_prec_stage) (void)hipHostFree(ctx->h_prec_stage);
    if (ctx->d_prec_stage) (void)hipFree(ctx->d_prec_stage);
    ctx->h_prec_stage = nullptr;
    ctx->d_prec_stage = nullptr;
    ctx->prec_stage_cap = 0;
    size_t cap = bytes;
    for (const auto& o : ctx->br) cap = std::max(cap, 16 * (size_t)o.P + 16);
    CK(hipHostMalloc((void**)&ctx->h_prec_stage, cap, hipHostMallocDefault));
    CK(hipMalloc((void**)&ctx->d_prec_stage, cap));
    if (!ctx->ev_prec) CK(hipEventCreateWithFlags(&ctx->ev_prec, hipEventDisableTiming));
    ctx->prec_stage_cap = cap;
    ctx->prec_ev_pending = false;
  }
  if (ctx->prec_ev_pending) CK(hipEventSynchronize(ctx->ev_prec));  // the last upload's copy has read the stage
  char* st = ctx->h_prec_stage;
  std::memcpy(st, sbase.data(), 8 * (size_t)h.P);
  std::memcpy(st + 8 * (size_t)h.P, lam.data(), 4 * (size_t)h.P);
  std::memcpy(st + 12 * (size_t)h.P, lamld.data(), 4 * (size_t)h.P);
  std::memcpy(st + 16 * (size_t)h.P, &ep, sizeof(float));
  CK(hipMemcpyAsync(ctx->d_prec_stage, st, bytes, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_scatter_prec, dim3((unsigned)((h.P + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_prec_stage,
                     (int)h.P, ctx->d_lam + h.dev.p_off, ctx->d_lamld + h.dev.p_off, ctx->d_stepbase + h.dev.p_off,
                     ctx->d_eprec + b);
  CK(hipGetLastError());
  CK(hipEventRecord(ctx->ev_prec, ctx->stream));
  ctx->prec_ev_pending = true;
  return BANN_OK;
}

extern "C" int bann_branch_set_precisions(bann_ctx* ctx, int32_t b, const float* prec) {
  if (!check_branch(ctx, b) || !prec) return fail(ctx, BANN_E_ARG, "bad branch or null precisions");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  ctx->br[b].prec.assign(prec, prec + ctx->br[b].nprec);
  return upload_precisions(ctx, b);
}

extern "C" int bann_branch_set_output_stats(bann_ctx* ctx, int32_t b, float reg_sum_others, float num_params) {
  if (!check_branch(ctx, b)) return fail(ctx, BANN_E_ARG, "bad branch");
  ctx->br[b].ows_reg_sum = reg_sum_others;
  ctx->br[b].ows_num = num_params;
  return BANN_OK;
}

extern "C" int bann_branch_get_step_sizes(bann_ctx* ctx, int32_t b, float* out) {
  if (!check_branch(ctx, b) || !out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  const BranchHost& h = ctx->br[b];
  CK(hipMemcpyAsync(out, ctx->d_eps + h.dev.p_off, h.P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_branch_get_precisions(bann_ctx* ctx, int32_t b, float* out) {
  if (!check_branch(ctx, b) || !out) return fail(ctx, BANN_E_ARG, "bad branch or null output");
  std::copy(ctx->br[b].prec.begin(), ctx->br[b].prec.end(), out);
  return BANN_OK;
}

extern "C" int bann_branch_set_target(bann_ctx* ctx, int32_t b, const float* y) {
  if (!check_branch(ctx, b) || !y) return fail(ctx, BANN_E_ARG, "bad branch or null target");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  CK(hipMemcpyAsync(ctx->d_y + (int64_t)b * ctx->n, y, ctx->n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_set_target_all(bann_ctx* ctx, const float* y) {
  if (!ctx || !ctx->finalized || !y) return fail(ctx, BANN_E_ARG, "not finalized or null target");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  for (size_t b = 0; b < ctx->br.size(); ++b)
    CK(hipMemcpyAsync(ctx->d_y + (int64_t)b * ctx->n, y, ctx->n * sizeof(float), hipMemcpyHostToDevice,
                      ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}
