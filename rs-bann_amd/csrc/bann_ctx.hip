// bann_ctx.hip — the context of include/bann.h: version, create / destroy, last error,
// synchronize, the kernels' by-value state (refresh_state) and the small setters and getters.
// bann_ctx_destroy frees nothing itself: every file that allocates context buffers has a
// release function beside the allocation (ctx_internal.h), called here in a fixed order.
#include <stdio.h>

#include <algorithm>

#include "ctx_internal.h"

#define BANN_VERSION "rs-bann_amd 0.1.0 (gfx950, HIP)"

void refresh_state(bann_ctx* ctx) {
  clear_graphs(ctx);  // captured kernel arguments hold the old state
  DevState& s = ctx->st;
  s.br = ctx->d_br;
  s.xu2 = ctx->d_xu2;
  s.xi = ctx->d_xi;
  s.dig = ctx->d_dig;
  s.fc = ctx->d_fc;
  s.mu = ctx->d_mub;
  s.sigma = ctx->d_sigb;
  s.theta = ctx->d_theta;
  s.mom = ctx->d_mom;
  s.eps = ctx->d_eps;
  s.theta0 = ctx->d_theta0;
  s.lam = ctx->d_lam;
  s.lamld = ctx->d_lamld;
  s.grad = ctx->d_grad;
  s.part = ctx->d_part;
  s.rss_part = ctx->d_rss_part;
  s.y = ctx->d_y;
  s.pred = ctx->d_pred;
  s.pred0 = ctx->d_pred0;
  s.scr = ctx->d_scr;
  s.dbg = ctx->d_dbg;
  s.eprec = ctx->d_eprec;
  s.h0 = ctx->d_h0;
  s.htrace = ctx->d_htrace;
  s.ld_out = ctx->d_ld;
  s.rss_out = ctx->d_rss;
  s.status = ctx->d_status;
  s.uturn = ctx->d_uturn;
  s.uacc = ctx->d_u;
  s.n = ctx->n;
  s.nfrag = ctx->nfrag;
  s.max_splits = ctx->max_splits;
  s.lint = ctx->htrace_cap - 1;
  s.phi = ctx->d_phi;
  s.phi0 = ctx->d_phi0;
  s.mphi = ctx->d_mphi;
  s.ephi = ctx->d_ephi;
  s.gphi = ctx->d_gphi;
  s.pidx = ctx->d_pidx;
  s.ows = ctx->d_ows;
}

bool check_branch(const bann_ctx* ctx, int32_t b) {
  return ctx && ctx->finalized && b >= 0 && b < (int32_t)ctx->br.size();
}

// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
extern "C" const char* bann_version(void) { return BANN_VERSION; }

extern "C" int bann_ctx_create(int device, bann_ctx** out) {
  if (!out) return BANN_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BANN_E_HIP;
  if (device < 0 || device >= ndev) return BANN_E_ARG;
  bann_ctx* ctx = new bann_ctx();  // reads every BANN_* switch, once (bann_ctx::opt)
  ctx->device = device;
  ctx->graph_replay = ctx->opt.hmc_graph > 0;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return BANN_E_HIP;
  }
  *out = ctx;
  return BANN_OK;
}

extern "C" int bann_ctx_destroy(bann_ctx* ctx) {
  if (!ctx) return BANN_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  // every allocating file releases its own buffers (ctx_internal.h); the order is fixed: what launches
  // or holds events first, then the state the others point into
  hmc_release(ctx);
  models_release(ctx);
  dist_release(ctx);
  gibbs_release(ctx);
  init_release(ctx);
  residual_release(ctx);
  plan_release(ctx);
  branch_release(ctx);  // prints the BANN_STAMPS sums, if any, before it frees them
  genotypes_release(ctx);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return BANN_OK;
}

extern "C" const char* bann_last_error(const bann_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int bann_synchronize(bann_ctx* ctx) {
  if (!ctx) return BANN_E_ARG;
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_num_branches(const bann_ctx* ctx) { return ctx ? (int)ctx->br.size() : BANN_E_ARG; }
extern "C" int64_t bann_num_params(const bann_ctx* ctx, int32_t b) {
  if (!ctx || b < 0 || b >= (int32_t)ctx->br.size()) return BANN_E_ARG;
  return ctx->br[b].P;
}
extern "C" int64_t bann_num_precisions(const bann_ctx* ctx, int32_t b) {
  if (!ctx || b < 0 || b >= (int32_t)ctx->br.size()) return BANN_E_ARG;
  return ctx->br[b].nprec;
}
extern "C" int bann_branch_info(const bann_ctx* ctx, int32_t b, int32_t* m, int32_t* num_layers, int32_t* widths_out,
                                int32_t widths_cap, int32_t* activation, int32_t* prior) {
  if (!ctx || b < 0 || b >= (int32_t)ctx->br.size()) return BANN_E_ARG;
  const BranchHost& h = ctx->br[b];
  if (m) *m = h.m;
  if (num_layers) *num_layers = h.L;
  if (widths_out)
    for (int l = 0; l < h.L && l < widths_cap; ++l) widths_out[l] = h.widths[l];
  if (activation) *activation = h.act;
  if (prior) *prior = h.prior;
  return BANN_OK;
}
extern "C" int bann_branch_kernel_path(const bann_ctx* ctx, int32_t b) {
  if (!check_branch(ctx, b)) return BANN_E_ARG;
  return ctx->br[b].dev.fused;
}
extern "C" const char* bann_fused_kernel_name(void) { return "k_fused_grad_fx"; }

extern "C" int bann_set_hidden_gemm_bf16(bann_ctx* ctx, int32_t enabled) {
  if (!ctx) return BANN_E_ARG;
  ctx->wide_bf16 = enabled != 0;
  std::fill(ctx->pred_ok.begin(), ctx->pred_ok.end(), 0);  // wide-branch predictions change with the GEMM precision
  return BANN_OK;
}
extern "C" int bann_set_fused_enabled(bann_ctx* ctx, int32_t enabled) {
  if (!ctx) return BANN_E_ARG;
  if (ctx->finalized) return fail(ctx, BANN_E_STATE, "set before bann_finalize");
  ctx->fused_enabled = enabled != 0;
  return BANN_OK;
}
extern "C" int bann_set_graph_replay(bann_ctx* ctx, int32_t enabled) {
  if (!ctx) return BANN_E_ARG;
  ctx->graph_replay = enabled != 0;
  return BANN_OK;
}
extern "C" int bann_get_graph_replay(const bann_ctx* ctx) { return ctx ? (ctx->graph_replay ? 1 : 0) : BANN_E_ARG; }
extern "C" int64_t bann_packed_genotype_bytes(const bann_ctx* ctx) { return ctx ? ctx->packed_bytes : 0; }

extern "C" int64_t bann_ctx_num_individuals(const bann_ctx* ctx) { return ctx ? ctx->n : BANN_E_ARG; }
