// bann_plan.hip — launch plans: a branch list turned into packed launch groups (build_plan),
// the context's scratch for per-call plans, and the launches every caller composes from a
// plan: gradient (run_grad), forward (run_forward), leapfrog update (run_update).
#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx_internal.h"
#include "gx_shapes.h"

// a per-call plan's scratch (bann_finalize): the gx branch list and tile prefix arrays, and
// the branch lists, fold jobs and work items in one device block, filled by ONE copy from a
// pinned stage (upload_plan_scratch; was three copies per bann_hmc_step call)
int plan_scratch_alloc(bann_ctx* ctx, const LayoutTotals& t) {
  CK(dalloc(&ctx->d_gen_scr, (int64_t)ctx->br.size()));
  CK(dalloc(&ctx->d_gxpre_scr, t.gxpre_cap));
  CK(hipMalloc((void**)&ctx->d_plan_scr, (size_t)t.plan_scr_bytes));
  CK(hipHostMalloc((void**)&ctx->h_plan_stage, (size_t)t.plan_scr_bytes, hipHostMallocDefault));
  CK(hipEventCreateWithFlags(&ctx->ev_plan, hipEventDisableTiming));
  ctx->d_list_scr = reinterpret_cast<int32_t*>(ctx->d_plan_scr);
  ctx->d_fold_scr = reinterpret_cast<FoldJob*>(ctx->d_plan_scr + t.plan_off_fold);
  ctx->d_items_scr = reinterpret_cast<GradItem*>(ctx->d_plan_scr + t.plan_off_items);
  return BANN_OK;
}

void plan_release(bann_ctx* ctx) {
  if (ctx->plan_ev_pending && ctx->ev_plan) (void)hipEventSynchronize(ctx->ev_plan);  // the copy has read the stage
  ctx->plan_ev_pending = false;
  dfree_all(ctx->d_gen_scr, ctx->d_gxpre_scr, ctx->d_plan_scr);
  if (ctx->h_plan_stage) (void)hipHostFree(ctx->h_plan_stage);
  if (ctx->ev_plan) (void)hipEventDestroy(ctx->ev_plan);
  ctx->h_plan_stage = nullptr;
  ctx->d_list_scr = nullptr;  // the three views into d_plan_scr
  ctx->d_fold_scr = nullptr;
  ctx->d_items_scr = nullptr;
  ctx->ev_plan = nullptr;
}

void free_plan(Plan& p) {
  if (p.owns) {
    dfree(p.d_all);
    dfree(p.d_gx);
    dfree(p.d_gxpre);
    dfree(p.d_fold);
    for (auto& g : p.groups) {
      dfree(g.d_items);
      dfree(g.d_nitems);
      dfree(g.d_nlist);
    }
  }
  p = Plan{};
}

// ---------------------------------------------------------------------------
// plans: build_plan = validation, three parts (fused groups, gx groups, branch lists), one upload
// ---------------------------------------------------------------------------
// the kernel instantiation that serves a fused branch, as the key of its launch group
static LaunchGroup group_key(const bann_ctx* ctx, const BranchHost& h) {
  const BranchDev& d = h.dev;
  LaunchGroup key;
  key.kind = d.fused;
  key.act = h.act;
  if (d.fused == PATH_FX) {  // fx: (L, act, exactly 8 chunks)
    key.L = h.L;
    key.full = d.nchunks == 8;
  } else if (d.fused == PATH_FXL) {  // fxl: (L, act, chunks per wave, waves, every wave full)
    key.L = h.L;
    key.cpw = fxl_cpw(d.nchunks, ctx->opt.fxl_cpw);
    key.nw = (d.nchunks + key.cpw - 1) / key.cpw;
    key.head = ctx->opt.fxl_head ? 1 : 0;
    key.full = d.nchunks == key.cpw * key.nw;
  } else if (d.fused == PATH_WX) {  // wx: (act, marker chunks: the plane kernel is compiled per chunk count)
    key.nw = d.nchunks;
  }
  return key;
}

// solo mode: too few work items to fill the GPU -> every fused branch re-split
// into its solo_items items, partials into the solo region, folded afterwards
static bool plan_goes_solo(const bann_ctx* ctx, const Plan& p) {
  int64_t items = 0, need = 0, need_rss = 0;
  for (int32_t b : p.all) {
    const BranchHost& h = ctx->br[b];
    if (h.dev.fused == PATH_GX) continue;
    items += h.dev.nsplits;
    need += (int64_t)h.solo_items * h.P;
    need_rss += h.solo_items;
  }
  return items > 0 && items < ctx->solo_threshold && need <= ctx->solo_part_cap && need_rss <= ctx->solo_rss_cap;
}

// the fused update (kernels_fx.hip tail): fx branches only, the small update, one round of items
static bool plan_fuses_update(const bann_ctx* ctx, const Plan& p, bool solo) {
  int64_t items = 0;
  bool ok = p.gx.empty() && ctx->d_upd_cnt != nullptr && ctx->opt.fuse_update;
  bool single = true;  // every branch one split: its one workgroup updates it
  for (const auto& g : p.groups) {
    ok = ok && g.kind == PATH_FX;
    items += (int64_t)g.items.size();
  }
  for (size_t i = 0; i < p.all.size() && ok; ++i) {
    const BranchHost& h = ctx->br[p.all[i]];
    ok = h.P <= 2048 && h.m <= 512 && !update_is_large(h.dev);
    single = single && h.dev.nsplits == 1;
  }
  // solo plans: the last arriving workgroup folds the branch's slabs, then updates it
  return ok && items > 0 && (solo || single || items <= 2ll * ctx->cus);
}

// part 1: the fused branches of p.all into launch groups of work items (with the solo and
// fuse-update decisions), the others into p.gx
static void plan_fused_groups(const bann_ctx* ctx, Plan& p) {
  const int32_t nbr = (int32_t)ctx->br.size();
  const int64_t nfrag = ctx->nfrag, ntile = (nfrag + BANN_TILE_FRAGS - 1) / BANN_TILE_FRAGS;
  const bool solo = plan_goes_solo(ctx, p);
  int64_t solo_part = ctx->part_total, solo_rss = (int64_t)nbr * ctx->max_splits;
  for (int32_t b : p.all) {
    const BranchHost& h = ctx->br[b];
    const BranchDev& d = h.dev;
    p.max_p = std::max(p.max_p, h.P);
    if (d.fused == PATH_GX) {
      p.gx.push_back(b);
      continue;
    }
    const LaunchGroup key = group_key(ctx, h);
    LaunchGroup* grp = nullptr;
    for (auto& g : p.groups)
      if (g.kind == key.kind && g.L == key.L && g.act == key.act && g.nw == key.nw && g.full == key.full &&
          g.cpw == key.cpw)
        grp = &g;
    if (!grp) {
      p.groups.push_back(key);
      grp = &p.groups.back();
    }
    const int spi = 1;  // partial slabs per work item
    const int ns = solo ? h.solo_items : d.nsplits;
    if (grp->items.empty()) grp->fi = true;
    if (d.fused == PATH_FX) {
      grp->fi = grp->fi && d.xi_off >= 0;
      grp->max_seg = std::max(grp->max_seg, (d.nchunks + 3) / 4);
    }
    for (int s = 0; s < ns; ++s) {  // splits on tile (4-fragment) boundaries
      GradItem it{};
      it.branch = b;
      it.split = s;
      it.frag_begin = (int32_t)(BANN_TILE_FRAGS * (ntile * s / ns));
      it.frag_end = (int32_t)std::min<int64_t>(nfrag, BANN_TILE_FRAGS * (ntile * (s + 1) / ns));
      it.tile0 = (int32_t)grp->tiles;
      grp->tiles += ((it.frag_end + 3) >> 2) - (it.frag_begin >> 2);
      it.part_at = solo ? solo_part + (int64_t)s * spi * h.P : d.part_off + (int64_t)s * spi * h.P;
      it.rss_at = solo ? solo_rss + (int64_t)s * spi : (int64_t)b * ctx->max_splits + (int64_t)s * spi;
      it.fold_ix = solo ? (int32_t)p.fold.size() : -1;  // this branch's job, pushed below
      grp->items.push_back(it);
    }
    if (solo) {
      p.fold.push_back(FoldJob{b, ns * spi, solo_part, solo_rss});
      solo_part += (int64_t)ns * spi * h.P;
      solo_rss += (int64_t)ns * spi;
    }
  }
  p.fuse_update = plan_fuses_update(ctx, p, solo);
}

// part 2: the gx branches grouped by scratch group, one tile prefix array per GEMM phase
static int plan_gx_groups(bann_ctx* ctx, Plan& p) {
  std::stable_sort(p.gx.begin(), p.gx.end(),
                   [&](int32_t a, int32_t b) { return ctx->br[a].gx_group < ctx->br[b].gx_group; });
  for (size_t i = 0; i < p.gx.size();) {
    size_t j = i;
    GxGroup g;
    int32_t maxL = 2;
    while (j < p.gx.size() && ctx->br[p.gx[j]].gx_group == ctx->br[p.gx[i]].gx_group) {
      maxL = std::max(maxL, ctx->br[p.gx[j]].L);
      g.max_splits = std::max(g.max_splits, ctx->br[p.gx[j]].dev.nsplits);
      ++j;
    }
    g.first = (int32_t)i;
    g.count = (int32_t)(j - i);
    std::vector<std::pair<int, int>> order;  // (phase, layer) in launch order
    order.push_back({GX_FWD0, 0});
    for (int l = 1; l < maxL - 1; ++l) order.push_back({GX_FWD, l});
    order.push_back({GX_HEAD, 0});
    for (int l = maxL - 2; l >= 1; --l) order.push_back({GX_BWD, l});
    for (int l = maxL - 2; l >= 1; --l) order.push_back({GX_GRAD, l});
    order.push_back({GX_GRAD0, 0});
    for (auto& o : order) {
      GxPhase ph;
      ph.ph = o.first;
      ph.l = o.second;
      if (ph.ph != GX_HEAD) {
        ph.pre_off = (int32_t)p.gx_pre.size();
        int64_t tot = 0;
        p.gx_pre.push_back(0);
        for (size_t k = i; k < j; ++k) {
          tot += gx_tiles(ctx->br[p.gx[k]].dev, ph.ph, ph.l, ctx->nfrag, ctx->opt.gx_exact);
          if (tot >= (1ll << 30)) return fail(ctx, BANN_E_SHAPE, "gx phase has too many tiles for one launch");
          p.gx_pre.push_back((int32_t)tot);
        }
        ph.total = (int32_t)tot;
        if (tot == 0) continue;
      }
      g.phases.push_back(ph);
    }
    p.gxg.push_back(std::move(g));
    i = j;
  }
  return BANN_OK;
}

// part 3: the device branch lists: p.all, then the update kernels' small and large branches
static std::vector<int32_t> plan_branch_lists(const bann_ctx* ctx, Plan& p) {
  const int32_t nb = (int32_t)p.all.size();
  std::vector<int32_t> lists(p.all);
  for (int32_t b : p.all)
    if (!update_is_large(ctx->br[b].dev)) lists.push_back(b);
  p.n_small = (int32_t)lists.size() - nb;
  for (int32_t b : p.all)
    if (update_is_large(ctx->br[b].dev)) lists.push_back(b);
  p.n_large = nb - p.n_small;
  return lists;
}

// a persistent plan owns its device arrays
static int upload_plan_persistent(bann_ctx* ctx, Plan& p, const std::vector<int32_t>& lists) {
  const int32_t nb = (int32_t)p.all.size();
  p.owns = true;
  CK(dalloc(&p.d_all, 2 * nb));
  CK(dalloc(&p.d_gx, (int64_t)p.gx.size()));
  CK(dalloc(&p.d_gxpre, (int64_t)p.gx_pre.size()));
  CK(dalloc(&p.d_fold, (int64_t)p.fold.size()));
  if (!p.fold.empty())
    CK(hipMemcpyAsync(p.d_fold, p.fold.data(), p.fold.size() * sizeof(FoldJob), hipMemcpyHostToDevice, ctx->stream));
  CK(hipMemcpyAsync(p.d_all, lists.data(), 2 * nb * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  if (!p.gx.empty()) {
    CK(hipMemcpyAsync(p.d_gx, p.gx.data(), p.gx.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(p.d_gxpre, p.gx_pre.data(), p.gx_pre.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                      ctx->stream));
  }
  for (auto& g : p.groups) {
    CK(dalloc(&g.d_items, (int64_t)g.items.size()));
    CK(hipMemcpyAsync(g.d_items, g.items.data(), g.items.size() * sizeof(GradItem), hipMemcpyHostToDevice,
                      ctx->stream));
  }
  return BANN_OK;
}

// a per-call plan lives in the context's plan scratch: lists, fold jobs and work items through
// the pinned stage in one copy (offsets: plan_layout)
static int upload_plan_scratch(bann_ctx* ctx, Plan& p, const std::vector<int32_t>& lists) {
  const int32_t nb = (int32_t)p.all.size();
  p.owns = false;
  p.d_all = ctx->d_list_scr;
  p.d_gx = ctx->d_gen_scr;
  p.d_gxpre = ctx->d_gxpre_scr;
  p.d_fold = ctx->d_fold_scr;
  if ((int64_t)p.gx_pre.size() > ctx->gxpre_cap) return fail(ctx, BANN_E_STATE, "gx plan scratch overflow");
  if (ctx->plan_ev_pending) CK(hipEventSynchronize(ctx->ev_plan));  // the last plan's copy has read the stage
  char* hs = ctx->h_plan_stage;
  std::memcpy(hs, lists.data(), 2 * nb * sizeof(int32_t));
  int64_t end = 2 * (int64_t)nb * (int64_t)sizeof(int32_t);
  if (!p.fold.empty()) {
    std::memcpy(hs + ctx->plan_off_fold, p.fold.data(), p.fold.size() * sizeof(FoldJob));
    end = ctx->plan_off_fold + (int64_t)(p.fold.size() * sizeof(FoldJob));
  }
  if (!p.gx.empty()) {
    CK(hipMemcpyAsync(p.d_gx, p.gx.data(), p.gx.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    CK(hipMemcpyAsync(p.d_gxpre, p.gx_pre.data(), p.gx_pre.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                      ctx->stream));
  }
  int64_t off = 0;
  for (auto& g : p.groups) {
    if (off + (int64_t)g.items.size() > ctx->items_cap) return fail(ctx, BANN_E_STATE, "work-item scratch overflow");
    g.d_items = ctx->d_items_scr + off;
    std::memcpy(hs + ctx->plan_off_items + off * (int64_t)sizeof(GradItem), g.items.data(),
                g.items.size() * sizeof(GradItem));
    off += (int64_t)g.items.size();
  }
  if (off > 0) end = ctx->plan_off_items + off * (int64_t)sizeof(GradItem);
  CK(hipMemcpyAsync(ctx->d_plan_scr, hs, (size_t)end, hipMemcpyHostToDevice, ctx->stream));
  CK(hipEventRecord(ctx->ev_plan, ctx->stream));
  ctx->plan_ev_pending = true;
  return BANN_OK;
}

int build_plan(bann_ctx* ctx, const int32_t* branches, int32_t nb, Plan& p, bool persistent) {
  free_plan(p);
  const int32_t nbr = (int32_t)ctx->br.size();
  if (nb > nbr) return fail(ctx, BANN_E_ARG, "branch list longer than the branch set");
  std::vector<char> seen(nbr, 0);
  for (int i = 0; i < nb; ++i) {
    const int b = branches[i];
    if (b < 0 || b >= nbr) return fail(ctx, BANN_E_SHAPE, "branch index out of range");
    if (seen[b]) return fail(ctx, BANN_E_ARG, "duplicate branch in list");
    seen[b] = 1;
  }
  p.all.assign(branches, branches + nb);
  plan_fused_groups(ctx, p);
  const int rc = plan_gx_groups(ctx, p);
  if (rc) return rc;
  const std::vector<int32_t> lists = plan_branch_lists(ctx, p);
  return persistent ? upload_plan_persistent(ctx, p, lists) : upload_plan_scratch(ctx, p, lists);
}

// launch_fused_grad_wx's mode: bf16 MFMA when opted in, else the exact-f32 MFMA (BANN_WX_EXACT=1) or the
// f32-accurate bf16 planes; plan_layout sized the wx splits for the same choice
static int wx_mode(const bann_ctx* ctx) { return ctx->wide_bf16 ? 1 : (ctx->opt.wx_exact ? 0 : 2); }

// the gradient launch of one fused group; upd_mode, upd_step, cnt, fo: fx's fused update (run_grad)
void launch_group_grad(const bann_ctx* ctx, const DevState& s, const LaunchGroup& g, int wp, int upd_mode,
                       int upd_step, int32_t* cnt, const FoldJob* fo) {
  const int32_t ni = (int32_t)g.items.size();
  if (g.kind == PATH_WX)
    launch_fused_grad_wx(s, g.d_items, ni, g.act, wx_mode(ctx), g.nw, wp, ctx->stream);
  else if (g.kind == PATH_FXL)
    launch_fused_grad_fxl(s, g.d_items, ni, g.L, g.act, g.nw, g.cpw, g.full, wp, g.head, ctx->stream);
  else
    launch_fused_grad_fx(s, g.d_items, ni, g.L, g.act, g.full, wp, upd_mode, upd_step, cnt, fo, ctx->stream);
}

// gx branches: scratch group by scratch group (the groups reuse one scratch), every phase of
// the group, or up to the head only: it writes the predictions, the backward is not needed
void launch_gx_phases(const bann_ctx* ctx, const DevState& s, const Plan& p, bool head_only) {
  for (const auto& g : p.gxg) {
    const int32_t* bl = p.d_gx + g.first;
    launch_gx_prep(s, bl, g.count, ctx->stream);
    for (const auto& ph : g.phases) {
      if (ph.ph == GX_HEAD) {
        launch_gx_head(s, bl, g.count, g.max_splits, ctx->opt.gx_exact, ctx->stream);
        if (head_only) break;
      } else {
        launch_gx_gemm(s, ph.ph, ph.l, bl, p.d_gxpre + ph.pre_off, g.count, ph.total, ctx->opt.gx_exact, ctx->stream);
      }
    }
  }
}

// gradient (partials) of every branch in the plan at the current theta.
// write_pred: 0 = no predictions (the layered path writes them anyway), 1 = the
// predictions f_b(theta) into pred, 2 = into pred0 (a trajectory's start: the
// restore copy and the residual change read them there)
// upd_mode >= 0 (a plan with fuse_update): the leapfrog update of that mode and
// step runs in the fx launch's tail -- the caller launches no update (traj_run, UPD_FUSED)
int run_grad(bann_ctx* ctx, const Plan& p, int write_pred, int upd_mode, int upd_step) {
  DevState s = ctx->st;
  if (write_pred == 2) s.pred = ctx->d_pred0;
  const int wp = write_pred != 0;
  int32_t* cnt = upd_mode >= 0 ? ctx->d_upd_cnt : nullptr;
  // a fused solo plan folds in the gradient launch's tail (kernels_fx.hip), not in k_fold_solo
  const FoldJob* fo = (cnt && !p.fold.empty()) ? p.d_fold : nullptr;
  for (const auto& g : p.groups) launch_group_grad(ctx, s, g, wp, upd_mode, upd_step, cnt, fo);
  if (!p.fold.empty() && !fo) launch_fold_solo(s, p.d_fold, (int32_t)p.fold.size(), p.max_p, ctx->stream);
  launch_gx_phases(ctx, s, p, false);
  CK(hipGetLastError());
  if (write_pred == 1) mark_predictions(ctx, p, true);
  return BANN_OK;
}

// predictions f_b(theta) of every branch in the plan: fx groups through the
// forward-only kernel (no target, no backward), every other path through its
// gradient launch with predictions (their partial slabs are scratch here)
int run_forward(bann_ctx* ctx, const Plan& p) {
  const DevState& s = ctx->st;
  for (const auto& g : p.groups) {
    const int32_t ni = (int32_t)g.items.size();
    if (g.kind != PATH_FX)
      launch_group_grad(ctx, s, g, 1, -1, 0, nullptr, nullptr);
    else if (g.fi)
      launch_forward_fi(s, g.d_items, ni, g.tiles, g.L, g.act, g.max_seg, ctx->cus, ctx->opt.fi_waves_per_simd,
                        ctx->stream);
    else
      launch_forward_fx(s, g.d_items, ni, g.L, g.act, g.full, ctx->stream);
  }
  launch_gx_phases(ctx, s, p, true);
  CK(hipGetLastError());
  mark_predictions(ctx, p, true);
  return BANN_OK;
}

void mark_predictions(bann_ctx* ctx, const Plan& p, bool current) {
  for (int32_t b : p.all) ctx->pred_ok[b] = current;
}

// the fused leapfrog update of every branch in the plan (small and large kernels)
void run_update(bann_ctx* ctx, const Plan& p, int32_t mode, int32_t step) {
  const int32_t nb = (int32_t)p.all.size();
  if (mode != MODE_GRAD && mode != MODE_PROFILE) mark_predictions(ctx, p, false);  // theta moves
  launch_update(ctx->st, p.d_all + nb, p.n_small, mode, step, ctx->stream, 0);
  launch_update(ctx->st, p.d_all + nb + p.n_small, p.n_large, mode, step, ctx->stream, 1);
}

