// finalize_layout.h — what bann_finalize decides before it touches the device: the kernel
// path of every branch, the split counts, every per-branch offset and the gx scratch
// groups; and build_net_groups' (R, k) chooser.  Pure integer arithmetic.  Host-only: no HIP
// call, no bann_ctx.  Checked by tests/finalize_layout_check.cpp.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/bann.h"
#include "bann_internal.h"
#include "env_options.h"
#include "fx_shapes.h"

struct BranchHost {
  std::vector<int32_t> snp_idx;
  std::vector<int32_t> widths;
  int32_t m = 0, L = 0, act = 0, prior = 0;
  int32_t P = 0, nprec = 0;
  std::vector<float> prec;  // precision_vec order
  float ows_reg_sum = 0.f;  // output-weight summary stat of the OTHER branches (joint HMC)
  float ows_num = -1.f;     // output-weight count of the network (< 0: this branch's own)
  int32_t gx_group = -1;    // gx path: scratch group (branches of one group share no scratch)
  int32_t solo_items = 1;   // fused path: work items of the branch in a solo-mode plan (~1 tile per wave)
  BranchDev dev{};
};

// a branch as bann_branch_add registers it (its arguments already checked): the shape, the
// param_vec offsets and the precision count; plan_layout fills the rest of dev
inline BranchHost make_branch(const int32_t* snp_idx, int32_t m, const int32_t* layer_widths, int32_t num_layers,
                              int32_t activation, int32_t prior) {
  BranchHost h;
  h.snp_idx.assign(snp_idx, snp_idx + m);
  h.widths.assign(layer_widths, layer_widths + num_layers);
  h.m = m;
  h.L = num_layers;
  h.act = activation;
  h.prior = prior;
  BranchDev& d = h.dev;
  d.m = m;
  d.L = num_layers;
  d.act = activation;
  d.prior = prior;
  int off = 0;
  for (int l = 0; l < num_layers; ++l) {
    d.widths[l] = h.widths[l];
    d.win[l] = l == 0 ? m : h.widths[l - 1];
    d.woff[l] = off;
    off += d.win[l] * d.widths[l];
  }
  for (int l = 0; l < num_layers - 1; ++l) {
    d.boff[l] = off;
    off += d.widths[l];
  }
  d.P = h.P = off;
  const bool ard = (prior == BANN_RIDGE_ARD || prior == BANN_LASSO_ARD);
  int np = 0;
  for (int l = 0; l < num_layers; ++l) np += (ard && l < num_layers - 1) ? d.win[l] : 1;
  h.nprec = np + (num_layers - 1) + 1;
  h.prec.assign(h.nprec, 1.f);
  return h;
}

// kernel path of a branch: fx (widths <= 4, <= 8 chunks), fxl (widths <= 4,
// 9..64 chunks), wx (one hidden layer up to 32 x 32, m <= 128), else gx (layered MFMA GEMMs)
inline int32_t classify_path(bool fused_enabled, int32_t L, const int32_t* widths, int32_t m) {
  const int32_t nchunks = (m + BANN_CHUNK - 1) / BANN_CHUNK;
  bool narrow = fused_enabled && L >= 2 && L <= 4;
  for (int l = 0; l < L; ++l) narrow = narrow && widths[l] <= BANN_FUSED_MAXW;
  if (narrow && nchunks <= BANN_FX_MAXCH) return PATH_FX;
  if (narrow && nchunks <= BANN_FXL_MAXCH) return PATH_FXL;
  if (fused_enabled && L == 3 && nchunks <= BANN_WIDE_MAXCH && widths[0] <= BANN_WIDE_MAXW &&
      widths[1] <= BANN_WIDE_MAXW)
    return PATH_WX;
  return PATH_GX;
}

// Splits: whole rounds of resident workgroups.  All items of a packed launch
// are equally long, so a launch costs ceil(items / slots) rounds of (per-item
// prologue/epilogue + tiles per wave); choose the split count minimising that
// (e.g. 125 fx branches on one GPU of an 8-GPU shard: 4 splits = 500 items in
// one round, where a 1024-item target gave 9 splits = 1125 items in 3 partly
// empty rounds).  Lower bound: <= BANN_MAX_TILES_PER_WAVE tiles per wave, so
// the int32 dW0 digit sums cannot overflow.
inline int32_t best_splits(int64_t ntile, int64_t nbr, int64_t slots, int64_t tiles_per_split_wave_div) {
  const int64_t min_sp = (ntile + tiles_per_split_wave_div * BANN_MAX_TILES_PER_WAVE - 1) /
                         (tiles_per_split_wave_div * BANN_MAX_TILES_PER_WAVE);
  int32_t best_sp = (int32_t)std::max<int64_t>(1, min_sp);
  double best = -1.0;
  for (int64_t sp = std::max<int64_t>(1, min_sp); nbr > 0 && sp <= std::max<int64_t>(64, min_sp); ++sp) {
    if (sp > min_sp && tiles_per_split_wave_div * sp > ntile) break;
    const int64_t rounds = (nbr * sp + slots - 1) / slots;
    const int64_t per_wave = (ntile + tiles_per_split_wave_div * sp - 1) / (tiles_per_split_wave_div * sp);
    const double cost = (double)rounds * (2.0 + (double)per_wave);  // ~2 tiles of prologue + epilogue
    if (best < 0.0 || cost < best) best = cost, best_sp = (int32_t)sp;
  }
  return best_sp;
}

// the split count of every fused path of one context; fxl by (chunks per wave 4?, waves)
struct SplitCounts {
  int32_t fx = 1, wx = 1, fxl[2][9] = {};
  int64_t frags_per_item = 1;  // wx (and fx under env_split) before best_splits replaces it
};
inline void fxl_key(int nch, int force_cpw, int& c4, int& nw) {
  const int cpw = fxl_cpw(nch, force_cpw);
  c4 = cpw == 4;
  nw = (nch + cpw - 1) / cpw;
}
inline SplitCounts choose_splits(const std::vector<BranchHost>& br, int32_t nfrag, int64_t ntile, int32_t cus,
                                 const EnvOptions& opt) {
  SplitCounts sc;
  int64_t total_frags = 0, nfx = 0, nwx = 0, nfxl[2][9] = {};
  for (const auto& h : br) {
    if (h.dev.fused != PATH_GX) total_frags += nfrag;
    nfx += h.dev.fused == PATH_FX;
    nwx += h.dev.fused == PATH_WX;
    if (h.dev.fused == PATH_FXL) {
      int c4, nw;
      fxl_key(h.dev.nchunks, opt.fxl_cpw, c4, nw);
      ++nfxl[c4][nw];
    }
  }
  // wx (and fx with BANN_TARGET_ITEMS / BANN_MIN_FRAGS): ~target_items work items (default 1024) of at
  // least min_frags fragments (default 64: >= 16 tiles per work item amortises the per-item prologue/epilogue)
  sc.frags_per_item = std::max<int64_t>(opt.min_frags, (total_frags + opt.target_items - 1) / opt.target_items);
  sc.fx = best_splits(ntile, nfx, 2 * (int64_t)cus, 4);  // fx: 2 workgroups of 4 waves per CU, tiles interleaved
  // wx: 4 two-wave workgroups per CU, a tile at a time (exact f32 MFMA); wx3: 2
  // four-wave workgroups per CU, two tiles at a time
  sc.wx = opt.wx_exact ? best_splits(ntile, nwx, 4 * (int64_t)cus, 1) : best_splits(ntile, nwx, 2 * (int64_t)cus, 2);
  for (int c4 = 0; c4 < 2; ++c4)
    for (int nw = 1; nw <= 8; ++nw) {  // fxl: all waves of a workgroup on one tile; LDS- and VGPR-limited residency
      const int64_t per_cu =
          std::max<int64_t>(1, std::min<int64_t>(163840 / fxl_lds_bytes(nw, 4, c4 ? 4 : 8), 8 / nw));
      sc.fxl[c4][nw] = best_splits(ntile, nfxl[c4][nw], per_cu * cus, 1);
    }
  return sc;
}
inline int32_t branch_splits(const BranchDev& d, const SplitCounts& sc, int32_t nfrag, int64_t ntile,
                             const EnvOptions& opt) {
  // gx: row splits of ~64 tiles (4096 individuals) for the K = n gradient GEMMs
  int32_t ns = d.fused != PATH_GX ? (int32_t)std::max<int64_t>(1, (nfrag + sc.frags_per_item - 1) / sc.frags_per_item)
                                  : (int32_t)((ntile + 63) / 64);
  if (d.fused == PATH_FX && !opt.env_split) ns = sc.fx;
  if (d.fused == PATH_FXL) {
    int c4, nw;
    fxl_key(d.nchunks, opt.fxl_cpw, c4, nw);
    ns = sc.fxl[c4][nw];
  }
  if (d.fused == PATH_WX) ns = sc.wx;
  if (d.fused == PATH_FX)  // overflow guard also under the env overrides
    ns = std::max<int32_t>(ns, (int32_t)((ntile + 4 * BANN_MAX_TILES_PER_WAVE - 1) / (4 * BANN_MAX_TILES_PER_WAVE)));
  return (int32_t)std::max<int64_t>(1, std::min<int64_t>(ns, ntile));
}

// precision coordinates in precision_vec order (params.rs:272-289)
inline void layout_precisions(BranchHost& h) {
  BranchDev& d = h.dev;
  const bool ard = (h.prior == BANN_RIDGE_ARD || h.prior == BANN_LASSO_ARD);
  int qo = 0;
  for (int l = 0; l < h.L; ++l) {
    d.qoff[l] = qo;
    qo += (ard && l < h.L - 1) ? d.win[l] : 1;
  }
  d.qbias = qo;
  d.nq = qo + (h.L - 1) + 1;
}

// gx scratch of one branch (kernels_gx.hip): padded weights, biases, A_l and H_l per layer,
// as int32 float offsets from its scr_off.  Returns its floats, or -1 and the message
inline int64_t layout_gx_scratch(BranchDev& d, int64_t ntile, const char*& msg) {
  const int L = d.L;
  const int64_t gx_rows = ntile * 64;
  if (d.widths[L - 2] > GX_HEAD_MAXW) {
    msg = "summary layer wider than 4096";
    return -1;
  }
  auto r4 = [](int64_t v) { return (v + 3) & ~3ll; };
  int64_t o = 0;
  for (int l = 0; l < L; ++l) {
    d.gx_wld[l] = (int32_t)r4(d.win[l]);
    d.gx_w[l] = (int32_t)o;
    o += (int64_t)d.widths[l] * d.gx_wld[l];
  }
  for (int l = 0; l < L - 1; ++l) {
    d.gx_b[l] = (int32_t)o;
    o += r4(d.widths[l]);
  }
  d.gx_w0p = (int32_t)o;  // 3 x w0 x 64 nchunks bf16
  o += r4((3ll * d.widths[0] * 64 * d.nchunks + 1) / 2);
  for (int l = 1; l < L - 1; ++l) {  // 3 x w_l x r32(win_l) bf16
    d.gx_wp[l] = (int32_t)o;
    o += r4((3ll * d.widths[l] * ((d.win[l] + 31) & ~31) + 1) / 2);
  }
  d.gx_dwo = (int32_t)o;
  o += 2 * ntile * r4(d.widths[L - 2]);
  d.gx_rss = (int32_t)o;
  o += r4(2 * ntile);
  d.gx_op = (int32_t)o;
  o += 2 * ((d.widths[L - 2] + 63) / 64) * gx_rows;
  d.gx_e = (int32_t)o;
  o += gx_rows;
  d.gx_wps = (int32_t)o;
  if (L >= 3) o += r4((3ll * d.widths[L - 2] * ((d.win[L - 2] + 31) & ~31) + 1) / 2);
  for (int l = 0; l < L - 1; ++l) {
    d.gx_ld[l] = (int32_t)r4(d.widths[l]);
    d.gx_a[l] = (int32_t)o;
    o += gx_rows * d.gx_ld[l];
    d.gx_h[l] = (int32_t)o;
    o += gx_rows * d.gx_ld[l];
    if (o >= (1ll << 31)) {
      msg = "gx scratch of one branch exceeds 2^31 floats";
      return -1;
    }
  }
  return o;
}

// plan_layout's totals: what bann_finalize allocates by
struct LayoutTotals {
  int err = BANN_OK;          // a shape failure, with its message; the other fields are then unset
  const char* msg = nullptr;
  int32_t nfrag = 0, max_splits = 1;
  int64_t tile_bytes = 0, fi_bytes = 0, dig_bytes = 0;  // the tile, fi and digit images
  int64_t total_p = 0, total_q = 0, total_markers = 0;
  int64_t part_total = 0, scr_floats = 0;  // partial slabs; one gx scratch group's worth
  int64_t fused_items = 0;                 // work items of a plan of every fused branch
  int64_t n_gx = 0;
  int32_t gx_ngroups = 0;  // index of the last scratch group
  int32_t solo_threshold = 0;
  int64_t solo_rss_cap = 0, solo_part_cap = 0;
  int64_t gxpre_cap = 0, items_cap = 0;
  int64_t plan_off_fold = 0, plan_off_items = 0, plan_scr_bytes = 0;  // a per-call plan's stage
};

// the layout of a context of n individuals and M markers on a device of cus compute units;
// gx_budget: floats of one gx scratch group.  Fills every BranchDev field that
// make_branch left open, BranchHost::gx_group and BranchHost::solo_items
inline LayoutTotals plan_layout(int64_t n, int64_t M, int32_t cus, int64_t gx_budget, bool fused_enabled,
                                const EnvOptions& opt, std::vector<BranchHost>& br) {
  LayoutTotals t;
  auto fail = [&t](const char* msg) {
    t.err = BANN_E_SHAPE;
    t.msg = msg;
    return t;
  };
  t.nfrag = (int32_t)((n + 15) / 16);
  const int64_t ntile = (t.nfrag + BANN_TILE_FRAGS - 1) / BANN_TILE_FRAGS;
  for (auto& h : br) {
    for (int i = 0; i < h.m; ++i)
      if (h.snp_idx[i] >= M) return fail("marker index out of range");
    h.dev.nchunks = (h.m + BANN_CHUNK - 1) / BANN_CHUNK;
    h.dev.fused = classify_path(fused_enabled, h.L, h.widths.data(), h.m);
  }
  const SplitCounts sc = choose_splits(br, t.nfrag, ntile, cus, opt);
  // gx scratch groups: branches in index order until the budget (BANN_GX_SCRATCH_MB,
  // default a quarter of the free device memory, at most 64 GiB) is full; every
  // group reuses the same device scratch.  Fewer, larger groups fill the GPU better
  // (c3def: 8 GiB = 40 branches per group 335 ms per evaluation, 32 GiB 321 ms)
  int64_t gx_cur = 0, max_p_fused = 0;
  for (size_t b = 0; b < br.size(); ++b) {
    BranchHost& h = br[b];
    BranchDev& d = h.dev;
    d.x_off = t.tile_bytes;  // byte offset of the branch's 2-bit tile image: [tile][chunk][1 KiB]
    t.tile_bytes += ntile * d.nchunks * 1024;
    // fx branches with BANN_FWD_FI=1: the individual-major image of the forward-only pass
    // (kernels_fi.hip), [frag][segment][1 KiB].  By default the LDS forward (k_forward_fx):
    // inside the network trajectory, interleaved with the gradient launches, it measured faster
    // (2.573 vs 2.660 ms per step, r4c/r4d), and it needs no second 2-bit image
    d.xi_off = -1;
    if (d.fused == PATH_FX && opt.fwd_fi) {
      d.xi_off = t.fi_bytes;
      t.fi_bytes += 4 * ntile * ((d.nchunks + 3) / 4) * 1024;
    }
    d.dig_off = t.dig_bytes;
    if (d.fused != PATH_GX) t.dig_bytes += (int64_t)d.nchunks * 1024 * (d.fused == PATH_WX ? 8 : 1);
    d.p_off = t.total_p;
    t.total_p += h.P;
    layout_precisions(h);
    d.q_off = t.total_q;
    t.total_q += d.nq;
    d.mk_off = t.total_markers;
    t.total_markers += h.m;
    d.y_off = (int64_t)b * n;
    d.nsplits = branch_splits(d, sc, t.nfrag, ntile, opt);
    t.max_splits = std::max(t.max_splits, d.nsplits);
    d.part_off = t.part_total;
    t.part_total += (int64_t)d.nsplits * h.P;
    if (d.fused != PATH_GX) {
      t.fused_items += d.nsplits;
      max_p_fused = std::max<int64_t>(max_p_fused, h.P);
      // solo mode (build_plan): ~one tile per wave for a branch alone on the GPU (BANN_SOLO_TPW: more
      // tiles per wave, fewer slabs to fold).  fx: 4 waves on their own tiles, solo_tpw tiles each;
      // fxl / wx: a tile at a time
      const int64_t per_item = d.fused == PATH_FX ? 4 * (int64_t)opt.solo_tpw : 1;
      h.solo_items =
          (int32_t)std::max<int64_t>(d.nsplits, std::min<int64_t>(2 * cus, (ntile + per_item - 1) / per_item));
      continue;
    }
    const int64_t o = layout_gx_scratch(d, ntile, t.msg);
    if (o < 0) return fail(t.msg);
    if (gx_cur > 0 && gx_cur + o > gx_budget) {  // a new scratch group
      ++t.gx_ngroups;
      gx_cur = 0;
    }
    h.gx_group = t.gx_ngroups;
    d.scr_off = gx_cur;
    gx_cur += o;
    t.scr_floats = std::max(t.scr_floats, gx_cur);
    ++t.n_gx;
  }
  t.solo_threshold = opt.solo ? cus : 0;  // BANN_SOLO=0: never re-split
  t.solo_rss_cap = 8ll * cus;
  t.solo_part_cap = t.solo_rss_cap * max_p_fused;
  t.gxpre_cap = (int64_t)(3 * BANN_MAXL) * (t.n_gx + t.gx_ngroups + 2);
  t.items_cap = t.fused_items + t.solo_rss_cap;  // a solo plan has <= solo_rss_cap items
  // a per-call plan's branch lists, fold jobs and work items: one device block, filled by
  // ONE copy from a pinned stage (build_plan; was three copies per bann_hmc_step call)
  auto al = [](int64_t v) { return (v + 255) & ~(int64_t)255; };
  const int64_t nb = (int64_t)br.size();
  t.plan_off_fold = al(2 * nb * (int64_t)sizeof(int32_t));
  t.plan_off_items = t.plan_off_fold + al(nb * (int64_t)sizeof(FoldJob));
  t.plan_scr_bytes = t.plan_off_items + t.items_cap * (int64_t)sizeof(GradItem);
  return t;
}

// build_net_groups' (R, k): an item takes up to 8 R branches over one of k tile ranges of
// T = ceil(ntile / k) <= tmax tiles; (R, k) minimise rounds (one workgroup per slot) x R x (T + 2),
// ties going to the larger R (fewer rows), then the larger k.  force_r > 0: that R only.
// found = false: no candidate -- no k <= 512 keeps T within tmax (ntile > 512 tmax), or force_r is
// beyond the largest R, 32
struct GsumChoice {
  int64_t R = 1, k = 1;
  bool found = false;
};
inline GsumChoice choose_gsum(int64_t ntile, int64_t nb, int64_t slots, int64_t tmax, int force_r) {
  GsumChoice c;
  int64_t best = -1;
  for (int64_t R = 1; R <= 32; ++R) {
    if (force_r && R != force_r) continue;
    const int64_t ng = (nb + 8 * R - 1) / (8 * R);
    for (int64_t k = (ntile + tmax - 1) / tmax; k <= std::min<int64_t>(ntile, 512); ++k) {
      const int64_t T = (ntile + k - 1) / k;
      const int64_t cost = ((ng * k + slots - 1) / slots) * R * (T + 2);
      if (best < 0 || cost <= best) best = cost, c.R = R, c.k = k, c.found = true;
    }
  }
  return c;
}
