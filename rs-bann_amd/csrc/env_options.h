// env_options.h — the BANN_* environment switches of the library, read once per context
// (bann_ctx_create) and fixed for its life.  Host-only: no HIP includes.  The one read outside
// read_env_options() is bann_net.cpp's GraphReplayScope, which sees the context only through the C ABI.
#pragma once
#include <stdint.h>
#include <stdlib.h>

struct EnvOptions {
  bool wx_exact = false;     // BANN_WX_EXACT=1: wx hidden GEMMs on the exact-f32 MFMA (k_fused_grad_wx)
  bool gx_exact = false;     // BANN_GX_EXACT=1: every gx phase on the exact-f32 MFMA path, eager head
  bool net_err = true;       // BANN_NET_ERR=0: per-branch targets for every kernel kind (diagnostics)
  bool net_gsum = true;      // BANN_NET_GSUM=0: per-branch output rows in every network step (A/B)
  int32_t net_gsum_r = 0;    // BANN_NET_GSUM_R: forces build_net_groups' R (tests), 1..32 (above: no group rows); 0: its own choice
  bool fwd_fi = false;       // BANN_FWD_FI=1: individual-major fi images and forward for the fx branches
  int32_t fi_waves_per_simd = 3;  // BANN_FI_WAVES_PER_SIMD: the fi forward's grid
  bool fxl_head = true;      // BANN_FXL_HEAD=0: fxl groups of 17..32 chunks off the head-wave kernel
  int32_t fxl_cpw = 0;       // BANN_FXL_CPW=8: 8 chunks per fxl wave at every size, the old scheme (A/B)
  // BANN_FUSE_UPDATE=1: the update in the gradient launch's tail (same bits either way):
  // one-split plans (the branch's one workgroup), one-round multi-split plans and solo
  // plans (the last arriving workgroup; solo: it folds the branch's slabs first).  Off
  // by default: measured slower everywhere (r4c: C3 747.7 vs 752.9 steps/s, N = 8 shard
  // 4 269 vs 4 531, sequential driver 6.5 vs 21.9 -- one workgroup adding 49 slabs)
  bool fuse_update = false;
  bool solo = true;          // BANN_SOLO=0: never re-split a small plan (unset: on)
  int32_t solo_tpw = 1;      // BANN_SOLO_TPW: tiles per wave of a solo plan, >= 1
  int64_t target_items = 1024;  // BANN_TARGET_ITEMS: ~work items of a fused launch, >= 1
  int64_t min_frags = 64;       // BANN_MIN_FRAGS: fragments per work item at least, >= 1
  bool env_split = false;    // either of the two is set: fx takes their split, not best_splits'
  int64_t gx_scratch_mb = 0;  // BANN_GX_SCRATCH_MB: gx scratch group budget, >= 1; 0 (unset): from the free memory
  bool stamps = false;       // BANN_STAMPS set (to anything): the phase-stamp buffer of an FX_STAMPS build
  int32_t hmc_graph = -1;    // BANN_HMC_GRAPH: 1 / 0 graph replay of bann_hmc_step on / off; -1 (unset): off here,
                             // on inside bann_net_train
};

inline EnvOptions read_env_options() {
  EnvOptions o;
  auto flag = [](const char* name, bool& v) {
    if (const char* e = getenv(name)) v = atoi(e) != 0;
  };
  flag("BANN_WX_EXACT", o.wx_exact);
  flag("BANN_GX_EXACT", o.gx_exact);
  flag("BANN_NET_ERR", o.net_err);
  flag("BANN_NET_GSUM", o.net_gsum);
  flag("BANN_FWD_FI", o.fwd_fi);
  flag("BANN_FXL_HEAD", o.fxl_head);
  flag("BANN_FUSE_UPDATE", o.fuse_update);
  flag("BANN_SOLO", o.solo);
  auto at_least_1 = [](long long v) { return v > 1 ? v : 1; };
  if (const char* e = getenv("BANN_NET_GSUM_R")) o.net_gsum_r = (int32_t)at_least_1(atoi(e));
  if (const char* e = getenv("BANN_FI_WAVES_PER_SIMD")) o.fi_waves_per_simd = atoi(e);
  if (const char* e = getenv("BANN_FXL_CPW")) o.fxl_cpw = atoi(e);
  if (const char* e = getenv("BANN_SOLO_TPW")) o.solo_tpw = (int32_t)at_least_1(atoi(e));
  if (const char* e = getenv("BANN_TARGET_ITEMS")) o.target_items = at_least_1(atoll(e)), o.env_split = true;
  if (const char* e = getenv("BANN_MIN_FRAGS")) o.min_frags = at_least_1(atoll(e)), o.env_split = true;
  if (const char* e = getenv("BANN_GX_SCRATCH_MB")) o.gx_scratch_mb = at_least_1(atoll(e));
  o.stamps = getenv("BANN_STAMPS") != nullptr;
  if (const char* e = getenv("BANN_HMC_GRAPH")) o.hmc_graph = atoi(e) != 0 ? 1 : 0;
  return o;
}
