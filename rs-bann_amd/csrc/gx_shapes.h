// gx_shapes.h — the tile shapes and the tile numbering of the gx GEMM phases (kernels_gx.hip,
// kernels_gx_b3.hip), for the kernels and for the host's plan (build_plan counts the
// tiles of a launch with gx_tiles).  No HIP call: a host-only program can include it.
#pragma once
#include "bann_internal.h"

// tile shape of k_gx_gemm_x3 per phase: wave tiles of 16 AX x 16 AY, 2 x 2 waves.
// FWD takes 64 x 128 tiles: its A block (activations, split into planes while
// staging) feeds twice the MFMAs of a 64 x 64 tile, 3 workgroups per CU (c3def
// FWD1: 2.78 -> 2.50 ms per 40-branch group).  Measured and not kept: 128 x 128
// (2 per CU: FWD 2.59, BWD 3.16 -> 3.59 ms), BWD at 64 x 128 (3.17: flat).
// gx_tiles and the head's slot count follow these.
template <int PH>
struct X3Shape {
  static constexpr int AX = 2, AY = PH == GX_BWD ? 2 : 4;
};

// the tile numbering of a phase for one branch: tmc x tnc tiles of TM x TN (64 x 64, the hidden
// phases of k_gx_gemm_x3 32 AX x 32 AY; the masked layer's are 64 x 64 always) in each of ns row splits
__host__ __device__ __forceinline__ void gx_dims(int32_t nfrag, const BranchDev& bd, int ph, int l, int& tmc, int& tnc,
                                                 int& ns, int TM = 64, int TN = 64) {
  const int ntile = (nfrag + 3) / 4;
  const int rt = (ntile * 64 + TM - 1) / TM;
  ns = 1;
  if (ph == GX_FWD0) {
    tmc = ntile;
    tnc = (bd.widths[0] + 63) / 64;
  } else if (ph == GX_FWD) {
    tmc = rt;
    tnc = (bd.widths[l] + TN - 1) / TN;
  } else if (ph == GX_BWD) {
    tmc = rt;
    tnc = (bd.widths[l - 1] + TN - 1) / TN;
  } else if (ph == GX_GRAD) {
    tmc = (bd.widths[l - 1] + TM - 1) / TM;
    tnc = (bd.widths[l] + TN - 1) / TN;
    ns = bd.nsplits;
  } else {  // GX_GRAD0
    tmc = bd.nchunks;
    tnc = (bd.widths[0] + 63) / 64;
    ns = bd.nsplits;
  }
}

// tiles of phase (ph, l) for one branch.  exact (EnvOptions::gx_exact): 64 x 64 tiles (k_gx_gemm), else
// k_gx_gemm_x3's; FWD / BWD / GRAD exist for the hidden and summary layers 1 <= l < L - 1 only
inline int64_t gx_tiles(const BranchDev& d, int ph, int l, int32_t nfrag, bool exact) {
  int TM = 64, TN = 64;
  if (ph == GX_FWD || ph == GX_BWD || ph == GX_GRAD) {
    if (l < 1 || l >= d.L - 1) return 0;
    if (!exact) {
      TM = 32 * (ph == GX_FWD ? X3Shape<GX_FWD>::AX : ph == GX_BWD ? X3Shape<GX_BWD>::AX : X3Shape<GX_GRAD>::AX);
      TN = 32 * (ph == GX_FWD ? X3Shape<GX_FWD>::AY : ph == GX_BWD ? X3Shape<GX_BWD>::AY : X3Shape<GX_GRAD>::AY);
    }
  }
  int tmc, tnc, ns;
  gx_dims(nfrag, d, ph, l, tmc, tnc, ns, TM, TN);
  return (int64_t)tmc * tnc * ns;
}
