// prec_expand.h — what bann_branch_set_precisions derives from a precision vector, on the
// device: the per-parameter prior multipliers lam / lamld and the Izmailov step bases
// (expand_precisions and step_bases of bann_branch.hip).  Shared by the Gibbs draw
// (kernels_gibbs.hip) and the model initialisation (kernels_init.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/bann.h"
#include "bann_internal.h"

// pq: the branch's precision vector (precision_vec order); pidx: DevState::pidx.  Every thread
// of the workgroup calls it (t of nthreads); the caller has made pq visible to the workgroup.
// Ridge weights and every bias: pi / (2 sqrt(lam)); lasso weights: 1 / (4 lam); std-normal
// branches: multipliers 1 (lamld also on the biases, std_normal_branch.rs:149-158) and the
// negated base, which the step-size factor does not scale.
__device__ inline void expand_branch_precisions(const BranchDev& d, const float* __restrict__ pq,
                                                const int32_t* __restrict__ pidx, float* __restrict__ lam,
                                                float* __restrict__ lamld, double* __restrict__ sbase, int t,
                                                int nthreads) {
  const bool lasso = d.prior == BANN_LASSO_ARD || d.prior == BANN_LASSO_BASE;
  const bool stdn = d.prior == BANN_STD_NORMAL;
  const double PI = 3.14159265358979323846;
  const int nweights = d.boff[0];
  for (int p = t; p < d.P; p += nthreads) {
    const float v = pq[pidx[d.p_off + p]];
    const bool weight = p < nweights;  // the biases carry no prior term in the density (branch_sampler.rs:106-112)
    lam[d.p_off + p] = weight ? (stdn ? 1.f : v) : 0.f;
    lamld[d.p_off + p] = stdn ? 1.f : (weight ? v : 0.f);
    const double lv = (double)v;
    const double e = (lasso && weight) ? 1.0 / (4.0 * lv) : PI / (2.0 * sqrt(lv));
    sbase[d.p_off + p] = stdn ? -e : e;
  }
}
