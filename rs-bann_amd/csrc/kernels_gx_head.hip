// kernels_gx_head.hip — the two ends of a gx evaluation that are no GEMM: k_gx_prep (the weights as
// the GEMM kernels read them) before the first phase, and k_gx_head / k_gx_head_red (output neuron,
// error, rss, predictions) between the forward and the backward phases; the path and its phases are
// described in kernels_gx.hip.
#include "activations.h"
#include "bann_internal.h"
#include "bf16_planes.h"
#include "gx_tile.h"
#include "kernel_util.h"

#define GX_PREP_Y 16  // k_gx_prep workgroups per branch

// ---------------------------------------------------------------------------
// PREP: padded weights, W0 / sigma, c0 = b0 - mu^T (W0 / sigma) (f64), biases
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gx_prep(DevState st, const int32_t* __restrict__ blist) {
  // grid (branches, GX_PREP_Y): every element is independent (computed from theta),
  // so the y blocks of a branch split every loop below
  const int b = blist[blockIdx.x];
  const BranchDev& bd = st.br[b];
  float* S = gx_base(st, bd);
  const float* th = st.theta + bd.p_off;
  const float* mu = st.mu + bd.mk_off;
  const float* sg = st.sigma + bd.mk_off;
  const int64_t g0 = (int64_t)blockIdx.y * 256 + threadIdx.x, gs = (int64_t)gridDim.y * 256;
  auto wval = [&](int l, int k, int j) -> float {  // Wp_l[k][j]: W_l (layer 0: W0 / sigma), 0 past the in width
    if (j >= bd.win[l]) return 0.f;
    const float v = th[bd.woff[l] + (int64_t)k * bd.win[l] + j];
    return l == 0 ? (sg[j] > 0.f ? v / sg[j] : 0.f) : v;
  };
  for (int l = 0; l < bd.L; ++l) {  // padded weights [out][gx_wld[l]]
    const int ld = bd.gx_wld[l];
    float* Wp = S + bd.gx_w[l];
    const int64_t tot = (int64_t)bd.widths[l] * ld;
    for (int64_t e = g0; e < tot; e += gs) Wp[e] = wval(l, (int)(e / ld), (int)(e % ld));
  }
  {  // W0 / sigma as three bf16 planes [3][w0][64 nchunks], zero padded (k_gx_gemm_b3)
    const int m64 = 64 * bd.nchunks;
    __bf16* P3 = reinterpret_cast<__bf16*>(S + bd.gx_w0p);
    const int64_t tot = (int64_t)bd.widths[0] * m64;
    for (int64_t e = g0; e < tot; e += gs) {
      __bf16 hh, mm, ll;
      split3(wval(0, (int)(e / m64), (int)(e % m64)), hh, mm, ll);
      P3[e] = hh;
      P3[tot + e] = mm;
      P3[2 * tot + e] = ll;
    }
  }
  for (int l = 1; l < bd.L - 1; ++l) {  // Wp_l as three bf16 planes [3][w_l][r32(win_l)], zero padded (k_gx_gemm_x3)
    const int l3 = (bd.win[l] + 31) & ~31;
    __bf16* P3 = reinterpret_cast<__bf16*>(S + bd.gx_wp[l]);
    const int64_t tot = (int64_t)bd.widths[l] * l3;
    for (int64_t e = g0; e < tot; e += gs) {
      __bf16 hh, mm, ll;
      split3(wval(l, (int)(e / l3), (int)(e % l3)), hh, mm, ll);
      P3[e] = hh;
      P3[tot + e] = mm;
      P3[2 * tot + e] = ll;
    }
  }
  if (bd.L >= 3 && dh_from_a(bd.act)) {  // lazy head: w_out[k] Wp_s[k][j] as three planes (k_gx_gemm_x3 BWD_s)
    const int l = bd.L - 2, l3 = (bd.win[l] + 31) & ~31;
    const float* wo = th + bd.woff[bd.L - 1];
    __bf16* P3 = reinterpret_cast<__bf16*>(S + bd.gx_wps);
    const int64_t tot = (int64_t)bd.widths[l] * l3;
    for (int64_t e = g0; e < tot; e += gs) {
      const int k = (int)(e / l3);
      __bf16 hh, mm, ll;
      split3(wo[k] * wval(l, k, (int)(e % l3)), hh, mm, ll);
      P3[e] = hh;
      P3[tot + e] = mm;
      P3[2 * tot + e] = ll;
    }
  }
  // c0 = b0 - sum_j mu_j Wp_0[k][j] (f64): one wave per unit, lane-strided partials
  // added in a fixed order; the other biases
  {
    const int lane = threadIdx.x & 63;
    const int gw = (int)blockIdx.y * 4 + (threadIdx.x >> 6), nw = (int)gridDim.y * 4;
    for (int k = gw; k < bd.widths[0]; k += nw) {
      double acc = 0.0;
      for (int j = lane; j < bd.m; j += 64) acc += (double)mu[j] * (double)wval(0, k, j);
      acc = wave_sum_d(acc);
      if (lane == 0) S[bd.gx_b[0] + k] = (float)((double)th[bd.boff[0] + k] - acc);
    }
  }
  for (int l = 1; l < bd.L - 1; ++l)
    for (int64_t k = g0; k < bd.widths[l]; k += gs) S[bd.gx_b[l] + k] = th[bd.boff[l] + k];
}

// ---------------------------------------------------------------------------
// HEAD: output neuron, error, rss, predictions, dW_out, delta of the summary layer.
// grid (row tiles, branches): wave w takes rows w, w + 4, ... of the tile (lanes
// across the summary units, coalesced), then thread t takes units t, t + 256, ...
// over the tile's 64 rows.  dW_out and the rss leave per-tile f64 partials in the
// scratch; k_gx_head_red adds them per split in tile order (deterministic).
// ---------------------------------------------------------------------------
// Lazy head (fuse, the bf16-plane path, a summary layer after a hidden one and an
// activation whose h' is a function of A): the summary layer's FWD epilogue left
// the per-wave partials of out in gx_op, so the head only adds them (in slot order),
// forms e, pred and the rss, and writes e; BWD_s and GRAD_s form delta_s while
// staging and GRAD_s adds dW_out: A_s is not read here and delta_s never stored.
__device__ __forceinline__ bool gx_lazy_head(const BranchDev& bd, int fuse) {
  return fuse && bd.L >= 3 && dh_from_a(bd.act);
}
__global__ void __launch_bounds__(256) k_gx_head(DevState st, const int32_t* __restrict__ blist, int fuse) {
  __shared__ float e_s[GX_T];
  __shared__ double r_s[4];
  const int b = blist[blockIdx.y];
  const BranchDev& bd = st.br[b];
  const int tile = blockIdx.x;
  if (tile >= (st.nfrag + 3) / 4) return;
  float* S = gx_base(st, bd);
  const int sl = bd.L - 2, Sw = bd.widths[sl];
  if (gx_lazy_head(bd, fuse)) {
    const int t = threadIdx.x;
    if (t >= GX_T) return;
    const int64_t rows = gx_rows(st), row = 64 * (int64_t)tile + t;
    constexpr int TNF = 32 * X3Shape<GX_FWD>::AY;  // the summary layer's FWD tiles (k_gx_gemm_x3)
    const int ns = 2 * ((Sw + TNF - 1) / TNF);
    const float* op = S + bd.gx_op + row;
    double acc = 0.0;
    for (int k = 0; k < ns; ++k) acc += (double)op[k * rows];
    const float out = (float)acc;
    float e = 0.f;
    if (row < st.n) {
      e = out - st.y[bd.y_off + row];
      st.pred[bd.y_off + row] = out;
    }
    S[bd.gx_e + row] = e;
    const double rss = wave_sum_d((double)e * (double)e);
    if (t == 0) ((double*)(S + bd.gx_rss))[tile] = rss;
    return;
  }
  const float* A = S + bd.gx_a[sl];
  float* H = S + bd.gx_h[sl];
  const int64_t ld = bd.gx_ld[sl];
  const float* wout = S + bd.gx_w[bd.L - 1];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int64_t r0 = 64 * (int64_t)tile;
  double rss = 0.0;
  for (int i = wv; i < GX_T; i += 4) {
    const int64_t row = r0 + i;
    const float* a = A + row * ld;
    double acc = 0.0;
    for (int k = lane; k < Sw; k += 64) acc += (double)a[k] * (double)wout[k];
    const float out = (float)wave_sum_d(acc);  // out = A_s w_out (the output layer has no bias)
    float e = 0.f;
    if (row < st.n) {
      e = out - st.y[bd.y_off + row];
      if (lane == 0) st.pred[bd.y_off + row] = out;
      rss += (double)e * (double)e;  // lane-uniform: counted once below
    }
    if (lane == 0) e_s[i] = e;
  }
  if (lane == 0) r_s[wv] = rss;
  __syncthreads();
  double* dwo = (double*)(S + bd.gx_dwo) + (int64_t)tile * Sw;
  const int act = bd.act;
  const bool fa = dh_from_a(act);
  for (int k = t; k < Sw; k += 256) {
    const float wk = wout[k];
    double d = 0.0;
#pragma unroll 8
    for (int i = 0; i < GX_T; ++i) {
      const float ei = e_s[i];
      const int64_t o = (r0 + i) * ld + k;
      const float a_o = A[o];
      d += (double)a_o * (double)ei;
      const float h = fa ? act_dh_a(a_o, act) : H[o];
      H[o] = h * (ei * wk);  // delta_s = h'(z_s) * (e w_out^T)
    }
    dwo[k] = d;
  }
  if (t == 0) ((double*)(S + bd.gx_rss))[tile] = ((r_s[0] + r_s[1]) + r_s[2]) + r_s[3];
}

// grid (splits, branches): dW_out and rss of each split, tiles in order
__global__ void __launch_bounds__(256) k_gx_head_red(DevState st, const int32_t* __restrict__ blist, int fuse) {
  const int b = blist[blockIdx.y];
  const BranchDev& bd = st.br[b];
  const int split = blockIdx.x;
  if (split >= bd.nsplits) return;
  const int ntile = (st.nfrag + 3) / 4;
  const int t0 = (int)((int64_t)ntile * split / bd.nsplits), t1 = (int)((int64_t)ntile * (split + 1) / bd.nsplits);
  const float* S = gx_base(st, bd);
  const int Sw = bd.widths[bd.L - 2];
  const double* dwo = (const double*)(S + bd.gx_dwo);
  float* part = st.part + bd.part_off + (int64_t)split * bd.P + bd.woff[bd.L - 1];
  for (int k = threadIdx.x; k < Sw && !gx_lazy_head(bd, fuse); k += 256) {  // lazy: GRAD_s writes dW_out
    double d = 0.0;
    for (int tl = t0; tl < t1; ++tl) d += dwo[(int64_t)tl * Sw + k];
    part[k] = (float)d;
  }
  if (threadIdx.x == 0) {
    const double* rs = (const double*)(S + bd.gx_rss);
    double r = 0.0;
    for (int tl = t0; tl < t1; ++tl) r += rs[tl];
    st.rss_part[(int64_t)b * st.max_splits + split] = r;
  }
}

void launch_gx_prep(const DevState& st, const int32_t* blist, int nb, hipStream_t s) {
  if (nb > 0) hipLaunchKernelGGL(k_gx_prep, dim3(nb, GX_PREP_Y), dim3(256), 0, s, st, blist);
}
void launch_gx_head(const DevState& st, const int32_t* blist, int nb, int max_splits, bool exact, hipStream_t s) {
  if (nb <= 0) return;
  const int fuse = exact ? 0 : 1;  // the lazy head pairs with the bf16-plane BWD / GRAD (k_gx_gemm_x3)
  hipLaunchKernelGGL(k_gx_head, dim3((st.nfrag + 3) / 4, nb), dim3(256), 0, s, st, blist, fuse);
  hipLaunchKernelGGL(k_gx_head_red, dim3(max_splits, nb), dim3(256), 0, s, st, blist, fuse);
}
