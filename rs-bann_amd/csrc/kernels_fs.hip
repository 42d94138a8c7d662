// kernels_fs.hip — branch statistics of the fx-shaped branches for SEVERAL parameter sets
// at once: per (model slot, branch) the rss of the branch output against one target
// vector (rs-bann branch-r2, net.rs:648-656) and the column sums of the effect-size
// chain's first-layer deltas, from which the population effect sizes follow (rs-bann
// population-effect-sizes, net.rs:529-543).  The pass up to the branch output (stream,
// chunk walk, head, bits and registers) is fe_stream.h's, shared with k_forward_fe; no
// row leaves the kernel.  This kernel's own part:
//
// Per model and tile, one individual per lane, after the head:
//   rss      e = out - y_i, e^2
//   effect   err[k] = out W_out[k]; for l = L-2 .. 1: delta[k] = h'(Z_l[k]) err[k],
//            err'[j] = sum_k delta[k] W_l(j, k) (k ascending, fmaf from 0, k_effect_back);
//            delta0[k] = h'(Z_0[k]) err[k]   (branch_sampler.rs:784-811)
// with rows >= n of the ragged last tile masked to zero.  Each lane adds its five
// values (e^2, delta0[0..3]) into f64 registers; at the item's end the lanes are
// combined by a fixed butterfly, the waves in wave order, and one record
// [model][item][5] is written.  k_stats_fold adds a branch's records in item order
// and forms pop_j = sum_k W0(j, k) s_k / n in f64 (k ascending; W0 the raw parameter:
// the derivative is with respect to the standardised genotype, as k_effect_pop).
// No floating-point atomics: same inputs and plan, same bits; a model's numbers do not
// depend on the other models of its pass.
//
// The target.  y comes in as ONE MORE COUNTED PIECE of a tile: a global_load_lds_dword
// issued with the tile's chunk pieces into 256 bytes beside the wave's slot
// (individual 64 t + lane, clamped to n - 1), as k_fused_grad_fx brings in its target.
// A tile is then nch + 1 vector-memory instructions (nch without y), the only ones of
// the tile loop, and the counted wait at a tile's top leaves exactly the next tile's
// in flight.
//
// Registers.  BANN_FS_KM models per pass (bann_internal.h); the resource numbers of
// every instantiation and the variant not kept: DESIGN.md 4.8.
#include <stdlib.h>

#include "fe_stream.h"

#define FS_NV 5  // rss, s_0 .. s_3

// the head of one model's tile (fe_head), then the effect-size chain on its kept layers down to delta0
template <int NL, int ACT>
__device__ __forceinline__ float fs_head(v4i (&facc)[4], float zk, const float (*hw)[20], float (&d0)[4]) {
  constexpr int NH = NL - 1;
  float z[NH][4], a[NH][4];
  const float out = fe_head<NL, ACT>(facc, zk, hw, z, a);
  float err[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) err[k] = out * hw[NL - 1][4 * k];
#pragma unroll
  for (int l = NH - 1; l >= 1; --l) {
    float dl[4], en[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dl[k] = act_dh_t<ACT>(z[l][k], a[l][k]) * err[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) s = fmaf(dl[k], hw[l][4 * j + k], s);
      en[j] = s;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) err[j] = en[j];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) d0[k] = act_dh_t<ACT>(z[0][k], a[0][k]) * err[k];
  return out;
}

// One instantiation per (layers, activation) serves every chunk count <= 8 (wave-uniform
// per-chunk guards, as k_forward_fe).  part: the pass's records, model j's at
// part + j model_stride, item i's five doubles at 5 i.  y = null: no rss (record entry 0)
template <int NL, int ACT>
__global__ void __launch_bounds__(64 * FE_WAVES, 2)
    k_stats_fe(DevState st, FsModels mm, const GradItem* __restrict__ items, const float* __restrict__ y,
               double* __restrict__ part, int64_t model_stride) {
  constexpr int KM = BANN_FS_KM, NW = FE_WAVES, NS = FE_NS;
  __shared__ __attribute__((aligned(16))) char s_x[NW][NS][FE_SLOT];
  __shared__ __attribute__((aligned(16))) float s_y[NW][NS][64];  // the tile's targets, individual 64 t + index
  __shared__ __attribute__((aligned(16))) float s_hw[KM][NL][20];
  __shared__ __attribute__((aligned(16))) v4i s_rs[KM][64];
  __shared__ double s_red[NW][KM][FS_NV];

  const GradItem it = items[blockIdx.x];
  const int b = it.branch;
  const BranchDev& bd = st.br[b];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nch = bd.nchunks;
  const int nk = mm.nk;
  const int64_t n = st.n;
  const bool has_y = y != nullptr;
  const int tb = it.frag_begin >> 2, te = (it.frag_end + 3) >> 2;

  // per model: head parameters and 64 x the digit row sums -> LDS, W0 digit operands and the lane's column
  // scale -> registers.  The same text as k_forward_fe (kernels_fe.hip): why not a function, fe_stream.h
  v4i A[KM][8];
  float zk[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    if (threadIdx.x < NL * 20) {
      const int l = threadIdx.x / 20, r = threadIdx.x - l * 20;
      const float* th = mm.theta[k] + bd.p_off;
      float v = 0.f;
      if (r < 16) {
        const int j = r >> 2, kk = r & 3;
        if (l >= 1 && (l < NL - 1 || kk == 0) && j < bd.win[l] && kk < bd.widths[l]) v = th[bd.woff[l] + kk * bd.win[l] + j];
      } else {
        const int kk = r - 16;
        if (l == 0 && kk < bd.widths[0]) v = mm.fc[k][b].c0[kk];
        if (l >= 1 && l < NL - 1 && kk < bd.widths[l]) v = th[bd.boff[l] + kk];
      }
      s_hw[k][l][r] = v;
    }
    zk[k] = fx_zk(mm.fc[k][b].scale[lane >> 4]);
    v4i rowsum64 = v4i{0, 0, 0, 0};
    const uint8_t* dg = mm.dig[k] + bd.dig_off + lane * 16;
#pragma unroll
    for (int c = 0; c < 8; ++c) A[k][c] = fe_digit_operand(dg, c, nch);
#pragma unroll
    for (int c = 0; c < 8; ++c) rowsum64 = rowsum64_acc(A[k][c], rowsum64);
    if (wave == 0) s_rs[k][lane] = rowsum64;  // the same in every wave
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // the head parameters are in LDS before any LDS-DMA is in flight

  // lane geometry, the same text as k_forward_fe (kernels_fe.hip)
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 1, tp = lane & 1;
  const int gsw = g & 1;
  const uint32_t fo0 = (uint32_t)((16 * g + tq + 8 * gsw) * 16 + 8 * (tp ^ gsw));
  const uint32_t fo1 = (uint32_t)((16 * g + tq + 8 * (1 ^ gsw)) * 16 + 8 * (tp ^ 1 ^ gsw));
  const int iota = 4 * i16 + g;
  const char* xsrc = reinterpret_cast<const char*>(st.xu2) + bd.x_off;
  const uint32_t xlane = (uint32_t)lane * 16u;
  const int64_t tile_bytes = (int64_t)nch * 1024;
  // the last chunk's padding rows are not streamed (as in k_forward_fx): their digit operands are zero
  const bool pad_row = 64 * (nch - 1) + 16 * (lane >> 4) + (((lane & 15) - 8 * ((lane >> 4) & 1)) & 15) >= bd.m;
  const int pieces = nch + (has_y ? 1 : 0);  // vector-memory instructions per tile
  auto issue_tile = [&](int tt, int sl) {  // the same loop as k_forward_fe's (kernels_fe.hip); why not a function: fe_stream.h
    for (int c = 0; c < nch; ++c) {
      if (c == nch - 1 && pad_row) continue;
      glds16_s(xsrc + (int64_t)tt * tile_bytes + c * 1024, xlane, &s_x[wave][sl][c * 1024]);
    }
    if (has_y) {  // every lane loads (the row clamped into [0, n)): one instruction per wave and tile
      const int64_t row = 64 * (int64_t)tt + lane;
      glds4(y + (row < n ? row : n - 1), &s_y[wave][sl][0]);
    }
  };

  double acc[KM][FS_NV];
#pragma unroll
  for (int k = 0; k < KM; ++k)
#pragma unroll
    for (int c = 0; c < FS_NV; ++c) acc[k][c] = 0.0;

  int tt = tb + wave, sl = 0;
  for (int j = 0; j < NS; ++j)
    if (tt + j * NW < te) issue_tile(tt + j * NW, j);
  for (; tt < te; tt += NW, sl ^= 1) {
    // younger than this tile's pieces: the next tile's, nothing else (no stores, no other loads)
    vm_wait<9>(tt + NW < te ? pieces : 0);
    const float yv = has_y ? s_y[wave][sl][iota] : 0.f;  // read before the refill
    const bool live = 64 * (int64_t)tt + iota < n;  // rows past n contribute to no sum
    // the chunk walk, the same text as k_forward_fe (kernels_fe.hip): the chunk's fragments once, then every model's
    // MFMAs against them; the next chunk's LDS read is in flight meanwhile
    const char* xs = &s_x[wave][sl][0];
    v4i facc[KM][4];
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      facc[k][0] = facc[k][1] = facc[k][2] = v4i{0, 0, 0, 0};
      facc[k][3] = s_rs[k][lane];
    }
    v4u Xn = (v4u)lds_tr8_pair(xs + fo0, xs + fo1);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c >= nch) break;
      const v4u X = Xn;
      if (c + 1 < 8 && c + 1 < nch) Xn = (v4u)lds_tr8_pair(xs + (c + 1) * 1024 + fo0, xs + (c + 1) * 1024 + fo1);
      const v4i f0 = (v4i)(X & 0x03030303u), f1 = (v4i)(X & 0x0F0F0F0Fu), f2 = (v4i)(X & 0x3F3F3F3Fu), f3 = (v4i)X;
#pragma unroll
      for (int k = 0; k < KM; ++k) {
        if (k < nk) fe_mfma4(A[k][c], f0, f1, f2, f3, facc[k]);  // wave-uniform
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every read of this slot has returned: refill it
    if (tt + NS * NW < te) issue_tile(tt + NS * NW, sl);
#pragma unroll
    for (int k = 0; k < KM; ++k) {
      if (k < nk) {
        float d0[4];
        const float out = fs_head<NL, ACT>(facc[k], zk[k], s_hw[k], d0);
        const float e = out - yv;
        acc[k][0] += (double)(live && has_y ? e * e : 0.f);
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[k][1 + c] += (double)(live ? d0[c] : 0.f);
      }
      asm volatile("" ::: "memory");  // one model's head parameters at a time
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // lanes by a fixed butterfly, waves in wave order, one record per model
#pragma unroll
  for (int k = 0; k < KM; ++k)
#pragma unroll
    for (int c = 0; c < FS_NV; ++c) {
      const double v = wave_sum_d(acc[k][c]);
      if (lane == 0) s_red[wave][k][c] = v;
    }
  __syncthreads();
  if ((int)threadIdx.x < nk * FS_NV) {
    const int k = threadIdx.x / FS_NV, c = threadIdx.x - k * FS_NV;
    double v = s_red[0][k][c];
#pragma unroll
    for (int w = 1; w < NW; ++w) v += s_red[w][k][c];
    part[(int64_t)k * model_stride + (int64_t)blockIdx.x * FS_NV + c] = v;
  }
}

// items: one fx launch group
void launch_stats_fe(const DevState& st, const FsModels& mm, const GradItem* items, int32_t nitems, int32_t L,
                     int32_t act, const float* y, double* part, int64_t model_stride, hipStream_t s) {
  if (nitems <= 0 || mm.nk <= 0) return;
  FsModels mf = mm;
  mf.fill_unused();
  fe_dispatch(L, act, [&](auto nl, auto a) {
    hipLaunchKernelGGL((k_stats_fe<decltype(nl)::value, decltype(a)::value>), dim3((unsigned)nitems),
                       dim3(64 * FE_WAVES), 0, s, st, mf, items, y, part, model_stride);
  });
}

// ---------------------------------------------------------------------------
// One workgroup per (fold job, model): the branch's records added in item order, then
// rss and pop_j = sum_k W0(j, k) s_k / n (f64, k ascending, rounded to f32 once)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_stats_fold(DevState st, const float* __restrict__ theta0, int64_t theta_stride,
                                                    const FsFoldJob* __restrict__ jobs,
                                                    const double* __restrict__ part, int64_t model_stride,
                                                    double* __restrict__ rss, int32_t rss_stride,
                                                    float* __restrict__ pop, int64_t pop_stride) {
  const FsFoldJob jb = jobs[blockIdx.x];
  const int k = blockIdx.y;
  const BranchDev& bd = st.br[jb.branch];
  __shared__ double s[FS_NV];
  if (threadIdx.x < FS_NV) {
    const double* p = part + (int64_t)k * model_stride + (int64_t)jb.item_begin * FS_NV + threadIdx.x;
    double v = 0.0;
    for (int i = 0; i < jb.item_count; ++i) v += p[(int64_t)i * FS_NV];
    s[threadIdx.x] = v;
  }
  __syncthreads();
  if (rss && threadIdx.x == 0) rss[(int64_t)k * rss_stride + jb.list_ix] = s[0];
  if (!pop) return;
  const float* W = theta0 + (int64_t)k * theta_stride + bd.p_off + bd.woff[0];
  const int m = bd.m, w0 = bd.widths[0];
  for (int j = threadIdx.x; j < m; j += 256) {
    double v = 0.0;
    for (int kk = 0; kk < w0; ++kk) v += (double)W[(int64_t)kk * m + j] * s[1 + kk];
    pop[(int64_t)k * pop_stride + jb.pop_off + j] = (float)(v / (double)st.n);
  }
}

void launch_stats_fold(const DevState& st, const float* theta0, int64_t theta_stride, int32_t nk,
                       const FsFoldJob* jobs, int32_t njobs, const double* part, int64_t model_stride, double* rss,
                       int32_t rss_stride, float* pop, int64_t pop_stride, hipStream_t s) {
  if (njobs <= 0 || nk <= 0 || (!rss && !pop)) return;
  hipLaunchKernelGGL(k_stats_fold, dim3((unsigned)njobs, (unsigned)nk), dim3(256), 0, s, st, theta0, theta_stride, jobs,
                     part, model_stride, rss, rss_stride, pop, pop_stride);
}

// rss of one prediction row against y (the branches of the other kernel paths): one
// workgroup, strided f64 partials and a fixed tree
__global__ void __launch_bounds__(256) k_row_rss(const float* __restrict__ row, const float* __restrict__ y, int64_t n,
                                                 double* __restrict__ out) {
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const float e = row[i] - y[i];
    v += (double)(e * e);
  }
  __shared__ double red[256];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = red[0];
}

void launch_row_rss(const float* row, const float* y, int64_t n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_row_rss, dim3(1), dim3(256), 0, s, row, y, n, out);
}
