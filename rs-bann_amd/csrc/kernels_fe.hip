// kernels_fe.hip — forward rows of the fx-shaped branches for SEVERAL parameter sets at
// once: the model slots of a context (bann_models_*), up to BANN_FE_KM models per
// genotype pass.  The pass (stream, chunk walk, head, bits and registers) is
// fe_stream.h's; this kernel's own part is the rows.
//
// Rows.  Each model stores its own row.  A tile's prediction stores are issued at the
// top of the NEXT tile, in front of that tile's refill: the counted wait on a tile
// then never waits for a store younger than one tile.  Resource numbers and the
// measured A/B: DESIGN.md 4.7.
#include <stdlib.h>

#include "fe_stream.h"

// This kernel's counted wait: vm_wait<8> (kernel_util.h) plus a case that no call reaches.  The
// switch has carried `case -1` (-> vmcnt(9)) since the wait was shared with k_stats_fe, whose ninth
// case it stood in for.  The compiler builds its compare tree from the case set, so dropping the case
// reorders the tree in the tile loop (about 50 instruction lines per instantiation,
// profiles/fx_split_refactor.md): a change of this kernel's instructions, to be measured on its own.
__device__ __forceinline__ void fe_vm_wait8(int k) {
  if (k == -1)
    asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
  else
    vm_wait<8>(k);
}

// One instantiation per (layers, activation) serves every chunk count <= 8: the per-chunk guards are
// wave-uniform scalar branches (an 8-chunk specialisation without them let the scheduler lengthen the
// fragments' live ranges into spills of the digit operands)
template <int NL, int ACT>
__global__ void __launch_bounds__(64 * FE_WAVES, 2)
    k_forward_fe(DevState st, FeModels mm, const GradItem* __restrict__ items) {
  constexpr int KM = BANN_FE_KM, NW = FE_WAVES, NS = FE_NS;
  __shared__ __attribute__((aligned(16))) char s_x[NW][NS][FE_SLOT];
  __shared__ __attribute__((aligned(16))) float s_hw[KM][NL][20];
  __shared__ __attribute__((aligned(16))) v4i s_rs[KM][64];

  const GradItem it = items[blockIdx.x];
  const int b = it.branch;
  const BranchDev& bd = st.br[b];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nch = bd.nchunks;
  const int nk = mm.nk;
  const int64_t n = st.n;
  const int tb = it.frag_begin >> 2, te = (it.frag_end + 3) >> 2;

  // per model: head parameters and 64 x the digit row sums -> LDS, W0 digit operands and the lane's column
  // scale -> registers.  The same text as k_stats_fe (kernels_fs.hip): why not a function, fe_stream.h
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

  // lane geometry, the same text as k_stats_fe (kernels_fs.hip)
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
  auto issue_tile = [&](int tt, int sl) {  // the same loop as k_stats_fe's (kernels_fs.hip); why not a function: fe_stream.h
    for (int c = 0; c < nch; ++c) {
      if (c == nch - 1 && pad_row) continue;
      glds16_s(xsrc + (int64_t)tt * tile_bytes + c * 1024, xlane, &s_x[wave][sl][c * 1024]);
    }
  };

  int tt = tb + wave, sl = 0;
  for (int j = 0; j < NS; ++j)
    if (tt + j * NW < te) issue_tile(tt + j * NW, j);
  float obuf[KM];  // the previous tile's outputs, stored at the top of the next tile
#pragma unroll
  for (int k = 0; k < KM; ++k) obuf[k] = 0.f;
  int64_t orow = -1;
  auto store_prev = [&]() {
    if (orow >= 0 && orow < n) {
#pragma unroll
      for (int k = 0; k < KM; ++k)
        if (k < nk) (mm.pred[k] + bd.y_off)[orow] = obuf[k];
    }
  };
  for (; tt < te; tt += NW, sl ^= 1) {
    // younger than this tile's pieces: the previous tile's stores (issued below, in front of the
    // refill) and the next tile's nch pieces, one vector-memory instruction per chunk.  Counting
    // the pieces alone is the safe side whether or not stores and loads retire in issue order
    fe_vm_wait8(tt + NW < te ? nch : 0);
    store_prev();
    // the chunk walk, the same text as k_stats_fe (kernels_fs.hip): the chunk's fragments once, then every model's
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
        float z[NL - 1][4], a[NL - 1][4];
        obuf[k] = fe_head<NL, ACT>(facc[k], zk[k], s_hw[k], z, a);
      }
      asm volatile("" ::: "memory");  // one model's head parameters at a time
    }
    orow = 64 * (int64_t)tt + iota;
  }
  store_prev();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// items: one fx launch group
void launch_forward_fe(const DevState& st, const FeModels& mm, const GradItem* items, int32_t nitems, int32_t L,
                       int32_t act, hipStream_t s) {
  if (nitems <= 0 || mm.nk <= 0) return;
  FeModels mf = mm;
  mf.fill_unused();
  for (int k = mm.nk; k < BANN_FE_KM; ++k) mf.pred[k] = mm.pred[0];
  fe_dispatch(L, act, [&](auto nl, auto a) {
    hipLaunchKernelGGL((k_forward_fe<decltype(nl)::value, decltype(a)::value>), dim3((unsigned)nitems),
                       dim3(64 * FE_WAVES), 0, s, st, mf, items);
  });
}

// ---------------------------------------------------------------------------
// Net::predict's sum (net.rs:546-557) on the device: one thread per individual and
// model, v = 0 + bias, then += the rows in branch order, all in f32 -- the bits of
// bann_net_predict's host loop
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_models_sum(const float* __restrict__ rows, int64_t model_stride, int32_t nb,
                                                   int64_t n, float b0, float b1, float b2, float b3,
                                                   float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const int j = blockIdx.y;
  if (i >= n) return;
  const float bias = j == 0 ? b0 : (j == 1 ? b1 : (j == 2 ? b2 : b3));
  const float* r = rows + (int64_t)j * model_stride + i;
  float v = 0.f + bias;
#pragma unroll 8
  for (int32_t b = 0; b < nb; ++b) v += r[(int64_t)b * n];
  out[(int64_t)j * n + i] = v;
}

void launch_models_sum(const FeModels& mm, int32_t nb, int64_t n, float* out, hipStream_t s) {
  if (mm.nk <= 0 || n <= 0) return;
  static_assert(BANN_FE_KM == 4, "k_models_sum takes four biases");
  // the rows of model j: mm.pred[j] = mm.pred[0] + j (nbranch n)
  const int64_t stride = mm.nk > 1 ? (int64_t)(mm.pred[1] - mm.pred[0]) : 0;
  hipLaunchKernelGGL(k_models_sum, dim3((unsigned)((n + 63) / 64), (unsigned)mm.nk), dim3(64), 0, s, mm.pred[0], stride,
                     nb, n, mm.bias[0], mm.bias[1], mm.bias[2], mm.bias[3], out);
}

// mean and two-pass sample variance over the nk rows (slot order), f64, rounded to f32 once
__global__ void __launch_bounds__(256) k_models_moments(const float* __restrict__ rows, int32_t nk, int64_t n,
                                                        float* __restrict__ mean, float* __restrict__ var) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int32_t k = 0; k < nk; ++k) s += (double)rows[(int64_t)k * n + i];
  const double mu = s / (double)nk;
  if (mean) mean[i] = (float)mu;
  if (var) {
    double q = 0.0;
    for (int32_t k = 0; k < nk; ++k) {
      const double d = (double)rows[(int64_t)k * n + i] - mu;
      q += d * d;
    }
    var[i] = nk > 1 ? (float)(q / (double)(nk - 1)) : 0.f;
  }
}

void launch_models_moments(const float* rows, int32_t nk, int64_t n, float* mean, float* var, hipStream_t s) {
  if (nk <= 0 || n <= 0 || (!mean && !var)) return;
  hipLaunchKernelGGL(k_models_moments, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, rows, nk, n, mean, var);
}
