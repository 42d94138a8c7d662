// kernels_fe.hip — forward-only pass of the fx-shaped branches (every width <= 4,
// m_b <= 512) for SEVERAL parameter sets at once: the model slots of a context
// (bann_models_*), up to BANN_FE_KM models per genotype pass.
//
// Why.  The single-model forward (k_forward_fx, kernels_fx.hip) is bound by the
// genotype stream: its i8 MFMA work per tile is a fraction of the time the tile
// takes to arrive.  Predicting a chain of K saved models one by one streams the
// same image K times.  Here every 64-individual tile is streamed once per pass:
// chunk by chunk its B operand (the quad-byte fragments, read from the wave's
// LDS slot with the transposing ds_read_b64_tr_b8) is brought into registers and
// masked into its four cumulative fragments once, and the MFMAs of every model
// of the pass run against them with that model's register-resident W0 digit
// operands (8 chunks x 4 VGPRs per model): 4 KM independent accumulator chains.
// Each model then runs its own head and stores its own row.
//
// Bits.  Per model the arithmetic is k_forward_fx's: the same tile image (field 3
// stored as code - 1, so the raw byte is the fourth cumulative fragment and its
// accumulator starts at the model's 64 x digit row sums), the same exact int32
// digit sums, the same digit combine, scale multiply, lane transpose and fmaf
// order in the head -- the row of (model, branch) is bitwise the row
// k_forward_fx writes for the same parameters (tests/test_models_gpu.py).
//
// Registers.  Head weights do not fit in scalar registers for four models (28-60
// values each), so they sit in LDS ([model][layer][20], as k_forward_fx stages
// them) with the models' digit row sums and are read per tile; the digit
// operands, which every MFMA needs, stay in registers.  Resource numbers and
// the measured A/B: DESIGN.md 4.7.
//
// Stream.  Two tile slots per wave, the stream two tiles ahead; a slot is
// refilled once its last chunk has been read.  A tile's prediction stores are
// issued at the top of the NEXT tile, in front of that tile's refill: the
// counted wait on a tile then never waits for a store younger than one tile.
#include <stdlib.h>

#include "activations.h"
#include "bann_internal.h"
#include "fe_util.h"
#include "kernel_util.h"

#define FE_WAVES 4
#define FE_SLOT 8192  // one tile image at <= 8 chunks
#define FE_KM BANN_FE_KM

// all but the youngest k (0 .. 8) vector-memory operations of this wave are complete
__device__ __forceinline__ void fe_vm_wait(int k) {
  switch (k) {
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// the head of one model's tile (k_forward_fx's head_out): in-place fields -> z (one
// individual per lane) -> f; hw = the model's [layer][20] LDS block (W_l[j][k] at
// 4 j + k for l >= 1, biases at 16 + k: c0 for l = 0)
template <int NL, int ACT>
__device__ __forceinline__ float fe_head(v4i (&facc)[4], float zscale, const float (*hw)[20]) {
  constexpr int NH = NL - 1;
  facc[3] -= facc[2];
  facc[2] -= facc[1];
  facc[1] -= facc[0];
  float z0 = zscale * fe_comb4(facc[0]), z1 = (0.25f * zscale) * fe_comb4(facc[1]);
  float z2 = (0.0625f * zscale) * fe_comb4(facc[2]), z3 = (0.015625f * zscale) * fe_comb4(facc[3]);
  fe_swap32(z0, z2);
  fe_swap32(z1, z3);
  fe_swap16(z0, z1);
  fe_swap16(z2, z3);
  float a[4];
  a[0] = act_h_t<ACT>(z0 + hw[0][16]);
  a[1] = act_h_t<ACT>(z1 + hw[0][17]);
  a[2] = act_h_t<ACT>(z2 + hw[0][18]);
  a[3] = act_h_t<ACT>(z3 + hw[0][19]);
#pragma unroll
  for (int l = 1; l < NH; ++l) {
    float an[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float s = hw[l][16 + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf(a[j], hw[l][4 * j + k], s);
      an[k] = act_h_t<ACT>(s);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = an[k];
  }
  float out = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) out = fmaf(a[j], hw[NL - 1][4 * j], out);
  return out;
}

// One instantiation per (layers, activation) serves every chunk count <= 8: the per-chunk guards are
// wave-uniform scalar branches (an 8-chunk specialisation without them let the scheduler lengthen the
// fragments' live ranges into spills of the digit operands)
template <int NL, int ACT>
__global__ void __launch_bounds__(64 * FE_WAVES, 2)
    k_forward_fe(DevState st, FeModels mm, const GradItem* __restrict__ items) {
  constexpr int NH = NL - 1;
  constexpr int NW = FE_WAVES;
  constexpr int NS = 2;  // tile slots per wave: the stream runs NS tiles ahead
  __shared__ __attribute__((aligned(16))) char s_x[NW][NS][FE_SLOT];
  __shared__ __attribute__((aligned(16))) float s_hw[FE_KM][NL][20];
  __shared__ __attribute__((aligned(16))) v4i s_rs[FE_KM][64];  // 64 x the digit row sums: the raw-byte accumulator's start

  const GradItem it = items[blockIdx.x];
  const int b = it.branch;
  const BranchDev& bd = st.br[b];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nch = bd.nchunks;
  const int nk = mm.nk;
  const int64_t n = st.n;
  const int tb = it.frag_begin >> 2, te = (it.frag_end + 3) >> 2;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 1, tp = lane & 1;

  // per model: head parameters -> LDS, W0 digit operands, their row sums and the lane's column scale ->
  // registers.  No branch on the model count here: the unused models of a short pass carry model 0's
  // pointers (launch_forward_fe), are loaded like it and skipped in the tile loop only
  v4i A[FE_KM][8];
  float zscale[FE_KM];
#pragma unroll
  for (int k = 0; k < FE_KM; ++k) {
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
        if (l >= 1 && l < NH && kk < bd.widths[l]) v = th[bd.boff[l] + kk];
      }
      s_hw[k][l][r] = v;
    }
    zscale[k] = mm.fc[k][b].scale[g];
    v4i rowsum64 = v4i{0, 0, 0, 0};
    const uint8_t* dg = mm.dig[k] + bd.dig_off + lane * 16;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int cc = c < nch ? c : nch - 1;  // a chunk of the branch's image; chunks past nch: zero operands
      const v4i a = *reinterpret_cast<const v4i*>(dg + (int64_t)cc * 1024);
      A[k][c] = c < nch ? a : v4i{0, 0, 0, 0};
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) rowsum64 = fe_rowsum64_acc(A[k][c], rowsum64);
    if (wave == 0) s_rs[k][lane] = rowsum64;  // the same in every wave
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();  // the head parameters are in LDS before any LDS-DMA is in flight

  const int gsw = g & 1;
  const uint32_t fo0 = (uint32_t)((16 * g + tq + 8 * gsw) * 16 + 8 * (tp ^ gsw));
  const uint32_t fo1 = (uint32_t)((16 * g + tq + 8 * (1 ^ gsw)) * 16 + 8 * (tp ^ 1 ^ gsw));
  const int iota = 4 * i16 + g;
  const char* xsrc = reinterpret_cast<const char*>(st.xu2) + bd.x_off;  // wave-uniform; the lane adds 16 lane
  const uint32_t xlane = (uint32_t)lane * 16u;
  const int64_t tile_bytes = (int64_t)nch * 1024;
  // the last chunk's padding rows are not streamed (as in k_forward_fx): their digit operands are zero
  const bool pad_row = 64 * (nch - 1) + 16 * (lane >> 4) + (((lane & 15) - 8 * ((lane >> 4) & 1)) & 15) >= bd.m;
  auto issue_tile = [&](int tt, int sl) {
    for (int c = 0; c < nch; ++c) {
      if (c == nch - 1 && pad_row) continue;
      glds16_s(xsrc + (int64_t)tt * tile_bytes + c * 1024, xlane, &s_x[wave][sl][c * 1024]);
    }
  };

  int tt = tb + wave, sl = 0;
  for (int j = 0; j < NS; ++j)
    if (tt + j * NW < te) issue_tile(tt + j * NW, j);
  float obuf[FE_KM];  // the previous tile's outputs, stored at the top of the next tile
#pragma unroll
  for (int k = 0; k < FE_KM; ++k) obuf[k] = 0.f;
  int64_t orow = -1;
  auto store_prev = [&]() {
    if (orow >= 0 && orow < n) {
#pragma unroll
      for (int k = 0; k < FE_KM; ++k)
        if (k < nk) (mm.pred[k] + bd.y_off)[orow] = obuf[k];
    }
  };
  for (; tt < te; tt += NW, sl ^= 1) {
    // younger than this tile's pieces: the previous tile's stores (issued below, in front of the
    // refill) and the next tile's nch pieces, one vector-memory instruction per chunk.  Counting
    // the pieces alone is the safe side whether or not stores and loads retire in issue order
    fe_vm_wait(tt + NW < te ? nch : 0);
    store_prev();
    const char* xs = &s_x[wave][sl][0];
    v4i facc[FE_KM][4];
#pragma unroll
    for (int k = 0; k < FE_KM; ++k) {
      facc[k][0] = facc[k][1] = facc[k][2] = v4i{0, 0, 0, 0};
      facc[k][3] = s_rs[k][lane];
    }
    // chunk by chunk: the chunk's four cumulative fragments once, then every model's MFMAs against
    // them (4 KM independent accumulator chains); the next chunk's LDS read is in flight meanwhile
    v4u Xn = (v4u)lds_tr8_pair(xs + fo0, xs + fo1);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (c >= nch) break;
      const v4u X = Xn;
      if (c + 1 < 8 && c + 1 < nch) Xn = (v4u)lds_tr8_pair(xs + (c + 1) * 1024 + fo0, xs + (c + 1) * 1024 + fo1);
      const v4i f0 = (v4i)(X & 0x03030303u), f1 = (v4i)(X & 0x0F0F0F0Fu), f2 = (v4i)(X & 0x3F3F3F3Fu), f3 = (v4i)X;
#pragma unroll
      for (int k = 0; k < FE_KM; ++k) {
        if (k < nk) {  // wave-uniform
          facc[k][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[k][c], f0, facc[k][0], 0, 0, 0);
          facc[k][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[k][c], f1, facc[k][1], 0, 0, 0);
          facc[k][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[k][c], f2, facc[k][2], 0, 0, 0);
          facc[k][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[k][c], f3, facc[k][3], 0, 0, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // every read of this slot has returned (the MFMAs consumed them): refill it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (tt + NS * NW < te) issue_tile(tt + NS * NW, sl);
#pragma unroll
    for (int k = 0; k < FE_KM; ++k) {
      if (k < nk) obuf[k] = fe_head<NL, ACT>(facc[k], zscale[k], s_hw[k]);
      asm volatile("" ::: "memory");  // one model's head parameters at a time
    }
    orow = 64 * (int64_t)tt + iota;
  }
  store_prev();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int NL>
static void launch_fe_nl(const DevState& st, const FeModels& mm, const GradItem* items, int32_t nitems, int act,
                         hipStream_t s) {
  const dim3 grid((unsigned)nitems), block(64 * FE_WAVES);
  switch (act) {
    case 0: hipLaunchKernelGGL((k_forward_fe<NL, 0>), grid, block, 0, s, st, mm, items); break;
    case 1: hipLaunchKernelGGL((k_forward_fe<NL, 1>), grid, block, 0, s, st, mm, items); break;
    case 2: hipLaunchKernelGGL((k_forward_fe<NL, 2>), grid, block, 0, s, st, mm, items); break;
    case 3: hipLaunchKernelGGL((k_forward_fe<NL, 3>), grid, block, 0, s, st, mm, items); break;
    default: hipLaunchKernelGGL((k_forward_fe<NL, 4>), grid, block, 0, s, st, mm, items); break;
  }
}

// items: one fx launch group
void launch_forward_fe(const DevState& st, const FeModels& mm, const GradItem* items, int32_t nitems, int32_t L,
                       int32_t act, hipStream_t s) {
  if (nitems <= 0 || mm.nk <= 0) return;
  FeModels mf = mm;  // unused models: model 0's pointers (the kernel's prologue reads every model)
  for (int k = mm.nk; k < BANN_FE_KM; ++k) {
    mf.theta[k] = mm.theta[0];
    mf.dig[k] = mm.dig[0];
    mf.fc[k] = mm.fc[0];
    mf.pred[k] = mm.pred[0];
  }
  switch (L) {
    case 2: launch_fe_nl<2>(st, mf, items, nitems, act, s); break;
    case 3: launch_fe_nl<3>(st, mf, items, nitems, act, s); break;
    case 4: launch_fe_nl<4>(st, mf, items, nitems, act, s); break;
    default: break;
  }
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
