// fe_stream.h — the multi-model tile pass over the fx-shaped branches (every width
// <= 4, m_b <= 512), shared by k_forward_fe (kernels_fe.hip: the rows of a chain of
// saved models) and k_stats_fe (kernels_fs.hip: its branch R² and effect-size sums).
// Both kernels are this pass up to the branch output; what a kernel does with `out`
// is its own and lives in its file.  The pass is described here, once.
//
// Why.  The single-model forward (k_forward_fx, kernels_fx_fwd.hip) is bound by the
// genotype stream: its i8 MFMA work per tile is a fraction of the time the tile
// takes to arrive, and a chain of K models one by one streams the same image K
// times.  Here every 64-individual tile is streamed once per pass of KM models.
//
// Stream.  Work items, tile ownership (tile tb + wave + FE_WAVES j), the padding-row
// rule and the counted vmcnt are k_forward_fx's.  Each wave owns FE_NS tile slots of
// FE_SLOT bytes and runs FE_NS tiles ahead; a slot is refilled once its last chunk has
// been read (the lgkmcnt(0) that ends the chunk walk).  A tile is one LDS-DMA piece per
// chunk, the last chunk's padding rows unstreamed: their digit operands are zero.
//
// Tile.  Chunk by chunk the B operand (the quad-byte fragments, read from the slot
// with the transposing ds_read_b64_tr_b8, the next chunk's read in flight) is masked
// into its four cumulative fragments ONCE, and the MFMAs of every model of the pass
// run against them with that model's register-resident W0 digit operands (8 chunks x
// 4 VGPRs per model): 4 KM independent int32 accumulator chains.  Models >= nk of a
// short pass are skipped by a wave-uniform branch; the host gives them model 0's
// pointers (FeModelSet::fill_unused), so the prologue needs no branch on nk.
//
// Bits.  Per model the arithmetic is k_forward_fx's: the same tile image (field 3
// stored as code - 1, so the raw byte is the fourth cumulative fragment and its
// accumulator starts at the model's 64 x digit row sums), the same exact int32
// digit sums, digit combine, scale multiply, lane transpose and fmaf order in the
// head -- `out` of (model, branch, individual) is bitwise the row element
// k_forward_fx writes (tests/test_models_gpu.py).
//
// Registers.  Head weights do not fit in scalar registers for several models (28-60
// values each), so they sit in LDS ([model][layer][20], as k_forward_fx stages them)
// with the models' digit row sums and are read per tile; the digit operands, which
// every MFMA needs, stay in registers.
//
// What is here and what is not.  Both kernels sit at 240-256 VGPRs with no spill, and
// k_stats_fe's backward chain has expressions the compiler may contract two ways (1 - h h
// times err); which way depends on the surrounding code.  Shared here is every piece whose
// sharing leaves k_stats_fe's instructions exactly as they were and k_forward_fe's
// registers, LDS-DMA sites and timing as they were: a digit operand,
// the four MFMAs of (chunk, model), the head's forward and the host dispatch.  The rest
// stays in the kernels, once each and the same text -- the lane geometry, the per-model
// prologue, the chunk walk's skeleton and the piece-issue loop: as functions over the
// A / facc arrays the prologue and the walk changed k_stats_fe's contraction (its effect
// sizes then differ in the last bits), the piece-issue loop had its last iteration peeled
// at every call site (twice the LDS-DMA instructions), the head parameter's value and
// the geometry rescheduled k_stats_fe.  Numbers: profiles/fe_stream_refactor.md.
#pragma once
#include <type_traits>

#include "activations.h"
#include "bann_internal.h"
#include "fe_util.h"

#define FE_WAVES 4
#define FE_SLOT 8192  // one tile image at <= 8 chunks
#define FE_NS 2       // tile slots per wave: the stream runs FE_NS tiles ahead

// prologue: the lane's W0 digit operand of chunk c (dg: the model's digit image of the branch + 16 lane); chunks past
// nch are zero operands, loaded from the last real chunk so that the load needs no branch
__device__ __forceinline__ v4i fe_digit_operand(const uint8_t* dg, int c, int nch) {
  const int cc = c < nch ? c : nch - 1;
  const v4i a = *reinterpret_cast<const v4i*>(dg + (int64_t)cc * 1024);
  return c < nch ? a : v4i{0, 0, 0, 0};
}
// chunk walk, per (chunk, model): the chunk's four cumulative fragments against the model's digit operand
__device__ __forceinline__ void fe_mfma4(v4i a, v4i f0, v4i f1, v4i f2, v4i f3, v4i (&facc)[4]) {
  facc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, f0, facc[0], 0, 0, 0);
  facc[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, f1, facc[1], 0, 0, 0);
  facc[2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, f2, facc[2], 0, 0, 0);
  facc[3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, f3, facc[3], 0, 0, 0);
}

// the head of one model's tile (k_forward_fx's head_out): in-place fields -> z (one individual per
// lane) -> f.  Every layer's pre-activation z[l] and activation a[l] is left to the caller (k_stats_fe's
// backward chain; dead in k_forward_fe); widths below 4 are zero-padded, so padded units carry exact zeros
template <int NL, int ACT>
__device__ __forceinline__ float fe_head(v4i (&facc)[4], float zk, const float (*hw)[20], float (&z)[NL - 1][4],
                                         float (&a)[NL - 1][4]) {
  constexpr int NH = NL - 1;
  float z0, z1, z2, z3;  // with the first-layer bias: the lane's column (lane >> 4) before the transpose
  fx_z0_cum(facc, zk, hw[0][16 + ((threadIdx.x >> 4) & 3)], z0, z1, z2, z3);
  swap32(z0, z2);
  swap32(z1, z3);
  swap16(z0, z1);
  swap16(z2, z3);
  z[0][0] = z0;
  z[0][1] = z1;
  z[0][2] = z2;
  z[0][3] = z3;
#pragma unroll
  for (int k = 0; k < 4; ++k) a[0][k] = act_h_t<ACT>(z[0][k]);
#pragma unroll
  for (int l = 1; l < NH; ++l) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float s = hw[l][16 + k];
#pragma unroll
      for (int j = 0; j < 4; ++j) s = fmaf(a[l - 1][j], hw[l][4 * j + k], s);
      z[l][k] = s;
      a[l][k] = act_h_t<ACT>(s);
    }
  }
  float out = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) out = fmaf(a[NH - 1][j], hw[NL - 1][4 * j], out);
  return out;
}

// host: f(integral_constant<layers>, integral_constant<activation>) for the (layers, activation) a kernel
// is instantiated for; other layer counts launch nothing, activations past 3 are the identity's
template <class F>
static void fe_dispatch(int32_t L, int32_t act, F&& f) {
  auto with_act = [&](auto nl) { act_dispatch(act, [&](auto a) { f(nl, a); }); };
  switch (L) {
    case 2: with_act(std::integral_constant<int, 2>{}); break;
    case 3: with_act(std::integral_constant<int, 3>{}); break;
    case 4: with_act(std::integral_constant<int, 4>{}); break;
    default: break;
  }
}
