// kernels_fx.hip — the "fx" fused gradient kernel (default): one WAVE owns a
// 64-individual tile of one branch across ALL of its marker chunks.
//
// Replaces BranchSampler::backpropagate (branch_sampler.rs:813-875) with its
// forward_feed (743-782) and the rss it stores (823-828), for every branch of a
// plan in one launch, and writes the same per-split partial slabs as the other
// fused variants (d(rss/2)/d(theta) in param_vec order, params.rs:700-715).
//
// Why this shape (measured on the chunk-wave kernels it replaces): with one
// wave per 64-marker chunk, every tile needs a cross-wave exchange of partial
// Z0 and of delta0 (two barriers), the per-individual head serialises on one
// wave, and every MFMA result is converted to f32 on its own -- issue- and
// latency-bound at 2.4 TB/s of 2-bit genotypes.  Here:
//   * the forward accumulates Z0 over all chunks in the MFMA's int32
//     accumulator (exact), converted once per tile;
//   * the head runs in every wave, one individual per lane;
//   * dW0 = G^T delta0 accumulates over ALL tiles of the item in int32 digit
//     sums with a per-column running power-of-two scale (rescaled exactly by
//     digit carry in the rare case a tile's |delta0| outgrows it), converted to
//     f32 once at the end;
//   * waves never wait for each other inside the tile loop: each streams its
//     own tiles into its own LDS slots (LDS-DMA, two tiles ahead, counted
//     vmcnt) -- the only barriers are the final workgroup reduction.
// The tile image and the helpers shared with the other fx-family kernels: fx_tile.h.
#include <stdlib.h>

#include "../../include/bann.h"
#include "activations.h"
#include "bann_internal.h"
#include "fx_shapes.h"
#include "fx_tile.h"
#include "update_core.h"

// Profiling builds only (tools/build_ab.sh <tag> "-DFX_STAMPS=1" / "-DFX_ABL=<bits>"); both 0 in the
// product, where they generate no code.  FX_STAMPS: per-phase shader-cycle sums of k_fused_grad_fx
// (s_memtime) into DevState::dbg, printed at bann_ctx_destroy under BANN_STAMPS=1: p0 wait for the
// tile, p1 forward, p2 head, p3 delta0 digits, p4 backward, p5 loop overhead, p6 realtime (100 MHz),
// p7 loop cycles.  FX_ABL (results wrong, timing only): 1 forward without the 2-bit unpack, 2 backward
// without it, 4 no head (delta0 = z0), 8 no MFMAs (the operands XORed into the accumulators), 16 no
// genotype / target stream (the loop computes on whatever the slots hold).
#ifndef FX_STAMPS
#define FX_STAMPS 0
#endif
#ifndef FX_ABL
#define FX_ABL 0
#endif
// The backward reads its genotype windows this many windows ahead, without a scheduling barrier per
// window (8 with the barrier, a barrier-free 8, 4 and 16 measured slower: profiles/r06_fx_knobs.txt)
constexpr int FXT_PD = 12;
// The guarded body (below) reads fewer ahead: the two bodies' loop-invariant values together would
// otherwise spill (8: 2 .. 5 vector registers in the ReLU / leaky / SiLU / identity instantiations)
constexpr int FXT_PD_EDGE = 4;
// k_fused_grad_fx runs its tiles from two loops over one body.  A tile whose successor two rounds on
// (tile tt + 2 NW, refilled into its slot) exists and is full, in a launch that writes no
// predictions, takes the steady instantiation: no more / more2 / valid / write_pred guards, a constant
// vmcnt, an unclamped target row -- its backward is one basic block.  Every other tile (a wave's last
// two, a partial last tile, a prediction-writing launch) takes the guarded one.  Same tile order, same
// accumulation order: bit-identical outputs.
// A steady tile's refill takes two 64-bit bases per tile and each piece as the instruction's immediate
// offset, which gfx950 adds to the LDS address too (bann_fx_dma_offset_probe), so M0 is written once
// per 4 KiB half slot; without it the two bodies spill vector registers.  The delta0 scale's two
// fallback forms (unset -> 5 / 255) live in registers (Rg, Rd), with Rg's threshold as a float (Tg: the
// growth test is one float compare per column), updated only in the rare rescale path.
// Measurements: DESIGN.md 4.
#if FX_STAMPS
#define FX_STAMP(i)                                            \
  do {                                                         \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
    ph[i] += t_ - t_last;                                      \
    t_last = t_;                                               \
  } while (0)
#else
#define FX_STAMP(i) \
  do {              \
  } while (0)
#endif
#if FX_ABL & 8
#define FX_MFMA(a, b, c) ((c) + ((a) ^ (b)))
#else
#define FX_MFMA(a, b, c) __builtin_amdgcn_mfma_i32_16x16x64_i8((a), (b), (c), 0, 0, 0)
#endif
// The stream runs TWO tiles ahead in the same two slots: chunk c of tile t + 2
// is issued into tile t's slot as soon as tile t's backward has read chunk c's
// last window (the target piece once the head has read the target), so a piece
// has a whole tile more to land than when it is issued in the forward (the
// one-tile-ahead and burst variants measured slower: DESIGN.md 4)

// NCH: 8 = every branch of the launch has exactly 8 chunks (no per-chunk guards,
// so the LDS reads of a whole phase issue back to back); 0 = any count <= 8.

// UPD: the instantiation with the fused update tail (bann_plan.hip fuse_update plans);
// the default one carries no tail code at all (its registers: the tail's live values
// made the tile loop spill scalar registers to vector lanes)
template <int NL, int ACT, int NCH, int UPD>
__global__ void __launch_bounds__(64 * FX_WAVES, NL == 4 ? 1 : 2)
    k_fused_grad_fx(DevState st, const GradItem* __restrict__ items, int write_pred, int upd_mode, int upd_step,
                    int32_t* __restrict__ upd_cnt, const FoldJob* __restrict__ folds) {
  constexpr int NH = NL - 1;  // layers with activations
  constexpr int NW = FX_WAVES;
  constexpr int NS = 8 + (NH - 1) * 20;  // head statistics per wave
  __shared__ __attribute__((aligned(16))) char s_x[NW][2][FX_SLOT];
  __shared__ __attribute__((aligned(16))) char s_dig[NW][4 * FX_DROW];
  __shared__ __attribute__((aligned(16))) float s_y[NW][2][64];
  __shared__ __attribute__((aligned(16))) char s_w0[8 * 1024];  // W0/sigma digits (A operand), per chunk
  __shared__ __attribute__((aligned(16))) float s_hw[NL][20];  // head: W_l (4 x 4) then b_l (4) per layer
  __shared__ float s_hs[NW][NS];
  __shared__ double s_rss[NW];

  const GradItem it = items[blockIdx.x];
  const int b = it.branch;
  const BranchDev& bd = st.br[b];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nch = NCH ? NCH : bd.nchunks;
  const int64_t n = st.n;
  const int tb = it.frag_begin >> 2, te = (it.frag_end + 3) >> 2;

  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 1, tp = lane & 1;
  // ---- per-lane LDS offsets ----
  const int gsw = g & 1;
  const uint32_t fo0 = (uint32_t)((16 * g + tq + 8 * gsw) * 16 + 8 * (tp ^ gsw));
  const uint32_t fo1 = (uint32_t)((16 * g + tq + 8 * (1 ^ gsw)) * 16 + 8 * (tp ^ 1 ^ gsw));
  const int pe = i16, po = (i16 + 8) & 15;
  const uint32_t boe = (uint32_t)(pe * 16 + 4 * (2 * ((g >> 1) ^ (pe >> 3)) + (g & 1)));
  const uint32_t boo = (uint32_t)(po * 16 + 4 * (2 * ((g >> 1) ^ (po >> 3)) + (g & 1)));
  const int iota = 4 * i16 + g;  // individual of this lane in the head (after the transpose)
  char* const sd = &s_dig[wave][0];
  char* const sd_w = sd + (i16 >> 2) * FX_DROW + (4 * g + (i16 & 3)) * 16;  // row K(iota)
  const char* const sd_r = sd + g * FX_DROW + tq * 16 + 8 * tp;
  // the tile's targets -- or, in network mode, the network's output error, the same
  // n-vector for every branch (bann_network_hmc_step)
  const bool net_err = st.nete != nullptr;
  const float* ybr = net_err ? st.nete : st.y + bd.y_off;
  float* predb = st.pred + bd.y_off;
  const int64_t tile_bytes = (int64_t)nch * 1024;
  // the stream's base in scalar registers: each piece is one global_load_lds in the saddr
  // form (one address VGPR, no 64-bit address arithmetic per piece: -0.7 % per launch)
  const uint64_t xb = (uint64_t)(uintptr_t)(reinterpret_cast<const char*>(st.xu2) + bd.x_off);
  const char* xbase_s = reinterpret_cast<const char*>(
      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(xb >> 32)) << 32) |
      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)xb));

  // LDS-DMA of the NEXT tile is spread over the current tile's forward phase
  // (one 1 KiB piece per chunk, the target piece in the head): issued in one
  // burst the pieces back-pressure the wave for thousands of cycles.
  // the last chunk's padding rows (markers >= m) are not streamed (C3: 12 of 512 rows):
  // their W0 digits are zero, so whatever the slot holds there adds nothing to Z0, and
  // their dW0 rows are dropped.  Lane L moves record L of a chunk: window L >> 4 at
  // position L & 15 holds row 16 (L >> 4) + ((L & 15) - 8 ((L >> 4) & 1)) & 15.
  // (Row 0 is never padding, so the wave's instruction -- one vmcnt count -- always issues.)
  const bool pad_row = 64 * (nch - 1) + 16 * (lane >> 4) + (((lane & 15) - 8 * ((lane >> 4) & 1)) & 15) >= bd.m;
  auto issue_chunk = [&](int tt, int sl, int c) {
    if (FX_ABL & 16) return;
    if (c == nch - 1 && pad_row) return;
    glds16_s(xbase_s + (uint64_t)tt * (uint64_t)tile_bytes + (uint64_t)(c * 1024), (uint32_t)lane * 16u,
             &s_x[wave][sl][c * 1024]);
  };
  auto issue_y = [&](int tt, int sl) {
    if (FX_ABL & 16) return;
    const int64_t row = 64 * (int64_t)tt + iota;
    glds4(ybr + (row < n ? row : n - 1), &s_y[wave][sl][0]);
  };
  auto issue_y_full = [&](int tt, int sl) {  // a full tile: no row clamp
    if (FX_ABL & 16) return;
    glds4(ybr + (64 * (int64_t)tt + iota), &s_y[wave][sl][0]);
  };
  // piece c of the tile image at nb into the slot at LDS byte address lb (both wave-uniform):
  // HBM image == LDS image, so the halves' bases and the immediate offset address both
  const uint64_t live_rows = __builtin_amdgcn_ballot_w64(!pad_row);  // the last chunk's streamed rows
  auto issue_piece = [&](const char* nb, uint32_t lb, int c) __attribute__((always_inline)) {
    if (FX_ABL & 16) return;
    const char* gb = nb + 4096 * (c >> 2);
    const uint32_t voff = (uint32_t)lane * 16u;
    const uint32_t m0v = lb + 4096u * (uint32_t)(c >> 2);
    if (NCH != 0 && c != NCH - 1) {
      switch (c & 3) {
        case 0: glds16_so<0>(gb, voff, m0v); break;
        case 1: glds16_so<1024>(gb, voff, m0v); break;
        case 2: glds16_so<2048>(gb, voff, m0v); break;
        default: glds16_so<3072>(gb, voff, m0v); break;
      }
    } else {  // the last chunk's padding rows are not streamed: exec-masked, as in issue_chunk
      const uint64_t mk = (NCH != 0 || c == nch - 1) ? live_rows : ~0ull;
      switch (c & 3) {
        case 0: glds16_so_masked<0>(gb, voff, m0v, mk); break;
        case 1: glds16_so_masked<1024>(gb, voff, m0v, mk); break;
        case 2: glds16_so_masked<2048>(gb, voff, m0v, mk); break;
        default: glds16_so_masked<3072>(gb, voff, m0v, mk); break;
      }
    }
  };
  // the item's first two tiles are issued before the prologue's loads, so their HBM latency
  // overlaps the W0-digit and head-weight loads (a solo item -- the sequential driver's
  // one-branch steps -- has one tile per wave: the launch was that latency longer)
  int tt = tb + wave, sl = 0;
  if (tt < te) {
    for (int c = 0; c < nch; ++c) issue_chunk(tt, 0, c);
    issue_y(tt, 0);
    if (tt + NW < te) {
      for (int c = 0; c < nch; ++c) issue_chunk(tt + NW, 1, c);
      issue_y(tt + NW, 1);
    }
  }
  // ---- branch constants: head weights (LDS, then scalar registers), W0 digits, column scale ----
  const float* th = st.theta + bd.p_off;
  for (int t = threadIdx.x; t < NL * 20; t += 64 * NW) {
    const int l = t / 20, r = t - l * 20;
    float v = 0.f;
    if (r < 16) {  // Wh[l][j][k] = W_l[j][k] (l >= 1), zero padded to 4 x 4
      const int j = r >> 2, k = r & 3;
      if (l >= 1 && j < bd.win[l] && k < bd.widths[l]) v = th[bd.woff[l] + k * bd.win[l] + j];
    } else {  // bias[0] = c0 (folded standardisation), bias[l] = b_l
      const int k = r - 16;
      if (l == 0 && k < bd.widths[0]) v = st.fc[b].c0[k];
      if (l >= 1 && l < NH && k < bd.widths[l]) v = th[bd.boff[l] + k];
    }
    s_hw[l][r] = v;
  }
  float zk = fx_zk(st.fc[b].scale[g]);
  for (int c = wave; c < nch; c += NW)  // W0 digit image -> LDS (shared by the four waves)
    *reinterpret_cast<v4i*>(&s_w0[c * 1024 + lane * 16]) =
        *reinterpret_cast<const v4i*>(st.dig + bd.dig_off + ((int64_t)c * 64 + lane) * 16);
  // retire the prologue loads and hide their provenance: inside the tile loop the
  // only vector-memory waits are the explicit, counted ones on this wave's DMAs
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" : "+v"(zk));
  __syncthreads();
  float zbias = s_hw[0][16 + g];  // the lane's column bias c0: the addend of Z0's last fma (fx_z0_cum)
  asm volatile("" : "+v"(zbias));
  v4i rowsum64 = v4i{0, 0, 0, 0};  // the forward's facc[3] start (field 3 stored as code - 1)
  for (int c = 0; c < nch; ++c) rowsum64 = rowsum64_acc(*reinterpret_cast<const v4i*>(&s_w0[c * 1024 + lane * 16]), rowsum64);
  // head weights as wave-uniform values: scalar registers for the whole item (the
  // per-tile LDS broadcasts serialised the head on their latencies)
  float uW[NL][4][4], uB[NH][4];
#pragma unroll
  for (int l = 0; l < NL; ++l) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        uW[l][j][k] = (l >= 1 && (l < NL - 1 || k == 0)) ? sgpr_f(s_hw[l][4 * j + k]) : 0.f;
    if (l < NH)
#pragma unroll
      for (int k = 0; k < 4; ++k) uB[l][k] = l >= 1 ? sgpr_f(s_hw[l][16 + k]) : 0.f;  // (b_0: zbias)
  }

  // ---- accumulators ----
  v4i acc[32];  // dW0 digit sums per 16-marker window u (lane: column g, marker 16u + i16)
#pragma unroll
  for (int u = 0; u < 32; ++u) acc[u] = v4i{0, 0, 0, 0};
  v4i acc3 = v4i{0, 0, 0, 0};  // 64 sum over K-group 3 of the digits: field 3's -1, every marker
  int R[4] = {0, 0, 0, 0};  // running delta0 scale exponent per column (0 = unset)
  double rss = 0.0;
  float db[NH][4], dWo[4];
  float dW[NL > 2 ? NL - 2 : 1][4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    dWo[k] = 0.f;
#pragma unroll
    for (int l = 0; l < NH; ++l) db[l][k] = 0.f;
#pragma unroll
    for (int l = 0; l < (NL > 2 ? NL - 2 : 1); ++l)
#pragma unroll
      for (int j = 0; j < 4; ++j) dW[l][j][k] = 0.f;
  }

#if FX_STAMPS
  unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ntl = 0;
  const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime(), mt0 = __builtin_amdgcn_s_memtime();
  unsigned long long t_last = mt0;
#endif
  int Rg[4] = {5, 5, 5, 5};          // R[k] ? R[k] : 5, the growth test's threshold
  // the same threshold as a float, 2^(Rg - 126): exponent field > Rg <=> |delta| >= it (unset: 2^-121)
  float Tg[4] = {fpow2(6), fpow2(6), fpow2(6), fpow2(6)};
  int Rd[4] = {255, 255, 255, 255};  // R[k] ? R[k] : 255, the digit exponent's
  // one tile; ST: the steady instantiation, whose guards are compile-time true / false
  auto tile = [&](auto steady_c) __attribute__((always_inline)) {
    constexpr bool ST = decltype(steady_c)::value;
    const bool more = ST || tt + NW < te;
    const bool more2 = ST || tt + 2 * NW < te;  // tile tt + 2 NW goes into this slot
    const bool wpred = !ST && write_pred;
    // tile tt (issued during tile tt - NW) has landed.  (An L2 prefetch of the
    // tile after it measured +3 %: with 8 waves/CU the L2 is already the DMA's
    // working set.)
    // the nch + 1 pieces of tile tt + NW are younger (loads return in order; a
    // younger pred store still outstanding only makes this wait longer)
    FX_STAMP(5);
    vm_wait<9, 2>(more ? nch + 1 : 0);  // nch >= 1; steady, NCH = 8: the constant vmcnt(9)
    FX_STAMP(0);
    const char* xs = &s_x[wave][sl][0];

    // ---- forward: Z0 of 64 individuals, exact int32 over all chunks ----
    // (software pipelined: the LDS reads of chunk c + 1 fly while chunk c's
    // four MFMAs issue; sched barriers keep the compiler from hoisting more)
    v4i facc[4] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, rowsum64};
    // the forward at raised priority too (with the stream issued in the backward:
    // -1.2 % per launch, A/B on one box)
    __builtin_amdgcn_s_setprio(1);
    {
      constexpr int FD = 2;  // two chunks ahead: an LDS read's latency exceeds one chunk's 4 MFMAs
      v4u Xq[FD];
      v4i Aq[FD];
#pragma unroll
      for (int c = 0; c < FD; ++c) {
        Xq[c] = v4u{0u, 0u, 0u, 0u};
        Aq[c] = v4i{0, 0, 0, 0};
        if (NCH != 0 || c < nch) {
          Xq[c] = (v4u)lds_tr8_pair(xs + c * 1024 + fo0, xs + c * 1024 + fo1);
          Aq[c] = *reinterpret_cast<const v4i*>(&s_w0[c * 1024 + lane * 16]);
        }
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (NCH == 0 && c >= nch) continue;
        const v4u Xc = Xq[c % FD];
        const v4i Ac = Aq[c % FD];
        if (c + FD < 8 && (NCH != 0 || c + FD < nch)) {
          Xq[c % FD] = (v4u)lds_tr8_pair(xs + (c + FD) * 1024 + fo0, xs + (c + FD) * 1024 + fo1);
          Aq[c % FD] = *reinterpret_cast<const v4i*>(&s_w0[(c + FD) * 1024 + lane * 16]);
        }
        // the cumulative fragments x & 0x03, x & 0x0F, x & 0x3F, x (header)
#if FX_ABL & 1
        const v4i B0 = (v4i)Xc, B1 = (v4i)Xc, B2 = (v4i)Xc, B3 = (v4i)Xc;
#else
        const v4i B0 = (v4i)(Xc & 0x03030303u);
        const v4i B1 = (v4i)(Xc & 0x0F0F0F0Fu);
        const v4i B2 = (v4i)(Xc & 0x3F3F3F3Fu);
        const v4i B3 = (v4i)Xc;
#endif
        facc[0] = FX_MFMA(Ac, B0, facc[0]);
        facc[1] = FX_MFMA(Ac, B1, facc[1]);
        facc[2] = FX_MFMA(Ac, B2, facc[2]);
        facc[3] = FX_MFMA(Ac, B3, facc[3]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    FX_STAMP(1);
    // the head + digit phase is a dependent VALU chain: at raised priority it
    // takes the SIMD's issue slots ahead of the partner wave's independent
    // MFMA/unpack stream (measured -1 %)
    __builtin_amdgcn_s_setprio(1);
    // lane (column g, slot i16) holds individual 4 i16 + q in register q; transpose
    // so that lane L holds all four columns of individual 4 (L & 15) + (L >> 4)
    float z0, z1, z2, z3;  // with the first-layer bias
    fx_z0_cum(facc, zk, zbias, z0, z1, z2, z3);
    swap32(z0, z2);
    swap32(z1, z3);
    swap16(z0, z1);
    swap16(z2, z3);

    // ---- head: one individual per lane ----
    const int64_t row = 64 * (int64_t)tt + iota;
    const bool valid = ST || row < n;
    const float yv = s_y[wave][sl][lane];
    float d[4];
#if FX_ABL & 4
    d[0] = z0 + yv, d[1] = z1, d[2] = z2, d[3] = z3;
    if (wpred && valid) predb[row] = z0;
    rss += (double)z1;
#else
    {
      const auto& Wh = uW;
      const auto& Bh = uB;
      float z[NH][4], a[NH][4];
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
          float s = Bh[l][k];
#pragma unroll
          for (int j = 0; j < 4; ++j) s = fmaf(a[l - 1][j], Wh[l][j][k], s);
          z[l][k] = s;
          a[l][k] = act_h_t<ACT>(s);
        }
      }
      float out = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) out = fmaf(a[NH - 1][j], Wh[NL - 1][j][0], out);
      const float e = valid ? (net_err ? yv : out - yv) : 0.f;
      if (wpred && valid) predb[row] = out;
      rss += (double)e * (double)e;
      float err[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dWo[j] = fmaf(a[NH - 1][j], e, dWo[j]);
        err[j] = e * Wh[NL - 1][j][0];
      }
#pragma unroll
      for (int l = NH - 1; l >= 0; --l) {
        float dl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          dl[k] = act_dh_t<ACT>(z[l][k], a[l][k]) * err[k];
          db[l][k] += dl[k];
        }
        if (l >= 1) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float sj = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              dW[l - 1][j][k] = fmaf(a[l - 1][j], dl[k], dW[l - 1][j][k]);
              sj = fmaf(dl[k], Wh[l][j][k], sj);
            }
            err[j] = sj;
          }
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) d[k] = dl[k];
        }
      }
    }
#endif

    if (more2) {  // the target has been read (yv in a register): its slot takes tile tt + 2 NW's
      asm volatile("" ::"v"(yv));
      if (ST)
        issue_y_full(tt + 2 * NW, sl);
      else
        issue_y(tt + 2 * NW, sl);
    }
    // the refill's two wave-uniform bases, once per tile
    const char* const nb = xbase_s + (uint64_t)(tt + 2 * NW) * (uint64_t)tile_bytes;
    const uint32_t lb = __builtin_amdgcn_readfirstlane(lds_off(&s_x[wave][sl][0]));
    __builtin_amdgcn_sched_barrier(0);
    FX_STAMP(2);
    // the backward's first genotype windows: their LDS reads fly under the digit phase
    constexpr int PD = ST ? FXT_PD : FXT_PD_EDGE;
    uint32_t wq[PD];
#pragma unroll
    for (int u = 0; u < PD; ++u)
      wq[u] = (NCH != 0 || u < 4 * nch) ? *reinterpret_cast<const uint32_t*>(xs + 256 * u + ((u & 1) ? boo : boe)) : 0u;
    // ---- delta0 -> signed digits at the running per-column scale 2^(R - 132) ----
    // running scale check: a column needs a (new) scale only when some lane's
    // |delta| reaches 2^(R - 126) (or R is unset); then the exact wave max of
    // the exponent fields sets it (rare after the first tile)
    int dl[4] = {0, 0, 0, 0};
    bool grow = false;
    {
      bool lane_need = false;  // one ballot for the four columns (no compare -> branch chain)
#pragma unroll
      for (int k = 0; k < 4; ++k) lane_need |= !(__builtin_fabsf(d[k]) < Tg[k]);  // (a NaN takes the rare path)
      if (__builtin_amdgcn_ballot_w64(lane_need) != 0) {
        const uint32_t e01 = wave_max_u16x2(((fbits(d[0]) >> 23) & 0xFFu) | (((fbits(d[1]) >> 23) & 0xFFu) << 16));
        const uint32_t e23 = wave_max_u16x2(((fbits(d[2]) >> 23) & 0xFFu) | (((fbits(d[3]) >> 23) & 0xFFu) << 16));
        const int E[4] = {(int)(e01 & 0xFFFFu), (int)(e01 >> 16), (int)(e23 & 0xFFFFu), (int)(e23 >> 16)};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          // the same test on the threshold: 5 while unset (E >= 6), R >= 8 once set (E > R)
          if (E[k] > Rg[k]) {
            if (Rg[k] != 5) {
              dl[k] = E[k] + 2 - Rg[k];
              grow = true;
            }
            Rg[k] = Rd[k] = E[k] + 2;
            Tg[k] = fpow2(E[k] + 3 < 255 ? E[k] + 3 : 255);  // (infinity: only an Inf / NaN delta passes it)
          }
        }
      }
    }
    if (grow) {  // rare: rescale the digit sums of the grown columns exactly
      const int sh = g == 0 ? dl[0] : g == 1 ? dl[1] : g == 2 ? dl[2] : dl[3];
#pragma unroll
      for (int u = 0; u < 32; ++u)
        if (NCH != 0 || u < 4 * nch) acc[u] = shr_digits(acc[u], sh);
      acc3 = shr_digits(acc3, sh);
    }
    v4u w;
    // this lane's individual sits in K-group p = g of the backward operand, whose
    // genotype codes stay in place (x 4^p): pre-divide its digits by 4^p
    const int kslot_sh = 2 * g;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = digits4_fx(d[k], 153 - kslot_sh - Rd[k]);
    *reinterpret_cast<v4u*>(sd_w) = w;

    __builtin_amdgcn_sched_barrier(0);
    FX_STAMP(3);
    __builtin_amdgcn_s_setprio(0);
    // ---- backward: dW0 digit sums += G^T delta0 (reads 4 windows ahead) ----
    const v4i A = lds_tr8_pair(sd_r, sd_r + 8 * 16);
    acc3 = FX_MFMA(A, FX_ONES3, acc3);
    {
      // every field in place (x 1, 4, 16, 64 (f3 - 1); the digits carry 4^-p): 4 VALU
      auto unpack = [](uint32_t wv) -> v4i {
#if FX_ABL & 2
        return v4i{(int)wv, (int)wv, (int)wv, (int)wv};
#else
        return fx_bwd_unpack(wv);
#endif
      };
      // window u + 2 is unpacked beside window u's MFMA: the MFMA's B operand was
      // written two iterations earlier, so no VALU -> MFMA hazard padding per window
      v4i Bn = unpack(wq[0]), Bn2 = unpack(wq[1]);
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        if (NCH == 0 && u >= 4 * nch) continue;
        const v4i Bv = Bn;
        Bn = Bn2;
        if (u + 2 < 32 && (NCH != 0 || u + 2 < 4 * nch)) Bn2 = unpack(wq[(u + 2) % PD]);
        if (more2 && (u & 3) == 1) {  // window 4c + 3, chunk c's last, is unpacked: refill chunk c
          asm volatile("" ::"v"(Bn2[0]), "v"(Bn2[1]), "v"(Bn2[2]), "v"(Bn2[3]));
          if (ST)
            issue_piece(nb, lb, u >> 2);
          else
            issue_chunk(tt + 2 * NW, sl, u >> 2);
        }
        if (u + PD < 32 && (NCH != 0 || u + PD < 4 * nch))  // slot of window u, consumed two iterations ago
          wq[u % PD] = *reinterpret_cast<const uint32_t*>(xs + 256 * (u + PD) + (((u + PD) & 1) ? boo : boe));
        acc[u] = FX_MFMA(A, Bv, acc[u]);
      }
    }
    FX_STAMP(4);
#if FX_STAMPS
    ++ntl;
#endif
  };
  {
    // steady tiles: tile tt + 2 NW exists and is full (so is tile tt: its target row needs no
    // clamp either), no prediction store
    const int64_t t_full = (n >> 6) - 2 * NW, t_more = (int64_t)te - 2 * NW;
    const int t_st = write_pred ? tt : (int)(t_full < t_more ? t_full : t_more);
    for (; tt < t_st; tt += NW, sl ^= 1) tile(std::true_type{});
  }
  for (; tt < te; tt += NW, sl ^= 1) tile(std::false_type{});
#pragma unroll
  for (int k = 0; k < 4; ++k) R[k] = Rg[k] != 5 ? Rg[k] : 0;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#if FX_STAMPS
  ph[6] = __builtin_amdgcn_s_memrealtime() - rt0;
  ph[7] = __builtin_amdgcn_s_memtime() - mt0;
  if (lane == 0 && st.dbg) {
    for (int i = 0; i < 8; ++i) atomicAdd(&st.dbg[i], ph[i]);
    atomicAdd(&st.dbg[15], ntl);
  }
#endif

  // ---- workgroup reduction (fixed order: deterministic) ----
  {
    const double rs = wave_sum_d(rss);
    float hs[NS];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hs[k] = wave_sum(db[0][k]);
      hs[4 + k] = wave_sum(dWo[k]);
    }
#pragma unroll
    for (int l = 1; l < NH; ++l)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hs[8 + (l - 1) * 20 + k] = wave_sum(db[l][k]);
#pragma unroll
        for (int j = 0; j < 4; ++j) hs[8 + (l - 1) * 20 + 4 + 4 * j + k] = wave_sum(dW[l - 1][j][k]);
      }
    if (lane == 0) {
      s_rss[wave] = rs;
#pragma unroll
      for (int q = 0; q < NS; ++q) s_hs[wave][q] = hs[q];
    }
  }
  __syncthreads();  // every wave is done with its tile slots
  {
    const int Rl = g == 0 ? R[0] : g == 1 ? R[1] : g == 2 ? R[2] : R[3];
    float* red = reinterpret_cast<float*>(&s_x[wave][0][0]);
#pragma unroll
    for (int u = 0; u < 32; ++u)
      if (u < 4 * nch) red[u * 64 + lane] = Rl ? __builtin_amdgcn_ldexpf(comb4_exact2(acc[u], acc3), Rl - 153) : 0.f;
  }
  __syncthreads();
  float* part = st.part + it.part_at;
  // a fused update with more than one workgroup per branch: the partials are handed
  // to the branch's last arriving workgroup inside the launch, stored write-through
  // (sc1: no release fence needed; MI355X_MICROARCH.md, inter-workgroup visibility)
  const bool pub = UPD && upd_cnt != nullptr && (folds != nullptr || bd.nsplits > 1);
  auto pst = [&](float* a, float v) {
    if (pub)
      __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      *a = v;
  };
  float db0[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) db0[k] = (s_hs[0][k] + s_hs[1][k]) + (s_hs[2][k] + s_hs[3][k]);
  const int m = bd.m;
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const int u = wave * 8 + jj;
    if (u < 4 * nch) {
      const int idx = u * 64 + lane;
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) s += reinterpret_cast<const float*>(&s_x[w][0][0])[idx];
      const int mk = 16 * u + i16, c = g;
      if (mk < m && c < bd.widths[0]) {
        const float mu = st.mu[bd.mk_off + mk], sg = st.sigma[bd.mk_off + mk];
        const float dbc = c == 0 ? db0[0] : c == 1 ? db0[1] : c == 2 ? db0[2] : db0[3];
        pst(part + bd.woff[0] + c * m + mk, sg > 0.f ? (s - mu * dbc) / sg : 0.f);
      }
    }
  }
  if (wave == 0 && lane < NS) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += s_hs[w][lane];
    const int q = lane;
    if (q < 4) {
      if (q < bd.widths[0]) pst(part + bd.boff[0] + q, v);
    } else if (q < 8) {
      const int j = q - 4;
      if (j < bd.win[NL - 1]) pst(part + bd.woff[NL - 1] + j, v);
    } else {
      const int l = 1 + (q - 8) / 20, r = (q - 8) % 20;
      if (r < 4) {
        if (r < bd.widths[l]) pst(part + bd.boff[l] + r, v);
      } else {
        const int j = (r - 4) >> 2, k = (r - 4) & 3;
        if (j < bd.win[l] && k < bd.widths[l]) pst(part + bd.woff[l] + k * bd.win[l] + j, v);
      }
    }
  }
  if (wave == 0 && lane == 0) {
    const double rs = (s_rss[0] + s_rss[1]) + (s_rss[2] + s_rss[3]);
    if (pub)
      __hip_atomic_store(st.rss_part + it.rss_at, rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      st.rss_part[it.rss_at] = rs;
  }
  if constexpr (UPD) {
    // fused leapfrog update (bann_plan.hip build_plan): the last of the branch's
    // workgroups to finish updates it here, with the update kernel's arithmetic and
    // reduction order (update_small as 512 virtual threads), instead of a second
    // launch -- after folding the branch's slabs first in a solo plan (folds: the
    // fold launch's order).  A branch of one split (no folds) has one workgroup:
    // this one, whose slab its own waves see after a workgroup barrier.  Otherwise
    // every wave drains its write-through partial stores, one lane counts the
    // arrival (agent scope), and the last arriver acquires before reading the slabs.
    __shared__ int s_last;
    __shared__ double s_redd[4 * 8];
    if (pub) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int narr = folds ? folds[it.fold_ix].nslab : bd.nsplits;
    if (threadIdx.x == 0)
      s_last = !pub || __hip_atomic_fetch_add(&upd_cnt[b], 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == narr - 1;
    __syncthreads();
    if (s_last) {
      if (pub) {
        if (threadIdx.x == 0) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          upd_cnt[b] = 0;  // for the next launch (ordered by the kernel boundary)
        }
        __syncthreads();
      }
      if (folds) {
        fold_solo_all<64 * FX_WAVES>(st, folds[it.fold_ix], bd);
        __syncthreads();  // slab 0 and its rss, written by this workgroup, read by update_small
      }
      float* s_th = reinterpret_cast<float*>(&s_x[0][0][0]);  // the tile slots are free: P <= 2048 floats
      update_small<64 * FX_WAVES, 1, 2>(st, b, bd, upd_mode, false, upd_step, s_redd, s_th);
    }
  }
}

template <int NL, int NCH, int UPD>
static void launch_fx_nlu(const DevState& st, const GradItem* items, int32_t nitems, int act, int wp, int um, int us,
                          int32_t* cnt, const FoldJob* fo, hipStream_t s) {
  const dim3 grid((unsigned)nitems), block(64 * FX_WAVES);
  act_dispatch(act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    hipLaunchKernelGGL((k_fused_grad_fx<NL, ACT, NCH, UPD>), grid, block, 0, s, st, items, wp, um, us, cnt, fo);
  });
}
template <int NL, int NCH>
static void launch_fx_nl(const DevState& st, const GradItem* items, int32_t nitems, int act, int wp, int um, int us,
                         int32_t* cnt, const FoldJob* fo, hipStream_t s) {
  if (cnt)
    launch_fx_nlu<NL, NCH, 1>(st, items, nitems, act, wp, um, us, cnt, fo, s);
  else
    launch_fx_nlu<NL, NCH, 0>(st, items, nitems, act, wp, um, us, nullptr, nullptr, s);
}

// full8: every branch of this launch group has exactly 8 chunks; upd_cnt != null:
// the fused leapfrog update in the launch's tail (mode upd_mode, step upd_step),
// folds != null: a solo plan's fold jobs, run by the tail before the update
void launch_fused_grad_fx(const DevState& st, const GradItem* items, int32_t nitems, int32_t L, int32_t act,
                          int full8, int write_pred, int upd_mode, int upd_step, int32_t* upd_cnt,
                          const FoldJob* folds, hipStream_t s) {
  if (nitems <= 0) return;
  const int wp = write_pred, um = upd_mode, us = upd_step;
  const FoldJob* fo = upd_cnt ? folds : nullptr;
  switch (L * 2 + (full8 ? 1 : 0)) {
    case 4: launch_fx_nl<2, 0>(st, items, nitems, act, wp, um, us, upd_cnt, fo, s); break;
    case 5: launch_fx_nl<2, 8>(st, items, nitems, act, wp, um, us, upd_cnt, fo, s); break;
    case 6: launch_fx_nl<3, 0>(st, items, nitems, act, wp, um, us, upd_cnt, fo, s); break;
    case 7: launch_fx_nl<3, 8>(st, items, nitems, act, wp, um, us, upd_cnt, fo, s); break;
    case 8: launch_fx_nl<4, 0>(st, items, nitems, act, wp, um, us, upd_cnt, fo, s); break;
    case 9: launch_fx_nl<4, 8>(st, items, nitems, act, wp, um, us, upd_cnt, fo, s); break;
    default: break;
  }
}

// Does the immediate offset of global_load_lds_dwordx4 advance the LDS address (M0's base) as well
// as the global one?  One wave copies 4 KiB as four pieces that differ in the offset alone (0, 1024,
// 2048, 3072; one M0) into a 4 KiB array preset to 0xFF, then the array goes out to dst.
__global__ void __launch_bounds__(64) k_glds_offset_probe(const char* __restrict__ src, uint32_t* __restrict__ dst) {
  __shared__ __attribute__((aligned(16))) uint32_t s_p[1024];
  for (int i = threadIdx.x; i < 1024; i += 64) s_p[i] = 0xFFFFFFFFu;
  __syncthreads();
  const uint32_t m0v = __builtin_amdgcn_readfirstlane(lds_off(&s_p[0]));
  const uint32_t voff = threadIdx.x * 16u;
  glds16_so<0>(src, voff, m0v);
  glds16_so<1024>(src, voff, m0v);
  glds16_so<2048>(src, voff, m0v);
  glds16_so<3072>(src, voff, m0v);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int i = threadIdx.x; i < 1024; i += 64) dst[i] = s_p[i];
}

extern "C" int bann_fx_dma_offset_probe(int32_t* lds_follows, int32_t* built_mode) {
  if (!lds_follows || !built_mode) return BANN_E_ARG;
  *built_mode = 2;  // the immediate offset on both addresses, the only mode built
  *lds_follows = -1;
  uint32_t h_src[1024], h_dst[1024];
  for (int i = 0; i < 1024; ++i) h_src[i] = 0x9E3779B1u * (uint32_t)(i + 1) & 0x7FFFFFFFu;  // never 0xFFFFFFFF
  void *d_src = nullptr, *d_dst = nullptr;
  bool ok = hipMalloc(&d_src, 4096) == hipSuccess && hipMalloc(&d_dst, 4096) == hipSuccess &&
            hipMemcpy(d_src, h_src, 4096, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_glds_offset_probe, dim3(1), dim3(64), 0, nullptr, (const char*)d_src, (uint32_t*)d_dst);
    ok = hipGetLastError() == hipSuccess && hipMemcpy(h_dst, d_dst, 4096, hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (d_src) (void)hipFree(d_src);
  if (d_dst) (void)hipFree(d_dst);
  if (!ok) return BANN_E_HIP;
  bool both = true, global_only = true;  // global only: the pieces land on each other, the last one stays
  for (int i = 0; i < 1024; ++i) {
    both = both && h_dst[i] == h_src[i];
    global_only = global_only && h_dst[i] == (i < 256 ? h_src[768 + i] : 0xFFFFFFFFu);
  }
  *lds_follows = both ? 1 : global_only ? 0 : -1;
  return BANN_OK;
}
