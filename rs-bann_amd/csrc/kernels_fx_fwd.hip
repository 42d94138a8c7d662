// kernels_fx_fwd.hip — the forward-only fx pass: f_b(theta) of every individual (forward_feed,
// branch_sampler.rs:743-782, at the output neuron), no target, no backward.
// Network-joint HMC needs the summed branch outputs before any branch can form
// its output error, so each of its leapfrog steps starts with this pass; the
// prediction paths (bann_predict*, stale rows before a target rebuild) use it
// too.  Same tiles, work items, W0 digits and head as k_fused_grad_fx; the
// stream runs two tiles ahead in the wave's two slots, the refill of a slot is
// issued once the forward has read it (the head's prediction store first, so
// the counted wait at the top never waits on a piece younger than the tile).
// Variants measured against this forward and not kept: DESIGN.md section 9.
// The tile image and the helpers shared with the other fx-family kernels: fx_tile.h.
#include "activations.h"
#include "bann_internal.h"
#include "fx_tile.h"

constexpr int FWD_NU = 3;  // 8-chunk tiles: half-tile units per wave (tiles of fewer chunks: 0, whole-tile slots)

// NU > 0 (8-chunk tiles): the half-tile ring, NU units of 4 KiB per wave and the W0 digits in
// registers (no LDS copy), so that 4 NU KiB per wave set the workgroups per CU
template <int NL, int ACT, int NCH, int NU>
__global__ void __launch_bounds__(64 * FX_WAVES, 2)
    k_forward_fx(DevState st, const GradItem* __restrict__ items) {
  constexpr int NH = NL - 1;
  constexpr int NW = FX_WAVES;
  constexpr int NS = 2;  // whole-tile ring (NU == 0): tile slots per wave, the stream runs NS tiles ahead
  static_assert(NU == 0 || NCH == 8, "the half-tile ring needs 8-chunk tiles");
  __shared__ __attribute__((aligned(16))) char s_x[NW][NU > 0 ? 1 : NS][NU > 0 ? NU * 4096 : FX_SLOT];
  __shared__ __attribute__((aligned(16))) char s_w0[NU > 0 ? 16 : 8 * 1024];
  __shared__ __attribute__((aligned(16))) float s_hw[NL][20];

  const GradItem it = items[blockIdx.x];
  const int b = it.branch;
  const BranchDev& bd = st.br[b];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nch = NCH ? NCH : bd.nchunks;
  const int64_t n = st.n;
  const int tb = it.frag_begin >> 2, te = (it.frag_end + 3) >> 2;

  const float* th = st.theta + bd.p_off;
  for (int t = threadIdx.x; t < NL * 20; t += 64 * NW) {
    const int l = t / 20, r = t - l * 20;
    float v = 0.f;
    if (r < 16) {
      const int j = r >> 2, k = r & 3;
      if (l >= 1 && j < bd.win[l] && k < bd.widths[l]) v = th[bd.woff[l] + k * bd.win[l] + j];
    } else {
      const int k = r - 16;
      if (l == 0 && k < bd.widths[0]) v = st.fc[b].c0[k];
      if (l >= 1 && l < NH && k < bd.widths[l]) v = th[bd.boff[l] + k];
    }
    s_hw[l][r] = v;
  }
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 1, tp = lane & 1;
  float zk = fx_zk(st.fc[b].scale[g]);
  v4i Areg[NU > 0 ? 8 : 1];  // the ring's W0 digit operands, one per chunk
  if constexpr (NU > 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) Areg[c] = *reinterpret_cast<const v4i*>(st.dig + bd.dig_off + ((int64_t)c * 64 + lane) * 16);
  } else {
    for (int c = wave; c < nch; c += NW)
      *reinterpret_cast<v4i*>(&s_w0[c * 1024 + lane * 16]) =
          *reinterpret_cast<const v4i*>(st.dig + bd.dig_off + ((int64_t)c * 64 + lane) * 16);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("" : "+v"(zk));
  __syncthreads();
  const float zbias = s_hw[0][16 + g];  // the lane's column bias c0 (fx_z0_cum)
  v4i rowsum64 = v4i{0, 0, 0, 0};  // facc[3]'s start (field 3 stored as code - 1)
  if constexpr (NU > 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) rowsum64 = rowsum64_acc(Areg[c], rowsum64);
  } else {
    for (int c = 0; c < nch; ++c) rowsum64 = rowsum64_acc(*reinterpret_cast<const v4i*>(&s_w0[c * 1024 + lane * 16]), rowsum64);
  }
  float uWm[NL][4][4], uB[NH][4];  // head weights W_l[j][k] (l >= 1; output layer: k = 0) and biases, scalar
#pragma unroll
  for (int l = 0; l < NL; ++l) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k)
        uWm[l][j][k] = (l >= 1 && (l < NL - 1 || k == 0)) ? sgpr_f(s_hw[l][4 * j + k]) : 0.f;
    if (l < NH)
#pragma unroll
      for (int k = 0; k < 4; ++k) uB[l][k] = sgpr_f(s_hw[l][16 + k]);
  }

  const int gsw = g & 1;
  const uint32_t fo0 = (uint32_t)((16 * g + tq + 8 * gsw) * 16 + 8 * (tp ^ gsw));
  const uint32_t fo1 = (uint32_t)((16 * g + tq + 8 * (1 ^ gsw)) * 16 + 8 * (tp ^ 1 ^ gsw));
  const int iota = 4 * i16 + g;
  float* predb = st.pred + bd.y_off;
  const char* xsrc = reinterpret_cast<const char*>(st.xu2) + bd.x_off + lane * 16;
  const int64_t tile_bytes = (int64_t)nch * 1024;
  // the last chunk's padding rows are not streamed (as in k_fused_grad_fx)
  const bool pad_row = 64 * (nch - 1) + 16 * (lane >> 4) + (((lane & 15) - 8 * ((lane >> 4) & 1)) & 15) >= bd.m;
  auto issue_chunk = [&](int tt, int sl, int c) {
    if (c == nch - 1 && pad_row) return;
    if constexpr (NU == 0) glds16(xsrc + (int64_t)tt * tile_bytes + c * 1024, &s_x[wave][sl][c * 1024]);
  };

  // the head of one tile: in-place fields -> z (one individual per lane) -> f
  auto head_out = [&](v4i (&facc)[4]) -> float {
    float z0, z1, z2, z3;  // with the first-layer bias
    fx_z0_cum(facc, zk, zbias, z0, z1, z2, z3);
    swap32(z0, z2);
    swap32(z1, z3);
    swap16(z0, z1);
    swap16(z2, z3);
    float a[4];
    a[0] = act_h_t<ACT>(z0);
    a[1] = act_h_t<ACT>(z1);
    a[2] = act_h_t<ACT>(z2);
    a[3] = act_h_t<ACT>(z3);
#pragma unroll
    for (int l = 1; l < NH; ++l) {
      float an[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float s = uB[l][k];
#pragma unroll
        for (int j = 0; j < 4; ++j) s = fmaf(a[j], uWm[l][j][k], s);
        an[k] = act_h_t<ACT>(s);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = an[k];
    }
    float out = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) out = fmaf(a[j], uWm[NL - 1][j][0], out);
    return out;
  };
  if constexpr (NU > 0) {
    // Half-tile ring: NU slots of one 4-chunk unit each (unit u = half u & 1 of the wave's
    // tile u >> 1); NU - 1 units are in flight while one is read.  A wave owns a contiguous
    // run of the item's tiles and writes its predictions PB tiles at a time (PB x 256 bytes,
    // back to back): single 256-byte stores between the stream's reads cost the launch a
    // fifth of its time (profiles/r05_fwd_store_ablation.md).
    constexpr int PB = 8;
    char* const xw = &s_x[wave][0][0];
    const int q = (te - tb + NW - 1) / NW;
    const int tw0 = tb + wave * q;
    const int nt = te - tw0 < 0 ? 0 : (te - tw0 < q ? te - tw0 : q);
    const int nu = 2 * nt;
    auto issue_unit = [&](int u) {
      const int64_t tt = tw0 + (u >> 1);
      char* dst = xw + (u % NU) * 4096;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int cc = 4 * (u & 1) + c;
        if (cc == nch - 1 && pad_row) continue;
        glds16(xsrc + tt * tile_bytes + cc * 1024, dst + c * 1024);
      }
    };
    for (int u = 0; u < NU && u < nu; ++u) issue_unit(u);
    for (int k0 = 0; k0 < nt; k0 += PB) {
      float obuf[PB];
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        const int k = k0 + j;
        obuf[j] = 0.f;
        if (k >= nt) break;
        v4i facc[4] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, rowsum64};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int u = 2 * k + h;
          // younger than unit u: the units issued after it (through u + NU - 1), four pieces each
          // (vector memory operations leave vmcnt in issue order on gfx9).  The bursts' prediction
          // stores are not counted, so a wait issued behind a burst also waits for its stores;
          // counting them measured slower inside the trajectory
          const int last = u + NU - 1 < nu - 1 ? u + NU - 1 : nu - 1;
          vm_wait<31>(4 * (last - u));
          const char* xs = xw + (u % NU) * 4096;
          v4u Xq[2];
#pragma unroll
          for (int c = 0; c < 2; ++c) Xq[c] = (v4u)lds_tr8_pair(xs + c * 1024 + fo0, xs + c * 1024 + fo1);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const v4u Xc = Xq[c % 2];
            if (c + 2 < 4) Xq[c % 2] = (v4u)lds_tr8_pair(xs + (c + 2) * 1024 + fo0, xs + (c + 2) * 1024 + fo1);
            fx_fwd_chunk(Areg[4 * h + c], Xc, facc);
            __builtin_amdgcn_sched_barrier(0);
          }
          // every read of this unit's slot has returned (the MFMAs consumed them): refill it
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (u + NU < nu) issue_unit(u + NU);
        }
        __builtin_amdgcn_sched_barrier(0);
        obuf[j] = head_out(facc);
      }
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        const int64_t row = 64 * (int64_t)(tw0 + k0 + j) + iota;
        if (k0 + j < nt && row < n) predb[row] = obuf[j];
      }
    }
  } else {
  // ring of NS slots: tile i of this wave in slot i % NS; the prologue fills the
  // ring, each iteration refills the slot it consumed with the tile NS ahead
  int tt = tb + wave, sl = 0;
  for (int j = 0; j < NS; ++j)
    if (tt + j * NW < te)
      for (int c = 0; c < nch; ++c) issue_chunk(tt + j * NW, j, c);
  for (; tt < te; tt += NW, sl = (sl + 1) % NS) {
    int ahead = 0;  // later tiles of the ring in flight: their pieces are younger than this tile's
    for (int j = 1; j < NS; ++j) ahead += tt + j * NW < te;
    vm_wait<31>(ahead * nch);
    const char* xs = &s_x[wave][sl][0];
    v4i facc[4] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, rowsum64};
    {
      constexpr int FD = 2;
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
        fx_fwd_chunk(Ac, Xc, facc);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      const float out = head_out(facc);
      const int64_t row = 64 * (int64_t)tt + iota;
      if (row < n) predb[row] = out;
    }
    // every read of this slot has returned (the MFMAs consumed them): refill it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (tt + NS * NW < te)
      for (int c = 0; c < nch; ++c) issue_chunk(tt + NS * NW, sl, c);
  }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int NL, int NCH>
static void launch_fwd_nl(const DevState& st, const GradItem* items, int32_t nitems, int act, hipStream_t s) {
  const dim3 grid((unsigned)nitems), block(64 * FX_WAVES);
  act_dispatch(act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    hipLaunchKernelGGL((k_forward_fx<NL, ACT, NCH, NCH == 8 ? FWD_NU : 0>), grid, block, 0, s, st, items);
  });
}

void launch_forward_fx(const DevState& st, const GradItem* items, int32_t nitems, int32_t L, int32_t act, int full8,
                       hipStream_t s) {
  if (nitems <= 0) return;
  switch (L * 2 + (full8 ? 1 : 0)) {
    case 4: launch_fwd_nl<2, 0>(st, items, nitems, act, s); break;
    case 5: launch_fwd_nl<2, 8>(st, items, nitems, act, s); break;
    case 6: launch_fwd_nl<3, 0>(st, items, nitems, act, s); break;
    case 7: launch_fwd_nl<3, 8>(st, items, nitems, act, s); break;
    case 8: launch_fwd_nl<4, 0>(st, items, nitems, act, s); break;
    case 9: launch_fwd_nl<4, 8>(st, items, nitems, act, s); break;
    default: break;
  }
}
