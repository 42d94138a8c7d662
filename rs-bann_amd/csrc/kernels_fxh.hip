// kernels_fxh.hip — k_fused_grad_fxh: fxl's one-tile-at-a-time scheme with the head in ONE wave.
//
// fxl repeats the head (hidden / summary / output layers, e, rss, delta0 and
// its digits) in every wave of the workgroup: at C2 (32 chunks, 8 waves) that
// is 8 x ~300 VALU per tile against 8 x 160 for the 2-bit unpack.  Here wave 0
// is the HEAD wave and waves 1 .. NC are COMPUTE waves owning <= 5 chunks each
// (C2: 7 waves of 5,5,5,5,4,4,4), software-pipelined two tiles deep with ONE
// workgroup barrier per phase p:
//   compute waves: backward of tile p - 2 (its delta0 digits published by the
//                  head wave in phase p - 1), then the LDS-DMA of tile
//                  p + NSL - 2 into the slot just freed, then the forward of
//                  tile p -> partial Z0 (f32, the per-column scale applied)
//                  into the exchange slot p % 2;
//   head wave:     the fixed-order sum of the NC partials of tile p - 1, the
//                  transpose to one individual per lane, the head, the delta0
//                  digits at the running per-column scale -> digit image
//                  (p - 1) % 2, with the scale shifts for the compute waves'
//                  digit sums.
// A tile stays resident in its compute waves' slots from its forward (phase
// p) to its backward (p + 2): NSL = 4 slots per wave (one tile two phases
// ahead in flight), 157 KiB of LDS at NC = 7: one workgroup per CU, two waves
// per SIMD, the head wave sharing its SIMD with one compute wave.
// Arithmetic per tile is fxl's (the same digits, int32 digit sums, head in
// f32); the Z0 partials are summed in compute-wave order, so the bits differ
// from fxl only through the partition of the chunks over waves.
// The tile image, FXL_PD and the helpers shared with the other fx-family kernels: fx_tile.h;
// FXH_CPW, FXH_MAXC, FXH_NSL, fxh_lds_bytes and fxh_takes: fx_shapes.h.
#include "activations.h"
#include "bann_internal.h"
#include "fx_shapes.h"
#include "fx_tile.h"

template <int NL, int ACT>
__global__ void __launch_bounds__(64 * (FXH_MAXC + 1), 1)
    k_fused_grad_fxh(DevState st, const GradItem* __restrict__ items, int write_pred, int slot_kib) {
  constexpr int NH = NL - 1;
  constexpr int NS = 8 + (NH - 1) * 20;
  constexpr int NSL = FXH_NSL;
  const int SLOT = __builtin_amdgcn_readfirstlane(slot_kib) * 1024;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int NC = __builtin_amdgcn_readfirstlane((int)(blockDim.x >> 6) - 1);
  char* const s_x = lds;                                                // [NC][NSL][SLOT]
  v4f* const s_zx = reinterpret_cast<v4f*>(s_x + NC * NSL * SLOT);      // [2][NC][64]
  char* const s_d = reinterpret_cast<char*>(s_zx + 2 * NC * 64);        // [2][4 * FX_DROW]
  float* const s_y = reinterpret_cast<float*>(s_d + 2 * 4 * FX_DROW);   // [3][64]
  int* const s_sc = reinterpret_cast<int*>(s_y + 3 * 64);               // [2][8]: shift[4], R[4]
  float* const s_hw = reinterpret_cast<float*>(s_sc + 16);              // [NL][20]
  float* const s_hs = s_hw + NL * 20;                                   // [NS]
  float* const s_db0 = s_hs + NS;                                       // [4]

  const GradItem it = items[blockIdx.x];
  const int b = it.branch;
  const BranchDev& bd = st.br[b];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int64_t n = st.n;
  const int tb = it.frag_begin >> 2, te = (it.frag_end + 3) >> 2;
  const int T = te > tb ? te - tb : 0;
  const int g = lane >> 4, i16 = lane & 15, tq = i16 >> 1, tp = lane & 1;
  float* const part = st.part + it.part_at;

  if (wave == 0) {
    // ================= head wave =================
    const float* th = st.theta + bd.p_off;
    for (int t = lane; t < NL * 20; t += 64) {
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
      s_hw[t] = v;
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    float uW[NL][4][4], uB[NH][4];
#pragma unroll
    for (int l = 0; l < NL; ++l) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
          uW[l][j][k] = (l >= 1 && (l < NL - 1 || k == 0)) ? sgpr_f(s_hw[l * 20 + 4 * j + k]) : 0.f;
      if (l < NH)
#pragma unroll
        for (int k = 0; k < 4; ++k) uB[l][k] = sgpr_f(s_hw[l * 20 + 16 + k]);
    }
    const int iota = 4 * i16 + g;
    // the tile's targets -- or, in network mode, the network's output error (as fx)
    const bool net_err = st.nete != nullptr;
    const float* ybr = net_err ? st.nete : st.y + bd.y_off;
    float* predb = st.pred + bd.y_off;
    auto issue_y = [&](int k) {
      const int64_t row = 64 * (int64_t)(tb + k) + iota;
      glds4(ybr + (row < n ? row : n - 1), s_y + (k % 3) * 64);
    };
    if (T > 0) issue_y(0);
    if (T > 1) issue_y(1);
    const int wp = write_pred != 0;
    const int kslot_sh = 2 * g;  // K-group g's genotype field in place (x 4^g): digits pre-divided
    int R[4] = {0, 0, 0, 0};
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
    for (int p = 0; p < T + 2; ++p) {
      if (p >= 1 && p <= T) {
        const int k = p - 1;
        // y(k) has landed: younger are store(k - 2), y(k + 1), store(k - 1)
        vm_wait<31>(wp * (k >= 2) + (k + 1 < T) + wp * (k >= 1));
        __builtin_amdgcn_s_setprio(1);
        // the NC partials in compute-wave order; FXH_MAXC loads issued together (past NC
        // they re-read the last partial, not added)
        const v4f* xz = s_zx + (k & 1) * NC * 64 + lane;
        v4f zp[FXH_MAXC];
#pragma unroll
        for (int w = 0; w < FXH_MAXC; ++w) zp[w] = xz[(w < NC ? w : NC - 1) * 64];
        v4f zs = zp[0];
#pragma unroll
        for (int w = 1; w < FXH_MAXC; ++w)
          if (w < NC) zs += zp[w];
        float z0 = zs[0], z1 = zs[1], z2 = zs[2], z3 = zs[3];
        swap32(z0, z2);
        swap32(z1, z3);
        swap16(z0, z1);
        swap16(z2, z3);
        const int64_t row = 64 * (int64_t)(tb + k) + iota;
        const bool valid = row < n;
        const float yv = s_y[(k % 3) * 64 + lane];
        if (k + 2 < T) issue_y(k + 2);  // slot (k + 2) % 3 = (k - 1) % 3, read in the previous phase
        float d[4];
        {
          float z[NH][4], a[NH][4];
          z[0][0] = z0 + uB[0][0];
          z[0][1] = z1 + uB[0][1];
          z[0][2] = z2 + uB[0][2];
          z[0][3] = z3 + uB[0][3];
#pragma unroll
          for (int q = 0; q < 4; ++q) a[0][q] = act_h_t<ACT>(z[0][q]);
#pragma unroll
          for (int l = 1; l < NH; ++l) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              float s = uB[l][q];
#pragma unroll
              for (int j = 0; j < 4; ++j) s = fmaf(a[l - 1][j], uW[l][j][q], s);
              z[l][q] = s;
              a[l][q] = act_h_t<ACT>(s);
            }
          }
          float out = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) out = fmaf(a[NH - 1][j], uW[NL - 1][j][0], out);
          const float e = valid ? (net_err ? yv : out - yv) : 0.f;
          rss += (double)e * (double)e;
          float err[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            dWo[j] = fmaf(a[NH - 1][j], e, dWo[j]);
            err[j] = e * uW[NL - 1][j][0];
          }
#pragma unroll
          for (int l = NH - 1; l >= 0; --l) {
            float dl[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              dl[q] = act_dh_t<ACT>(z[l][q], a[l][q]) * err[q];
              db[l][q] += dl[q];
            }
            if (l >= 1) {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                float sj = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  dW[l - 1][j][q] = fmaf(a[l - 1][j], dl[q], dW[l - 1][j][q]);
                  sj = fmaf(dl[q], uW[l][j][q], sj);
                }
                err[j] = sj;
              }
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q) d[q] = dl[q];
            }
          }
          if (wp && valid) predb[row] = out;
        }
        // delta0 -> signed digits at the running per-column scale (fxl's rule)
        int sh[4] = {0, 0, 0, 0};
        {
          bool lane_need = false;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int eq = (int)((fbits(d[q]) >> 23) & 0xFFu);
            lane_need |= eq > (R[q] ? R[q] : 5);
          }
          if (__builtin_amdgcn_ballot_w64(lane_need) != 0) {
            const uint32_t e01 =
                wave_max_u16x2(((fbits(d[0]) >> 23) & 0xFFu) | (((fbits(d[1]) >> 23) & 0xFFu) << 16));
            const uint32_t e23 =
                wave_max_u16x2(((fbits(d[2]) >> 23) & 0xFFu) | (((fbits(d[3]) >> 23) & 0xFFu) << 16));
            const int E[4] = {(int)(e01 & 0xFFFFu), (int)(e01 >> 16), (int)(e23 & 0xFFFFu), (int)(e23 >> 16)};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              if (E[q] >= 6 && (R[q] == 0 || E[q] > R[q])) {
                if (R[q] != 0) sh[q] = E[q] + 2 - R[q];
                R[q] = E[q] + 2;
              }
            }
          }
        }
        v4u w;
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = digits4_fx(d[q], 153 - kslot_sh - (R[q] ? R[q] : 255));
        char* const sd = s_d + (k & 1) * 4 * FX_DROW;
        *reinterpret_cast<v4u*>(sd + (i16 >> 2) * FX_DROW + (4 * g + (i16 & 3)) * 16) = w;
        if (lane == 0) {
          *reinterpret_cast<v4i*>(s_sc + (k & 1) * 8) = v4i{sh[0], sh[1], sh[2], sh[3]};
          *reinterpret_cast<v4i*>(s_sc + (k & 1) * 8 + 4) = v4i{R[0], R[1], R[2], R[3]};
        }
        __builtin_amdgcn_s_setprio(0);
      }
      LDS_BARRIER();
    }
    // head statistics -> the partial slab; sum delta0 per column for the compute waves
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
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
#pragma unroll
      for (int q = 0; q < NS; ++q) s_hs[q] = hs[q];
#pragma unroll
      for (int k = 0; k < 4; ++k) s_db0[k] = hs[k];
      st.rss_part[it.rss_at] = rs;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane < NS) {
      const float v = s_hs[lane];
      const int q = lane;
      if (q < 4) {
        if (q < bd.widths[0]) part[bd.boff[0] + q] = v;
      } else if (q < 8) {
        const int j = q - 4;
        if (j < bd.win[NL - 1]) part[bd.woff[NL - 1] + j] = v;
      } else {
        const int l = 1 + (q - 8) / 20, r = (q - 8) % 20;
        if (r < 4) {
          if (r < bd.widths[l]) part[bd.boff[l] + r] = v;
        } else {
          const int j = (r - 4) >> 2, k = (r - 4) & 3;
          if (j < bd.win[l] && k < bd.widths[l]) part[bd.woff[l] + k * bd.win[l] + j] = v;
        }
      }
    }
    LDS_BARRIER();
    return;
  }

  // ================= compute waves =================
  const int cwi = wave - 1;
  const int nch = bd.nchunks;
  const int cbase = nch / NC, crem = nch - cbase * NC;
  const int c0 = cwi * cbase + (cwi < crem ? cwi : crem);
  const int cw = cbase + (cwi < crem ? 1 : 0);  // 1 .. CPW chunks of this wave
  float zscale = st.fc[b].scale[g];
  const uint32_t gsw = g & 1;
  const uint32_t fo0 = (uint32_t)((16 * g + tq + 8 * gsw) * 16 + 8 * (tp ^ gsw));
  const uint32_t fo1 = (uint32_t)((16 * g + tq + 8 * (1 ^ gsw)) * 16 + 8 * (tp ^ 1 ^ gsw));
  const int pe = i16, po = (i16 + 8) & 15;
  const uint32_t boe = (uint32_t)(pe * 16 + 4 * (2 * ((g >> 1) ^ (pe >> 3)) + (g & 1)));
  const uint32_t boo = (uint32_t)(po * 16 + 4 * (2 * ((g >> 1) ^ (po >> 3)) + (g & 1)));
  const int64_t tile_bytes = (int64_t)nch * 1024;
  const char* xsrc = reinterpret_cast<const char*>(st.xu2) + bd.x_off + (int64_t)c0 * 1024 + lane * 16;
  const char* dsrc = reinterpret_cast<const char*>(st.dig) + bd.dig_off + (int64_t)c0 * 1024 + lane * 16;
  char* const xslot0 = s_x + cwi * NSL * SLOT;
  const char* const sd_r0 = s_d + g * FX_DROW + tq * 16 + 8 * tp;
  // the chunk count as a compile-time constant (4 or 5 for every group fxh_takes: nch in
  // (4 (nw - 1), 4 nw], NC = ceil(4 nw / 5)): no per-chunk / per-window guards, so each
  // phase is one basic block the compiler schedules across (guards collapse the LDS
  // prefetch distance to one window)
  auto run = [&](auto cw_const) {
    constexpr int CW = decltype(cw_const)::value, NWC = 4 * CW;
    auto issue_tile = [&](int k) {
      const int sl = k % NSL;
#pragma unroll
      for (int c = 0; c < CW; ++c)
        glds16(xsrc + (int64_t)(tb + k) * tile_bytes + c * 1024, xslot0 + sl * SLOT + c * 1024);
    };
    v4i Dres[CW];
#pragma unroll
    for (int c = 0; c < CW; ++c) Dres[c] = *reinterpret_cast<const v4i*>(dsrc + c * 1024);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int c = 0; c < CW; ++c) asm volatile("" : "+v"(Dres[c]));
    asm volatile("" : "+v"(zscale));
    v4i rowsum64 = v4i{0, 0, 0, 0};  // facc[3]'s start (field 3 stored as code - 1)
#pragma unroll
    for (int c = 0; c < CW; ++c) rowsum64 = rowsum64_acc(Dres[c], rowsum64);
    for (int k = 0; k < NSL && k < T; ++k) issue_tile(k);  // every slot filled; tile k + NSL refills slot k in B(k)
    v4i acc[NWC];
#pragma unroll
    for (int u = 0; u < NWC; ++u) acc[u] = v4i{0, 0, 0, 0};
    v4i acc3 = v4i{0, 0, 0, 0};  // field 3's -1: 64 sum over K-group 3 of the digits, every marker
    int Rg = 0;  // the running delta0 scale of this lane's column (published by the head wave)

    for (int p = 0; p < T + 2; ++p) {
      // ---- backward of tile p - 2: dW0 digit sums of this wave's chunks += G^T delta0 ----
      if (p >= 2) {
        const int k = p - 2;
        const int* sc = s_sc + (k & 1) * 8;
        const int sh = sc[g];
        Rg = sc[4 + g];
        if (__builtin_amdgcn_ballot_w64(sh != 0) != 0) {
#pragma unroll
          for (int u = 0; u < NWC; ++u) acc[u] = shr_digits(acc[u], sh);
          acc3 = shr_digits(acc3, sh);
        }
        const char* sd_r = sd_r0 + (k & 1) * 4 * FX_DROW;
        const v4i A = lds_tr8_pair(sd_r, sd_r + 8 * 16);
        acc3 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, FX_ONES3, acc3, 0, 0, 0);
        const char* xs = xslot0 + (k % NSL) * SLOT;
        const bool refill = k + NSL < T;  // tile k + NSL into this slot, chunk by chunk
        const char* rsrc = xsrc + (int64_t)(tb + k + NSL) * tile_bytes;
        constexpr int PD = FXL_PD < NWC ? FXL_PD : NWC;
        uint32_t wq[PD];
#pragma unroll
        for (int u = 0; u < PD; ++u) wq[u] = *reinterpret_cast<const uint32_t*>(xs + 256 * u + ((u & 1) ? boo : boe));
        auto unpack = [](uint32_t wv) -> v4i { return fx_bwd_unpack(wv); };
        v4i Bn = unpack(wq[0]), Bn2 = unpack(wq[1]);
#pragma unroll
        for (int u = 0; u < NWC; ++u) {
          const v4i Bv = Bn;
          Bn = Bn2;
          if (u + 2 < NWC) Bn2 = unpack(wq[(u + 2) % PD]);
          if (u + PD < NWC)
            wq[u % PD] = *reinterpret_cast<const uint32_t*>(xs + 256 * (u + PD) + (((u + PD) & 1) ? boo : boe));
          acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, Bv, acc[u], 0, 0, 0);
          // chunk u >> 2's last window (u | 3) was unpacked at u = 4c + 1: its LDS bytes are free
          if ((u & 3) == 1) {
            asm volatile("" ::"v"(Bn2));
            if (refill) glds16(rsrc + (u >> 2) * 1024, xslot0 + (k % NSL) * SLOT + (u >> 2) * 1024);
          }
        }
      }
      // ---- forward of tile p: partial Z0 over this wave's chunks -> exchange slot p % 2 ----
      if (p < T) {
        // pieces younger than tile p's: tiles p + 1 .. min(max(p + NSL - 2, NSL - 1), T - 1) (the
        // prologue's NSL tiles, then one refill per backward, tile p + NSL - 2 in phase p)
        const int hi = p + NSL - 2 > NSL - 1 ? p + NSL - 2 : NSL - 1;
        vm_wait<31>(CW * ((hi < T - 1 ? hi : T - 1) - p));
        const char* xs = xslot0 + (p % NSL) * SLOT;
        v4i facc[4] = {v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, v4i{0, 0, 0, 0}, rowsum64};
        __builtin_amdgcn_s_setprio(1);
        v4u Xc = (v4u)lds_tr8_pair(xs + fo0, xs + fo1);
#pragma unroll
        for (int c = 0; c < CW; ++c) {
          v4u Xn = Xc;
          if (c + 1 < CW) Xn = (v4u)lds_tr8_pair(xs + (c + 1) * 1024 + fo0, xs + (c + 1) * 1024 + fo1);
          fx_fwd_chunk(Dres[c], Xc, facc);
          Xc = Xn;
        }
        fx_fwd_fields(facc);
        const float z0 = zscale * comb4(facc[0]), z1 = (0.25f * zscale) * comb4(facc[1]);
        const float z2 = (0.0625f * zscale) * comb4(facc[2]), z3 = (0.015625f * zscale) * comb4(facc[3]);
        lds_st_v4f(s_zx + ((p & 1) * NC + cwi) * 64 + lane, v4f{z0, z1, z2, z3});
        __builtin_amdgcn_s_setprio(0);
      }
      LDS_BARRIER();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    LDS_BARRIER();  // the head wave's delta0 column sums
    {  // this wave's markers: dW0 = (G^T delta0 - mu sum delta0) / sigma
      const float dbc = s_db0[g];
      const int m = bd.m;
#pragma unroll
      for (int u = 0; u < NWC; ++u) {
        const int mk = 16 * (4 * c0 + u) + i16;
        if (mk < m && g < bd.widths[0]) {
          const float s = Rg ? __builtin_amdgcn_ldexpf(comb4_exact2(acc[u], acc3), Rg - 153) : 0.f;
          const float mu = st.mu[bd.mk_off + mk], sg = st.sigma[bd.mk_off + mk];
          part[bd.woff[0] + g * m + mk] = sg > 0.f ? (s - mu * dbc) / sg : 0.f;
        }
      }
    }
  };
  if (cw == 5)
    run(std::integral_constant<int, 5>{});
  else
    run(std::integral_constant<int, 4>{});
}

template <int NL>
static void launch_fxh_nl(const DevState& st, const GradItem* items, int32_t nitems, int act, int nc, int wp,
                          int slot_kib, hipStream_t s) {
  const dim3 grid((unsigned)nitems), block(64 * (nc + 1));
  const size_t shm = (size_t)fxh_lds_bytes(nc, NL, slot_kib);
  act_dispatch(act, [&](auto a) {
    constexpr int ACT = decltype(a)::value;
    static bool attr_ = false;  // once per kernel instantiation
    if (!attr_) {
      (void)hipFuncSetAttribute((const void*)k_fused_grad_fxh<NL, ACT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                fxh_lds_bytes(FXH_MAXC, 4, FXH_CPW));
      attr_ = true;
    }
    hipLaunchKernelGGL((k_fused_grad_fxh<NL, ACT>), grid, block, shm, s, st, items, wp, slot_kib);
  });
}

// the fxl groups fxh_takes (fx_shapes.h), handed on by launch_fused_grad_fxl: nc compute waves of at most
// slot_kib chunks each, plus the head wave
void launch_fused_grad_fxh(const DevState& st, const GradItem* items, int32_t nitems, int32_t L, int32_t act,
                           int nc, int write_pred, int slot_kib, hipStream_t s) {
  if (nitems <= 0) return;
  if (L == 2) launch_fxh_nl<2>(st, items, nitems, act, nc, write_pred, slot_kib, s);
  if (L == 3) launch_fxh_nl<3>(st, items, nitems, act, nc, write_pred, slot_kib, s);
  if (L == 4) launch_fxh_nl<4>(st, items, nitems, act, nc, write_pred, slot_kib, s);
}
