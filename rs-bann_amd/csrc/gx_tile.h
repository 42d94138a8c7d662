// gx_tile.h — the device helpers that more than one file of the gx path uses: k_gx_gemm
// and k_gx_gemm_x3 (kernels_gx.hip), k_gx_gemm_b3 (kernels_gx_b3.hip) and the prep /
// head kernels (kernels_gx_head.hip).  The branch's scratch, the staging of a 64 x 64 f32 block and of
// a genotype chunk into LDS, h' as a function of the activation, and the epilogue of an output tile.
// The tile numbering is gx_dims (gx_shapes.h), the bf16 planes are in bf16_planes.h.
#pragma once
#include <type_traits>

#include "activations.h"
#include "bann_internal.h"
#include "gx_shapes.h"
#include "kernel_util.h"

#define GX_T 64   // output tile edge of k_gx_gemm and k_gx_gemm_b3, their K block depth; rows per head tile
#define GX_LD 68  // f32 LDS row stride (floats) of the stages below
// bf16-plane kernels: 64-deep K blocks of f32 accumulation before the f64 sum (256 rows / markers; settled in round 3)
constexpr int GX_F64_BLOCKS = 4;

__device__ __forceinline__ int64_t gx_rows(const DevState& st) { return (int64_t)((st.nfrag + 3) / 4) * 64; }
__device__ __forceinline__ float* gx_base(const DevState& st, const BranchDev& bd) { return st.scr + bd.scr_off; }

// a 64 x 64 block of a row-major f32 matrix M[r][c] (row stride ld, a multiple of
// 4): element (r, c) of the block = M[r0 + r][c0 + c] when r0 + r < rmax and
// c0 + c < cmax, else 0.  Thread t holds rows (t + 256 u) >> 4, columns 4 (t & 15).
// The loads are only issued here; the edge masking waits until blk_fix, after the
// K block's MFMAs (masking right after the load would make the compiler wait for
// the data there and expose the full memory latency every block).  blk_fix
// recomputes the bounds instead of keeping them in registers.
struct Blk {
  v4f v[4];
};
struct BlkBounds {
  int64_t r0, rmax;
  int c0, cmax;
};
__device__ __forceinline__ int blk_nv(const BlkBounds& k, int u) {
  const int e = threadIdx.x + 256 * u;
  const int64_t r = k.r0 + (e >> 4);
  const int c = k.c0 + 4 * (e & 15);
  return r < k.rmax ? min(max(k.cmax - c, 0), 4) : 0;
}
__device__ __forceinline__ void blk_load(Blk& s, const float* __restrict__ M, int64_t ld, const BlkBounds& k) {
  const int t = threadIdx.x;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = t + 256 * u;
    v4f x = {0.f, 0.f, 0.f, 0.f};
    if (blk_nv(k, u) > 0) x = *(const v4f*)(M + (k.r0 + (e >> 4)) * ld + k.c0 + 4 * (e & 15));  // rows padded to 4
    s.v[u] = x;
  }
}
__device__ __forceinline__ void blk_fix(Blk& s, const BlkBounds& k) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int nv = blk_nv(k, u);
    if (nv < 2) s.v[u].y = 0.f;
    if (nv < 3) s.v[u].z = 0.f;
    if (nv < 4) s.v[u].w = 0.f;
  }
}
// LDS [r][c] (the block's rows are the MFMA rows, its columns the K index)
__device__ __forceinline__ void blk_store(Blk& s, const BlkBounds& k, float* L) {
  blk_fix(s, k);
  const int t = threadIdx.x;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = t + 256 * u;
    *(v4f*)(L + (e >> 4) * GX_LD + 4 * (e & 15)) = s.v[u];
  }
}
// LDS [c][r] (the block's columns are the MFMA rows, its rows the K index)
__device__ __forceinline__ void blk_store_t(Blk& s, const BlkBounds& k, float* L) {
  blk_fix(s, k);
  const int t = threadIdx.x;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = t + 256 * u;
    const int r = e >> 4, c = 4 * (e & 15);
    L[(c + 0) * GX_LD + r] = s.v[u].x;
    L[(c + 1) * GX_LD + r] = s.v[u].y;
    L[(c + 2) * GX_LD + r] = s.v[u].z;
    L[(c + 3) * GX_LD + r] = s.v[u].w;
  }
}

// one 1 KiB chunk image (64 marker rows x 64 individuals of one tile; u2t layout,
// fx_tile.h): thread t holds the dword at byte 4 t -- physical row
// position pos = t >> 2, i.e. logical marker row 16 w + ((P - 8 (w & 1)) & 15)
// (w = pos >> 4, P = pos & 15), and individuals 16 dq .. 16 dq + 15 at bits 2 s,
// dq = (t & 3) ^ (P >= 8 ? 2 : 0) (the swapped 8-byte halves).
__device__ __forceinline__ uint32_t geno_load(const uint8_t* __restrict__ img) {
  return *(const uint32_t*)(img + 4 * threadIdx.x);
}
__device__ __forceinline__ void geno_pos(int& jl, int& dq) {
  const int t = threadIdx.x, pos = t >> 2, w = pos >> 4, P = pos & 15;
  jl = 16 * w + ((P - 8 * (w & 1)) & 15);
  dq = (t & 3) ^ ((P >> 3) << 1);
}
// LDS [individual][marker] (FWD0: individuals are the MFMA rows)
__device__ __forceinline__ void geno_store_im(uint32_t g, float* L) {
  int jl, dq;
  geno_pos(jl, dq);
#pragma unroll
  for (int s = 0; s < 16; ++s) L[(16 * dq + s) * GX_LD + jl] = (float)((g >> (2 * s)) & 3u);
}
// LDS [marker][individual] (GRAD0: markers are the MFMA rows)
__device__ __forceinline__ void geno_store_mi(uint32_t g, float* L) {
  int jl, dq;
  geno_pos(jl, dq);
  float* p = L + jl * GX_LD + 16 * dq;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint32_t b = g >> (8 * q);
    *(v4f*)(p + 4 * q) = v4f{(float)(b & 3u), (float)((b >> 2) & 3u), (float)((b >> 4) & 3u), (float)((b >> 6) & 3u)};
  }
}

// a lane of the same row of 16 (DPP control CTRL)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// h'(z) as a function of a = h(z) for the activations where it is one (tanh:
// 1 - a^2; ReLU / leaky ReLU: a > 0 <=> z > 0; identity): those layers store A_l
// only, and the backward phases form H_l from it (SiLU keeps H_l)
__device__ __forceinline__ bool dh_from_a(int act) { return act != 3; }
// the same without branches: h' = base(a) - tq a^2 with base = bp (a > 0), bn (a < 0),
// bz (a = 0) and the four constants of the activation (identical values)
struct DhA {
  float tq, bp, bn, bz;
};
__device__ __forceinline__ DhA dh_a_consts(int act) {
  switch (act) {
    case 0: return DhA{1.f, 1.f, 1.f, 1.f};
    case 1: return DhA{0.f, 1.f, 0.f, 0.f};
    case 2: return DhA{0.f, 1.f, 0.01f, 0.f};
    default: return DhA{0.f, 1.f, 1.f, 1.f};
  }
}
__device__ __forceinline__ float dh_a(float a, const DhA& k) {
  const float base = a > 0.f ? k.bp : (a < 0.f ? k.bn : k.bz);
  return k.tq != 0.f ? 1.f - a * a : base;
}
__device__ __forceinline__ float act_dh_a(float a, int act) {
  switch (act) {
    case 0: return 1.f - a * a;
    case 1: return a > 0.f ? 1.f : 0.f;
    case 2: return a > 0.f ? 1.f : (a < 0.f ? 0.01f : 0.f);
    default: return 1.f;
  }
}

// BWD: the h' operands of the lane's outputs (A_{l-1}, or H_{l-1} for SiLU), column
// and row clamped into the layer (the clamped ones are not used)
template <int AX, int AY>
__device__ __forceinline__ void gx_bwd_hload(const DevState& st, const BranchDev& bd, const float* S, int l, int tm,
                                             int tn, int wo, int ar, int bc, int li, int lq, float* hv) {
  constexpr int TM = 32 * AX, TN = 32 * AY;
  const int64_t rmax = gx_rows(st);
  const float* Hsrc = S + (dh_from_a(bd.act) ? bd.gx_a[l - 1] : bd.gx_h[l - 1]);
  const int64_t ld = bd.gx_ld[l - 1];
#pragma unroll
  for (int x = 0; x < AX * AY; ++x) {
    const int X = x / AY, Y = x % AY;
    const int jc = min(TN * tn + bc + 16 * Y + li, wo - 1);
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int64_t row = min(TM * (int64_t)tm + ar + 16 * X + 4 * lq + y, rmax - 1);
      hv[4 * x + y] = Hsrc[row * ld + jc];
    }
  }
}

// the epilogue of a TM x TN output tile (TM = 32 AX, TN = 32 AY; 64 x 64 unless
// k_gx_gemm_x3 says otherwise): lane holds rows ar + 16 X + 4 lq + y and columns
// bc + 16 Y + li of accumulator x = AY X + Y (f32 acc, or the f64 dacc when F64).
// FWD0 / FWD: A = h(Z + b), H = h'(Z + b); BWD: delta_{l-1} = H * acc in place;
// GRAD / GRAD0: the weight gradient into the split's partial slab (GRAD0 with the
// standardisation, column sums cs_col of delta0 in LDS) and, in the tm == 0 tiles,
// db from the column sum cs of thread t < TN.
template <int PH, bool F64, int AX = 2, int AY = 2>
__device__ __forceinline__ void gx_epilogue(const DevState& st, const BranchDev& bd, float* S, int l, int tm, int tn,
                                            int split, int wi, int wo, int ar, int bc, int li, int lq,
                                            const v4f (&acc)[AX * AY], const double (&dacc)[AX * AY][4], double cs,
                                            const double* cs_col, bool lazy = false, double cs2 = 0.0,
                                            const float* pre = nullptr) {
  constexpr int TM = 32 * AX, TN = 32 * AY;
  const int t = threadIdx.x;
  const int64_t rmax = gx_rows(st);  // FWD / BWD: rows past the last tile (TM = 128) are not written
  if constexpr (PH == GX_FWD0 || PH == GX_FWD) {
    const int lay = PH == GX_FWD0 ? 0 : l;
    const float* bias = S + bd.gx_b[lay];
    float* Ao = S + bd.gx_a[lay];
    float* Ho = S + bd.gx_h[lay];
    const int64_t ld = bd.gx_ld[lay];
    // the summary layer (lazy head, k_gx_head): the wave's partial of out = A_s w_out
    // over its TN / 2 columns, per row
    const bool head = PH == GX_FWD && l == bd.L - 2 && dh_from_a(bd.act);
    const float* wout = S + bd.gx_w[bd.L - 1];
    float po[AX][4];
#pragma unroll
    for (int X = 0; X < AX; ++X) po[X][0] = po[X][1] = po[X][2] = po[X][3] = 0.f;
    // the lane's columns' bias and w_out (pre: loaded by the caller before its K loop)
    float bq[AY], wq[AY];
#pragma unroll
    for (int Y = 0; Y < AY; ++Y) {
      const int j = TN * tn + bc + 16 * Y + li;
      bq[Y] = pre ? pre[Y] : (j < wo ? bias[j] : 0.f);
      wq[Y] = pre ? pre[AY + Y] : (head && j < wo ? wout[j] : 0.f);
    }
    // the activation as a compile-time kind (activations.h)
    auto out = [&](auto kind) {
      constexpr int ACT = decltype(kind)::value;
#pragma unroll
      for (int x = 0; x < AX * AY; ++x) {
        const int X = x / AY, Y = x % AY;
        const int j = TN * tn + bc + 16 * Y + li;
        if (j >= wo) continue;
        const float bj = bq[Y];
        const float wj = wq[Y];
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          const int64_t row = TM * (int64_t)tm + ar + 16 * X + 4 * lq + y;
          if (TM > 64 && row >= rmax) continue;
          const float z = (F64 ? (float)dacc[x][y] : acc[x][y]) + bj;  // mid_layer_pre_activation: matmul + bias
          const float a = ACT == 0 ? fast_tanh(z) : act_h_t<ACT>(z);  // tanh to ~2 ulp (layer outputs feed GEMMs)
          Ao[row * ld + j] = a;
          if constexpr (ACT == 3) Ho[row * ld + j] = act_dh_t<ACT>(z, a);
          po[X][y] += a * wj;  // columns 16 Y + li, Y in order
        }
      }
    };
    switch (bd.act) {
      case 0: out(std::integral_constant<int, 0>{}); break;
      case 1: out(std::integral_constant<int, 1>{}); break;
      case 2: out(std::integral_constant<int, 2>{}); break;
      case 3: out(std::integral_constant<int, 3>{}); break;
      default: out(std::integral_constant<int, 4>{}); break;
    }
    if (head) {  // fixed butterfly over the 16 column lanes; lane li = 0 writes slot 2 tn + (column half)
      float* op = S + bd.gx_op + (int64_t)(2 * tn + (bc != 0 ? 1 : 0)) * rmax;
#pragma unroll
      for (int X = 0; X < AX; ++X)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          float v = po[X][y];
          v += dpp_f<0xB1>(v);   // quad_perm [1, 0, 3, 2]
          v += dpp_f<0x4E>(v);   // quad_perm [2, 3, 0, 1]
          v += dpp_f<0x141>(v);  // row_half_mirror
          v += dpp_f<0x140>(v);  // row_mirror: every lane of the 16 holds the same sum
          const int64_t row = TM * (int64_t)tm + ar + 16 * X + 4 * lq + y;
          if (li == 0 && (TM == 64 || row < rmax)) op[row] = v;
        }
    }
  } else if constexpr (PH == GX_BWD) {
    float* Hd = S + bd.gx_h[l - 1];
    const float* Ad = S + bd.gx_a[l - 1];
    const int64_t ld = bd.gx_ld[l - 1];
    const int act = bd.act;
    const bool fa = dh_from_a(act);
    // every h' operand is loaded first, unconditionally (gx_bwd_hload), so the loads
    // issue back to back: one memory latency per tile instead of one per guarded
    // group (BWD1 at c3def: 3.2 -> 2.9 ms per group).  Measured and not kept: the
    // same loads issued during the last K block's MFMAs (3.27 ms)
    float hv[AX * AY][4];
    gx_bwd_hload<AX, AY>(st, bd, S, l, tm, tn, wo, ar, bc, li, lq, &hv[0][0]);
#pragma unroll
    for (int x = 0; x < AX * AY; ++x) {
      const int X = x / AY, Y = x % AY;
      const int j = TN * tn + bc + 16 * Y + li;
      if (j >= wo) continue;
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const int64_t row = TM * (int64_t)tm + ar + 16 * X + 4 * lq + y;
        if (TM > 64 && row >= rmax) continue;
        const float h = fa ? act_dh_a(hv[x][y], act) : hv[x][y];
        // delta = h'(z) * (delta_next W^T); lazy head: the accumulator lacks e of the row
        Hd[row * ld + j] = h * (lazy ? pre[4 * X + y] * acc[x][y] : acc[x][y]);
      }
    }
  } else {
    float* part = st.part + bd.part_off + (int64_t)split * bd.P;
    const int lay = PH == GX_GRAD ? l : 0;
    const int win = bd.win[lay];
    // GRAD0: sigma and mu of the lane's 4 AX markers, loaded together (index clamped)
    float sgv[AX][4], muv[AX][4];
    if constexpr (PH == GX_GRAD0) {
#pragma unroll
      for (int X = 0; X < AX; ++X)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          const int ic = min(TM * tm + ar + 16 * X + 4 * lq + y, wi - 1);
          sgv[X][y] = st.sigma[bd.mk_off + ic];
          muv[X][y] = st.mu[bd.mk_off + ic];
        }
    }
#pragma unroll
    for (int x = 0; x < AX * AY; ++x) {
      const int X = x / AY, Y = x % AY;
      const int j = TN * tn + bc + 16 * Y + li;
      if (j >= wo) continue;
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const int i = TM * tm + ar + 16 * X + 4 * lq + y;
        if (i >= wi) continue;
        double v = dacc[x][y];
        if (PH == GX_GRAD && lazy) v *= (double)pre[Y];  // lazy head: times w_out of the column
        if constexpr (PH == GX_GRAD0) {  // X = (g - mu) / sigma; zero-variance markers contribute 0
          const float sg = sgv[X][y];
          v = sg > 0.f ? (v - (double)muv[X][y] * cs_col[bc + 16 * Y + li]) / (double)sg : 0.0;
        }
        part[bd.woff[lay] + (int64_t)j * win + i] = (float)v;  // param_vec: W_l[out j][in i]
      }
    }
    if (tm == 0 && t < TN && TN * tn + t < wo) {
      part[bd.boff[lay] + TN * tn + t] = (float)cs;                // db_l
      if (lazy) part[bd.woff[bd.L - 1] + TN * tn + t] = (float)cs2;  // dW_out = A_s^T e (lazy head)
    }
  }
}
