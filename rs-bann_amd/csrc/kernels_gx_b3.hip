// kernels_gx_b3.hip — the masked layer of the gx path on the bf16 MFMA ("b3"): FWD0
// (Z0 = G Wp_0^T) and GRAD0 (G^T delta0); the path and its phases are described in kernels_gx.hip.
// The genotype codes 0..2 are exact in bf16; the f32 operand x
// is split into three bf16 planes hi + mid + lo (hi = bf16(x), mid =
// bf16(x - hi), lo = bf16(x - hi - mid): 24 significant bits, bf16_planes.h), so one 32-deep
// K step is 3 v_mfma_f32_16x16x32_bf16 (48 cycles) where the f32 MFMA needs 8
// (256 cycles): 5.3x the masked layer's rate, products exact, f32 accumulation
// inside 64-deep K blocks and f64 across them as in k_gx_gemm.  The f32 path
// stays selectable (BANN_GX_EXACT=1: exact f32 products, k_gx_gemm).
// One LDS stage of images [row][k] with 80-element rows (GX_LDH).
#include "bann_internal.h"
#include "bf16_planes.h"
#include "gx_tile.h"
#include "kernel_util.h"

#define GX_LDH 80  // bf16 row stride (elements): 40 dwords, conflict-free row and transposing reads (below)

// K slot of logical k (0..63) of a 64-deep K block in the b3 stages: the K slots
// 8 lq + j of half ks are k = 32 ks + 16 (j >> 2) + 4 lq + (j & 3), so the two
// 16-lane groups of a transposing read (rows 4 lq + tq) take rows 0-3 / 4-7 of an
// 8-row bank window; operands read along their rows store logical K group c (4
// consecutive k) at this element offset
__device__ __forceinline__ int b3_kpos(int c) { return 32 * (c >> 3) + 8 * (c & 3) + 4 * ((c >> 2) & 1); }

// LDS: the genotype chunk as G[marker][individual] (16 consecutive individuals per
// thread: two 16-byte stores; GRAD0, whose K is the individuals, four 8-byte stores
// at b3_kpos); FWD0 takes its A fragments (rows = individuals,
// K = markers) from it by transposing reads and its B fragments from the W0 planes
// [column][marker] (pre-split by k_gx_prep); GRAD0 takes A (rows = markers, K =
// individuals) by row reads and B from the delta0 planes [individual][column]
// (split on staging, 8-byte stores) by transposing reads.
template <int PH>
__global__ void __launch_bounds__(256, PH == GX_GRAD0 ? 3 : 4)
    k_gx_gemm_b3(DevState st, const int32_t* __restrict__ blist, const int32_t* __restrict__ prefix, int nb,
                 int total, int per) {
  __shared__ __attribute__((aligned(16))) __bf16 Gs[GX_T * GX_LDH];     // [marker][individual]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[3][GX_T * GX_LDH];  // FWD0 [column][marker], GRAD0 [individual][column]
  const int q = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);  // XCD-aware numbering (k_gx_gemm)
  if (q >= total) return;
  int lo_ = 0, hi_ = nb;
  while (hi_ - lo_ > 1) {
    const int mid = (lo_ + hi_) >> 1;
    if (prefix[mid] <= q) lo_ = mid;
    else hi_ = mid;
  }
  const int b = blist[lo_];
  const BranchDev& bd = st.br[b];
  int tmc, tnc, ns;
  gx_dims(st.nfrag, bd, PH, 0, tmc, tnc, ns);
  int r = q - prefix[lo_];
  const int split = r / (tmc * tnc);
  r -= split * tmc * tnc;
  const int tm = r / tnc, tn = r % tnc;
  const int64_t rows = gx_rows(st);
  float* S = gx_base(st, bd);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int ar = 32 * (wv >> 1), bc = 32 * (wv & 1);
  const uint8_t* img = st.xu2 + bd.x_off;
  const int64_t tstride = (int64_t)bd.nchunks * 1024;
  const int wo = bd.widths[0];
  const int m64 = 64 * bd.nchunks;
  int kb0 = 0, kb1;
  if constexpr (PH == GX_FWD0) {
    kb1 = bd.nchunks;
  } else {
    const int ntile = (st.nfrag + 3) / 4;
    kb0 = (int)((int64_t)ntile * split / ns);
    kb1 = (int)((int64_t)ntile * (split + 1) / ns);
  }
  const __bf16* W0p = reinterpret_cast<const __bf16*>(S + bd.gx_w0p);
  const float* Dm = S + bd.gx_h[0];
  const int64_t ldd = bd.gx_ld[0];
  Blk rb;
  v4i rw[6];
  uint32_t rg = 0;
  auto load = [&](int kb) {
    if constexpr (PH == GX_FWD0) {
      rg = geno_load(img + (int64_t)tm * tstride + (int64_t)kb * 1024);
#pragma unroll
      for (int u = 0; u < 6; ++u) {  // 3 planes x 64 columns x 8 pieces of 8 markers
        const int e = t + 256 * u, pl = e >> 9, row = (e >> 3) & 63, pc = e & 7;
        const int col = 64 * tn + row;
        v4i v = v4i{0, 0, 0, 0};
        if (col < wo) v = *reinterpret_cast<const v4i*>(W0p + ((int64_t)pl * wo + col) * m64 + 64 * kb + 8 * pc);
        rw[u] = v;
      }
    } else {
      rg = geno_load(img + (int64_t)kb * tstride + (int64_t)tm * 1024);
      blk_load(rb, Dm, ldd, BlkBounds{64 * (int64_t)kb, rows, 64 * tn, wo});
    }
  };
  double csp[4] = {0.0, 0.0, 0.0, 0.0};  // GRAD0: column sums of delta0, columns 4 (t & 15) + x
  float cspf[4] = {0.f, 0.f, 0.f, 0.f};  //   their f32 part since the last f64 sum (with dacc's)
  auto store = [&](int kb) {
    int jl, dq;
    geno_pos(jl, dq);
    {
      bf16x8 v0, v1;
#pragma unroll
      for (int s2 = 0; s2 < 8; ++s2) {
        v0[s2] = (__bf16)(float)((rg >> (2 * s2)) & 3u);
        v1[s2] = (__bf16)(float)((rg >> (2 * s2 + 16)) & 3u);
      }
      if constexpr (PH == GX_FWD0) {
        *(bf16x8*)&Gs[jl * GX_LDH + 16 * dq] = v0;
        *(bf16x8*)&Gs[jl * GX_LDH + 16 * dq + 8] = v1;
      } else {
        *(bf16x4*)&Gs[jl * GX_LDH + b3_kpos(4 * dq)] = bf16x4{v0[0], v0[1], v0[2], v0[3]};
        *(bf16x4*)&Gs[jl * GX_LDH + b3_kpos(4 * dq + 1)] = bf16x4{v0[4], v0[5], v0[6], v0[7]};
        *(bf16x4*)&Gs[jl * GX_LDH + b3_kpos(4 * dq + 2)] = bf16x4{v1[0], v1[1], v1[2], v1[3]};
        *(bf16x4*)&Gs[jl * GX_LDH + b3_kpos(4 * dq + 3)] = bf16x4{v1[4], v1[5], v1[6], v1[7]};
      }
    }
    if constexpr (PH == GX_FWD0) {
#pragma unroll
      for (int u = 0; u < 6; ++u) {
        const int e = t + 256 * u, pl = e >> 9, row = (e >> 3) & 63, pc = e & 7;
        *(v2i*)&Bs[pl][row * GX_LDH + b3_kpos(2 * pc)] = v2i{rw[u][0], rw[u][1]};
        *(v2i*)&Bs[pl][row * GX_LDH + b3_kpos(2 * pc + 1)] = v2i{rw[u][2], rw[u][3]};
      }
    } else {
      blk_fix(rb, BlkBounds{64 * (int64_t)kb, rows, 64 * tn, wo});
#pragma unroll
      for (int u = 0; u < 4; ++u) {  // Bs[p][individual][column], four columns per store
        const int e = t + 256 * u, rr = e >> 4, c4 = 4 * (e & 15);
        bf16x4 h4, m4, l4;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          __bf16 hh, mm, ll;
          split3(rb.v[u][x], hh, mm, ll);
          h4[x] = hh;
          m4[x] = mm;
          l4[x] = ll;
          cspf[x] += rb.v[u][x];
        }
        *(bf16x4*)&Bs[0][rr * GX_LDH + c4] = h4;
        *(bf16x4*)&Bs[1][rr * GX_LDH + c4] = m4;
        *(bf16x4*)&Bs[2][rr * GX_LDH + c4] = l4;
      }
    }
  };

  v4f acc[4];
  double dacc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    acc[x] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int y = 0; y < 4; ++y) dacc[x][y] = 0.0;
  }
  const int tq = li >> 2, tp = li & 3;  // transposing reads: lane 4 tq + tp
  if (kb0 < kb1) load(kb0);
  for (int kb = kb0; kb < kb1; ++kb) {
    store(kb);
    __syncthreads();
    if (kb + 1 < kb1) load(kb + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int ko = 32 * ks + 8 * lq;          // this lane group's 8 K slots (row reads)
      const int kr = 32 * ks + 4 * lq + tq;     // their rows 0-3 (+ 16: 4-7) in transposing reads
      bf16x8 a0, a1;
      if constexpr (PH == GX_FWD0) {  // rows = individuals, K = markers: transposed from Gs
        a0 = tr16_pair(&Gs[kr * GX_LDH + ar + 4 * tp], &Gs[(kr + 16) * GX_LDH + ar + 4 * tp]);
        a1 = tr16_pair(&Gs[kr * GX_LDH + ar + 16 + 4 * tp], &Gs[(kr + 16) * GX_LDH + ar + 16 + 4 * tp]);
      } else {  // rows = markers, K = individuals: row reads
        a0 = *(const bf16x8*)&Gs[(ar + li) * GX_LDH + ko];
        a1 = *(const bf16x8*)&Gs[(ar + 16 + li) * GX_LDH + ko];
      }
#pragma unroll
      for (int pl = 2; pl >= 0; --pl) {  // small planes first
        bf16x8 b0, b1;
        if constexpr (PH == GX_FWD0) {  // B[k = marker][n = column] from Bs[column][marker]
          b0 = *(const bf16x8*)&Bs[pl][(bc + li) * GX_LDH + ko];
          b1 = *(const bf16x8*)&Bs[pl][(bc + 16 + li) * GX_LDH + ko];
        } else {  // B[k = individual][n = column] transposed from Bs[individual][column]
          b0 = tr16_pair(&Bs[pl][kr * GX_LDH + bc + 4 * tp], &Bs[pl][(kr + 16) * GX_LDH + bc + 4 * tp]);
          b1 = tr16_pair(&Bs[pl][kr * GX_LDH + bc + 16 + 4 * tp], &Bs[pl][(kr + 16) * GX_LDH + bc + 16 + 4 * tp]);
        }
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[3], 0, 0, 0);
      }
    }
    if (((kb - kb0) & (GX_F64_BLOCKS - 1)) == GX_F64_BLOCKS - 1 || kb + 1 == kb1) {  // f64 across 256-deep K
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        dacc[x][0] += (double)acc[x].x;
        dacc[x][1] += (double)acc[x].y;
        dacc[x][2] += (double)acc[x].z;
        dacc[x][3] += (double)acc[x].w;
        acc[x] = v4f{0.f, 0.f, 0.f, 0.f};
        if constexpr (PH == GX_GRAD0) {
          csp[x] += (double)cspf[x];
          cspf[x] = 0.f;
        }
      }
    }
    __syncthreads();  // every wave is done with the stage before it is refilled
  }

  if constexpr (PH == GX_FWD0) {
    gx_epilogue<GX_FWD0, true>(st, bd, S, 0, tm, tn, split, 0, wo, ar, bc, li, lq, acc, dacc, 0.0, nullptr);
  } else {
    // column sums: 16 threads per column group, added in thread order (deterministic)
    double* cs_s = reinterpret_cast<double*>(&Bs[0][0]);  // [16][64], the staging is free now
#pragma unroll
    for (int x = 0; x < 4; ++x) cs_s[(t >> 4) * 64 + 4 * (t & 15) + x] = csp[x];
    __syncthreads();
    double* cs_f = reinterpret_cast<double*>(&Gs[0]);  // [64]
    if (t < GX_T) {
      double c = 0.0;
      for (int k = 0; k < 16; ++k) c += cs_s[k * 64 + t];
      cs_f[t] = c;
    }
    __syncthreads();
    float* part = st.part + bd.part_off + (int64_t)split * bd.P;
    const int wi = bd.m, win = bd.m;
    float sgv[2][4], muv[2][4];  // the lane's eight markers, loaded together (index clamped)
#pragma unroll
    for (int X = 0; X < 2; ++X)
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const int ic = min(64 * tm + ar + 16 * X + 4 * lq + y, wi - 1);
        sgv[X][y] = st.sigma[bd.mk_off + ic];
        muv[X][y] = st.mu[bd.mk_off + ic];
      }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int jc = bc + 16 * (x & 1) + li;
      const int j = 64 * tn + jc;
      if (j >= wo) continue;
      const double cs = cs_f[jc];
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        const int i = 64 * tm + ar + 16 * (x >> 1) + 4 * lq + y;
        if (i >= wi) continue;
        const float sg = sgv[x >> 1][y];
        const double v = sg > 0.f ? (dacc[x][y] - (double)muv[x >> 1][y] * cs) / (double)sg : 0.0;
        part[bd.woff[0] + (int64_t)j * win + i] = (float)v;
      }
    }
    if (tm == 0 && t < GX_T && 64 * tn + t < wo) part[bd.boff[0] + 64 * tn + t] = (float)cs_f[t];  // db0
  }
}

void launch_gx_gemm_b3(const DevState& st, int ph, const int32_t* blist, const int32_t* prefix, int nb, int total,
                       int per, hipStream_t s) {
  const dim3 g(8 * per), blk(256);
  if (ph == GX_FWD0) hipLaunchKernelGGL(k_gx_gemm_b3<GX_FWD0>, g, blk, 0, s, st, blist, prefix, nb, total, per);
  else hipLaunchKernelGGL(k_gx_gemm_b3<GX_GRAD0>, g, blk, 0, s, st, blist, prefix, nb, total, per);
}
