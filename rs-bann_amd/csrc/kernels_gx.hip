// kernels_gx.hip — "gx": the layered gradient path for every branch shape the
// fused single-pass kernels do not take (fx/fxl: every width <= 4; wx: one hidden
// layer <= 32 x 32 over <= 128 markers): any depth, any widths, any marker count
// -- among them the reference's default architecture, hidden and summary widths
// m_b / 2 (cli.rs:365-375, rs-bann.rs:433-435).
//
// BranchSampler::backpropagate (branch_sampler.rs:813-875) with forward_feed
// (743-782) as a chain of batched GEMMs over the branches of one scratch group,
// accumulating in f32 inside K blocks and in f64 across them where K is long (m
// markers, n individuals), so those reductions do not grow the f32 error with K:
//   PREP    Wp_l = W_l as [out][in] rows padded to 4; Wp_0 = W0 / sigma and
//           c0 = b0 - sum_j mu_j Wp_0[.][j] (f64): standardisation folded into W0;
//           the same weights as three bf16 planes for the bf16-plane kernels
//   FWD0    Z0 = G Wp_0^T + c0 (G decoded from the 2-bit tile image)   -> A0 = h(Z0), H0 = h'(Z0)
//   FWD l   Z_l = A_{l-1} Wp_l^T + b_l                                  -> A_l, H_l
//           (H_l = h'(Z_l) is stored for SiLU only: for tanh, ReLU, leaky ReLU and
//           identity h' is a function of A_l, formed where it is used)
//   HEAD    out = A_s w_out (775-782), e = out - y, rss (823-828), pred,
//           dW_out = A_s^T e (830-835), delta_s = H_s * e w_out (844-847, in place over H_s)
//   BWD l   delta_{l-1} = H_{l-1} * (delta_l Wp_l)          (855-861, in place over H_{l-1})
//   GRAD l  dW_l = A_{l-1}^T delta_l, db_l = 1^T delta_l    (849-852; K = individuals, row splits)
//   GRAD0   dW0 = (G^T delta0 - mu (1^T delta0)) / sigma, db0 (863-866)
//
// Three GEMM kernels; launch_gx_gemm below picks per phase:
//   phase               default                                 BANN_GX_EXACT=1
//   FWD0, GRAD0         k_gx_gemm_b3 (kernels_gx_b3.hip)        k_gx_gemm (this file)
//   FWD, BWD, GRAD l    k_gx_gemm_x3 (this file)                k_gx_gemm
// (k_gx_gemm_x3 shares this file with k_gx_gemm because their BWD instantiations share one
// instantiation of gx_epilogue: alone in a file, k_gx_gemm<GX_BWD> compiles to other
// instructions, profiles/gx_split_refactor.md.)
// k_gx_gemm_b3 and k_gx_gemm_x3 run on v_mfma_f32_16x16x32_bf16 with the f32 operands
// as three bf16 planes (bf16_planes.h): products of f32 accuracy at 3 (masked layer:
// the genotype codes are exact in bf16) or 6 MFMAs per 32-deep K step.  k_gx_gemm runs
// on v_mfma_f32_16x16x4_f32 (exact f32 products, 8 MFMAs per 32-deep step).
// Every workgroup computes one output tile with 4 waves: 64 x 64 (32 x 32 per wave, four
// 16 x 16 accumulators) in k_gx_gemm and k_gx_gemm_b3, 32 AX x 32 AY of X3Shape
// (gx_shapes.h) in k_gx_gemm_x3.  Operands are staged through registers into ONE LDS
// stage per operand: the next K block's loads are issued before the MFMAs of the
// current one and stored to the stage after them, behind a barrier (a second stage at
// 2 workgroups per CU measured -30 %).  Tiles are numbered (gx_dims,
// gx_shapes.h; the host counts them with gx_tiles there) so that consecutive ones
// share an operand block (the row block of a forward, the row range of a gradient
// split) and are mapped to ONE XCD, so the shared block is read from HBM once into
// that XCD's L2.
// PREP and HEAD are k_gx_prep, k_gx_head and k_gx_head_red (kernels_gx_head.hip).  By
// default the head is lazy where it can be (a summary layer after a hidden one, h' a
// function of A): the summary layer's FWD epilogue leaves the partials of out, k_gx_head
// only adds them and forms e, pred and the rss, and BWD_s / GRAD_s form delta_s while
// staging, so delta_s is never stored; BANN_GX_EXACT=1, SiLU and one-layer branches keep
// the HEAD line above.  What more than one of these files uses (the f32 block and genotype
// staging, h' from A, the tile epilogue) is in gx_tile.h.
//
// Scratch (per branch, f32, offsets in BranchDev::gx_*): Wp_l, bias_l, A_l and
// H_l of [rows][ld_l] for every hidden/summary layer, the weight planes, the head's
// per-tile f64 partials, rows = 64 * ntile (rows >= n
// carry zero genotypes; their error is 0, so they add nothing to any gradient).
// Gradients go to the branch's partial slabs part[split][P] (reduced in a fixed
// order by k_update), the rss to rss_part: bitwise reproducible.
#include "bann_internal.h"
#include "bf16_planes.h"
#include "gx_tile.h"
#include "kernel_util.h"

#define GX_LDS (GX_T * GX_LD)  // floats per operand block: 17 KiB, two of them per workgroup (4 per CU)

// ---------------------------------------------------------------------------
// the exact-f32 GEMM of every phase: operands staged as [row][k] images with 68-float
// rows (the MFMA's one-float A/B reads -- lane (i, q) at row i, k = 4 s + q -- hit 64
// distinct banks)
// ---------------------------------------------------------------------------
// GRAD (two staged operands + f64 accumulators) at 3 workgroups per CU: 4 would spill
template <int PH>
__global__ void __launch_bounds__(256, PH == GX_GRAD ? 3 : 4)
    k_gx_gemm(DevState st, const int32_t* __restrict__ blist, const int32_t* __restrict__ prefix, int nb, int l,
              int total, int per) {
  __shared__ float As[GX_LDS];
  __shared__ float Bs[GX_LDS];
  __shared__ double cs_s[GX_T];
  // XCD-aware numbering: workgroup i runs on XCD i % 8, so the logical tiles of
  // one XCD are the contiguous range [xcd * per, (xcd + 1) * per)
  const int q = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (q >= total) return;
  int lo = 0, hi = nb;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= q) lo = mid;
    else hi = mid;
  }
  const int b = blist[lo];
  const BranchDev& bd = st.br[b];
  int tmc, tnc, ns;
  gx_dims(st.nfrag, bd, PH, l, tmc, tnc, ns);
  int r = q - prefix[lo];
  const int split = r / (tmc * tnc);
  r -= split * tmc * tnc;
  const int tm = r / tnc, tn = r % tnc;
  const int64_t rows = gx_rows(st);
  float* S = gx_base(st, bd);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int ar = 32 * (wv >> 1), bc = 32 * (wv & 1);

  // K range (in blocks of 64) and the operands of this phase
  int kb0 = 0, kb1;
  int64_t kcount;  // valid K
  const float* Am = nullptr;
  const float* Bm = nullptr;
  int64_t lda = 0, ldb = 0;
  int wi = 0, wo = 0;  // GEMM output M / N extent (rows of the output are individuals for FWD/BWD)
  const uint8_t* img = st.xu2 + bd.x_off;
  const int64_t tstride = (int64_t)bd.nchunks * 1024;
  if constexpr (PH == GX_FWD0) {
    kcount = bd.m;
    kb1 = bd.nchunks;
    Bm = S + bd.gx_w[0];
    ldb = bd.gx_wld[0];
    wo = bd.widths[0];
  } else if constexpr (PH == GX_FWD) {
    kcount = bd.widths[l - 1];
    kb1 = (int)((kcount + 63) / 64);
    Am = S + bd.gx_a[l - 1];
    lda = bd.gx_ld[l - 1];
    Bm = S + bd.gx_w[l];
    ldb = bd.gx_wld[l];
    wo = bd.widths[l];
  } else if constexpr (PH == GX_BWD) {
    kcount = bd.widths[l];
    kb1 = (int)((kcount + 63) / 64);
    Am = S + bd.gx_h[l];  // delta_l
    lda = bd.gx_ld[l];
    Bm = S + bd.gx_w[l];  // Wp_l [k = out][j = in]: loaded transposed
    ldb = bd.gx_wld[l];
    wo = bd.widths[l - 1];
  } else {  // GRAD / GRAD0: K = the split's rows
    const int ntile = (st.nfrag + 3) / 4;
    kb0 = (int)((int64_t)ntile * split / ns);
    kb1 = (int)((int64_t)ntile * (split + 1) / ns);
    kcount = rows;
    if constexpr (PH == GX_GRAD) {
      Am = S + bd.gx_a[l - 1];
      lda = bd.gx_ld[l - 1];
      wi = bd.widths[l - 1];
      Bm = S + bd.gx_h[l];
      ldb = bd.gx_ld[l];
      wo = bd.widths[l];
    } else {
      wi = bd.m;
      Bm = S + bd.gx_h[0];
      ldb = bd.gx_ld[0];
      wo = bd.widths[0];
    }
  }
  const bool want_cs = (PH == GX_GRAD0) || (PH == GX_GRAD && tm == 0);

  // stage K block kb into registers
  Blk ra, rb;
  uint32_t rg = 0;
  // the operand blocks of K block kb
  auto bnd_a = [&](int kb) -> BlkBounds {
    if constexpr (PH == GX_GRAD) return BlkBounds{64 * (int64_t)kb, rows, 64 * tm, wi};
    return BlkBounds{64 * (int64_t)tm, rows, 64 * kb, (int)kcount};
  };
  auto bnd_b = [&](int kb) -> BlkBounds {
    if constexpr (PH == GX_FWD0 || PH == GX_FWD) return BlkBounds{64 * (int64_t)tn, wo, 64 * kb, (int)kcount};
    if constexpr (PH == GX_BWD) return BlkBounds{64 * (int64_t)kb, kcount, 64 * tn, wo};
    return BlkBounds{64 * (int64_t)kb, rows, 64 * tn, wo};
  };
  auto load = [&](int kb) {
    if constexpr (PH == GX_FWD0) rg = geno_load(img + (int64_t)tm * tstride + (int64_t)kb * 1024);
    if constexpr (PH == GX_GRAD0) rg = geno_load(img + (int64_t)kb * tstride + (int64_t)tm * 1024);
    if constexpr (PH == GX_FWD || PH == GX_BWD || PH == GX_GRAD) blk_load(ra, Am, lda, bnd_a(kb));
    blk_load(rb, Bm, ldb, bnd_b(kb));
  };
  auto store = [&](int kb) {
    if constexpr (PH == GX_FWD0) {
      geno_store_im(rg, As);
      blk_store(rb, bnd_b(kb), Bs);
    } else if constexpr (PH == GX_FWD) {
      blk_store(ra, bnd_a(kb), As);
      blk_store(rb, bnd_b(kb), Bs);
    } else if constexpr (PH == GX_BWD) {
      blk_store(ra, bnd_a(kb), As);
      blk_store_t(rb, bnd_b(kb), Bs);
    } else if constexpr (PH == GX_GRAD) {
      blk_store_t(ra, bnd_a(kb), As);
      blk_store_t(rb, bnd_b(kb), Bs);
    } else {
      geno_store_mi(rg, As);
      blk_store_t(rb, bnd_b(kb), Bs);
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
  // f64 accumulation across K blocks where K is long (m markers, n individuals);
  // the hidden-layer GEMMs (K = a layer width) keep the f32 MFMA chain
  constexpr bool F64 = PH != GX_FWD && PH != GX_BWD;
  double cs = 0.0;  // want_cs: column sum of the B block (delta) over the K range, thread t < 64 = column t
  if (kb0 < kb1) {
    load(kb0);
    store(kb0);
  }
  __syncthreads();
  for (int kb = kb0; kb < kb1; ++kb) {
    if (kb + 1 < kb1) load(kb + 1);
    const float* A = As;
    const float* B = Bs;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int ko = 4 * s + lq;
      const float a0 = A[(ar + li) * GX_LD + ko], a1 = A[(ar + 16 + li) * GX_LD + ko];
      const float b0 = B[(bc + li) * GX_LD + ko], b1 = B[(bc + 16 + li) * GX_LD + ko];
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[3], 0, 0, 0);
    }
    if (want_cs && t < GX_T) {
      const float* Br = B + t * GX_LD;
      float c = 0.f;
#pragma unroll 16
      for (int k = 0; k < GX_T; ++k) c += Br[k];
      cs += (double)c;
    }
    if constexpr (F64) {
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        dacc[x][0] += (double)acc[x].x;
        dacc[x][1] += (double)acc[x].y;
        dacc[x][2] += (double)acc[x].z;
        dacc[x][3] += (double)acc[x].w;
        acc[x] = v4f{0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();  // every wave is done with the stage before it is refilled
    if (kb + 1 < kb1) store(kb + 1);
    __syncthreads();
  }

  if constexpr (PH == GX_GRAD0) {
    if (t < GX_T) cs_s[t] = cs;
    __syncthreads();
  }
  gx_epilogue<PH, F64>(st, bd, S, l, tm, tn, split, wi, wo, ar, bc, li, lq, acc, dacc, cs, cs_s);
}

// ---------------------------------------------------------------------------
// the hidden-layer GEMMs on the bf16 MFMA ("x3"): FWD l, BWD l and GRAD l with
// BOTH f32 operands split into three bf16 planes (x = x0 + x1 + x2, 24
// significant bits, split3 in bf16_planes.h) and the six plane products of weight >= 2^-16:
//   a b = a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0) + O(2^-24 |a b|),
// every product keeps f32's accuracy; a 32-deep K step is six
// v_mfma_f32_16x16x32_bf16 (96 cycles) where the f32 MFMA takes eight 16x16x4
// (256 cycles).  K blocks of 32: the 3 + 3 planes of a stage take 30 KiB, four
// workgroups per CU.  An operand whose MFMA rows are contiguous in memory (FWD:
// A_{l-1} and Wp_l; BWD: delta_l) is staged [row][k] and read as 16-byte
// fragments; the others (BWD: Wp_l read transposed; GRAD: A_{l-1} and delta_l,
// K = individuals) are staged [k][row] and read with ds_read_b64_tr_b16.  f32
// accumulation inside a K block, f64 across blocks where K is long (GRAD: the
// rows).
// ---------------------------------------------------------------------------
#define GX_KB 32  // K block depth
#define GX_RK 40  // [row][k] stride (bf16 elements): 80-byte rows

namespace {
// LDS geometry of a staged operand block of R (MFMA) rows x 32 K as three bf16 planes:
// [row][k] rows of GX_RK, or [k][row] rows of KRS = R + 16.  Bank conflicts
// (MI355X_MICROARCH.md LDS table; PMC: SQ_LDS_BANK_CONFLICT was 20-45 % of the
// phases' LDS cycles before this layout):
//  - [row][k]: the 16-byte K chunk q of row r sits at chunk q ^ rk_sw(r), which
//    makes the fragment reads (ds_read_b128, lane groups {0-3,12-15,20-27}, ...)
//    conflict-free at the 80-byte stride;
//  - [k][row]: the K slots 8 lq + j of a fragment are rows 16 (j >> 2) + 4 lq +
//    (j & 3) (kr_row), so the two 16-lane groups of a transposing read take rows
//    0-3 / 4-7 of an 8-row window (conflict-free at R + 16); a [row][k] operand
//    paired with a [k][row] one (BWD's A) stores logical k at that K slot (PERM).
template <int R, bool RK>
struct Geo {
  static constexpr int KRS = R + 16;
  static constexpr int PL = RK ? R * GX_RK : GX_KB * KRS;  // elements per plane
};
__device__ __forceinline__ int rk_sw(int r) { return ((r >> 2) ^ (r >> 3)) & 1; }
// element offset of logical K group c (4 consecutive k) of [row][k] row r
template <bool PERM>
__device__ __forceinline__ int rk_off(int r, int c) {
  const int p = PERM ? 8 * (c & 3) + 4 * (c >> 2) : 4 * c;  // K slot of logical k = 4 c
  return r * GX_RK + 8 * ((p >> 3) ^ rk_sw(r)) + (p & 7);
}
// an R (MFMA rows) x 32 (K) block of an f32 matrix, R / 32 x 4 consecutive elements
// per thread.  RK: M[r][k], thread e = t + 256 u holds row e >> 3, k 4 (e & 7) .. +3.
// KR: M[k][r], thread e holds k e / (R / 4), rows 4 (e % (R / 4)) .. +3.  Elements
// outside r < rmax, k < kmax are 0 (masked at the store, as blk_fix).
template <int R>
struct Blk2 {
  v4f v[R / 32];
};
struct Blk2Bounds {
  int64_t r0, rmax, k0, kmax;
};
template <bool RK, int R>
__device__ __forceinline__ int blk2_nv(const Blk2Bounds& k, int u) {
  const int e = threadIdx.x + 256 * u;
  if constexpr (RK) {
    const int64_t r = k.r0 + (e >> 3), c = k.k0 + 4 * (e & 7);
    return r < k.rmax ? (int)min(max(k.kmax - c, (int64_t)0), (int64_t)4) : 0;
  } else {
    const int64_t kk = k.k0 + e / (R / 4), r = k.r0 + 4 * (e % (R / 4));
    return kk < k.kmax ? (int)min(max(k.rmax - r, (int64_t)0), (int64_t)4) : 0;
  }
}
template <bool RK, int R>
__device__ __forceinline__ void blk2_load(Blk2<R>& s, const float* __restrict__ M, int64_t ld, const Blk2Bounds& k) {
#pragma unroll
  for (int u = 0; u < R / 32; ++u) {
    const int e = threadIdx.x + 256 * u;
    v4f x = {0.f, 0.f, 0.f, 0.f};
    if (blk2_nv<RK, R>(k, u) > 0)
      x = RK ? *(const v4f*)(M + (k.r0 + (e >> 3)) * ld + k.k0 + 4 * (e & 7))    // rows padded to 4
             : *(const v4f*)(M + (k.k0 + e / (R / 4)) * ld + k.r0 + 4 * (e % (R / 4)));
    s.v[u] = x;
  }
}
// mask, split into the three planes P[3][PL] and store; csp (KR only) += the
// masked values per row of the thread's four
template <bool RK, bool CS, int R, bool PERM = false>
__device__ __forceinline__ void blk2_store(Blk2<R>& s, const Blk2Bounds& k, __bf16* P, double (&csp)[4]) {
  constexpr int PL = Geo<R, RK>::PL, KRS = Geo<R, RK>::KRS;
#pragma unroll
  for (int u = 0; u < R / 32; ++u) {
    const int e = threadIdx.x + 256 * u;
    const int nv = blk2_nv<RK, R>(k, u);
    v4f x = s.v[u];
    if (nv < 1) x.x = 0.f;
    if (nv < 2) x.y = 0.f;
    if (nv < 3) x.z = 0.f;
    if (nv < 4) x.w = 0.f;
    bf16x4 h4, m4, l4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      __bf16 hh, mm, ll;
      split3(x[c], hh, mm, ll);
      h4[c] = hh;
      m4[c] = mm;
      l4[c] = ll;
      if constexpr (CS) csp[c] += (double)x[c];
    }
    const int off = RK ? rk_off<PERM>(e >> 3, e & 7) : (e / (R / 4)) * KRS + 4 * (e % (R / 4));
    *(bf16x4*)&P[off] = h4;
    *(bf16x4*)&P[PL + off] = m4;
    *(bf16x4*)&P[2 * PL + off] = l4;
  }
}
// the bf16x8 fragment (MFMA rows rb .. rb + 15, K slots 8 lq .. 8 lq + 7) of plane pl
template <bool RK, int R>
__device__ __forceinline__ bf16x8 frag3(const __bf16* P, int pl, int rb, int li, int lq) {
  constexpr int PL = Geo<R, RK>::PL, KRS = Geo<R, RK>::KRS;
  if constexpr (RK) {
    return *(const bf16x8*)&P[pl * PL + (rb + li) * GX_RK + 8 * (lq ^ rk_sw(li))];  // rb: a multiple of 16
  } else {
    const int tq = li >> 2, tp = li & 3;
    return tr16_pair(&P[pl * PL + (4 * lq + tq) * KRS + rb + 4 * tp],
                     &P[pl * PL + (16 + 4 * lq + tq) * KRS + rb + 4 * tp]);
  }
}
}  // namespace

// tiles of X3Shape<PH> (gx_shapes.h): 32 AX x 32 AY, 2 x 2 waves
template <int PH>
__global__ void __launch_bounds__(256, PH == GX_FWD ? 3 : (PH == GX_GRAD ? 2 : 4))
    k_gx_gemm_x3(DevState st, const int32_t* __restrict__ blist, const int32_t* __restrict__ prefix, int nb, int l,
                 int total, int per) {
  constexpr int AX = X3Shape<PH>::AX, AY = X3Shape<PH>::AY, TM = 32 * AX, TN = 32 * AY;
  constexpr bool ARK = PH != GX_GRAD;  // A staged [row][k]
  constexpr bool BRK = PH == GX_FWD;   // B staged [row][k]
  constexpr bool F64 = PH == GX_GRAD;
  constexpr int PLA = Geo<TM, ARK>::PL, PLB = Geo<TN, BRK>::PL, KRSB = Geo<TN, BRK>::KRS;
  __shared__ __attribute__((aligned(16))) __bf16 As[3 * PLA];
  __shared__ __attribute__((aligned(16))) __bf16 Bs[3 * PLB];
  __shared__ double cs_s[PH == GX_GRAD ? 1024 / TN : 1][TN];  // GRAD's column sums only
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
  gx_dims(st.nfrag, bd, PH, l, tmc, tnc, ns, TM, TN);
  int r = q - prefix[lo_];
  const int split = r / (tmc * tnc);
  r -= split * tmc * tnc;
  const int tm = r / tnc, tn = r % tnc;
  const int64_t rows = gx_rows(st);
  float* S = gx_base(st, bd);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int ar = (TM / 2) * (wv >> 1), bc = (TN / 2) * (wv & 1);
  // lazy head (k_gx_head): delta_s = h'(A_s) * e * w_out is never stored.  BWD_s:
  // A = h'(A_s), B = the w_out-scaled planes of Wp_s (k_gx_prep), the epilogue
  // multiplies row i by e_i; GRAD_s: B = h'(A_s) * e (e of the block's rows, per K
  // block), the epilogue multiplies column j by w_out_j; its column sums give db_s
  // (times w_out) and dW_out = A_s^T e (f64, from the raw A_s values)
  const bool lazy = PH != GX_FWD && l == bd.L - 2 && dh_from_a(bd.act);
  const float* ev = S + bd.gx_e;
  const float* wout = S + bd.gx_w[bd.L - 1];

  int64_t kb0 = 0, kb1, kcount;
  const float* Am;
  const float* Bm;
  int64_t lda, ldb;
  int wi = 0, wo;
  if constexpr (PH == GX_FWD) {  // Z_l = A_{l-1} Wp_l^T: A [individual][in], B = Wp_l [out][in]
    kcount = bd.widths[l - 1];
    Am = S + bd.gx_a[l - 1];
    lda = bd.gx_ld[l - 1];
    Bm = S + bd.gx_w[l];
    ldb = bd.gx_wld[l];
    wo = bd.widths[l];
  } else if constexpr (PH == GX_BWD) {  // delta_l Wp_l: A = delta_l [individual][out], B = Wp_l [out = k][in]
    kcount = bd.widths[l];
    Am = S + (lazy ? bd.gx_a[l] : bd.gx_h[l]);
    lda = bd.gx_ld[l];
    Bm = S + bd.gx_w[l];
    ldb = bd.gx_wld[l];
    wo = bd.widths[l - 1];
  } else {  // GRAD: dW_l = A_{l-1}^T delta_l over the split's rows (K = individuals)
    const int ntile = (st.nfrag + 3) / 4;
    kcount = rows;
    Am = S + bd.gx_a[l - 1];
    lda = bd.gx_ld[l - 1];
    wi = bd.widths[l - 1];
    Bm = S + (lazy ? bd.gx_a[l] : bd.gx_h[l]);
    ldb = bd.gx_ld[l];
    wo = bd.widths[l];
    kb0 = 2 * ((int64_t)ntile * split / ns);  // 64-row tiles -> 32-deep K blocks
    kb1 = 2 * ((int64_t)ntile * (split + 1) / ns);
  }
  if constexpr (PH != GX_GRAD) kb1 = (kcount + GX_KB - 1) / GX_KB;
  // the operand blocks of K block kb: rows of the A block are output rows (TM tm ..),
  // rows of the B block output columns (TN tn ..)
  auto bnd_a = [&](int64_t kb) {
    return Blk2Bounds{TM * (int64_t)tm, PH == GX_GRAD ? (int64_t)wi : rows, GX_KB * kb, kcount};
  };
  auto bnd_b = [&](int64_t kb) { return Blk2Bounds{TN * (int64_t)tn, (int64_t)wo, GX_KB * kb, kcount}; };
  Blk2<TM> ra;
  Blk2<TN> rb;
  double csa[4] = {0.0, 0.0, 0.0, 0.0}, csp[4] = {0.0, 0.0, 0.0, 0.0};  // GRAD: column sums of delta_l
  // FWD / BWD: B = Wp_l from its pre-split planes [3][out][r32(in)] (k_gx_prep): TN / 64
  // 16-byte pieces of 8 elements per plane and thread, copied to the stage as is.
  // FWD stages it [out][in] (piece p: out row p >> 2, in 8 (p & 3) ..), BWD [out = k][in]
  // (piece p: out row p / (TN / 8), in 8 (p % (TN / 8)) ..); rows past the layer and
  // pieces past the in width are zero (the planes' padding covers the rest of a piece)
  constexpr bool BP = PH != GX_GRAD;
  constexpr int NP = TN / 64;
  v4i rbp[NP][3];
  const __bf16* Wp3 = BP ? reinterpret_cast<const __bf16*>(S + (PH == GX_BWD && lazy ? bd.gx_wps : bd.gx_wp[l]))
                         : nullptr;
  const int64_t l3 = BP ? ((bd.win[l] + 31) & ~31) : 0, p3 = BP ? (int64_t)bd.widths[l] * l3 : 0;
  auto load_bp = [&](int64_t kb) {
#pragma unroll
    for (int v = 0; v < NP; ++v) {
      const int pc = t + 256 * v;
      int64_t row, col;
      bool ok;
      if constexpr (PH == GX_FWD) {
        row = TN * (int64_t)tn + (pc >> 2);
        col = GX_KB * kb + 8 * (pc & 3);
        ok = row < wo;
      } else {
        row = GX_KB * kb + pc / (TN / 8);
        col = TN * (int64_t)tn + 8 * (pc % (TN / 8));
        ok = row < kcount && col < wo;
      }
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
        rbp[v][pl] = ok ? *reinterpret_cast<const v4i*>(Wp3 + pl * p3 + row * l3 + col) : v4i{0, 0, 0, 0};
    }
  };
  auto store_bp = [&]() {
#pragma unroll
    for (int v = 0; v < NP; ++v) {
      const int pc = t + 256 * v;
      const int off = PH == GX_FWD ? (pc >> 2) * GX_RK + 8 * ((pc & 3) ^ rk_sw(pc >> 2))
                                   : (pc / (TN / 8)) * KRSB + 8 * (pc % (TN / 8));
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<v4i*>(&Bs[pl * PLB + off]) = rbp[v][pl];
    }
  };
  const bool want_cs = PH == GX_GRAD && tm == 0;

  v4f acc[AX * AY];
  double dacc[AX * AY][4];
#pragma unroll
  for (int x = 0; x < AX * AY; ++x) {
    acc[x] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int y = 0; y < 4; ++y) dacc[x][y] = 0.0;
  }
  float le[4] = {0.f, 0.f, 0.f, 0.f};
  double csq[4] = {0.0, 0.0, 0.0, 0.0};  // GRAD_s, tm == 0: dW_out column sums
  auto lazy_load = [&](int64_t kb) {
    if constexpr (PH == GX_GRAD) {
#pragma unroll
      for (int u = 0; u < TN / 32; ++u) le[u] = ev[GX_KB * kb + (t + 256 * u) / (TN / 4)];
    }
  };
  const DhA dk = dh_a_consts(bd.act);
  const bool tanh_act = bd.act == 0;
  auto lazy_h = [&](auto& rr) {  // rr = h'(A_s) (* e of the row: GRAD)
    constexpr int NU = sizeof(rr.v) / sizeof(v4f);
    if (tanh_act) {
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float a = rr.v[u][c];
          rr.v[u][c] = PH == GX_GRAD ? (1.f - a * a) * le[u] : 1.f - a * a;
        }
    } else {
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float h = dh_a(rr.v[u][c], dk);
          rr.v[u][c] = PH == GX_GRAD ? h * le[u] : h;
        }
    }
  };
  auto lazy_dwo = [&](const Blk2<TN>& rr) {
#pragma unroll
    for (int u = 0; u < TN / 32; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) csq[c] += (double)rr.v[u][c] * (double)le[u];
  };
  // values the epilogue needs, loaded before the K loop (gx_epilogue): FWD the bias
  // and w_out of the lane's AY columns, lazy BWD_s the e of its 4 AX rows, lazy
  // GRAD_s w_out of its AY columns
  float pre[4 * AX > 2 * AY ? 4 * AX : 2 * AY];
#pragma unroll
  for (int i = 0; i < (int)(sizeof(pre) / sizeof(float)); ++i) pre[i] = 0.f;
  if constexpr (PH == GX_FWD) {
    const bool head = l == bd.L - 2 && dh_from_a(bd.act);
#pragma unroll
    for (int Y = 0; Y < AY; ++Y) {
      const int j = TN * tn + bc + 16 * Y + li;
      pre[Y] = j < wo ? S[bd.gx_b[l] + j] : 0.f;
      pre[AY + Y] = head && j < wo ? wout[j] : 0.f;
    }
  } else if constexpr (PH == GX_BWD) {
    if (lazy)
#pragma unroll
      for (int X = 0; X < AX; ++X)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          const int64_t row = TM * (int64_t)tm + ar + 16 * X + 4 * lq + y;
          pre[4 * X + y] = row < rows ? ev[row] : 0.f;
        }
  } else {
    if (lazy)
#pragma unroll
      for (int Y = 0; Y < AY; ++Y) {
        const int j = TN * tn + bc + 16 * Y + li;
        pre[Y] = j < wo ? wout[j] : 0.f;
      }
  }
  auto load = [&](int64_t kb) {
    if (lazy) lazy_load(kb);
    blk2_load<ARK, TM>(ra, Am, lda, bnd_a(kb));
    if constexpr (BP) load_bp(kb);
    else blk2_load<BRK, TN>(rb, Bm, ldb, bnd_b(kb));
  };
  auto stage = [&](int64_t kb) {
    if constexpr (PH == GX_BWD) {
      if (lazy) lazy_h(ra);
    } else if constexpr (PH == GX_GRAD) {
      if (lazy) {
        if (want_cs) lazy_dwo(rb);
        lazy_h(rb);
      }
    }
    blk2_store<ARK, false, TM, PH == GX_BWD>(ra, bnd_a(kb), As, csa);  // BWD: A [row][k] beside B [k][row]
    if constexpr (BP) store_bp();
    else if (want_cs) blk2_store<BRK, true, TN>(rb, bnd_b(kb), Bs, csp);
    else blk2_store<BRK, false, TN>(rb, bnd_b(kb), Bs, csp);
  };
  auto compute = [&](int64_t kb) {
    bf16x8 a[AX][3];
#pragma unroll
    for (int X = 0; X < AX; ++X)
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) a[X][pl] = frag3<ARK, TM>(As, pl, ar + 16 * X, li, lq);
#pragma unroll
    for (int Y = 0; Y < AY; ++Y) {
      bf16x8 bq[3];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) bq[pl] = frag3<BRK, TN>(Bs, pl, bc + 16 * Y, li, lq);
#pragma unroll
      for (int X = 0; X < AX; ++X) {
        v4f& c = acc[AY * X + Y];
        // small products first
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[X][2], bq[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[X][1], bq[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[X][0], bq[2], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[X][1], bq[0], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[X][0], bq[1], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[X][0], bq[0], c, 0, 0, 0);
      }
    }
    if constexpr (F64) {
      constexpr int EVERY = GX_F64_BLOCKS * 64 / GX_KB;  // the same 256 rows in 32-deep K blocks
      if ((kb & (EVERY - 1)) == EVERY - 1) {  // f64 across 256-deep K
#pragma unroll
        for (int x = 0; x < AX * AY; ++x) {
          dacc[x][0] += (double)acc[x].x;
          dacc[x][1] += (double)acc[x].y;
          dacc[x][2] += (double)acc[x].z;
          dacc[x][3] += (double)acc[x].w;
          acc[x] = v4f{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  };
  if (kb0 < kb1) load(kb0);
  for (int64_t kb = kb0; kb < kb1; ++kb) {
    stage(kb);
    __syncthreads();
    if (kb + 1 < kb1) load(kb + 1);  // lands during this block's MFMAs
    compute(kb);
    __syncthreads();  // every wave is done with the stage before it is refilled
  }
  if constexpr (F64) {  // an odd block count leaves one block in acc
#pragma unroll
    for (int x = 0; x < AX * AY; ++x) {
      dacc[x][0] += (double)acc[x].x;
      dacc[x][1] += (double)acc[x].y;
      dacc[x][2] += (double)acc[x].z;
      dacc[x][3] += (double)acc[x].w;
    }
  }
  double cs = 0.0, cs2 = 0.0;
  if (want_cs) {  // 1024 / TN threads per 4-column group, added in thread order (deterministic)
    constexpr int RW = TN / 4;
#pragma unroll
    for (int x = 0; x < 4; ++x) cs_s[t / RW][4 * (t % RW) + x] = csp[x];
    __syncthreads();
    if (t < TN)
      for (int k = 0; k < 1024 / TN; ++k) cs += cs_s[k][t];
    if (lazy) {  // db_s = w_out * (column sums of h'(A_s) e); the dW_out column sums, same order
      cs *= (t < TN && TN * tn + t < wo) ? (double)wout[TN * tn + t] : 0.0;
      __syncthreads();
#pragma unroll
      for (int x = 0; x < 4; ++x) cs_s[t / RW][4 * (t % RW) + x] = csq[x];
      __syncthreads();
      if (t < TN)
        for (int k = 0; k < 1024 / TN; ++k) cs2 += cs_s[k][t];
    }
  }
  gx_epilogue<PH, F64, AX, AY>(st, bd, S, l, tm, tn, split, wi, wo, ar, bc, li, lq, acc, dacc, cs, nullptr, lazy, cs2,
                               PH == GX_FWD || lazy ? pre : nullptr);
}

// one launch of phase (ph, l) over `total` tiles (the sum of gx_tiles over blist; prefix: its running
// sum per branch).  exact: EnvOptions::gx_exact, the same value for the tile count and the launch
void launch_gx_gemm(const DevState& st, int ph, int l, const int32_t* blist, const int32_t* prefix, int nb,
                    int total, bool exact, hipStream_t s) {
  if (nb <= 0 || total <= 0) return;
  const int per = (total + 7) / 8;
  const dim3 g(8 * per), blk(256);
  if (!exact) {
    switch (ph) {
      case GX_FWD: hipLaunchKernelGGL(k_gx_gemm_x3<GX_FWD>, g, blk, 0, s, st, blist, prefix, nb, l, total, per); break;
      case GX_BWD: hipLaunchKernelGGL(k_gx_gemm_x3<GX_BWD>, g, blk, 0, s, st, blist, prefix, nb, l, total, per); break;
      case GX_GRAD: hipLaunchKernelGGL(k_gx_gemm_x3<GX_GRAD>, g, blk, 0, s, st, blist, prefix, nb, l, total, per); break;
      default: launch_gx_gemm_b3(st, ph, blist, prefix, nb, total, per, s); break;  // FWD0, GRAD0
    }
    return;
  }
  switch (ph) {
    case GX_FWD0: hipLaunchKernelGGL(k_gx_gemm<GX_FWD0>, g, blk, 0, s, st, blist, prefix, nb, l, total, per); break;
    case GX_FWD: hipLaunchKernelGGL(k_gx_gemm<GX_FWD>, g, blk, 0, s, st, blist, prefix, nb, l, total, per); break;
    case GX_BWD: hipLaunchKernelGGL(k_gx_gemm<GX_BWD>, g, blk, 0, s, st, blist, prefix, nb, l, total, per); break;
    case GX_GRAD: hipLaunchKernelGGL(k_gx_gemm<GX_GRAD>, g, blk, 0, s, st, blist, prefix, nb, l, total, per); break;
    default: hipLaunchKernelGGL(k_gx_gemm<GX_GRAD0>, g, blk, 0, s, st, blist, prefix, nb, l, total, per); break;
  }
}
