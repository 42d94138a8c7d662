// kernels_ld.hip — windowed pairwise r^2 between markers (the LD band) from the
// 2-bit variant-major cohort image of kernels_data.hip, in exact integers.
//
// Replaces the PLINK --r2 run that the reference's group-by-ld needs before
// CorrGraph::from_plink_ld (group/centered.rs:54-89) can read anything: the
// reference does not compute LD.  For markers j < k <= j + window
//
//   s_j = sum_i g_ij    q_j = sum_i g_ij^2    S_jk = sum_i g_ij g_ik    (int32)
//   cov = n S_jk - s_j s_k     v_j = n q_j - s_j^2                      (int64)
//   r2  = ((double)cov * (double)cov) / ((double)v_j * (double)v_k)     (f64)
//
// r2 = 0 when v_j or v_k is 0.  g is the image's value (a missing .bed code is
// 0, bed_lookup_tables.rs:4; PLINK leaves missing pairs out).  n <= 2^29 - 1
// keeps S <= 4 n inside int32 and every product inside int64.
//
// S is a banded X^T X on v_mfma_i32_16x16x64_i8.  A K step is 256 individuals
// = 64 bytes of a marker's row (the kernel's loop runs over stages t of two K
// steps u = 0, 1): lane (r = lane & 15, s = lane >> 4) takes the 16 bytes of
// marker r's 64-individual tile 8 t + 4 u + s, and field p of those bytes
// ((x >> 2p) & 0x03030303: 16 int8 values) is the lane's operand of MFMA p.
// Row and column fragments are decoded alike, so both sides of every product
// carry the same individual at the same K position whatever the instruction's
// K lane map is; only the C/D map (col = lane & 15, row = 4 (lane >> 4) + reg)
// is relied on.  A wave holds 4 row and 4 column fragments and issues 16 MFMAs
// per field: a 64 x 64 block of pairs per K step, 8 decodes for 64 MFMAs.  A
// workgroup is 2 x 2 such waves (128 x 128 pairs): it stages two K steps (one
// 128-byte line per marker) of its 128 + 128 markers through LDS still packed,
// so every line is fetched once per workgroup and whole.  K is split over
// workgroups (blockIdx.y) and combined with int32 atomicAdd into the S band:
// exact and order-independent.
//
// The pairwise-complete r2 (bann.h: a pair's missing individuals left out, as
// PLINK does) needs five more bands of the same shape, with the presence image
// (kernels_data.hip: field 1 = the call is there) on one or both sides and the
// genotype field squared on one: N, a, b, qa, qb.  The kernel body is a template
// over what each side stages and how it decodes a field (ld_band_tile<RA, RB>);
// k_ld_band is its <genotype, genotype> case, k_ld_band_pw<RA, RB> the other
// five, one launch each: the kernel is bound by decode and MFMA issue, not by
// loads, and six accumulator sets do not fit two waves per SIMD.
#include "bann_internal.h"

typedef int v4i __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// s_j and q_j of markers j0 .. j0 + m, from the two bit planes (as k_col_stats)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ld_stats(const uint8_t* __restrict__ raw, int64_t rowb, int64_t j0,
                                                  int32_t* __restrict__ s_out, int32_t* __restrict__ q_out) {
  __shared__ int32_t red[2][4];
  const int64_t j = j0 + blockIdx.x;
  const uint32_t* row = reinterpret_cast<const uint32_t*>(raw + j * rowb);  // rowb is a multiple of 16
  int32_t s1 = 0, s2 = 0;
  for (int64_t w = threadIdx.x; w < rowb / 4; w += blockDim.x) {
    const uint32_t v = row[w];
    const uint32_t lo = v & 0x55555555u, hi = (v >> 1) & 0x55555555u;
    const int c_lo = __builtin_popcount(lo), c_hi = __builtin_popcount(hi), c_both = __builtin_popcount(lo & hi);
    s1 += c_lo + 2 * c_hi;
    s2 += c_lo + 4 * c_hi + 4 * c_both;
  }
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s1;
    red[1][threadIdx.x >> 6] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s_out[blockIdx.x] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    q_out[blockIdx.x] = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  }
}

void launch_ld_stats(const uint8_t* raw, int64_t rowb, int64_t j0, int64_t m, int32_t* s_out, int32_t* q_out,
                     hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_ld_stats, dim3((unsigned)m), dim3(256), 0, s, raw, rowb, j0, s_out, q_out);
}

// ---------------------------------------------------------------------------
// the S band of rows row0 .. row0 + rows: S[(j - row0) window + d - 1] += the
// K chunk's part of S(j, j + d), d = 1 .. window
// ---------------------------------------------------------------------------
struct LdFrag {
  uint4 a[4], b[4];
};

__device__ __forceinline__ uint4 ld_load16(const uint8_t* __restrict__ raw, int64_t rowb, int64_t M, int64_t j,
                                           int64_t off) {
  // a row past the last marker or a tile past the row's end is all zeros
  return (j < M && off < rowb) ? *reinterpret_cast<const uint4*>(raw + j * rowb + off) : make_uint4(0, 0, 0, 0);
}

// what one side of a product is: the genotype image's field, the presence image's field (0 / 1), or
// the genotype field squared: on packed bytes of {0,1,2}, x + (x & 0x02020202) gives {0,1,4}
enum { LD_G = 0, LD_P = 1, LD_G2 = 2 };

template <int P, int SIDE>
__device__ __forceinline__ v4i ld_field(const uint4 x) {
  uint32_t v[4] = {(x.x >> (2 * P)) & 0x03030303u, (x.y >> (2 * P)) & 0x03030303u, (x.z >> (2 * P)) & 0x03030303u,
                   (x.w >> (2 * P)) & 0x03030303u};
  if constexpr (SIDE == LD_G2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += v[i] & 0x02020202u;
  }
  return v4i{(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
}

template <int P, int RA, int RB>
__device__ __forceinline__ void ld_mma(const LdFrag& f, v4i (&acc)[4][4]) {
  v4i A[4], B[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    A[t] = ld_field<P, RA>(f.a[t]);
    B[t] = ld_field<P, RB>(f.b[t]);
  }
#pragma unroll
  for (int ta = 0; ta < 4; ++ta)
#pragma unroll
    for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[ta], B[tb], acc[ta][tb], 0, 0, 0);
}

// the band of sum_i A_ij B_ik: the row markers' lines come from img_a and are decoded as RA, the column
// markers' from img_b as RB (both images have the cohort image's layout)
template <int RA, int RB>
__device__ __forceinline__ void ld_band_tile(const uint8_t* __restrict__ img_a, const uint8_t* __restrict__ img_b,
                                             int64_t rowb, int64_t M, int64_t row0, int32_t rows, int32_t window,
                                             int32_t ncol, int32_t ksteps, int32_t kchunk, int32_t* __restrict__ S) {
  // one K stage (512 individuals = 128 B = 8 pieces of 16 B per marker) of the 128 row and the 128
  // column markers; piece p of row R sits at p ^ ((R >> 1) & 7): the stores of a row and the
  // ds_read_b128 lane groups of a fragment both meet every bank once
  __shared__ uint4 tile[2][128][8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t rt = blockIdx.x / ncol, c = blockIdx.x - rt * ncol;
  const int64_t row_end = row0 + rows < M ? row0 + rows : M;
  const int64_t ja = row0 + 128 * rt, kb = row0 + 128 * (rt + c);
  if (ja >= row_end || kb >= M) return;  // the whole workgroup: before any barrier
  const int64_t j0 = ja + 64 * (w >> 1);  // the wave's 64 row markers
  const int64_t k0 = kb + 64 * (w & 1);   // its 64 column markers
  // nothing of the band in this 64 x 64 block (no row, no column, all k <= j, or all k - j > window):
  // the wave only helps to load
  const bool active = !(j0 >= row_end || k0 >= M || k0 + 63 <= j0 || k0 - (j0 + 63) > window);
  const int r = lane & 15, s = lane >> 4;
  const int t_begin = blockIdx.y * kchunk;
  const int t_end = t_begin + kchunk < ksteps ? t_begin + kchunk : ksteps;
  v4i acc[4][4];
#pragma unroll
  for (int ta = 0; ta < 4; ++ta)
#pragma unroll
    for (int tb = 0; tb < 4; ++tb) acc[ta][tb] = v4i{0, 0, 0, 0};
  // thread -> (row, piece) of the stage: 8 consecutive threads read one marker's whole 128-B line
  const int lrow = threadIdx.x >> 3, lpiece = threadIdx.x & 7;
  uint4 pre[8];
  auto gload = [&](int t) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      pre[i] = ld_load16(i < 4 ? img_a : img_b, rowb, M, (i < 4 ? ja : kb) + lrow + 32 * (i & 3),
                         (int64_t)t * 128 + 16 * lpiece);
  };
  gload(t_begin);
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();  // the previous stage has been read
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int R = lrow + 32 * (i & 3);
      tile[i >> 2][R][lpiece ^ ((R >> 1) & 7)] = pre[i];
    }
    __syncthreads();
    if (t + 1 < t_end) gload(t + 1);
    if (active) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        LdFrag f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int Ra = 64 * (w >> 1) + 16 * q + r, Rb = 64 * (w & 1) + 16 * q + r;
          f.a[q] = tile[0][Ra][(4 * u + s) ^ ((Ra >> 1) & 7)];
          f.b[q] = tile[1][Rb][(4 * u + s) ^ ((Rb >> 1) & 7)];
        }
        ld_mma<0, RA, RB>(f, acc);
        ld_mma<1, RA, RB>(f, acc);
        ld_mma<2, RA, RB>(f, acc);
        ld_mma<3, RA, RB>(f, acc);
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int ta = 0; ta < 4; ++ta)
#pragma unroll
    for (int tb = 0; tb < 4; ++tb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t j = j0 + 16 * ta + 4 * s + i, k = k0 + 16 * tb + r;
        const int64_t d = k - j;
        if (j < row_end && k < M && d >= 1 && d <= window) atomicAdd(&S[(j - row0) * window + d - 1], acc[ta][tb][i]);
      }
}

__global__ void __launch_bounds__(256, 2) k_ld_band(const uint8_t* __restrict__ raw, int64_t rowb, int64_t M,
                                                    int64_t row0, int32_t rows, int32_t window, int32_t ncol,
                                                    int32_t ksteps, int32_t kchunk, int32_t* __restrict__ S) {
  ld_band_tile<LD_G, LD_G>(raw, raw, rowb, M, row0, rows, window, ncol, ksteps, kchunk, S);
}

// the five further sums of the pairwise-complete r2 (bann.h): RA / RB name the row and the column side
template <int RA, int RB>
__global__ void __launch_bounds__(256, 2) k_ld_band_pw(const uint8_t* __restrict__ raw,
                                                       const uint8_t* __restrict__ pres, int64_t rowb, int64_t M,
                                                       int64_t row0, int32_t rows, int32_t window, int32_t ncol,
                                                       int32_t ksteps, int32_t kchunk, int32_t* __restrict__ out) {
  ld_band_tile<RA, RB>(RA == LD_P ? pres : raw, RB == LD_P ? pres : raw, rowb, M, row0, rows, window, ncol, ksteps,
                       kchunk, out);
}

namespace {
struct LdGrid {
  int32_t ncol, ksteps, kchunk;
  dim3 grid;
};
}  // namespace

static LdGrid ld_grid(int64_t rowb, int32_t rows, int32_t window, int32_t ksplit_target) {
  LdGrid g;
  g.ncol = (127 + window) / 128 + 1;  // column tiles from the row tile to the one holding j + window
  const int32_t nrt = (rows + 127) / 128;
  g.ksteps = (int32_t)((rowb + 127) / 128);  // K stages of 512 individuals
  const int64_t pairs = (int64_t)nrt * g.ncol;
  // K split: enough workgroups for the device, at least 4 K stages per chunk where the cohort has them
  int64_t split = (ksplit_target + pairs - 1) / pairs;
  const int64_t max_split = (g.ksteps + 3) / 4;
  if (split > max_split) split = max_split;
  if (split < 1) split = 1;
  g.kchunk = (int32_t)((g.ksteps + split - 1) / split);
  const int32_t ny = (g.ksteps + g.kchunk - 1) / g.kchunk;
  g.grid = dim3((unsigned)pairs, (unsigned)ny);
  return g;
}

void launch_ld_band(const uint8_t* raw, int64_t rowb, int64_t M, int64_t row0, int32_t rows, int32_t window,
                    int32_t ksplit_target, int32_t* S, hipStream_t s) {
  if (rows <= 0 || window <= 0) return;
  const LdGrid g = ld_grid(rowb, rows, window, ksplit_target);
  hipLaunchKernelGGL(k_ld_band, g.grid, dim3(256), 0, s, raw, rowb, M, row0, rows, window, g.ncol, g.ksteps, g.kchunk,
                     S);
}

// bands[b * stride ..], b = LD_BAND_N, _A, _B, _QA, _QB (bann_internal.h); the S band is launch_ld_band's
void launch_ld_band_pw(const uint8_t* raw, const uint8_t* pres, int64_t rowb, int64_t M, int64_t row0, int32_t rows,
                       int32_t window, int32_t ksplit_target, int32_t* bands, int64_t stride, hipStream_t s) {
  if (rows <= 0 || window <= 0) return;
  const LdGrid g = ld_grid(rowb, rows, window, ksplit_target);
#define LD_PW(RA, RB, B)                                                                                          \
  hipLaunchKernelGGL((k_ld_band_pw<RA, RB>), g.grid, dim3(256), 0, s, raw, pres, rowb, M, row0, rows, window, g.ncol, \
                     g.ksteps, g.kchunk, bands + (B) * stride)
  LD_PW(LD_P, LD_P, LD_BAND_N);
  LD_PW(LD_G, LD_P, LD_BAND_A);
  LD_PW(LD_P, LD_G, LD_BAND_B);
  LD_PW(LD_G2, LD_P, LD_BAND_QA);
  LD_PW(LD_P, LD_G2, LD_BAND_QB);
#undef LD_PW
}

// ---------------------------------------------------------------------------
// S -> r2.  st / qt: s and q of markers stat0 .. (int32); v and cov in int64
// ---------------------------------------------------------------------------
__device__ __forceinline__ double ld_r2(int64_t n, int32_t S, int32_t sj, int32_t qj, int32_t sk, int32_t qk) {
  const int64_t vj = n * (int64_t)qj - (int64_t)sj * sj, vk = n * (int64_t)qk - (int64_t)sk * sk;
  if (vj == 0 || vk == 0) return 0.0;
  const int64_t cov = n * (int64_t)S - (int64_t)sj * sk;
  const double num = (double)cov * (double)cov;
  const double den = (double)vj * (double)vk;
  return num / den;
}

// in place: the int32 S band of the block becomes its f32 r2 band (0 where j + d >= M)
__global__ void __launch_bounds__(256) k_ld_r2(int32_t* __restrict__ S, int64_t total, int32_t window, int64_t row0,
                                               int64_t M, int64_t n, int64_t stat0, const int32_t* __restrict__ st,
                                               const int32_t* __restrict__ qt) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t jl = e / window;
    const int64_t j = row0 + jl, k = j + (e - jl * window) + 1;
    float out = 0.f;
    if (k < M) out = (float)ld_r2(n, S[e], st[j - stat0], qt[j - stat0], st[k - stat0], qt[k - stat0]);
    reinterpret_cast<float*>(S)[e] = out;
  }
}

void launch_ld_r2(int32_t* S, int32_t rows, int32_t window, int64_t row0, int64_t M, int64_t n, int64_t stat0,
                  const int32_t* st, const int32_t* qt, hipStream_t s) {
  const int64_t total = (int64_t)rows * window;
  if (total <= 0) return;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_ld_r2, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, S, total, window,
                     row0, M, n, stat0, st, qt);
}

// forward edge mask of the block's markers: bit (d - 1) & 31 of mask[(j - row0) words + (d - 1) / 32] is set
// iff j + d < M, r2(j, j + d) >= r2_min (on the f64 value) and, with chrom / bp given, both markers are on
// one chromosome and (max_bp <= 0 or |bp_j - bp_k| <= max_bp); st, qt, chrom and bp start at marker stat0
__global__ void __launch_bounds__(256) k_ld_mask(const int32_t* __restrict__ S, int32_t rows, int32_t window,
                                                 int32_t words, int64_t row0, int64_t M, int64_t n, int64_t stat0,
                                                 const int32_t* __restrict__ st, const int32_t* __restrict__ qt,
                                                 double r2_min, const int32_t* __restrict__ chrom,
                                                 const int64_t* __restrict__ bp, int64_t max_bp,
                                                 uint32_t* __restrict__ mask) {
  const int64_t total = (int64_t)rows * words;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t jl = e / words;
    const int32_t wd = (int32_t)(e - jl * words);
    const int64_t j = row0 + jl;
    const int32_t sj = st[j - stat0], qj = qt[j - stat0];
    uint32_t bits = 0;
    for (int b = 0; b < 32; ++b) {
      const int32_t d = 32 * wd + b + 1;
      const int64_t k = j + d;
      if (d > window || k >= M) break;
      bool edge = ld_r2(n, S[jl * window + d - 1], sj, qj, st[k - stat0], qt[k - stat0]) >= r2_min;
      if (edge && chrom) {
        const int64_t bj = bp[j - stat0], bk = bp[k - stat0];
        const int64_t dist = bk > bj ? bk - bj : bj - bk;
        edge = chrom[j - stat0] == chrom[k - stat0] && (max_bp <= 0 || dist <= max_bp);
      }
      bits |= (uint32_t)edge << b;
    }
    mask[e] = bits;
  }
}

void launch_ld_mask(const int32_t* S, int32_t rows, int32_t window, int32_t words, int64_t row0, int64_t M, int64_t n,
                    int64_t stat0, const int32_t* st, const int32_t* qt, double r2_min, const int32_t* chrom,
                    const int64_t* bp, int64_t max_bp, uint32_t* mask, hipStream_t s) {
  const int64_t total = (int64_t)rows * words;
  if (total <= 0) return;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_ld_mask, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, S, rows, window,
                     words, row0, M, n, stat0, st, qt, r2_min, chrom, bp, max_bp, mask);
}

// ---------------------------------------------------------------------------
// the pairwise-complete r2 (bann.h): six bands of the block, band b at bands[b * stride]
// ---------------------------------------------------------------------------
__device__ __forceinline__ double ld_r2_pw(const int32_t* __restrict__ bands, int64_t stride, int64_t e) {
  const int64_t N = bands[LD_BAND_N * stride + e], a = bands[LD_BAND_A * stride + e], b = bands[LD_BAND_B * stride + e];
  const int64_t qa = bands[LD_BAND_QA * stride + e], qb = bands[LD_BAND_QB * stride + e], S = bands[LD_BAND_S * stride + e];
  const int64_t va = N * qa - a * a, vb = N * qb - b * b;
  if (va == 0 || vb == 0) return 0.0;
  const int64_t cov = N * S - a * b;
  const double num = (double)cov * (double)cov;
  const double den = (double)va * (double)vb;
  return num / den;
}

// in place: the int32 S band of the block becomes its f32 r2 band (0 where j + d >= M); the N band stays as
// it is (0 where j + d >= M: nothing was added there)
__global__ void __launch_bounds__(256) k_ld_r2_pw(int32_t* __restrict__ bands, int64_t stride, int64_t total,
                                                  int32_t window, int64_t row0, int64_t M) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t jl = e / window;
    const int64_t k = row0 + jl + (e - jl * window) + 1;
    float out = 0.f;
    if (k < M) out = (float)ld_r2_pw(bands, stride, e);
    reinterpret_cast<float*>(bands + LD_BAND_S * stride)[e] = out;
  }
}

void launch_ld_r2_pw(int32_t* bands, int64_t stride, int32_t rows, int32_t window, int64_t row0, int64_t M,
                     hipStream_t s) {
  const int64_t total = (int64_t)rows * window;
  if (total <= 0) return;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_ld_r2_pw, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, bands, stride,
                     total, window, row0, M);
}

// k_ld_mask on the pairwise-complete r2; chrom and bp start at marker stat0
__global__ void __launch_bounds__(256) k_ld_mask_pw(const int32_t* __restrict__ bands, int64_t stride, int32_t rows,
                                                    int32_t window, int32_t words, int64_t row0, int64_t M,
                                                    int64_t stat0, double r2_min, const int32_t* __restrict__ chrom,
                                                    const int64_t* __restrict__ bp, int64_t max_bp,
                                                    uint32_t* __restrict__ mask) {
  const int64_t total = (int64_t)rows * words;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t jl = e / words;
    const int32_t wd = (int32_t)(e - jl * words);
    const int64_t j = row0 + jl;
    uint32_t bits = 0;
    for (int b = 0; b < 32; ++b) {
      const int32_t d = 32 * wd + b + 1;
      const int64_t k = j + d;
      if (d > window || k >= M) break;
      bool edge = ld_r2_pw(bands, stride, jl * window + d - 1) >= r2_min;
      if (edge && chrom) {
        const int64_t bj = bp[j - stat0], bk = bp[k - stat0];
        const int64_t dist = bk > bj ? bk - bj : bj - bk;
        edge = chrom[j - stat0] == chrom[k - stat0] && (max_bp <= 0 || dist <= max_bp);
      }
      bits |= (uint32_t)edge << b;
    }
    mask[e] = bits;
  }
}

void launch_ld_mask_pw(const int32_t* bands, int64_t stride, int32_t rows, int32_t window, int32_t words, int64_t row0,
                       int64_t M, int64_t stat0, double r2_min, const int32_t* chrom, const int64_t* bp, int64_t max_bp,
                       uint32_t* mask, hipStream_t s) {
  const int64_t total = (int64_t)rows * words;
  if (total <= 0) return;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_ld_mask_pw, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, bands, stride,
                     rows, window, words, row0, M, stat0, r2_min, chrom, bp, max_bp, mask);
}
