// kernels_subset.hip — a cohort from chosen individuals and markers of another cohort, on the device.
//
// Replaces the PLINK run of the reference's scripts/split_train_test.sh (plink --keep .. --make-bed):
// field (j', i') of the destination image is field (markers[j'], individuals[i']) of the source
// image (kernels_data.hip: row = marker, rowb = ceil(n / 64) * 16 bytes, individual 4q + p at bits 2p
// of byte q), and the same for the presence image.  Both lists may repeat and reorder.
//
// A destination row costs 1/4 byte per kept individual, the index list 4 bytes: read once per row it
// would be 16 x the genotype traffic.  So a lane owns one destination dword (SUBSET_FPL = 16 kept
// individuals) and keeps their source positions in registers; a workgroup's lanes form a strip of
// consecutive dwords of the row (up to SUBSET_STRIP = 4096 individuals) and walk a block of marker
// rows with those registers.  A narrow destination (fewer dwords than lanes) folds the spare lanes
// over rows: S = 2^sh lanes per row, 256 / S rows at a time.  Per dword and row: 16 byte loads from
// one source row (cached: neighbouring lanes of an ascending list share bytes), one dword store.
// Fields at i' >= n_keep and the row padding up to rowb_dst are written as 0, the invariant of every
// reader of the image.  The destination's code-3 flag comes from the dwords already in registers; a
// wave that finds a 3 stores the constant 1 (every writer the same value: no atomic).
#include <algorithm>

#include "bann_internal.h"

__global__ void __launch_bounds__(256) k_subset(const uint8_t* __restrict__ src_g, const uint8_t* __restrict__ src_p,
                                                int64_t rowb_src, const int32_t* __restrict__ ind,
                                                const int32_t* __restrict__ mk, uint8_t* __restrict__ dst_g,
                                                uint8_t* __restrict__ dst_p, int64_t rowb_dst, int64_t n_keep,
                                                int64_t m_keep, int64_t rows_per_block, int32_t sh,
                                                int32_t* __restrict__ flag) {
  const int S = 1 << sh;
  const int lane = threadIdx.x & (S - 1), sub = threadIdx.x >> sh, nsub = 256 >> sh;
  const int64_t w = (int64_t)blockIdx.x * S + lane;  // destination dword of every row
  if (w >= rowb_dst / 4) return;
  // the strip: byte offset and bit shift of the 16 source fields, 0 / masked out past n_keep
  int32_t off[SUBSET_FPL];
  uint32_t shv = 0, keep = 0;  // 2 bits per field: (position & 3), and 11 where the field exists
#pragma unroll
  for (int k = 0; k < SUBSET_FPL; ++k) {
    const int64_t i = w * SUBSET_FPL + k;
    const int32_t p = i < n_keep ? ind[i] : 0;
    off[k] = p >> 2;
    shv |= (uint32_t)(p & 3) << (2 * k);
    keep |= (i < n_keep ? 3u : 0u) << (2 * k);
  }
  const int64_t r1 = min(m_keep, ((int64_t)blockIdx.y + 1) * rows_per_block);
  uint32_t three = 0;
  for (int64_t r = (int64_t)blockIdx.y * rows_per_block + sub; r < r1; r += nsub) {
    const int64_t base = (int64_t)(mk ? mk[r] : (int32_t)r) * rowb_src;
    uint32_t b[SUBSET_FPL];
#pragma unroll
    for (int k = 0; k < SUBSET_FPL; ++k) b[k] = src_g[base + off[k]];
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < SUBSET_FPL; ++k) v |= ((b[k] >> (2 * ((shv >> (2 * k)) & 3u))) & 3u) << (2 * k);
    v &= keep;
    three |= v & (v >> 1) & 0x55555555u;
    reinterpret_cast<uint32_t*>(dst_g + r * rowb_dst)[w] = v;
    if (src_p) {
#pragma unroll
      for (int k = 0; k < SUBSET_FPL; ++k) b[k] = src_p[base + off[k]];
      v = 0;
#pragma unroll
      for (int k = 0; k < SUBSET_FPL; ++k) v |= ((b[k] >> (2 * ((shv >> (2 * k)) & 3u))) & 3u) << (2 * k);
      reinterpret_cast<uint32_t*>(dst_p + r * rowb_dst)[w] = v & keep;
    }
  }
  if (three) *flag = 1;
}

// every individual, in order: destination row r = source row mk[r], copied in 16-byte pieces (both
// images have the source's rowb, and its zero padding)
__global__ void __launch_bounds__(256) k_subset_rows(const uint8_t* __restrict__ src_g,
                                                     const uint8_t* __restrict__ src_p, int64_t rowb,
                                                     const int32_t* __restrict__ mk, uint8_t* __restrict__ dst_g,
                                                     uint8_t* __restrict__ dst_p, int64_t m_keep,
                                                     int32_t* __restrict__ flag) {
  const int64_t pieces = rowb / 16, total = pieces * m_keep;
  uint32_t three = 0;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = t / pieces, q = t - r * pieces;
    const int64_t s = (int64_t)mk[r] * rowb + 16 * q, d = r * rowb + 16 * q;
    const uint4 v = *reinterpret_cast<const uint4*>(src_g + s);
    three |= (v.x & (v.x >> 1)) | (v.y & (v.y >> 1)) | (v.z & (v.z >> 1)) | (v.w & (v.w >> 1));
    *reinterpret_cast<uint4*>(dst_g + d) = v;
    if (src_p) *reinterpret_cast<uint4*>(dst_p + d) = *reinterpret_cast<const uint4*>(src_p + s);
  }
  if (three & 0x55555555u) *flag = 1;
}

void launch_subset(const uint8_t* src_g, const uint8_t* src_p, int64_t rowb_src, const int32_t* ind,
                   const int32_t* mk, uint8_t* dst_g, uint8_t* dst_p, int64_t rowb_dst, int64_t n_keep, int64_t m_keep,
                   int32_t* flag, hipStream_t s) {
  if (n_keep <= 0 || m_keep <= 0 || (!ind && !mk)) return;  // no list at all: the caller copies the images
  if (!ind) {  // rowb_dst == rowb_src
    const int64_t blocks = (rowb_dst / 16 * m_keep + 255) / 256;
    hipLaunchKernelGGL(k_subset_rows, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, s, src_g, src_p,
                       rowb_dst, mk, dst_g, dst_p, m_keep, flag);
    return;
  }
  const int64_t dwords = rowb_dst / 4;
  int32_t sh = 8;  // lanes per row: the smallest power of two that holds the row, at most the workgroup
  while (sh > 0 && (int64_t(1) << (sh - 1)) >= dwords) --sh;
  const int64_t strips = (dwords + (int64_t(1) << sh) - 1) >> sh;
  // about 8 workgroups per CU over strips x row blocks; a row block is at least one round of the
  // workgroup's rows, so that the strip's 16 index loads are paid once per 256 >> sh rows or more
  const int64_t round = 256 >> sh;
  int64_t yb = std::max<int64_t>(1, std::min<int64_t>(2048 / std::min<int64_t>(strips, 2048), (m_keep + round - 1) / round));
  const int64_t rpb = (m_keep + yb - 1) / yb;
  yb = (m_keep + rpb - 1) / rpb;
  hipLaunchKernelGGL(k_subset, dim3((unsigned)strips, (unsigned)yb), dim3(256), 0, s, src_g, src_p, rowb_src, ind, mk,
                     dst_g, dst_p, rowb_dst, n_keep, m_keep, rpb, sh, flag);
}
