// bann_ld.hip — the LD band and the LD graph of the resident cohort (kernels_ld.hip).
//
// The reference's group-by-ld reads a PLINK --r2 table (CorrGraph::from_plink_ld,
// group/centered.rs:54-89); here the table's content comes from the 2-bit cohort
// image on the device.  The markers are processed in blocks of rows, each with its
// own S band, statistics, masks and chrom / bp slices, so that the device scratch of
// a call is bounded whatever M is (bann_ctx::ld_scratch for the S band, LD_SCRATCH_BYTES
// at most; below 256 MiB in all); everything is allocated in the call and freed at its end.
//
// The pairwise calls (bann_genotypes_keep_missing) run the same blocks with six bands in place of
// one, S, N, a, b, qa, qb (bann.h), which together stay inside bann_ctx::ld_scratch, and need no
// s / q.  A cohort without a missing call has no presence image: there N = n, a = s_j, b = s_k,
// qa = q_j, qb = q_k, the formula is the plain one, and the plain path runs.
#include <algorithm>
#include <vector>

#include "ctx_internal.h"

// the S band of one block, at most.  Beside it: s, q, chrom, bp of the block's rows + window markers
// (20 B each, at most 2^20 + 2^18 markers: 25 MiB) and the masks (an eighth of the S band, rounded up
// to whole words per row: 16 MiB + 4 MiB)
static const int64_t LD_SCRATCH_BYTES = int64_t(128) << 20;
static const int64_t LD_MAX_N = 536870911;                   // 4 n < 2^31: S (and qa, qb) stay inside int32

namespace {
struct LdScratch {
  int32_t* S = nullptr;
  int32_t* st = nullptr;
  int32_t* qt = nullptr;
  uint32_t* mask = nullptr;
  int32_t* chrom = nullptr;
  int64_t* bp = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~LdScratch() {
    dfree(S);
    dfree(st);
    dfree(qt);
    dfree(mask);
    dfree(chrom);
    dfree(bp);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};
}  // namespace

// bands: 1, or LD_BANDS for the pairwise sums
static int ld_check(bann_ctx* ctx, int32_t window, int32_t bands, int32_t* weff) {
  if (!ctx->d_g) return fail(ctx, BANN_E_STATE, "the cohort image is not resident (no genotypes loaded, or freed at bann_finalize)");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "not inside a leapfrog session");
  if (window <= 0) return fail(ctx, BANN_E_ARG, "window must be positive");
  if (ctx->n > LD_MAX_N) return fail(ctx, BANN_E_SHAPE, "n > 536870911: the integer sums would leave int32");
  // no pair lies further apart than M - 1
  *weff = (int32_t)std::min<int64_t>(window, std::max<int64_t>(ctx->M - 1, 1));
  if ((int64_t)*weff * 4 * 128 * bands > ctx->ld_scratch) return fail(ctx, BANN_E_ARG, "window too large for the scratch bound");
  return BANN_OK;
}

// rows of one block: whole 128-marker tiles inside the scratch bound
static int64_t ld_block_rows(const bann_ctx* ctx, int32_t weff, int32_t bands) {
  const int64_t r = ctx->ld_scratch / (4 * (int64_t)weff * bands) / 128 * 128;
  return std::max<int64_t>(128, std::min<int64_t>(r, int64_t(1) << 20));
}

// the band scratch of a block (band b at S + b * brows * weff) and, for the plain r2, the s / q of
// its rows and of the window markers after them
static int ld_prepare(bann_ctx* ctx, LdScratch& sc, int32_t weff, int32_t bands, int64_t count, int64_t* brows) {
  CK(hipSetDevice(ctx->device));
  *brows = std::min<int64_t>(ld_block_rows(ctx, weff, bands), std::max<int64_t>(count, 1));
  CK(dalloc(&sc.S, *brows * weff * bands));
  if (bands == 1) {
    CK(dalloc(&sc.st, *brows + weff));
    CK(dalloc(&sc.qt, *brows + weff));
  }
  CK(hipEventCreate(&sc.ev0));
  CK(hipEventCreate(&sc.ev1));
  return BANN_OK;
}

// rows of weff entries on the device -> rows of window entries on the host, the tail (past M - 1) zero
template <typename T>
static int ld_copy_rows(bann_ctx* ctx, const void* src, int32_t rows, int32_t weff, int32_t window, std::vector<T>& stage,
                        T* dst) {
  if (weff == window) {
    CK(hipMemcpyAsync(dst, src, (size_t)rows * weff * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return BANN_OK;
  }
  stage.resize((size_t)rows * weff);
  CK(hipMemcpyAsync(stage.data(), src, (size_t)rows * weff * 4, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  for (int64_t j = 0; j < rows; ++j) {
    std::copy(stage.begin() + j * weff, stage.begin() + (j + 1) * weff, dst + j * window);
    std::fill(dst + j * window + weff, dst + (j + 1) * window, T(0));
  }
  return BANN_OK;
}

// pairwise: the six-band path (the caller has checked keep_missing and that the presence image is there)
static int ld_band_impl(bann_ctx* ctx, int32_t window, int64_t first, int64_t count, float* r2_out,
                        int32_t* npairs_out, bool pairwise) {
  const int32_t bands = pairwise ? LD_BANDS : 1;
  int32_t weff = 0;
  if (int rc = ld_check(ctx, window, bands, &weff)) return rc;
  if (first < 0 || count < 0 || first + count > ctx->M) return fail(ctx, BANN_E_ARG, "marker range outside the cohort");
  if (!r2_out) return fail(ctx, BANN_E_ARG, "r2_out is null");
  ctx->ld_ms = 0.0;
  if (count == 0) return BANN_OK;
  LdScratch sc;
  int64_t brows = 0;
  if (int rc = ld_prepare(ctx, sc, weff, bands, count, &brows)) return rc;
  const int64_t stride = brows * weff;
  std::vector<float> stage;
  std::vector<int32_t> stage_n;
  double ms = 0.0;
  for (int64_t r0 = first; r0 < first + count; r0 += brows) {
    const int32_t rows = (int32_t)std::min<int64_t>(brows, first + count - r0);
    CK(hipEventRecord(sc.ev0, ctx->stream));
    if (pairwise) {
      CK(hipMemsetAsync(sc.S, 0, (size_t)stride * LD_BANDS * 4, ctx->stream));
      launch_ld_band(ctx->d_g, ctx->rowb, ctx->M, r0, rows, weff, 4 * ctx->cus, sc.S + LD_BAND_S * stride, ctx->stream);
      launch_ld_band_pw(ctx->d_g, ctx->d_pm, ctx->rowb, ctx->M, r0, rows, weff, 4 * ctx->cus, sc.S, stride, ctx->stream);
      launch_ld_r2_pw(sc.S, stride, rows, weff, r0, ctx->M, ctx->stream);
    } else {
      launch_ld_stats(ctx->d_g, ctx->rowb, r0, std::min<int64_t>(ctx->M, r0 + rows + weff) - r0, sc.st, sc.qt, ctx->stream);
      CK(hipMemsetAsync(sc.S, 0, (size_t)rows * weff * 4, ctx->stream));
      launch_ld_band(ctx->d_g, ctx->rowb, ctx->M, r0, rows, weff, 4 * ctx->cus, sc.S, ctx->stream);
      launch_ld_r2(sc.S, rows, weff, r0, ctx->M, ctx->n, r0, sc.st, sc.qt, ctx->stream);
    }
    CK(hipEventRecord(sc.ev1, ctx->stream));
    CK(hipGetLastError());
    if (int rc = ld_copy_rows(ctx, sc.S + LD_BAND_S * stride, rows, weff, window, stage,
                              r2_out + (r0 - first) * window))
      return rc;
    if (pairwise && npairs_out)
      if (int rc = ld_copy_rows(ctx, sc.S + LD_BAND_N * stride, rows, weff, window, stage_n,
                                npairs_out + (r0 - first) * window))
        return rc;
    float t = 0.f;
    CK(hipEventElapsedTime(&t, sc.ev0, sc.ev1));
    ms += t;
  }
  ctx->ld_ms = ms;
  return BANN_OK;
}

extern "C" int bann_genotypes_ld_band(bann_ctx* ctx, int32_t window, int64_t first, int64_t count, float* r2_out) {
  if (!ctx) return BANN_E_ARG;
  return ld_band_impl(ctx, window, first, count, r2_out, nullptr, false);
}

static int ld_pairwise_check(bann_ctx* ctx) {
  if (!ctx->keep_missing) return fail(ctx, BANN_E_STATE, "missing calls are not kept (bann_genotypes_keep_missing)");
  return BANN_OK;
}

extern "C" int bann_genotypes_ld_band_pairwise(bann_ctx* ctx, int32_t window, int64_t first, int64_t count,
                                               float* r2_out, int32_t* npairs_out) {
  if (!ctx) return BANN_E_ARG;
  if (int rc = ld_pairwise_check(ctx)) return rc;
  // the six-band bound holds whether the image is there or not: a window is accepted or refused for the
  // cohort's shape, not for its content
  int32_t weff = 0;
  if (int rc = ld_check(ctx, window, LD_BANDS, &weff)) return rc;
  if (ctx->d_pm) return ld_band_impl(ctx, window, first, count, r2_out, npairs_out, true);
  if (int rc = ld_band_impl(ctx, window, first, count, r2_out, nullptr, false)) return rc;
  if (npairs_out)  // everyone is present
    for (int64_t j = first; j < first + count; ++j)
      for (int64_t d = 1; d <= window; ++d)
        npairs_out[(j - first) * window + d - 1] = j + d < ctx->M ? (int32_t)ctx->n : 0;
  return BANN_OK;
}

static int ld_graph_impl(bann_ctx* ctx, int32_t window, float r2_min, const int32_t* chrom, const int64_t* bp,
                         int64_t max_bp, int64_t* num_edges, bool pairwise) {
  const int32_t bands = pairwise ? LD_BANDS : 1;
  int32_t weff = 0;
  if (int rc = ld_check(ctx, window, bands, &weff)) return rc;
  if ((chrom == nullptr) != (bp == nullptr)) return fail(ctx, BANN_E_ARG, "chrom and bp are given together or not at all");
  if (!(r2_min == r2_min)) return fail(ctx, BANN_E_ARG, "r2_min is NaN");
  const int64_t M = ctx->M;
  ctx->ld_ms = 0.0;
  ctx->ld_have = false;
  ctx->ld_off.clear();
  ctx->ld_nb.clear();
  LdScratch sc;
  int64_t brows = 0;
  if (int rc = ld_prepare(ctx, sc, weff, bands, M, &brows)) return rc;
  const int64_t stride = brows * weff;
  const int32_t words = (weff + 31) / 32;
  CK(dalloc(&sc.mask, brows * words));
  if (chrom) {
    CK(dalloc(&sc.chrom, brows + weff));
    CK(dalloc(&sc.bp, brows + weff));
  }
  std::vector<uint32_t> mask((size_t)(M * words));
  double ms = 0.0;
  for (int64_t r0 = 0; r0 < M; r0 += brows) {
    const int32_t rows = (int32_t)std::min<int64_t>(brows, M - r0);
    const int64_t nstat = std::min<int64_t>(M, r0 + rows + weff) - r0;  // the block's rows and their partners
    if (chrom) {
      CK(hipMemcpyAsync(sc.chrom, chrom + r0, (size_t)nstat * 4, hipMemcpyHostToDevice, ctx->stream));
      CK(hipMemcpyAsync(sc.bp, bp + r0, (size_t)nstat * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    CK(hipEventRecord(sc.ev0, ctx->stream));
    if (pairwise) {
      CK(hipMemsetAsync(sc.S, 0, (size_t)stride * LD_BANDS * 4, ctx->stream));
      launch_ld_band(ctx->d_g, ctx->rowb, M, r0, rows, weff, 4 * ctx->cus, sc.S + LD_BAND_S * stride, ctx->stream);
      launch_ld_band_pw(ctx->d_g, ctx->d_pm, ctx->rowb, M, r0, rows, weff, 4 * ctx->cus, sc.S, stride, ctx->stream);
      launch_ld_mask_pw(sc.S, stride, rows, weff, words, r0, M, r0, (double)r2_min, sc.chrom, sc.bp, max_bp, sc.mask,
                        ctx->stream);
    } else {
      launch_ld_stats(ctx->d_g, ctx->rowb, r0, nstat, sc.st, sc.qt, ctx->stream);
      CK(hipMemsetAsync(sc.S, 0, (size_t)rows * weff * 4, ctx->stream));
      launch_ld_band(ctx->d_g, ctx->rowb, M, r0, rows, weff, 4 * ctx->cus, sc.S, ctx->stream);
      launch_ld_mask(sc.S, rows, weff, words, r0, M, ctx->n, r0, sc.st, sc.qt, (double)r2_min, sc.chrom, sc.bp, max_bp,
                     sc.mask, ctx->stream);
    }
    CK(hipEventRecord(sc.ev1, ctx->stream));
    CK(hipGetLastError());
    CK(hipMemcpyAsync(mask.data() + r0 * words, sc.mask, (size_t)rows * words * 4, hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    float t = 0.f;
    CK(hipEventElapsedTime(&t, sc.ev0, sc.ev1));
    ms += t;
  }
  ctx->ld_ms = ms;
  // the masks are per marker and are expanded in marker order: the CSR does not depend on how the
  // device work was cut.  Node k lists its lower neighbours (ascending, as the rows j < k meet it) first.
  std::vector<int64_t> lower((size_t)M, 0), upper((size_t)M, 0);
  int64_t edges = 0;
  for (int64_t j = 0; j < M; ++j)
    for (int32_t w = 0; w < words; ++w)
      for (uint32_t b = mask[(size_t)(j * words + w)]; b; b &= b - 1) {
        const int64_t k = j + 32 * w + __builtin_ctz(b) + 1;
        ++upper[(size_t)j];
        ++lower[(size_t)k];
        ++edges;
      }
  ctx->ld_off.assign((size_t)M + 1, 0);
  for (int64_t j = 0; j < M; ++j) ctx->ld_off[(size_t)j + 1] = ctx->ld_off[(size_t)j] + lower[(size_t)j] + upper[(size_t)j];
  ctx->ld_nb.assign((size_t)(2 * edges), 0);
  std::vector<int64_t> lo_cur((size_t)M, 0);
  for (int64_t j = 0; j < M; ++j) {
    int64_t up = ctx->ld_off[(size_t)j] + lower[(size_t)j];
    for (int32_t w = 0; w < words; ++w)
      for (uint32_t b = mask[(size_t)(j * words + w)]; b; b &= b - 1) {
        const int64_t k = j + 32 * w + __builtin_ctz(b) + 1;
        ctx->ld_nb[(size_t)up++] = (int32_t)k;
        ctx->ld_nb[(size_t)(ctx->ld_off[(size_t)k] + lo_cur[(size_t)k]++)] = (int32_t)j;
      }
  }
  ctx->ld_have = true;
  if (num_edges) *num_edges = edges;
  return BANN_OK;
}

extern "C" int bann_genotypes_ld_graph(bann_ctx* ctx, int32_t window, float r2_min, const int32_t* chrom,
                                       const int64_t* bp, int64_t max_bp, int64_t* num_edges) {
  if (!ctx) return BANN_E_ARG;
  return ld_graph_impl(ctx, window, r2_min, chrom, bp, max_bp, num_edges, false);
}

extern "C" int bann_genotypes_ld_graph_pairwise(bann_ctx* ctx, int32_t window, float r2_min, const int32_t* chrom,
                                                const int64_t* bp, int64_t max_bp, int64_t* num_edges) {
  if (!ctx) return BANN_E_ARG;
  if (int rc = ld_pairwise_check(ctx)) return rc;
  int32_t weff = 0;
  if (int rc = ld_check(ctx, window, LD_BANDS, &weff)) return rc;
  return ld_graph_impl(ctx, window, r2_min, chrom, bp, max_bp, num_edges, ctx->d_pm != nullptr);
}

extern "C" int bann_genotypes_ld_graph_get(bann_ctx* ctx, int64_t* offsets, int32_t* neighbours) {
  if (!ctx) return BANN_E_ARG;
  if (!ctx->ld_have) return fail(ctx, BANN_E_STATE, "no LD graph: call bann_genotypes_ld_graph first");
  if (!offsets || !neighbours) return fail(ctx, BANN_E_ARG, "null output");
  std::copy(ctx->ld_off.begin(), ctx->ld_off.end(), offsets);
  std::copy(ctx->ld_nb.begin(), ctx->ld_nb.end(), neighbours);
  return BANN_OK;
}

extern "C" int bann_genotypes_ld_timing(const bann_ctx* ctx, double* kernel_ms) {
  if (!ctx || !kernel_ms) return BANN_E_ARG;
  *kernel_ms = ctx->ld_ms;
  return BANN_OK;
}

extern "C" int bann_genotypes_ld_scratch_limit(bann_ctx* ctx, int64_t bytes) {
  if (!ctx) return BANN_E_ARG;
  if (bytes > LD_SCRATCH_BYTES) return fail(ctx, BANN_E_ARG, "the band scratch is at most 128 MiB");
  ctx->ld_scratch = bytes <= 0 ? LD_SCRATCH_BYTES : bytes;
  return BANN_OK;
}
