// bann_genotypes.hip — genotype ingestion of include/bann.h: the 2-bit cohort image and its
// presence image, upload (int8, .bed payload), synthetic cohorts, marker statistics, download.
#include <algorithm>
#include <vector>

#include "ctx_internal.h"

// the cohort image, its presence image and the marker statistics
void genotypes_release(bann_ctx* ctx) {
  dfree_all(ctx->d_g, ctx->d_pm, ctx->d_mu, ctx->d_sigma);
}

int alloc_genotypes(bann_ctx* ctx, int64_t n, int64_t M) {
  if (ctx->finalized) return fail(ctx, BANN_E_STATE, "genotypes must be set before bann_finalize");
  if (n <= 0 || M <= 0) return fail(ctx, BANN_E_SHAPE, "n and num_markers must be positive");
  CK(hipSetDevice(ctx->device));
  genotypes_release(ctx);
  ctx->missing_total = 0;
  ctx->has_code3 = false;
  ctx->n = n;
  ctx->M = M;
  ctx->rowb = (n + 63) / 64 * 16;
  CK(dalloc(&ctx->d_g, ctx->rowb * M));
  CK(dalloc(&ctx->d_mu, M));
  CK(dalloc(&ctx->d_sigma, M));
  return BANN_OK;
}

int alloc_presence(bann_ctx* ctx) {
  if (!ctx->keep_missing) return BANN_OK;
  CK(dalloc(&ctx->d_pm, ctx->rowb * ctx->M));
  return BANN_OK;
}

int finish_presence(bann_ctx* ctx) {
  if (!ctx->d_pm) return BANN_OK;
  int32_t* d_cnt = nullptr;
  CK(dalloc(&d_cnt, ctx->M));
  std::vector<int32_t> cnt((size_t)ctx->M);
  launch_missing_counts(ctx->d_pm, ctx->rowb, ctx->n, 0, ctx->M, d_cnt, ctx->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(cnt.data(), d_cnt, (size_t)ctx->M * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  dfree(d_cnt);
  CK(e);
  ctx->missing_total = 0;
  for (int32_t c : cnt) ctx->missing_total += c;
  if (ctx->missing_total == 0) {  // everyone is present: the pairwise calls need no image for that
    dfree(ctx->d_pm);
    ctx->d_pm = nullptr;
  }
  return BANN_OK;
}

extern "C" int bann_genotypes_keep_missing(bann_ctx* ctx, int32_t keep) {
  if (!ctx) return BANN_E_ARG;
  if (ctx->M > 0) return fail(ctx, BANN_E_STATE, "bann_genotypes_keep_missing comes before the genotypes are loaded");
  ctx->keep_missing = keep != 0;
  return BANN_OK;
}

extern "C" int bann_genotypes_missing_counts(bann_ctx* ctx, int64_t first, int64_t count, int32_t* out) {
  if (!ctx) return BANN_E_ARG;
  if (!ctx->keep_missing) return fail(ctx, BANN_E_STATE, "missing calls are not kept (bann_genotypes_keep_missing)");
  if (!ctx->d_g) return fail(ctx, BANN_E_STATE, "the cohort image is not resident (no genotypes loaded, or freed at bann_finalize)");
  if (first < 0 || count < 0 || first + count > ctx->M) return fail(ctx, BANN_E_ARG, "marker range outside the cohort");
  if (count == 0) return BANN_OK;
  if (!out) return fail(ctx, BANN_E_ARG, "out is null");
  if (!ctx->d_pm) {  // no missing call in the cohort
    std::fill(out, out + count, 0);
    return BANN_OK;
  }
  CK(hipSetDevice(ctx->device));
  int32_t* d_cnt = nullptr;
  CK(dalloc(&d_cnt, count));
  launch_missing_counts(ctx->d_pm, ctx->rowb, ctx->n, first, count, d_cnt, ctx->stream);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_cnt, (size_t)count * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  dfree(d_cnt);
  CK(e);
  return BANN_OK;
}

// markers per staged block: ~256 MiB of host input per copy
int64_t stage_markers(int64_t bytes_per_marker, int64_t M) {
  return std::max<int64_t>(1, std::min<int64_t>(M, (int64_t(256) << 20) / std::max<int64_t>(1, bytes_per_marker)));
}

extern "C" int bann_genotypes_upload(bann_ctx* ctx, const int8_t* g, int64_t n, int64_t num_markers) {
  if (!ctx || !g) return BANN_E_ARG;
  int rc = alloc_genotypes(ctx, n, num_markers);
  if (rc) return rc;
  // int8 [M][n] streamed through a bounded staging block, packed to 2 bits on the device
  const int64_t blk = stage_markers(n, num_markers);
  int8_t* d_st = nullptr;
  int32_t* d_flag = nullptr;
  int32_t flag = 0;
  CK(dalloc(&d_st, blk * n));
  CK(dalloc(&d_flag, 1));
  CK(hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream));
  for (int64_t j0 = 0; j0 < num_markers; j0 += blk) {
    const int64_t m = std::min(blk, num_markers - j0);
    CK(hipMemcpyAsync(d_st, g + j0 * n, (size_t)(m * n), hipMemcpyHostToDevice, ctx->stream));
    launch_i8_to_raw(d_st, n, m, ctx->d_g + j0 * ctx->rowb, ctx->rowb, d_flag, ctx->stream);
    CK(hipGetLastError());
  }
  launch_col_stats(ctx->d_g, ctx->rowb, ctx->d_mu, ctx->d_sigma, n, num_markers, ctx->stream);
  CK(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  dfree(d_st);
  dfree(d_flag);
  if (flag & 1) return fail(ctx, BANN_E_ARG, "genotypes must be 2-bit codes in 0..3 (.bed semantics)");
  ctx->has_code3 = (flag & 2) != 0;
  return BANN_OK;
}

extern "C" int bann_genotypes_upload_bed(bann_ctx* ctx, const uint8_t* payload, int64_t n, int64_t num_markers) {
  if (!ctx || !payload) return BANN_E_ARG;
  int rc = alloc_genotypes(ctx, n, num_markers);
  if (!rc) rc = alloc_presence(ctx);
  if (rc) return rc;
  // payload rows streamed through a bounded staging block, decoded into the 2-bit image
  const int64_t bpc = (n + 3) / 4;
  const int64_t blk = stage_markers(bpc, num_markers);
  uint8_t* d_st = nullptr;
  CK(dalloc(&d_st, blk * bpc));
  for (int64_t j0 = 0; j0 < num_markers; j0 += blk) {
    const int64_t m = std::min(blk, num_markers - j0);
    CK(hipMemcpyAsync(d_st, payload + j0 * bpc, (size_t)(m * bpc), hipMemcpyHostToDevice, ctx->stream));
    launch_bed_to_raw(d_st, n, m, ctx->d_g + j0 * ctx->rowb, ctx->rowb, ctx->stream);
    if (ctx->d_pm) launch_bed_to_presence(d_st, n, m, ctx->d_pm + j0 * ctx->rowb, ctx->rowb, ctx->stream);
    CK(hipGetLastError());
  }
  launch_col_stats(ctx->d_g, ctx->rowb, ctx->d_mu, ctx->d_sigma, n, num_markers, ctx->stream);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->stream));
  dfree(d_st);
  return finish_presence(ctx);
}

extern "C" int bann_genotypes_synthetic(bann_ctx* ctx, int64_t n, int64_t num_markers, uint64_t seed) {
  if (!ctx) return BANN_E_ARG;
  int rc = alloc_genotypes(ctx, n, num_markers);
  if (rc) return rc;
  launch_synthetic_genotypes(ctx->d_g, ctx->rowb, ctx->d_mu, ctx->d_sigma, n, num_markers, nullptr, seed, ctx->stream);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->stream));
  return BANN_OK;
}

extern "C" int bann_genotypes_synthetic_maf(bann_ctx* ctx, int64_t n, int64_t num_markers, const float* maf,
                                            uint64_t seed) {
  if (!ctx) return BANN_E_ARG;
  if (!maf) return fail(ctx, BANN_E_ARG, "maf is null");
  for (int64_t j = 0; j < num_markers; ++j)
    if (!(maf[j] >= 0.f && maf[j] <= 1.f)) return fail(ctx, BANN_E_ARG, "an allele frequency outside [0, 1]");
  int rc = alloc_genotypes(ctx, n, num_markers);
  if (rc) return rc;
  float* d_maf = nullptr;
  CK(dalloc(&d_maf, num_markers));
  hipError_t e = hipMemcpyAsync(d_maf, maf, (size_t)num_markers * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    launch_synthetic_genotypes(ctx->d_g, ctx->rowb, ctx->d_mu, ctx->d_sigma, n, num_markers, d_maf, seed, ctx->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  dfree(d_maf);
  CK(e);
  return BANN_OK;
}

// a caller's index list as the device's int32 list, checked against [0, limit)
static bool subset_list(const int64_t* idx, int64_t count, int64_t limit, std::vector<int32_t>& out) {
  out.resize((size_t)count);
  for (int64_t t = 0; t < count; ++t) {
    if (idx[t] < 0 || idx[t] >= limit) return false;
    out[(size_t)t] = (int32_t)idx[t];
  }
  return true;
}

// plink --keep / --extract --make-bed (scripts/split_train_test.sh) between two resident cohorts
extern "C" int bann_genotypes_subset(bann_ctx* dst, bann_ctx* src, const int64_t* individuals, int64_t n_keep,
                                     const int64_t* markers, int64_t m_keep) {
  if (!dst || !src) return BANN_E_ARG;
  bann_ctx* ctx = dst;
  if (dst == src) return fail(ctx, BANN_E_ARG, "bann_genotypes_subset needs two contexts");
  if (dst->device != src->device) return fail(ctx, BANN_E_ARG, "source and destination are on different devices");
  if (dst->finalized) return fail(ctx, BANN_E_STATE, "genotypes must be set before bann_finalize");
  if (!src->d_g) return fail(ctx, BANN_E_STATE, "the source's cohort image is not resident (no genotypes loaded, or freed at bann_finalize)");
  if (src->n > INT32_MAX || src->M > INT32_MAX) return fail(ctx, BANN_E_SHAPE, "the source cohort exceeds 32-bit indices");
  if ((individuals && n_keep <= 0) || (markers && m_keep <= 0)) return fail(ctx, BANN_E_ARG, "an index list needs at least one entry");
  std::vector<int32_t> ind, mk;
  if (individuals && !subset_list(individuals, n_keep, src->n, ind)) return fail(ctx, BANN_E_SHAPE, "individual index out of range");
  if (markers && !subset_list(markers, m_keep, src->M, mk)) return fail(ctx, BANN_E_SHAPE, "marker index out of range");
  const int64_t n = individuals ? n_keep : src->n, M = markers ? m_keep : src->M;
  int rc = alloc_genotypes(dst, n, M);
  if (rc) return rc;
  dst->keep_missing = src->keep_missing;
  if (src->d_pm) CK(dalloc(&dst->d_pm, dst->rowb * M));
  dst->subset_ms = 0.0;
  int32_t *d_ind = nullptr, *d_mk = nullptr, *d_flag = nullptr;
  hipEvent_t ev_src = nullptr, ev0 = nullptr, ev1 = nullptr;
  int32_t flag = 0;
  float ms = 0.f;
  auto run = [&]() -> hipError_t {
    hipError_t e;
#define SUB_TRY(call) \
  if ((e = (call)) != hipSuccess) return e
    // after everything the source's stream has been given
    SUB_TRY(hipEventCreateWithFlags(&ev_src, hipEventDisableTiming));
    SUB_TRY(hipEventRecord(ev_src, src->stream));
    SUB_TRY(hipStreamWaitEvent(dst->stream, ev_src, 0));
    SUB_TRY(hipEventCreate(&ev0));
    SUB_TRY(hipEventCreate(&ev1));
    if (individuals) {
      SUB_TRY(dalloc(&d_ind, n));
      SUB_TRY(hipMemcpyAsync(d_ind, ind.data(), (size_t)n * 4, hipMemcpyHostToDevice, dst->stream));
    }
    if (markers) {
      SUB_TRY(dalloc(&d_mk, M));
      SUB_TRY(hipMemcpyAsync(d_mk, mk.data(), (size_t)M * 4, hipMemcpyHostToDevice, dst->stream));
    }
    SUB_TRY(dalloc(&d_flag, 1));
    SUB_TRY(hipMemsetAsync(d_flag, 0, sizeof(int32_t), dst->stream));
    SUB_TRY(hipEventRecord(ev0, dst->stream));
    if (!individuals && !markers) {  // a copy: the same rows, the same rowb
      SUB_TRY(hipMemcpyAsync(dst->d_g, src->d_g, (size_t)(dst->rowb * M), hipMemcpyDeviceToDevice, dst->stream));
      if (dst->d_pm)
        SUB_TRY(hipMemcpyAsync(dst->d_pm, src->d_pm, (size_t)(dst->rowb * M), hipMemcpyDeviceToDevice, dst->stream));
    } else {
      launch_subset(src->d_g, src->d_pm, src->rowb, d_ind, d_mk, dst->d_g, dst->d_pm, dst->rowb, n, M, d_flag,
                    dst->stream);
      SUB_TRY(hipGetLastError());
    }
    SUB_TRY(hipEventRecord(ev1, dst->stream));
    launch_col_stats(dst->d_g, dst->rowb, dst->d_mu, dst->d_sigma, n, M, dst->stream);
    SUB_TRY(hipGetLastError());
    SUB_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, dst->stream));
    SUB_TRY(hipStreamSynchronize(dst->stream));
    SUB_TRY(hipEventElapsedTime(&ms, ev0, ev1));
#undef SUB_TRY
    return hipSuccess;
  };
  const hipError_t e = run();
  dfree(d_ind);
  dfree(d_mk);
  dfree(d_flag);
  if (ev_src) (void)hipEventDestroy(ev_src);
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  CK(e);
  dst->subset_ms = ms;
  dst->has_code3 = (!individuals && !markers) ? src->has_code3 : flag != 0;
  return finish_presence(dst);
}

extern "C" int bann_genotypes_subset_timing(const bann_ctx* ctx, double* kernel_ms) {
  if (!ctx || !kernel_ms) return BANN_E_ARG;
  *kernel_ms = ctx->subset_ms;
  return BANN_OK;
}

// plink --fill-missing-a2 (scripts/fill_missing_a2.sh): the image already holds a missing call as 0, the
// homozygous-A2 value, so filling is forgetting which calls were missing
extern "C" int bann_genotypes_fill_missing_a2(bann_ctx* ctx) {
  if (!ctx) return BANN_E_ARG;
  if (ctx->M <= 0 || !ctx->d_mu) return fail(ctx, BANN_E_STATE, "no genotypes");
  CK(hipSetDevice(ctx->device));
  CK(hipStreamSynchronize(ctx->stream));
  dfree(ctx->d_pm);
  ctx->d_pm = nullptr;
  ctx->missing_total = 0;
  return BANN_OK;
}

extern "C" int bann_genotypes_stats(bann_ctx* ctx, float* mu, float* sigma) {
  if (!ctx || !ctx->d_mu) return fail(ctx, BANN_E_STATE, "no genotypes");
  if (mu) CK(hipMemcpy(mu, ctx->d_mu, ctx->M * sizeof(float), hipMemcpyDeviceToHost));
  if (sigma) CK(hipMemcpy(sigma, ctx->d_sigma, ctx->M * sizeof(float), hipMemcpyDeviceToHost));
  return BANN_OK;
}

extern "C" int bann_genotypes_set_stats(bann_ctx* ctx, const float* mu, const float* sigma) {
  if (!ctx || !mu || !sigma) return BANN_E_ARG;
  if (!ctx->d_mu) return fail(ctx, BANN_E_STATE, "no genotypes");
  if (ctx->finalized) return fail(ctx, BANN_E_STATE, "statistics are folded at bann_finalize; set them before");
  CK(hipMemcpy(ctx->d_mu, mu, ctx->M * sizeof(float), hipMemcpyHostToDevice));
  CK(hipMemcpy(ctx->d_sigma, sigma, ctx->M * sizeof(float), hipMemcpyHostToDevice));
  return BANN_OK;
}

extern "C" int bann_genotypes_download(bann_ctx* ctx, const int32_t* snp_idx, int32_t m, int8_t* g_out) {
  if (!ctx || !snp_idx || !g_out || m <= 0) return BANN_E_ARG;
  if (!ctx->d_g) return fail(ctx, BANN_E_STATE, "raw genotypes not resident (freed at finalize?)");
  for (int i = 0; i < m; ++i)
    if (snp_idx[i] < 0 || snp_idx[i] >= ctx->M) return fail(ctx, BANN_E_SHAPE, "marker index out of range");
  int32_t* d_idx = nullptr;
  int8_t* d_out = nullptr;
  CK(dalloc(&d_idx, m));
  CK(dalloc(&d_out, (int64_t)m * ctx->n));
  CK(hipMemcpyAsync(d_idx, snp_idx, m * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  launch_unpack_markers(ctx->d_g, ctx->rowb, d_idx, m, ctx->n, d_out, ctx->stream);
  CK(hipMemcpyAsync(g_out, d_out, (size_t)m * ctx->n, hipMemcpyDeviceToHost, ctx->stream));
  CK(hipStreamSynchronize(ctx->stream));
  dfree(d_idx);
  dfree(d_out);
  return BANN_OK;
}

