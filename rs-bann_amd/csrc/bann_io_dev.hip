// bann_io_dev.hip — BedVM::from_file (io/bed.rs:193-245) onto the device: the
// .bed signature is checked (variant-major only, as the reference), the dims
// come from stem.dims or the .fam/.bim line counts, and the payload streams from
// the file through a bounded pinned block into the 2-bit genotype image
// (kernels_data.hip) -- the file is never held whole in host memory.
#include <stdio.h>

#include <algorithm>
#include <string>

#include "ctx_internal.h"

extern "C" int bann_genotypes_load_bed(bann_ctx* ctx, const char* stem) {
  if (!ctx || !stem) return BANN_E_ARG;
  int64_t n = 0, M = 0;
  if (bann_bed_dims(stem, &n, &M) != BANN_OK) return fail(ctx, BANN_E_ARG, "no .dims or .fam/.bim next to the .bed");
  const std::string path = std::string(stem) + ".bed";
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return fail(ctx, BANN_E_ARG, "cannot open " + path);
  unsigned char sig[3] = {0, 0, 0};
  if (fread(sig, 1, 3, f) != 3 || sig[0] != 0x6c || sig[1] != 0x1b || (sig[2] != 0x00 && sig[2] != 0x01)) {
    fclose(f);
    return fail(ctx, BANN_E_ARG, "unexpected .bed signature (bed.rs:104-117)");
  }
  if (sig[2] == 0x00) {
    fclose(f);
    return fail(ctx, BANN_E_ARG, "sample-major .bed is not supported (bed.rs:200-202)");
  }
  int rc = alloc_genotypes(ctx, n, M);
  if (!rc) rc = alloc_presence(ctx);
  if (rc) {
    fclose(f);
    return rc;
  }
  const int64_t bpc = (n + 3) / 4;
  const int64_t blk = stage_markers(bpc, M);
  uint8_t *h = nullptr, *d = nullptr;
  if (hipHostMalloc((void**)&h, (size_t)(blk * bpc), hipHostMallocDefault) != hipSuccess || dalloc(&d, blk * bpc)) {
    fclose(f);
    if (h) (void)hipHostFree(h);
    return fail(ctx, BANN_E_OOM, "staging buffers");
  }
  for (int64_t j0 = 0; j0 < M && rc == BANN_OK; j0 += blk) {
    const int64_t m = std::min(blk, M - j0);
    if (fread(h, 1, (size_t)(m * bpc), f) != (size_t)(m * bpc)) {
      rc = fail(ctx, BANN_E_SHAPE, ".bed payload shorter than the dims announce");
      break;
    }
    if (hipMemcpyAsync(d, h, (size_t)(m * bpc), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = BANN_E_HIP;
    launch_bed_to_raw(d, n, m, ctx->d_g + j0 * ctx->rowb, ctx->rowb, ctx->stream);
    if (ctx->d_pm) launch_bed_to_presence(d, n, m, ctx->d_pm + j0 * ctx->rowb, ctx->rowb, ctx->stream);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, BANN_E_HIP, "bed decode");  // h is reused
  }
  fclose(f);
  (void)hipHostFree(h);
  dfree(d);
  if (rc) return rc;
  launch_col_stats(ctx->d_g, ctx->rowb, ctx->d_mu, ctx->d_sigma, n, M, ctx->stream);
  CK(hipGetLastError());
  CK(hipStreamSynchronize(ctx->stream));
  return finish_presence(ctx);
}

// BedVM::to_file (io/bed.rs:248-264): the image back to .bed codes on the device, block by block through
// the same bounded pinned stage, then stem.dims
extern "C" int bann_genotypes_save_bed(bann_ctx* ctx, const char* stem) {
  if (!ctx || !stem) return BANN_E_ARG;
  if (!ctx->d_g) return fail(ctx, BANN_E_STATE, "the cohort image is not resident (no genotypes loaded, or freed at bann_finalize)");
  if (ctx->lf_active) return fail(ctx, BANN_E_STATE, "a leapfrog session is active");
  CK(hipSetDevice(ctx->device));
  const int64_t n = ctx->n, M = ctx->M;
  const std::string path = std::string(stem) + ".bed";
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return fail(ctx, BANN_E_ARG, "cannot create " + path);
  const unsigned char sig[3] = {0x6c, 0x1b, 0x01};
  const int64_t bpc = (n + 3) / 4;
  const int64_t blk = stage_markers(bpc, M);
  uint8_t *h = nullptr, *d = nullptr;
  int32_t* d_flag = nullptr;
  int32_t flag = 0;
  int rc = BANN_OK;
  if (hipHostMalloc((void**)&h, (size_t)(blk * bpc), hipHostMallocDefault) != hipSuccess || dalloc(&d, blk * bpc) ||
      dalloc(&d_flag, 1) || hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream) != hipSuccess)
    rc = fail(ctx, BANN_E_OOM, "staging buffers");
  if (!rc && fwrite(sig, 1, 3, f) != 3) rc = fail(ctx, BANN_E_ARG, "cannot write " + path);
  for (int64_t j0 = 0; j0 < M && rc == BANN_OK; j0 += blk) {
    const int64_t m = std::min(blk, M - j0);
    launch_raw_to_bed(ctx->d_g, ctx->d_pm, ctx->rowb, n, j0, m, d, d_flag, ctx->stream);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(h, d, (size_t)(m * bpc), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = fail(ctx, BANN_E_HIP, "bed encode");
    else if (flag)
      rc = fail(ctx, BANN_E_ARG, "a genotype field holds 3: no .bed code stands for it");
    else if (fwrite(h, 1, (size_t)(m * bpc), f) != (size_t)(m * bpc))
      rc = fail(ctx, BANN_E_ARG, "cannot write " + path);
  }
  if (fclose(f) != 0 && !rc) rc = fail(ctx, BANN_E_ARG, "cannot write " + path);
  if (h) (void)hipHostFree(h);
  dfree(d);
  dfree(d_flag);
  if (rc) {
    remove(path.c_str());
    return rc;
  }
  const std::string dpath = std::string(stem) + ".dims";
  FILE* g = fopen(dpath.c_str(), "wb");
  if (!g) return fail(ctx, BANN_E_ARG, "cannot create " + dpath);
  const bool ok = fprintf(g, "%lld\t%lld", (long long)n, (long long)M) > 0;
  if (fclose(g) != 0 || !ok) return fail(ctx, BANN_E_ARG, "cannot write " + dpath);
  return BANN_OK;
}
