// Host-only check of the gx tile numbering (rs-bann_amd/csrc/gx_shapes.h).  Prints gx_tiles for a fixed
// table -- every phase and layer of the gx parity shapes and of a branch with the widest summary layer,
// exact and not, 1 and 3 row splits, n from 1 to 10^7 -- one line per (exact, splits, shape, n) with
// `phase:count of layer 0,count of layer 1,...`, which tests/test_gx_shapes.py compares with
// tests/golden/gx_tiles.txt.  Independently of that file it asserts that every count is the
// tmc * tnc * ns of gx_dims at the phase's tile edges, is 0 for FWD / BWD / GRAD of a layer outside
// 1 <= l < L - 1, and stays below the 2^30 tiles of one launch (build_plan's limit); it exits 1 naming
// the first failures (stderr).  Built with the host C++ compiler; no GPU.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "gx_shapes.h"

static int failures = 0;
#define EXPECT(cond, ...)                                             \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (failures < 20) {                                            \
        std::fprintf(stderr, "line %d: %s: ", __LINE__, #cond);       \
        std::fprintf(stderr, __VA_ARGS__);                            \
        std::fprintf(stderr, "\n");                                   \
      }                                                               \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

struct Shape {
  int32_t m;
  std::vector<int32_t> widths;
};
// the gx shapes of tests/test_gpu_parity.py (default architecture, one layer, deep and ragged stacks)
// and a summary layer of GX_HEAD_MAXW units
static const std::vector<Shape> kShapes = {
    {300, {150, 150, 1}}, {40, {300, 1}}, {200, {100, 70, 40, 1}}, {77, {33, 5, 1}}, {129, {64, 65, 3, 1}},
    {100, {64, GX_HEAD_MAXW, 1}},
};
static const int64_t kN[] = {1, 64, 65, 1200, 4500, 50000, 10000000};

static BranchDev branch(const Shape& s, int32_t nsplits) {
  BranchDev d{};
  d.m = s.m;
  d.nchunks = (s.m + 63) / 64;
  d.L = (int32_t)s.widths.size();
  d.nsplits = nsplits;
  for (int l = 0; l < d.L; ++l) {
    d.widths[l] = s.widths[l];
    d.win[l] = l ? s.widths[l - 1] : s.m;
  }
  return d;
}

// the tile edges of phase ph: 64 x 64, the hidden phases of the bf16-plane kernel X3Shape's
static void tile_edges(int ph, bool exact, int& TM, int& TN) {
  TM = TN = 64;
  if (exact) return;
  if (ph == GX_FWD) TM = 32 * X3Shape<GX_FWD>::AX, TN = 32 * X3Shape<GX_FWD>::AY;
  if (ph == GX_BWD) TM = 32 * X3Shape<GX_BWD>::AX, TN = 32 * X3Shape<GX_BWD>::AY;
  if (ph == GX_GRAD) TM = 32 * X3Shape<GX_GRAD>::AX, TN = 32 * X3Shape<GX_GRAD>::AY;
}

static void check(const BranchDev& d, int ph, int l, int32_t nfrag, bool exact, int64_t got) {
  const bool hidden = ph == GX_FWD || ph == GX_BWD || ph == GX_GRAD;
  EXPECT(got >= 0 && got < (1ll << 30), "ph %d l %d nfrag %d: %" PRId64, ph, l, nfrag, got);
  if (hidden && (l < 1 || l >= d.L - 1)) {
    EXPECT(got == 0, "ph %d l %d: %" PRId64, ph, l, got);
    return;
  }
  int TM, TN, tmc, tnc, ns;
  tile_edges(ph, exact, TM, TN);
  gx_dims(nfrag, d, ph, l, tmc, tnc, ns, TM, TN);
  EXPECT(tmc > 0 && tnc > 0 && ns == (ph == GX_GRAD || ph == GX_GRAD0 ? d.nsplits : 1),
         "ph %d l %d: %d x %d x %d", ph, l, tmc, tnc, ns);
  EXPECT(got == (int64_t)tmc * tnc * ns, "ph %d l %d exact %d: %" PRId64 " != %d x %d x %d", ph, l, (int)exact, got,
         tmc, tnc, ns);
}

template <typename F>
static void print_table(F tiles, bool checked) {
  for (int exact = 0; exact < 2; ++exact)
    for (int32_t nsplits : {1, 3})
      for (const Shape& s : kShapes)
        for (int64_t n : kN) {
          const BranchDev d = branch(s, nsplits);
          const int32_t nfrag = (int32_t)((n + 15) / 16);
          std::printf("exact=%d splits=%d m=%d widths=", exact, nsplits, s.m);
          for (size_t i = 0; i < s.widths.size(); ++i) std::printf("%s%d", i ? "," : "", s.widths[i]);
          std::printf(" n=%" PRId64 " :", n);
          for (int ph = GX_FWD0; ph <= GX_GRAD0; ++ph) {
            std::printf(" %d:", ph);
            for (int l = 0; l < d.L; ++l) {
              const int64_t t = tiles(d, ph, l, nfrag, exact != 0);
              if (checked) check(d, ph, l, nfrag, exact != 0, t);
              std::printf("%s%" PRId64, l ? "," : "", t);
            }
          }
          std::printf("\n");
        }
}

int main() {
  print_table(gx_tiles, true);
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  return failures ? 1 : 0;
}
