// Host-only check of plan_layout and choose_gsum (rs-bann_amd/csrc/finalize_layout.h).  Prints the
// planned layout of a fixed table of cases in a canonical text form, one `case.branch.field = value`
// per line, which tests/test_finalize_layout.py compares with tests/golden/finalize_layout.txt; a
// case of more than 8 branches prints its first two and its last branch and a hash over all of
// them.  Independently of that file it asserts the invariants every layout must keep, and exits 1
// naming the first that failed (stderr).  Built with the host C++ compiler; no GPU.
#include <cinttypes>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "finalize_layout.h"

static int failures = 0;
static std::string g_case;
#define EXPECT(cond)                                                                    \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      if (failures < 20) std::fprintf(stderr, "%s: line %d: %s\n", g_case.c_str(), __LINE__, #cond); \
      ++failures;                                                                       \
    }                                                                                   \
  } while (0)

struct Shape {
  int32_t m;
  std::vector<int32_t> widths;
  int32_t prior;
};
static const int64_t kBudget = 8192ll << 18;  // bann_finalize's floor of the gx scratch budget

static std::vector<BranchHost> branches(const std::vector<Shape>& shapes) {
  std::vector<BranchHost> br;
  for (const Shape& s : shapes) {
    std::vector<int32_t> idx(s.m);
    for (int i = 0; i < s.m; ++i) idx[i] = i;
    br.push_back(make_branch(idx.data(), s.m, s.widths.data(), (int32_t)s.widths.size(), 0, s.prior));
  }
  return br;
}

// every planned field of one branch, through put(name, value)
template <typename F>
static void branch_fields(const BranchHost& h, F put) {
  const BranchDev& d = h.dev;
  char nm[32];
  auto arr = [&](const char* name, const int32_t* v, int cnt, int from = 0) {
    for (int l = from; l < cnt; ++l) {
      std::snprintf(nm, sizeof nm, "%s[%d]", name, l);
      put(nm, (int64_t)v[l]);
    }
  };
  put("fused", d.fused), put("nchunks", d.nchunks), put("nsplits", d.nsplits), put("solo_items", h.solo_items);
  put("x_off", d.x_off), put("xi_off", d.xi_off), put("dig_off", d.dig_off), put("p_off", d.p_off);
  put("mk_off", d.mk_off), put("part_off", d.part_off), put("y_off", d.y_off);
  put("q_off", d.q_off), put("nq", d.nq), put("qbias", d.qbias);
  arr("qoff", d.qoff, h.L);
  if (d.fused != PATH_GX) return;
  put("gx_group", h.gx_group), put("scr_off", d.scr_off);
  arr("gx_w", d.gx_w, h.L), arr("gx_wld", d.gx_wld, h.L), arr("gx_b", d.gx_b, h.L - 1);
  put("gx_w0p", d.gx_w0p);
  arr("gx_wp", d.gx_wp, h.L - 1, 1);
  put("gx_dwo", d.gx_dwo), put("gx_rss", d.gx_rss), put("gx_op", d.gx_op), put("gx_e", d.gx_e);
  put("gx_wps", d.gx_wps);
  arr("gx_a", d.gx_a, h.L - 1), arr("gx_h", d.gx_h, h.L - 1), arr("gx_ld", d.gx_ld, h.L - 1);
}

static void fnv(uint64_t& hash, int64_t v) {  // FNV-1a, a byte at a time
  for (int k = 0; k < 8; ++k) hash = (hash ^ ((uint64_t)v >> (8 * k) & 255)) * 1099511628211ull;
}

// prints the case; returns a hash of every total and every planned field of every branch
static uint64_t print_layout(const std::vector<BranchHost>& br, const LayoutTotals& t) {
  const char* c = g_case.c_str();
  uint64_t all = 1469598103934665603ull;
  auto tot = [&](const char* name, int64_t v) {
    fnv(all, v);
    std::printf("%s.total.%s = %" PRId64 "\n", c, name, v);
  };
  tot("nfrag", t.nfrag), tot("max_splits", t.max_splits);
  tot("tile_bytes", t.tile_bytes), tot("fi_bytes", t.fi_bytes), tot("dig_bytes", t.dig_bytes);
  tot("total_p", t.total_p), tot("total_q", t.total_q), tot("total_markers", t.total_markers);
  tot("part_total", t.part_total), tot("scr_floats", t.scr_floats), tot("fused_items", t.fused_items);
  tot("n_gx", t.n_gx), tot("gx_ngroups", t.gx_ngroups);
  tot("solo_threshold", t.solo_threshold), tot("solo_rss_cap", t.solo_rss_cap), tot("solo_part_cap", t.solo_part_cap);
  tot("gxpre_cap", t.gxpre_cap), tot("items_cap", t.items_cap);
  tot("plan_off_fold", t.plan_off_fold), tot("plan_off_items", t.plan_off_items);
  tot("plan_scr_bytes", t.plan_scr_bytes);
  const size_t nb = br.size();
  uint64_t hash = 1469598103934665603ull;  // over every field of every branch
  for (size_t b = 0; b < nb; ++b) {
    const bool show = nb <= 8 || b < 2 || b == nb - 1;
    branch_fields(br[b], [&](const char* name, int64_t v) {
      fnv(hash, v);
      if (show) std::printf("%s.%zu.%s = %" PRId64 "\n", c, b, name, v);
    });
  }
  if (nb > 8) std::printf("%s.total.branch_hash = %016" PRIx64 "\n", c, hash);
  fnv(all, (int64_t)hash);
  return all;
}

// floats of a gx branch's scratch: its last region's end
static int64_t gx_scratch_floats(const BranchHost& h, int64_t ntile) {
  return h.dev.gx_h[h.L - 2] + ntile * 64 * h.dev.gx_ld[h.L - 2];
}

static void check_invariants(const std::vector<BranchHost>& br, const LayoutTotals& t, int32_t cus, int64_t budget) {
  const int64_t ntile = (t.nfrag + BANN_TILE_FRAGS - 1) / BANN_TILE_FRAGS;
  // consecutive branches tile every region exactly: no gap, no overlap
  int64_t x = 0, xi = 0, dig = 0, p = 0, q = 0, mk = 0, part = 0, items = 0, group_end = 0, scr_max = 0;
  int32_t group = 0, group_count = 0, max_splits = 1;
  for (const BranchHost& h : br) {
    const BranchDev& d = h.dev;
    EXPECT(d.x_off == x && d.dig_off == dig && d.p_off == p && d.q_off == q && d.mk_off == mk && d.part_off == part);
    EXPECT(d.xi_off == -1 || (d.xi_off == xi && d.fused == PATH_FX));
    EXPECT(d.nq == h.nprec);
    EXPECT(1 <= d.nsplits && d.nsplits <= ntile);
    x += ntile * d.nchunks * 1024;
    if (d.xi_off >= 0) xi += 4 * ntile * ((d.nchunks + 3) / 4) * 1024;
    if (d.fused != PATH_GX) dig += (int64_t)d.nchunks * 1024 * (d.fused == PATH_WX ? 8 : 1);
    p += h.P, q += d.nq, mk += h.m, part += (int64_t)d.nsplits * h.P;
    max_splits = std::max(max_splits, d.nsplits);
    if (d.fused == PATH_FX)  // the int32 dW0 digit sums of a wave
      EXPECT((ntile + 4 * d.nsplits - 1) / (4 * d.nsplits) <= BANN_MAX_TILES_PER_WAVE);
    if (d.fused != PATH_GX) {
      items += d.nsplits;
      EXPECT(d.nsplits <= h.solo_items && h.solo_items <= std::max<int64_t>(d.nsplits, 2 * cus));
      continue;
    }
    // gx offsets in layout order: multiples of 4, increasing, below 2^31
    std::vector<int64_t> seq;
    for (int l = 0; l < h.L; ++l) seq.push_back(d.gx_w[l]);
    for (int l = 0; l < h.L - 1; ++l) seq.push_back(d.gx_b[l]);
    seq.push_back(d.gx_w0p);
    for (int l = 1; l < h.L - 1; ++l) seq.push_back(d.gx_wp[l]);
    seq.push_back(d.gx_dwo), seq.push_back(d.gx_rss), seq.push_back(d.gx_op), seq.push_back(d.gx_e);
    const size_t wps_at = seq.size();
    seq.push_back(d.gx_wps);
    for (int l = 0; l < h.L - 1; ++l) seq.push_back(d.gx_a[l]), seq.push_back(d.gx_h[l]);
    seq.push_back(gx_scratch_floats(h, ntile));
    EXPECT(seq[0] == 0);
    for (size_t i = 0; i < seq.size(); ++i) {
      EXPECT(seq[i] % 4 == 0 && seq[i] >= 0 && seq[i] < (1ll << 31));
      // Wp_s is empty without a hidden layer (L = 2): the one region that may have no extent
      if (i > 0) EXPECT(seq[i] > seq[i - 1] || (i == wps_at + 1 && h.L < 3 && seq[i] == seq[i - 1]));
    }
    for (int l = 0; l < h.L; ++l) EXPECT(d.gx_wld[l] % 4 == 0 && d.gx_wld[l] >= d.win[l]);
    for (int l = 0; l < h.L - 1; ++l) EXPECT(d.gx_ld[l] % 4 == 0 && d.gx_ld[l] >= d.widths[l]);
    // scratch groups: in index order, branches back to back, over the budget only alone
    EXPECT(h.gx_group == group || h.gx_group == group + 1);
    if (h.gx_group != group) group = h.gx_group, group_end = 0, group_count = 0;
    EXPECT(d.scr_off >= group_end && d.scr_off % 4 == 0);
    group_end = d.scr_off + gx_scratch_floats(h, ntile);
    ++group_count;
    EXPECT(group_end <= budget || group_count == 1);
    scr_max = std::max(scr_max, group_end);
  }
  EXPECT(x == t.tile_bytes && xi == t.fi_bytes && dig == t.dig_bytes && p == t.total_p && q == t.total_q);
  EXPECT(mk == t.total_markers && part == t.part_total && items == t.fused_items && scr_max == t.scr_floats);
  EXPECT(max_splits == t.max_splits && group == t.gx_ngroups);
  EXPECT(t.items_cap == t.fused_items + t.solo_rss_cap);
  EXPECT(t.plan_off_fold % 256 == 0 && t.plan_off_fold >= 8 * (int64_t)br.size());
  EXPECT(t.plan_off_items % 256 == 0 &&
         t.plan_off_items >= t.plan_off_fold + (int64_t)(br.size() * sizeof(FoldJob)));
  EXPECT(t.plan_scr_bytes == t.plan_off_items + t.items_cap * (int64_t)sizeof(GradItem));
}

struct Case {
  const char* name;
  int64_t n;
  std::vector<Shape> shapes;
  int32_t cus = 256;
  int64_t budget = kBudget;
  bool fused_enabled = true;
  EnvOptions opt{};
  int64_t M = 1 << 20;
};

static std::map<std::string, uint64_t> g_hash;  // case -> print_layout's hash

static LayoutTotals run_case(const Case& c, std::vector<BranchHost>* out = nullptr) {
  g_case = c.name;
  std::vector<BranchHost> br = branches(c.shapes);
  const LayoutTotals t = plan_layout(c.n, c.M, c.cus, c.budget, c.fused_enabled, c.opt, br);
  if (t.err) {
    std::printf("%s.error = %d %s\n", c.name, t.err, t.msg);
  } else {
    g_hash[c.name] = print_layout(br, t);
    check_invariants(br, t, c.cus, c.budget);
  }
  if (out) *out = br;
  return t;
}

static const int32_t RB = BANN_RIDGE_BASE, RA = BANN_RIDGE_ARD, LA = BANN_LASSO_ARD, LB = BANN_LASSO_BASE;

static Case with_opt(const char* name, void (*set)(EnvOptions&), std::vector<Shape> shapes, int64_t n = 50000) {
  Case c{name, n, std::move(shapes)};
  set(c.opt);
  return c;
}

int main() {
  const Shape fx500{500, {4, 4, 1}, RB};
  const std::vector<Shape> four_paths = {{500, {4, 4, 1}, RA},   {2000, {4, 4, 1}, RB}, {128, {32, 32, 1}, LA},
                                         {100, {50, 50, 1}, LB}, {300, {3, 1}, RA},     {600, {16, 8, 4, 1}, RA}};
  const size_t NFXL = 20;  // fxl branches of m 2000: 4 or 8 chunks per wave split them differently
  const std::vector<Shape> five_gx(5, Shape{1000, {64, 32, 1}, RB});
  // the path every one-branch boundary case must take
  const std::map<std::string, int> paths = {
      {"smoke", PATH_FX}, {"m512", PATH_FX},   {"m500", PATH_FX},   {"m513", PATH_FXL},  {"m2000", PATH_FXL},
      {"m2049", PATH_FXL}, {"m4096", PATH_FXL}, {"m4097", PATH_GX},  {"w5", PATH_GX},     {"w5_l4", PATH_GX},
      {"w5_wx", PATH_WX}, {"l5", PATH_GX},     {"wx128", PATH_WX},  {"wx129", PATH_GX},  {"gx100", PATH_GX}};
  std::vector<Case> cases = {
      {"smoke", 1000, {{100, {4, 4, 1}, RB}}},
      // path boundaries by m
      {"m512", 5000, {{512, {4, 4, 1}, RB}}},
      {"m500", 5000, {fx500}},
      {"m513", 5000, {{513, {4, 4, 1}, RB}}},
      {"m2000", 5000, {{2000, {4, 4, 1}, RB}}},
      {"m2049", 5000, {{2049, {4, 4, 1}, RB}}},
      {"m4096", 5000, {{4096, {4, 4, 1}, RB}}},
      {"m4097", 5000, {{4097, {4, 4, 1}, RB}}},
      // path boundaries by width and depth
      {"w5", 5000, {{500, {5, 4, 1}, RB}}},
      {"w5_l4", 5000, {{100, {5, 4, 4, 1}, RB}}},
      {"w5_wx", 5000, {{100, {5, 4, 1}, RB}}},  // one hidden layer, m <= 128: not narrow, but wx takes it
      {"l5", 5000, {{100, {4, 4, 4, 4, 1}, RB}}},
      {"wx128", 5000, {{128, {32, 32, 1}, RB}}},
      {"wx129", 5000, {{129, {32, 32, 1}, RB}}},
      {"gx100", 5000, {{100, {50, 50, 1}, RB}}},
      {"four_paths", 20000, four_paths},
      {"unfused", 20000, four_paths, 256, kBudget, false},
      {"cus32", 50000, std::vector<Shape>(125, fx500), 32},
      // every EnvOptions field the planner reads, flipped once
      with_opt("wx_exact", [](EnvOptions& o) { o.wx_exact = true; }, std::vector<Shape>(40, Shape{128, {32, 32, 1}, RB})),
      with_opt("wx_default", [](EnvOptions&) {}, std::vector<Shape>(40, Shape{128, {32, 32, 1}, RB})),
      with_opt("fwd_fi", [](EnvOptions& o) { o.fwd_fi = true; }, four_paths),
      with_opt("fwd_fi_default", [](EnvOptions&) {}, four_paths),
      with_opt("fxl_cpw8", [](EnvOptions& o) { o.fxl_cpw = 8; }, std::vector<Shape>(NFXL, Shape{2000, {4, 4, 1}, RB})),
      with_opt("fxl_cpw0", [](EnvOptions&) {}, std::vector<Shape>(NFXL, Shape{2000, {4, 4, 1}, RB})),
      with_opt("solo_default", [](EnvOptions&) {}, {fx500}),
      with_opt("solo_off", [](EnvOptions& o) { o.solo = false; }, {fx500}),
      with_opt("solo_tpw4", [](EnvOptions& o) { o.solo_tpw = 4; }, {fx500}),
      with_opt("target_items", [](EnvOptions& o) { o.target_items = 4096, o.env_split = true; },
               std::vector<Shape>(125, fx500)),
      with_opt("min_frags", [](EnvOptions& o) { o.min_frags = 16, o.env_split = true; }, {fx500, {128, {32, 32, 1}, RB}}),
      with_opt("min_frags_default", [](EnvOptions&) {}, {fx500, {128, {32, 32, 1}, RB}}),
      // the int32 digit-sum guard holds under the env split too
      with_opt("env_split_10m", [](EnvOptions& o) { o.min_frags = 1 << 30, o.env_split = true; }, {fx500}, 10000000),
      // 5 gx branches of 9 981 596 floats each under a budget of 25 M: groups of 2, 2, 1
      {"gx_three_groups", 50000, five_gx, 256, 25000000},
      {"gx_one_group", 50000, five_gx},
      {"gx_over_budget_alone", 50000, five_gx, 256, 5000000},
      // the gx shape errors, and a marker past M
      {"err_summary_width", 5000, {{100, {8, 4100, 1}, RB}}},
      {"err_scratch_2g", 10000000, {{100, {64, 64, 1}, RB}}},
      {"err_marker", 5000, {fx500}, 256, kBudget, true, EnvOptions{}, 499},
  };
  static char names[24][32];
  int k = 0;
  for (int64_t n : {1ll, 16ll, 63ll, 64ll, 65ll, 1000ll, 50000ll, 10000000ll})
    for (int nb : {1, 125, 1000}) {
      std::snprintf(names[k], sizeof names[k], "n%lld_b%d", (long long)n, nb);
      cases.push_back({names[k++], n, std::vector<Shape>((size_t)nb, fx500)});
    }
  for (const Case& c : cases) {
    std::vector<BranchHost> br;
    const LayoutTotals t = run_case(c, &br);
    const std::string nm = c.name;
    if (nm.rfind("err_", 0) == 0) EXPECT(t.err == BANN_E_SHAPE);
    else EXPECT(t.err == BANN_OK);
    // the example of best_splits' own comment: 500 items in one round at 49 tiles per wave,
    // against 66 at 3 splits and two rounds at 5
    if (nm == "n50000_b125") EXPECT(br[0].dev.nsplits == 4 && t.fused_items == 500);
    const auto want = paths.find(nm);
    if (want != paths.end()) EXPECT(br.size() == 1 && br[0].dev.fused == want->second);
    if (nm == "gx_three_groups") EXPECT(t.gx_ngroups == 2 && br[1].gx_group == 0 && br[2].gx_group == 1 && br[4].gx_group == 2);
  }
  // a flipped option is seen: its layout differs from the same case at the defaults
  g_case = "flips";
  const char* const flips[][2] = {{"wx_exact", "wx_default"},   {"fwd_fi", "fwd_fi_default"},
                                  {"fxl_cpw8", "fxl_cpw0"},     {"solo_off", "solo_default"},
                                  {"solo_tpw4", "solo_default"}, {"target_items", "n50000_b125"},
                                  {"min_frags", "min_frags_default"}, {"cus32", "n50000_b125"},
                                  {"unfused", "four_paths"}};
  for (const auto& f : flips) {
    if (g_hash.count(f[0]) && g_hash.count(f[1]) && g_hash[f[0]] != g_hash[f[1]]) continue;
    std::fprintf(stderr, "flips: %s plans as %s\n", f[0], f[1]);
    ++failures;
  }
  // the premise of tests/test_fxl_items_gpu.py, which cannot see a split count: 64 same-shape fxl
  // branches at n = 3000 (47 tiles), never re-split (BANN_SOLO=0), make items of at least 5 tiles --
  // more than fxh's FXH_NSL slots, so its slot refill runs -- with or without the head-wave kernel
  // (the split count of an fxl group does not depend on fxl_head), while one such branch alone gets
  // one tile per item.  Not printed: the golden file keeps its cases
  g_case = "long_items";
  {
    struct Row {
      int32_t m, nsplits;
    };
    const Row rows[] = {{577, 8}, {1100, 4}, {2048, 4}, {2100, 4}};
    const int64_t n = 3000, ntile = 47;
    EnvOptions opt;
    opt.solo = false;
    for (const Row& r : rows)
      for (int head : {1, 0})
        for (int32_t layers : {2, 3, 4}) {
          std::vector<int32_t> widths((size_t)layers, 4);
          widths.back() = 1;
          opt.fxl_head = head != 0;
          std::vector<BranchHost> br = branches(std::vector<Shape>(64, Shape{r.m, widths, RA}));
          const LayoutTotals t = plan_layout(n, 1 << 20, 256, kBudget, true, opt, br);
          EXPECT(t.err == BANN_OK && t.solo_threshold == 0);
          EXPECT((t.nfrag + BANN_TILE_FRAGS - 1) / BANN_TILE_FRAGS == ntile);
          for (const BranchHost& h : br) {
            EXPECT(h.dev.fused == PATH_FXL && h.dev.nchunks == (r.m + 63) / 64);
            EXPECT(h.dev.nsplits == r.nsplits);
            for (int64_t s = 0; s < h.dev.nsplits; ++s)
              EXPECT(ntile * (s + 1) / h.dev.nsplits - ntile * s / h.dev.nsplits > FXH_NSL);
          }
          std::vector<BranchHost> one = branches({Shape{r.m, widths, RA}});
          const LayoutTotals t1 = plan_layout(n, 1 << 20, 256, kBudget, true, opt, one);
          EXPECT(t1.err == BANN_OK && one[0].dev.fused == PATH_FXL && one[0].dev.nsplits == ntile);
        }
  }
  // the (R, k) of the network forward's group sums: an item never spans more than tmax tiles
  g_case = "gsum";
  const int64_t tmax = 100, slots = 256;
  for (int64_t ntile : {1ll, 100ll, 101ll, 782ll, 51200ll, 51201ll, 156250ll})
    for (int64_t nb : {1ll, 8ll, 9ll, 1000ll})
      for (int force_r : {0, 2}) {
        const GsumChoice c = choose_gsum(ntile, nb, slots, tmax, force_r);
        std::printf("gsum.ntile%lld.nb%lld.r%d = ", (long long)ntile, (long long)nb, force_r);
        if (c.found) std::printf("%lld %lld\n", (long long)c.R, (long long)c.k);
        else std::printf("none\n");
        EXPECT(c.found == (ntile <= 512 * tmax));
        EXPECT(!choose_gsum(ntile, nb, slots, tmax, 33).found);  // no R above 32
        if (!c.found) continue;
        EXPECT(c.R >= 1 && c.R <= 32 && (!force_r || c.R == force_r) && c.k >= 1 && c.k <= 512);
        for (int64_t s = 0; s < c.k; ++s) EXPECT(ntile * (s + 1) / c.k - ntile * s / c.k <= tmax);
      }
  if (failures) {
    std::fprintf(stderr, "%d invariant(s) failed\n", failures);
    return 1;
  }
  return 0;
}
