// Host-only check of read_env_options (rs-bann_amd/csrc/env_options.h): the documented default of
// every field with nothing set, and the parse of each kind of switch.  Built and run by
// tests/test_env_options.py with the host C++ compiler; exits 0 and prints "ok", or names the
// first expectation that failed.
#include <cstdio>
#include <cstdlib>

#include "env_options.h"

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);    \
      ++failures;                                                \
    }                                                            \
  } while (0)

static const char* const kAll[] = {
    "BANN_WX_EXACT",   "BANN_GX_EXACT", "BANN_NET_ERR",     "BANN_NET_GSUM",  "BANN_NET_GSUM_R",    "BANN_FWD_FI",
    "BANN_FI_WAVES_PER_SIMD", "BANN_FXL_HEAD", "BANN_FXL_CPW", "BANN_FUSE_UPDATE", "BANN_SOLO",     "BANN_SOLO_TPW",
    "BANN_TARGET_ITEMS", "BANN_MIN_FRAGS", "BANN_GX_SCRATCH_MB", "BANN_STAMPS",   "BANN_HMC_GRAPH"};

static void clear_all() {
  for (const char* v : kAll) unsetenv(v);
}
// the options with exactly one variable set
static EnvOptions with(const char* name, const char* value) {
  clear_all();
  setenv(name, value, 1);
  return read_env_options();
}

int main() {
  clear_all();
  {  // nothing set: INTEGRATION.md's defaults
    const EnvOptions o = read_env_options();
    EXPECT(!o.wx_exact && !o.gx_exact);
    EXPECT(o.net_err && o.net_gsum && o.net_gsum_r == 0);
    EXPECT(!o.fwd_fi && o.fi_waves_per_simd == 3);
    EXPECT(o.fxl_head && o.fxl_cpw == 0);
    EXPECT(!o.fuse_update);
    EXPECT(o.solo && o.solo_tpw == 1);
    EXPECT(o.target_items == 1024 && o.min_frags == 64 && !o.env_split);
    EXPECT(o.gx_scratch_mb == 0);
    EXPECT(!o.stamps);
    EXPECT(o.hmc_graph == -1);
  }
  // booleans: atoi(...) != 0, whichever way the default points
  EXPECT(with("BANN_WX_EXACT", "1").wx_exact && !with("BANN_WX_EXACT", "0").wx_exact);
  EXPECT(with("BANN_GX_EXACT", "1").gx_exact && !with("BANN_GX_EXACT", "0").gx_exact);
  EXPECT(with("BANN_GX_EXACT", "2").gx_exact && !with("BANN_GX_EXACT", "yes").gx_exact);
  EXPECT(with("BANN_NET_ERR", "1").net_err && !with("BANN_NET_ERR", "0").net_err);
  EXPECT(with("BANN_NET_GSUM", "1").net_gsum && !with("BANN_NET_GSUM", "0").net_gsum);
  EXPECT(with("BANN_FWD_FI", "1").fwd_fi && !with("BANN_FWD_FI", "0").fwd_fi);
  EXPECT(with("BANN_FXL_HEAD", "1").fxl_head && !with("BANN_FXL_HEAD", "0").fxl_head);
  EXPECT(with("BANN_FUSE_UPDATE", "1").fuse_update && !with("BANN_FUSE_UPDATE", "0").fuse_update);
  // plain numbers
  EXPECT(with("BANN_FI_WAVES_PER_SIMD", "2").fi_waves_per_simd == 2);
  EXPECT(with("BANN_FXL_CPW", "8").fxl_cpw == 8 && with("BANN_FXL_CPW", "4").fxl_cpw == 4);
  // clamped to >= 1
  EXPECT(with("BANN_SOLO_TPW", "4").solo_tpw == 4 && with("BANN_SOLO_TPW", "0").solo_tpw == 1);
  EXPECT(with("BANN_NET_GSUM_R", "3").net_gsum_r == 3 && with("BANN_NET_GSUM_R", "0").net_gsum_r == 1);
  EXPECT(with("BANN_TARGET_ITEMS", "0").target_items == 1 && with("BANN_TARGET_ITEMS", "-5").target_items == 1);
  EXPECT(with("BANN_TARGET_ITEMS", "5000000000").target_items == 5000000000ll);
  EXPECT(with("BANN_MIN_FRAGS", "0").min_frags == 1 && with("BANN_MIN_FRAGS", "16").min_frags == 16);
  // unset is not "0": either split variable, at any value, takes fx off its own split
  EXPECT(with("BANN_TARGET_ITEMS", "1024").env_split && with("BANN_TARGET_ITEMS", "1024").min_frags == 64);
  EXPECT(with("BANN_MIN_FRAGS", "64").env_split && with("BANN_MIN_FRAGS", "64").target_items == 1024);
  EXPECT(with("BANN_GX_SCRATCH_MB", "0").gx_scratch_mb == 1 && with("BANN_GX_SCRATCH_MB", "8192").gx_scratch_mb == 8192);
  EXPECT(with("BANN_SOLO", "0").solo == false && with("BANN_SOLO", "1").solo == true);  // unset: on (above)
  EXPECT(with("BANN_HMC_GRAPH", "0").hmc_graph == 0 && with("BANN_HMC_GRAPH", "1").hmc_graph == 1);  // unset: -1
  EXPECT(with("BANN_STAMPS", "0").stamps && with("BANN_STAMPS", "1").stamps);  // set at all
  // one variable leaves the others at their defaults
  EXPECT(!with("BANN_WX_EXACT", "1").gx_exact && with("BANN_WX_EXACT", "1").net_err);
  if (failures) return 1;
  std::puts("ok");
  return 0;
}
