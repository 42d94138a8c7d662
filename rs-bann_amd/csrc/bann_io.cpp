// bann_io.cpp — the files on either side of the path (host only): PLINK .bed
// dims, ExternalGrouping / UniformGrouping marker index lists and the bincode
// .phen phenotypes.  bann_genotypes_load_bed (device streaming) is in bann_io_dev.hip.
//
//   BedDims::from_dims_file / from_plink_fileset     io/dims.rs:15-34
//   ExternalGrouping::from_file                       group/external.rs:15-60
//   UniformGrouping::new                              group/uniform.rs:11-23
//   Phenotypes::from_file / to_file (bincode Vec<f32>) data/phenotypes.rs:28-36
//   SNPId2Ix::from_bim, CorrGraph::from_plink_ld      group/centered.rs:15-42, 54-89
//   CorrGraph::centered_grouping                      group/centered.rs:91-133
//   MarkerGrouping::to_file                           group/grouping.rs:16-31
//   BlockNetCfg::add_branch (the width rules)         net/architectures.rs:93-122
//   PhenStats::to_file                                data/phen_stats.rs:6-24
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/bann.h"

static thread_local std::string io_err;

// the message of the last failing host-only call of this thread; the functions that only return a
// code clear it, so that bann_io_last_error never describes an earlier call
static int io_fail(int code, const std::string& msg) {
  io_err = msg;
  return code;
}

extern "C" const char* bann_io_last_error(void) { return io_err.c_str(); }

static int64_t count_lines(const std::string& path) {
  std::ifstream f(path);
  if (!f) return -1;
  int64_t k = 0;
  std::string line;
  while (std::getline(f, line)) ++k;
  return k;
}

extern "C" int bann_bed_dims(const char* stem, int64_t* n_out, int64_t* num_markers_out) {
  io_err.clear();
  if (!stem || !n_out || !num_markers_out) return BANN_E_ARG;
  const std::string s(stem);
  std::ifstream dims(s + ".dims");
  if (dims) {  // "num_individuals num_markers" on the first line
    int64_t n = -1, m = -1;
    std::string line;
    std::getline(dims, line);
    std::istringstream ls(line);
    if (!(ls >> n >> m) || n <= 0 || m <= 0) return BANN_E_SHAPE;
    *n_out = n;
    *num_markers_out = m;
    return BANN_OK;
  }
  const int64_t n = count_lines(s + ".fam"), m = count_lines(s + ".bim");  // one line per individual / marker
  if (n <= 0 || m <= 0) return BANN_E_ARG;
  *n_out = n;
  *num_markers_out = m;
  return BANN_OK;
}

// two-column text "marker_ix group_ix" (0-based); groups must be 0 .. G-1; markers
// keep their file order within a group.  CSR result: offsets[G+1], markers[entries].
extern "C" int bann_grouping_read(const char* path, int32_t* num_groups, int64_t* num_entries, int64_t* offsets,
                                  int32_t* markers) {
  io_err.clear();
  if (!path || !num_groups || !num_entries) return BANN_E_ARG;
  std::ifstream f(path);
  if (!f) return BANN_E_ARG;
  std::map<int64_t, std::vector<int32_t>> groups;
  std::string line;
  int64_t entries = 0;
  while (std::getline(f, line)) {
    std::istringstream ls(line);
    int64_t mk, g;
    if (!(ls >> mk >> g)) {
      if (line.find_first_not_of(" \t\r") == std::string::npos) continue;  // blank line
      return BANN_E_SHAPE;
    }
    if (mk < 0 || g < 0 || mk > INT32_MAX) return BANN_E_SHAPE;
    groups[g].push_back((int32_t)mk);
    ++entries;
  }
  const int64_t G = (int64_t)groups.size();
  if (G > 0 && groups.rbegin()->first != G - 1) return BANN_E_SHAPE;  // continuous 0-based indices (external.rs:46-49)
  *num_groups = (int32_t)G;
  *num_entries = entries;
  if (offsets && markers) {
    int64_t o = 0;
    for (int64_t g = 0; g < G; ++g) {
      offsets[g] = o;
      for (int32_t mk : groups[g]) markers[o++] = mk;
    }
    offsets[G] = o;
  }
  return BANN_OK;
}

extern "C" int bann_grouping_uniform(int32_t num_groups, int32_t group_size, int64_t* offsets, int32_t* markers) {
  io_err.clear();
  if (num_groups <= 0 || group_size <= 0 || !offsets || !markers) return BANN_E_ARG;
  for (int64_t g = 0; g <= num_groups; ++g) offsets[g] = g * group_size;
  for (int64_t i = 0; i < (int64_t)num_groups * group_size; ++i) markers[i] = (int32_t)i;
  return BANN_OK;
}

// bincode 1.3 (legacy config) of `struct Phenotypes { y: Vec<f32> }`: u64 length, then the values, little endian
extern "C" int bann_phen_read(const char* path, int64_t* n_out, float* y_out) {
  io_err.clear();
  if (!path || !n_out) return BANN_E_ARG;
  FILE* f = fopen(path, "rb");
  if (!f) return BANN_E_ARG;
  uint64_t len = 0;
  int rc = BANN_OK;
  if (fread(&len, 8, 1, f) != 1) {
    rc = BANN_E_SHAPE;
  } else {
    *n_out = (int64_t)len;
    if (y_out && fread(y_out, sizeof(float), len, f) != len) rc = BANN_E_SHAPE;
  }
  fclose(f);
  return rc;
}

extern "C" int bann_phen_write(const char* path, const float* y, int64_t n) {
  io_err.clear();
  if (!path || !y || n < 0) return BANN_E_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) return BANN_E_ARG;
  const uint64_t len = (uint64_t)n;
  const bool ok = fwrite(&len, 8, 1, f) == 1 && fwrite(y, sizeof(float), (size_t)n, f) == (size_t)n;
  return (fclose(f) == 0 && ok) ? BANN_OK : BANN_E_ARG;
}

static std::vector<std::string> split_ws(const std::string& line) {
  std::vector<std::string> f;
  std::istringstream ls(line);
  std::string w;
  while (ls >> w) f.push_back(w);
  return f;
}

// the .bim lines as fields; blank lines are skipped
static int bim_lines(const char* path, size_t min_fields, std::vector<std::vector<std::string>>& out) {
  std::ifstream f(path);
  if (!f) return io_fail(BANN_E_ARG, std::string("cannot open ") + path);
  std::string line;
  while (std::getline(f, line)) {
    std::vector<std::string> fld = split_ws(line);
    if (fld.empty()) continue;
    if (fld.size() < min_fields)
      return io_fail(BANN_E_SHAPE, std::string(path) + ": line " + std::to_string(out.size() + 1) + " has " +
                                       std::to_string(fld.size()) + " columns, " + std::to_string(min_fields) + " needed");
    out.push_back(std::move(fld));
  }
  return BANN_OK;
}

extern "C" int bann_bim_read(const char* path, int64_t* num_markers, int32_t* chrom_out, int64_t* bp_out) {
  if (!path || !num_markers) return io_fail(BANN_E_ARG, "null argument");
  std::vector<std::vector<std::string>> rows;
  if (int rc = bim_lines(path, 4, rows)) return rc;
  std::map<std::string, int32_t> chroms;
  for (size_t j = 0; j < rows.size(); ++j) {
    const int32_t c = chroms.emplace(rows[j][0], (int32_t)chroms.size()).first->second;
    size_t used = 0;
    long long bp = 0;
    try {
      bp = std::stoll(rows[j][3], &used);
    } catch (...) {
      used = 0;
    }
    if (used == 0 || used != rows[j][3].size())
      return io_fail(BANN_E_SHAPE, std::string(path) + ": position '" + rows[j][3] + "' is no integer");
    if (chrom_out) chrom_out[j] = c;
    if (bp_out) bp_out[j] = (int64_t)bp;
  }
  *num_markers = (int64_t)rows.size();
  return BANN_OK;
}

extern "C" int bann_ld_graph_read_plink(const char* ld_path, const char* bim_path, int64_t* num_markers,
                                        int64_t* num_edges, int64_t* offsets, int32_t* neighbours) {
  if (!ld_path || !bim_path || !num_markers || !num_edges) return io_fail(BANN_E_ARG, "null argument");
  std::vector<std::vector<std::string>> rows;
  if (int rc = bim_lines(bim_path, 2, rows)) return rc;
  const int64_t M = (int64_t)rows.size();
  if (M > INT32_MAX) return io_fail(BANN_E_SHAPE, "more markers than int32 holds");
  std::map<std::string, int32_t> id2ix;
  for (int64_t j = 0; j < M; ++j) id2ix[rows[j][1]] = (int32_t)j;
  std::ifstream f(ld_path);
  if (!f) return io_fail(BANN_E_ARG, std::string("cannot open ") + ld_path);
  std::vector<std::pair<int32_t, int32_t>> dir;  // both directions
  std::string line;
  for (int64_t lix = 0; std::getline(f, line); ++lix) {
    if (lix == 0) continue;  // header
    const std::vector<std::string> fld = split_ws(line);
    if (fld.empty()) continue;
    if (fld.size() < 6)
      return io_fail(BANN_E_SHAPE, std::string(ld_path) + ": line " + std::to_string(lix + 1) + " has " +
                                       std::to_string(fld.size()) + " fields, 6 needed");
    int32_t ix[2];
    for (int e = 0; e < 2; ++e) {
      const auto it = id2ix.find(fld[e == 0 ? 2 : 5]);
      if (it == id2ix.end())
        return io_fail(BANN_E_ARG, std::string(ld_path) + ": line " + std::to_string(lix + 1) + ": SNP id '" +
                                       fld[e == 0 ? 2 : 5] + "' is not in " + bim_path);
      ix[e] = it->second;
    }
    if (ix[0] == ix[1]) continue;  // a self pair is dropped
    dir.emplace_back(ix[0], ix[1]);
    dir.emplace_back(ix[1], ix[0]);
  }
  std::sort(dir.begin(), dir.end());
  dir.erase(std::unique(dir.begin(), dir.end()), dir.end());
  *num_markers = M;
  *num_edges = (int64_t)dir.size() / 2;
  if (offsets && neighbours) {
    for (int64_t j = 0; j <= M; ++j) offsets[j] = 0;
    for (const auto& e : dir) ++offsets[e.first + 1];
    for (int64_t j = 0; j < M; ++j) offsets[j + 1] += offsets[j];
    for (size_t e = 0; e < dir.size(); ++e) neighbours[e] = dir[e].second;  // sorted by (node, neighbour)
  }
  return BANN_OK;
}

extern "C" int bann_grouping_centered(int64_t num_markers, const int64_t* offsets, const int32_t* neighbours,
                                      int32_t min_group_size, int32_t* num_groups, int64_t* num_entries,
                                      int64_t* g_offsets, int32_t* g_markers, int64_t* num_ungrouped) {
  if (num_markers < 0 || num_markers > INT32_MAX || !offsets || !num_groups || !num_entries || min_group_size < 0 ||
      (num_markers > 0 && offsets[num_markers] > 0 && !neighbours))
    return io_fail(BANN_E_ARG, "bann_grouping_centered: invalid argument");
  const int64_t M = num_markers;
  for (int64_t j = 0; j < M; ++j)
    if (offsets[j + 1] < offsets[j]) return io_fail(BANN_E_SHAPE, "bann_grouping_centered: offsets decrease");
  for (int64_t e = 0; e < (M > 0 ? offsets[M] : 0); ++e)
    if (neighbours[e] < 0 || neighbours[e] >= M) return io_fail(BANN_E_SHAPE, "bann_grouping_centered: neighbour out of range");
  std::vector<int32_t> order((size_t)M);
  for (int64_t j = 0; j < M; ++j) order[(size_t)j] = (int32_t)j;
  auto deg = [&](int32_t j) { return offsets[j + 1] - offsets[j]; };
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return deg(a) > deg(b); });
  std::vector<char> no_center((size_t)M, 0);
  std::vector<std::vector<int32_t>> groups;
  int64_t ungrouped = 0;
  for (const int32_t cix : order) {
    if (no_center[(size_t)cix]) continue;
    if (deg(cix) > 0 && deg(cix) > (int64_t)min_group_size) {
      std::vector<int32_t> g(neighbours + offsets[cix], neighbours + offsets[cix + 1]);
      g.push_back(cix);
      for (int32_t mk : g) no_center[(size_t)mk] = 1;
      groups.push_back(std::move(g));
    } else {  // the closest group BY GROUP INDEX to the node's index
      const int64_t G = (int64_t)groups.size();
      bool found = false;
      for (int64_t d = 1; d < 100 && !found; ++d) {
        const int64_t lo = (int64_t)cix - d, hi = (int64_t)cix + d;
        if (lo >= 0 && lo < G) {
          groups[(size_t)lo].push_back(cix);
          found = true;
        } else if (hi < G) {
          groups[(size_t)hi].push_back(cix);
          found = true;
        }
      }
      if (!found) ++ungrouped;
    }
  }
  if (groups.size() > (size_t)INT32_MAX) return io_fail(BANN_E_SHAPE, "more groups than int32 holds");
  int64_t entries = 0;
  for (auto& g : groups) {
    std::sort(g.begin(), g.end());
    g.erase(std::unique(g.begin(), g.end()), g.end());  // a duplicate edge in the caller's CSR
    entries += (int64_t)g.size();
  }
  *num_groups = (int32_t)groups.size();
  *num_entries = entries;
  if (num_ungrouped) *num_ungrouped = ungrouped;
  if (g_offsets && g_markers) {
    int64_t o = 0;
    for (size_t g = 0; g < groups.size(); ++g) {
      g_offsets[g] = o;
      for (int32_t mk : groups[g]) g_markers[o++] = mk;
    }
    g_offsets[groups.size()] = o;
  }
  return BANN_OK;
}

extern "C" int bann_grouping_write(const char* path, int32_t num_groups, const int64_t* offsets,
                                   const int32_t* markers) {
  if (!path || num_groups < 0 || !offsets || (num_groups > 0 && offsets[num_groups] > 0 && !markers))
    return io_fail(BANN_E_ARG, "bann_grouping_write: invalid argument");
  FILE* f = fopen(path, "wb");
  if (!f) return io_fail(BANN_E_ARG, std::string("cannot open ") + path);
  bool ok = true;
  for (int32_t g = 0; g < num_groups && ok; ++g)
    for (int64_t e = offsets[g]; e < offsets[g + 1] && ok; ++e) ok = fprintf(f, "%d\t%d\n", (int)markers[e], (int)g) > 0;
  return (fclose(f) == 0 && ok) ? BANN_OK : io_fail(BANN_E_ARG, std::string("write failed: ") + path);
}

// BlockNetCfg::add_branch (architectures.rs:93-122): the hidden width is formed whatever the depth,
// the summary width derives from it
extern "C" int bann_arch_layer_widths(int32_t m, int32_t depth, int32_t hidden_rule, int32_t hidden_fixed,
                                      float hidden_fraction, int32_t summary_rule, int32_t summary_fixed,
                                      float summary_fraction, int32_t* layer_widths_out) {
  if (!layer_widths_out) return io_fail(BANN_E_ARG, "bann_arch_layer_widths: null output");
  if (m < 1 || depth < 0 || depth + 2 > 8) return io_fail(BANN_E_ARG, "bann_arch_layer_widths: m < 1 or depth outside 0..6");
  // (size_t)((float)a * f).max(1): the f32 product truncated toward zero; a product beyond int32 is refused
  auto fraction_of = [](int32_t a, float f, int32_t& out) {
    if (!(f >= 0.f)) return false;
    const float v = (float)a * f;
    if (!(v < 2147483648.f)) return false;
    out = (int32_t)v < 1 ? 1 : (int32_t)v;
    return true;
  };
  int32_t hidden = 0, summary = 0;
  if (hidden_rule == 0) {
    if (hidden_fixed < 1) return io_fail(BANN_E_ARG, "bann_arch_layer_widths: fixed hidden width < 1");
    hidden = hidden_fixed;
  } else if (hidden_rule != 1 || !fraction_of(m, hidden_fraction, hidden)) {
    return io_fail(BANN_E_ARG, "bann_arch_layer_widths: unknown hidden rule or bad fraction");
  }
  if (summary_rule == 0) {
    if (summary_fixed < 1)
      return io_fail(BANN_E_ARG, "bann_arch_layer_widths: a branch cannot have summary layer width 0");
    summary = summary_fixed;
  } else if (summary_rule == 1) {
    summary = hidden;
  } else if (summary_rule != 2 || !fraction_of(hidden, summary_fraction, summary)) {
    return io_fail(BANN_E_ARG, "bann_arch_layer_widths: unknown summary rule or bad fraction");
  }
  io_err.clear();
  for (int32_t l = 0; l < depth; ++l) layer_widths_out[l] = hidden;
  layer_widths_out[depth] = summary;
  layer_widths_out[depth + 1] = 1;
  return depth + 2;
}

// a JSON number that reads back to the same f32: the fewest significant digits that do, with a
// fraction part or an exponent (serde_json writes floats so); non-finite: null
static std::string json_f32(float v) {
  if (!std::isfinite(v)) return "null";
  char buf[40];
  for (int p = 1; p <= 9; ++p) {
    snprintf(buf, sizeof(buf), "%.*g", p, (double)v);
    if (strtof(buf, nullptr) == v) break;
  }
  std::string s(buf);
  if (s.find_first_of(".e") == std::string::npos) s += ".0";
  return s;
}

extern "C" int bann_phen_stats_write(const char* path, float mean, float variance, float env_variance) {
  if (!path) return io_fail(BANN_E_ARG, "bann_phen_stats_write: null path");
  FILE* f = fopen(path, "wb");
  if (!f) return io_fail(BANN_E_ARG, std::string("cannot open ") + path);
  const std::string text = "{\n  \"mean\": " + json_f32(mean) + ",\n  \"variance\": " + json_f32(variance) +
                           ",\n  \"env_variance\": " + json_f32(env_variance) + "\n}";
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  io_err.clear();
  return (fclose(f) == 0 && ok) ? BANN_OK : io_fail(BANN_E_ARG, std::string("write failed: ") + path);
}
