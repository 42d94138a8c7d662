// Stand-alone host check of the group-by-ld file functions of csrc/bann_io.cpp (built by
// test_ld_grouping_cpu.py with -fsanitize=address,undefined and run as a child process):
// the reference's own known answer (centered.rs:174-192), an empty graph, a graph that founds
// no group, a truncated .ld and a one-column .bim.
//   usage: ld_grouping_check <small.ld> <small.bim> <scratch dir>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../include/bann.h"

static int fails = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      printf("FAIL line %d: %s (%s)\n", __LINE__, #c, bann_io_last_error()); \
      ++fails;                                                   \
    }                                                            \
  } while (0)

static void write_text(const std::string& path, const char* text) {
  FILE* f = fopen(path.c_str(), "wb");
  if (f) {
    fputs(text, f);
    fclose(f);
  }
}

static std::vector<std::vector<int32_t>> grouping(int64_t M, const std::vector<int64_t>& off,
                                                  const std::vector<int32_t>& nb, int32_t min_size, int64_t* ungrouped,
                                                  int* rc_out) {
  int32_t G = -1;
  int64_t E = -1;
  std::vector<std::vector<int32_t>> out;
  *rc_out = bann_grouping_centered(M, off.data(), nb.data(), min_size, &G, &E, nullptr, nullptr, ungrouped);
  if (*rc_out != BANN_OK) return out;
  std::vector<int64_t> go((size_t)G + 1, -1);
  std::vector<int32_t> gm((size_t)E + 1, -1);
  *rc_out = bann_grouping_centered(M, off.data(), nb.data(), min_size, &G, &E, go.data(), gm.data(), ungrouped);
  for (int32_t g = 0; g < G; ++g) out.emplace_back(gm.begin() + go[g], gm.begin() + go[g + 1]);
  return out;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string ld = argv[1], bim = argv[2], dir = argv[3];
  int rc = 0;
  // the reference's known answer
  {
    int64_t M = 0, E = 0;
    EXPECT(bann_ld_graph_read_plink(ld.c_str(), bim.c_str(), &M, &E, nullptr, nullptr) == BANN_OK);
    EXPECT(M == 11 && E == 7);
    std::vector<int64_t> off((size_t)M + 1);
    std::vector<int32_t> nb((size_t)(2 * E) + 1);
    EXPECT(bann_ld_graph_read_plink(ld.c_str(), bim.c_str(), &M, &E, off.data(), nb.data()) == BANN_OK);
    int64_t un = -1;
    const auto g = grouping(M, off, nb, 1, &un, &rc);
    const std::vector<std::vector<int32_t>> want = {{0, 1, 2, 3}, {3, 4, 5}, {6, 7, 8, 9, 10}};
    EXPECT(rc == BANN_OK && g == want && un == 0);
    // writer and reader round trip
    const std::string out = dir + "/kat.groups";
    std::vector<int64_t> go = {0, 4, 7, 12};
    std::vector<int32_t> gm = {0, 1, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10};
    EXPECT(bann_grouping_write(out.c_str(), 3, go.data(), gm.data()) == BANN_OK);
    int32_t G = 0;
    int64_t N = 0;
    EXPECT(bann_grouping_read(out.c_str(), &G, &N, nullptr, nullptr) == BANN_OK && G == 3 && N == 12);
    std::vector<int64_t> ro(4);
    std::vector<int32_t> rm(12);
    EXPECT(bann_grouping_read(out.c_str(), &G, &N, ro.data(), rm.data()) == BANN_OK && ro == go && rm == gm);
    // .bim columns 1 and 4
    int64_t mb = 0;
    std::vector<int32_t> chrom(11);
    std::vector<int64_t> bp(11);
    EXPECT(bann_bim_read(bim.c_str(), &mb, chrom.data(), bp.data()) == BANN_OK && mb == 11);
    for (int j = 0; j < 11; ++j) EXPECT(chrom[j] == 0 && bp[j] == j + 1);
  }
  // an empty graph: no markers, then markers without a single edge
  {
    std::vector<int64_t> off = {0};
    std::vector<int32_t> nb = {0};
    int64_t un = -1;
    auto g = grouping(0, off, nb, 1, &un, &rc);
    EXPECT(rc == BANN_OK && g.empty() && un == 0);
    off.assign(6, 0);
    g = grouping(5, off, nb, 1, &un, &rc);
    EXPECT(rc == BANN_OK && g.empty() && un == 5);
    const std::string out = dir + "/empty.groups";
    EXPECT(bann_grouping_write(out.c_str(), 0, off.data(), nb.data()) == BANN_OK);
    int32_t G = -1;
    int64_t N = -1;
    EXPECT(bann_grouping_read(out.c_str(), &G, &N, nullptr, nullptr) == BANN_OK && G == 0 && N == 0);
  }
  // edges, but no node's degree exceeds min_group_size: no group at all
  {
    std::vector<int64_t> off = {0, 1, 3, 4};  // the path 0 - 1 - 2
    std::vector<int32_t> nb = {1, 0, 2, 1};
    int64_t un = -1;
    const auto g = grouping(3, off, nb, 2, &un, &rc);
    EXPECT(rc == BANN_OK && g.empty() && un == 3);
    std::vector<int32_t> bad = {1, 0, 3, 1};
    grouping(3, off, bad, 2, &un, &rc);
    EXPECT(rc == BANN_E_SHAPE);
  }
  // a truncated .ld, an unknown id, a one-column .bim, missing files
  {
    int64_t M = 0, E = 0;
    const std::string cut = dir + "/cut.ld";
    write_text(cut, " CHR_A BP_A SNP_A CHR_B BP_B SNP_B R2\n 19 1 rs1 19 2 rs2 1\n 19 1 rs1 19\n");
    EXPECT(bann_ld_graph_read_plink(cut.c_str(), bim.c_str(), &M, &E, nullptr, nullptr) == BANN_E_SHAPE);
    const std::string unk = dir + "/unknown.ld";
    write_text(unk, " CHR_A BP_A SNP_A CHR_B BP_B SNP_B R2\n 19 1 rs1 19 2 rs77 1\n");
    EXPECT(bann_ld_graph_read_plink(unk.c_str(), bim.c_str(), &M, &E, nullptr, nullptr) == BANN_E_ARG);
    EXPECT(strstr(bann_io_last_error(), "rs77") != nullptr);
    const std::string self = dir + "/self.ld";
    write_text(self, "header\n 19 1 rs1 19 1 rs1 1\n 19 1 rs2 19 1 rs1 1\n 19 1 rs1 19 1 rs2 1\n\n");
    EXPECT(bann_ld_graph_read_plink(self.c_str(), bim.c_str(), &M, &E, nullptr, nullptr) == BANN_OK && M == 11 && E == 1);
    const std::string one = dir + "/one.bim";
    write_text(one, "19\n19\n");
    EXPECT(bann_ld_graph_read_plink(ld.c_str(), one.c_str(), &M, &E, nullptr, nullptr) == BANN_E_SHAPE);
    int64_t mb = 0;
    EXPECT(bann_bim_read(one.c_str(), &mb, nullptr, nullptr) == BANN_E_SHAPE);
    const std::string none = dir + "/missing";
    EXPECT(bann_ld_graph_read_plink(none.c_str(), bim.c_str(), &M, &E, nullptr, nullptr) == BANN_E_ARG);
    EXPECT(bann_ld_graph_read_plink(ld.c_str(), none.c_str(), &M, &E, nullptr, nullptr) == BANN_E_ARG);
    EXPECT(bann_bim_read(none.c_str(), &mb, nullptr, nullptr) == BANN_E_ARG);
  }
  printf(fails ? "%d failures\n" : "ok\n", fails);
  return fails ? 1 : 0;
}
