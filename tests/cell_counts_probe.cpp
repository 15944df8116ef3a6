// tests/cell_counts_probe.cpp -- test infrastructure: the posting counts a cell keeps for the indexed image form (t4_assembler.cpp:
// cellCount / recount / stageImage) driven through the C ABI on the emulator build of the kernels, as a program of its own so that
// the host code can run under the sanitizers. The builder and this file are instrumented, the emulator and the kernels it runs on its
// fibers are not (their thread-local thread ids are not UBSan's business):
//   F="-O1 -g -std=c++17 -DT4_TEST_KNOBS -ffp-contract=off -I tests/hipemu"; S="-fsanitize=address,undefined -fno-sanitize-recover=undefined"
//   g++ $F -c -x c++ trust4_amd/csrc/t4_api.hip -o api.o && g++ $F -c tests/hipemu/hip_emu.cpp -o emu.o
//   g++ $F $S -c trust4_amd/csrc/t4_assembler.cpp -o asm.o && g++ $F $S -c tests/cell_counts_probe.cpp -o probe.o
//   g++ $S -o cell_counts_probe probe.o asm.o api.o emu.o -lz -lpthread
//   echo leak:run_blocks > lsan.supp && LSAN_OPTIONS=suppressions=lsan.supp ./cell_counts_probe      (the emulator keeps its fiber stacks)
// One cell set in the indexed form and a twin in the compact form: novel reads, adds that extend to the right and to the left and
// that join two contigs, ChangeKmerLength, further adds, the release of the finished barcode. Every add must answer the same in both;
// every indexed image's counts are held against the cell's own index (T4_TEST_IMAGE_CROSSCHECK). Prints "ok ..." or the first
// difference (exit 1).
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <vector>

#include "../include/trust4_hip.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ < 0) { fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, t4_last_error(ctx)); return 1; } } while (0)

int main() {
  setenv("T4_TEST_IMAGE_CROSSCHECK", "1", 1);
  t4_ctx *ctx = nullptr;
  if (t4_init(0, &ctx)) { fprintf(stderr, "t4_init failed\n"); return 1; }
  std::mt19937 rnd(77);
  const int nCells = 3;
  std::vector<std::string> tmpl(nCells);
  for (std::string &t : tmpl) for (int i = 0; i < 420; ++i) t += "ACGT"[rnd() & 3];
  t4_cellset *sets[2] = {nullptr, nullptr};
  for (int s = 0; s < 2; ++s) {
    CHECK(t4_cellset_create(ctx, 9, &sets[s]));
    CHECK(t4_cellset_set_params(sets[s], 13, 10, 0.9));
  }
  // (the first contig of cell 0 before the form is chosen: its counts are taken from the index)
  for (int s = 0; s < 2; ++s) { t4_assembler *a; CHECK(t4_cellset_cell(sets[s], 0, &a)); CHECK(t4_assembler_input_novel_read(a, "Novel", tmpl[0].substr(100, 100).c_str(), 1, 0)); }
  CHECK(t4_cellset_set_image_form(sets[0], T4_CELL_IMAGE_INDEXED));
  int adds = 0;
  auto add = [&](int bc, const std::string &read, int *ret) -> int {
    int got[2], st[2];
    for (int s = 0; s < 2; ++s) {
      t4_assembler *a;
      CHECK(t4_cellset_cell(sets[s], bc, &a));
      const char *rd = read.c_str();
      int zero = 0;
      CHECK(t4_cellset_prefetch(sets[s], 1, &a, &rd, &zero, 0));
      st[s] = 0;
      got[s] = t4_assembler_add_read(a, rd, "", &st[s], bc, 1, 0, 0.9);
    }
    if (got[0] != got[1] || st[0] != st[1]) { fprintf(stderr, "cell %d add %d: indexed %d/%d, compact %d/%d\n", bc, adds, got[0], st[0], got[1], st[1]); return 1; }
    ++adds;
    *ret = got[0];
    return 0;
  };
  for (int bc = 0; bc < nCells; ++bc) {
    const std::string &t = tmpl[bc];
    for (int s = 0; s < 2; ++s) {
      t4_assembler *a;
      CHECK(t4_cellset_cell(sets[s], bc, &a));
      if (bc > 0) CHECK(t4_assembler_input_novel_read(a, "Novel", t.substr(100, 100).c_str(), 1, bc));
      CHECK(t4_assembler_input_novel_read(a, "Novel", t.substr(260, 100).c_str(), 1, bc));
    }
    int r;
    const int cuts[][2] = {{150, 100}, {60, 100}, {300, 100}, {190, 130}, {100, 100}};
    for (const auto &c : cuts) { if (add(bc, t.substr(c[0], c[1]), &r)) return 1; if (r < 0) { fprintf(stderr, "cell %d: add of [%d, +%d) returned %d\n", bc, c[0], c[1], r); return 1; } }
    for (int s = 0; s < 2; ++s) { t4_assembler *a; CHECK(t4_cellset_cell(sets[s], bc, &a)); CHECK(t4_assembler_change_kmer_length(a, 9)); }
    const int cuts2[][2] = {{20, 90}, {330, 90}, {150, 110}};
    for (const auto &c : cuts2) { if (add(bc, t.substr(c[0], c[1]), &r)) return 1; if (r < 0) { fprintf(stderr, "cell %d: add of [%d, +%d) returned %d\n", bc, c[0], c[1], r); return 1; } }
    for (int s = 0; s < 2; ++s) {
      t4_assembler *a;
      CHECK(t4_cellset_cell(sets[s], bc, &a));
      CHECK(t4_assembler_release_finished_barcode(a, bc, 0));
      CHECK(t4_cellset_close_cell(sets[s], a));
    }
  }
  int64_t ix[6] = {0, 0, 0, 0, 0, 0}, im[4] = {0, 0, 0, 0};
  CHECK(t4_cellset_indexed_stats(sets[0], ix, 6));
  CHECK(t4_cellset_image_stats(sets[0], im, 4));
  if (ix[0] <= 0 || ix[0] != ix[5] || ix[4] != 0 || im[1] != 0) { fprintf(stderr, "counters: indexed %lld, crosschecked %lld, fallen back %lld, key records %lld\n", (long long)ix[0], (long long)ix[5], (long long)ix[4], (long long)im[1]); return 1; }
  for (int s = 0; s < 2; ++s) t4_cellset_destroy(sets[s]);
  t4_destroy(ctx);
  printf("ok %d adds equal in both forms, %lld indexed images checked against the index, %lld postings built on the device\n", adds, (long long)ix[0], (long long)ix[2]);
  return 0;
}
