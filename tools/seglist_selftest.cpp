// tools/seglist_selftest.cpp -- stand-alone check of the segment-list
// packer's pure core (tempi_amd/csrc/core/seglist_core.hpp: run merging and
// table building over integer arrays; no MPI, no HIP). Meant to run under the
// host sanitizers:
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -Itempi_amd/csrc/core tools/seglist_selftest.cpp -o build/seglist_selftest
//   build/seglist_selftest
// (one command line; `make selftest` does both)
//
// Exits non-zero on the first mismatch.
#include "seglist_core.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using tempi::seg::Table;
using tempi::seg::build_table;

namespace {

int failures = 0;

typedef std::vector<int64_t> V;

void expect(bool ok, const char *what, const char *name) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s: %s\n", name, what);
  failures++;
}

// run build_table on (disp, len) and compare with the expected table
void check(const char *name, const V &disp, const V &len, int64_t extent, int64_t cap, bool fits, const V &edisp,
           const V &elen, int64_t lowest, int64_t runAlign, int64_t align) {
  Table t;
  // exact-size heap copies: a read past either end is an ASan report
  int64_t *d = new int64_t[disp.size()], *l = new int64_t[len.size()];
  for (size_t i = 0; i < disp.size(); ++i) d[i] = disp[i], l[i] = len[i];
  const bool ok = build_table(d, l, int64_t(disp.size()), extent, cap, &t);
  delete[] d;
  delete[] l;
  expect(ok == fits, "cap verdict", name);
  if (!fits) {
    expect(t.disp.empty() && t.len.empty() && t.pre.empty() && t.size == 0, "over the cap leaves an empty table", name);
    return;
  }
  expect(t.disp == edisp, "displacements", name);
  expect(t.len == elen, "lengths", name);
  expect(t.pre.size() == edisp.size() + 1 && t.pre[0] == 0, "prefix shape", name);
  int64_t sum = 0;
  for (size_t i = 0; i < elen.size() && i + 1 < t.pre.size(); ++i) {
    expect(t.pre[i] == sum, "prefix value", name);
    sum += elen[i];
  }
  expect(t.size == sum && t.pre.back() == sum, "size", name);
  expect(t.extent == extent, "extent", name);
  if (!edisp.empty()) expect(t.lowest == lowest, "lowest displacement", name);
  expect(t.runAlign == runAlign, "run alignment", name);
  expect(t.align == align, "alignment", name);
}

} // namespace

int main() {
  // empty input
  check("empty", {}, {}, 0, 8, true, {}, {}, 0, 16, 16);
  {
    Table t;
    expect(build_table(nullptr, nullptr, 0, 24, 0, &t) && t.size == 0 && t.pre.size() == 1, "null arrays, n = 0", "empty");
  }
  // all-zero lengths: every run dropped, nothing counts against the cap
  check("zero lengths", {0, 8, 100}, {0, 0, 0}, 128, 0, true, {}, {}, 0, 16, 16);
  // a single run
  check("single", {48}, {32}, 96, 1, true, {48}, {32}, 48, 16, 16);
  check("single odd", {3}, {5}, 9, 1, true, {3}, {5}, 3, 1, 1);
  // fully mergeable: each run starts where the previous one ends
  check("mergeable", {8, 16, 24, 40}, {8, 8, 16, 8}, 64, 1, true, {8}, {40}, 8, 8, 8);
  // zero-length runs between mergeable ones do not break the merge
  check("mergeable with holes", {0, 4, 4, 8}, {4, 0, 4, 4}, 12, 1, true, {0}, {12}, 0, 4, 4);
  // out of order and negative: kept in type-map order, never sorted, and a
  // run that ends where an EARLIER run starts is not merged
  check("out of order", {40, -16, 8, 0}, {4, 2, 6, 8}, 48, 8, true, {40, -16, 8, 0}, {4, 2, 6, 8}, -16, 2, 2);
  check("negative merge", {-32, -16, 64}, {16, 16, 16}, -64, 8, true, {-32, 64}, {32, 16}, -32, 16, 16);
  check("backwards neighbours", {8, 0}, {8, 8}, 16, 8, true, {8, 0}, {8, 8}, 0, 8, 8);
  // the extent narrows `align` but not `runAlign`
  check("extent alignment", {0, 32}, {16, 16}, 52, 8, true, {0, 32}, {16, 16}, 0, 16, 4);
  // beyond 2^31
  check("large", {0, (int64_t(1) << 31) + 64, 3 * (int64_t(1) << 30) + 8}, {24, 8, 40}, int64_t(1) << 32, 8, true,
        {0, (int64_t(1) << 31) + 64, 3 * (int64_t(1) << 30) + 8}, {24, 8, 40}, 0, 8, 8);
  // exactly at the cap, and one past it
  {
    V d, l;
    for (int i = 0; i < 1000; ++i) d.push_back(3 * i), l.push_back(1 + i % 2);
    // (odd i: 2 bytes reach 3 * i + 2, one short of the next run: nothing merges)
    check("at the cap", d, l, 3000, 1000, true, d, l, 0, 1, 1);
    check("one past the cap", d, l, 3000, 999, false, {}, {}, 0, 0, 0);
    // merged runs are what counts: 1000 blocks, 500 runs
    V d2, l2, ed, el;
    for (int i = 0; i < 500; ++i) {
      d2.push_back(16 * i), l2.push_back(4);
      d2.push_back(16 * i + 4), l2.push_back(4);
      ed.push_back(16 * i), el.push_back(8);
    }
    check("merged at the cap", d2, l2, 8000, 500, true, ed, el, 0, 8, 8);
    check("merged past the cap", d2, l2, 8000, 499, false, {}, {}, 0, 0, 0);
  }
  if (failures) {
    std::fprintf(stderr, "seglist_selftest: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("seglist_selftest: ok\n");
  return 0;
}
