// tempi_amd/csrc/core/seglist_core.hpp -- the pure core of the segment-list
// packer: run merging and table building over integer arrays. No MPI, no HIP,
// header-only, so that it compiles alone (tools/seglist_selftest.cpp runs it
// under ASan + UBSan).
//
// A segment list is the type map of ONE element as byte runs (disp, len) in
// MPI type-map order. A run is merged with the previous one only when it
// starts exactly where that one ends (the rule of oracle/typemap.c:27-29);
// runs are never sorted and never merged out of order, displacements are
// 64-bit and may be negative or out of order, zero-length runs are dropped.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace tempi {
namespace seg {

// lowest set bit of (16 | every value): the largest power of two <= 16 that
// divides them all (two's complement keeps the low bits of negative values)
inline int64_t align_of(uint64_t bits) {
  bits |= 16;
  return int64_t(bits & (~bits + 1));
}

// Runs pushed one at a time. Once more than `cap` merged runs would be held,
// over() is set and nothing more is stored: memory stays bounded by the cap.
class Merger {
public:
  explicit Merger(int64_t cap) : cap_(cap < 0 ? 0 : cap) {}

  // false once the cap has been passed
  bool push(int64_t disp, int64_t len) {
    if (over_) return false;
    if (len <= 0) return true;
    bytes_ += len;
    if (!disp_.empty() && disp_.back() + len_.back() == disp) {
      len_.back() += len;
      return true;
    }
    if (int64_t(disp_.size()) >= cap_) {
      over_ = true;
      return false;
    }
    disp_.push_back(disp);
    len_.push_back(len);
    return true;
  }

  bool over() const { return over_; }
  int64_t bytes() const { return bytes_; }
  int64_t size() const { return int64_t(disp_.size()); }
  const std::vector<int64_t> &disp() const { return disp_; }
  const std::vector<int64_t> &len() const { return len_; }

private:
  int64_t cap_;
  bool over_ = false;
  int64_t bytes_ = 0;
  std::vector<int64_t> disp_, len_;
};

// What the packer keeps for a committed type.
struct Table {
  std::vector<int64_t> disp, len; // merged runs, type-map order
  std::vector<int64_t> pre;       // exclusive prefix of len, n + 1 entries (pre[n] = size)
  int64_t size = 0;               // packed bytes of one element
  int64_t extent = 0;
  int64_t lowest = 0;    // the smallest disp: a byte the type really touches
  int64_t runAlign = 16; // gcd of every disp and len, capped at 16
  int64_t align = 16;    // ... and of the extent
};

// Merge n input runs and build the table. False (and *out empty) when the
// merged run count exceeds `cap`. An input with no bytes gives an empty table
// (size 0, no runs) and true.
inline bool build_table(const int64_t *disp, const int64_t *len, int64_t n, int64_t extent, int64_t cap,
                        Table *out) {
  *out = Table();
  Merger m(cap);
  for (int64_t i = 0; i < n; ++i)
    if (!m.push(disp[i], len[i])) return false;
  out->disp = m.disp();
  out->len = m.len();
  out->extent = extent;
  out->pre.assign(out->disp.size() + 1, 0);
  uint64_t bits = 0;
  for (size_t i = 0; i < out->disp.size(); ++i) {
    out->pre[i + 1] = out->pre[i] + out->len[i];
    bits |= uint64_t(out->disp[i]) | uint64_t(out->len[i]);
    if (i == 0 || out->disp[i] < out->lowest) out->lowest = out->disp[i];
  }
  out->size = out->pre.back();
  out->runAlign = align_of(bits);
  out->align = align_of(bits | uint64_t(extent));
  return true;
}

} // namespace seg
} // namespace tempi
