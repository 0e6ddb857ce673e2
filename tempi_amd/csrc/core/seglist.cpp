// tempi_amd/csrc/core/seglist.cpp -- see seglist.hpp
#include "seglist.hpp"

#include "counters.hpp"
#include "log.hpp"
#include "next_mpi.hpp"

namespace tempi {

namespace {

// the type map of one element of a (sub)type, as merged runs
struct Node {
  explicit Node(int64_t cap) : runs(cap) {}
  bool ok = false;
  seg::Merger runs;
  int64_t extent = 0;
};

// as types.cpp's: child handles from MPI_Type_get_contents are freed unless
// predefined, straight through the library
void release_child(MPI_Datatype t) {
  int ni, na, nd, comb;
  MPI_Type_get_envelope(t, &ni, &na, &nd, &comb);
  if (comb != MPI_COMBINER_NAMED) next.MPI_Type_free(&t);
}

int64_t type_extent(MPI_Datatype t) {
  MPI_Aint lb, ext;
  MPI_Type_get_extent(t, &lb, &ext);
  return int64_t(ext);
}

// `blen` copies of child `c`, extent apart, the first at byte `d`; false once
// the cap is passed
bool add_block(seg::Merger &m, const Node &c, int64_t d, int64_t blen) {
  const int64_t n = c.runs.size();
  if (blen <= 0 || n == 0) return !m.over();
  const std::vector<int64_t> &cd = c.runs.disp(), &cl = c.runs.len();
  if (n == 1 && cl[0] == c.extent) return m.push(d + cd[0], blen * c.extent); // dense child: the copies abut
  for (int64_t j = 0; j < blen; ++j)
    for (int64_t k = 0; k < n; ++k)
      if (!m.push(d + j * c.extent + cd[size_t(k)], cl[size_t(k)])) return false;
  return true;
}

Node flatten(MPI_Datatype t, int64_t cap) {
  Node r(cap);
  r.extent = type_extent(t);
  int ni = 0, na = 0, nd = 0, comb = 0;
  MPI_Type_get_envelope(t, &ni, &na, &nd, &comb);

  if (comb == MPI_COMBINER_NAMED) {
    int size = 0;
    MPI_Aint lb, ext;
    MPI_Type_size(t, &size);
    MPI_Type_get_extent(t, &lb, &ext);
    // dense predefined types only; the pair types stay with the library
    if (size > 0 && lb == 0 && int64_t(ext) == size) r.ok = r.runs.push(0, size);
    return r;
  }

  std::vector<int> ints(ni > 0 ? ni : 1);
  std::vector<MPI_Aint> addrs(na > 0 ? na : 1);
  std::vector<MPI_Datatype> types(nd > 0 ? nd : 1);
  MPI_Type_get_contents(t, ni, na, nd, ints.data(), addrs.data(), types.data());

  // every constructor but struct has one child
  Node child(cap);
  if (nd >= 1 && comb != MPI_COMBINER_STRUCT) child = flatten(types[0], cap);
  const int64_t ce = child.extent;
  bool ok = child.ok;

  switch (comb) {
  case MPI_COMBINER_DUP:
  case MPI_COMBINER_RESIZED: // new lb / extent markers, same type map
    ok = ok && add_block(r.runs, child, 0, 1);
    break;
  case MPI_COMBINER_CONTIGUOUS:
    ok = ok && add_block(r.runs, child, 0, ints[0]);
    break;
  case MPI_COMBINER_VECTOR:
  case MPI_COMBINER_HVECTOR:
#ifdef MPI_COMBINER_HVECTOR_INTEGER
  case MPI_COMBINER_HVECTOR_INTEGER:
#endif
  {
    const int64_t stride = comb == MPI_COMBINER_VECTOR    ? int64_t(ints[2]) * ce
                           : comb == MPI_COMBINER_HVECTOR ? int64_t(addrs[0])
                                                          : int64_t(ints[2]);
    for (int64_t i = 0; ok && i < ints[0]; ++i) ok = add_block(r.runs, child, i * stride, ints[1]);
    break;
  }
  case MPI_COMBINER_INDEXED:
  case MPI_COMBINER_HINDEXED:
#ifdef MPI_COMBINER_HINDEXED_INTEGER
  case MPI_COMBINER_HINDEXED_INTEGER:
#endif
  {
    const int n = ints[0];
    for (int i = 0; ok && i < n; ++i) {
      const int64_t d = comb == MPI_COMBINER_INDEXED    ? int64_t(ints[1 + n + i]) * ce
                        : comb == MPI_COMBINER_HINDEXED ? int64_t(addrs[i])
                                                        : int64_t(ints[1 + n + i]);
      ok = add_block(r.runs, child, d, ints[1 + i]);
    }
    break;
  }
  case MPI_COMBINER_INDEXED_BLOCK:
  case MPI_COMBINER_HINDEXED_BLOCK: {
    const int n = ints[0];
    for (int i = 0; ok && i < n; ++i) {
      const int64_t d = comb == MPI_COMBINER_INDEXED_BLOCK ? int64_t(ints[2 + i]) * ce : int64_t(addrs[i]);
      ok = add_block(r.runs, child, d, ints[1]);
    }
    break;
  }
  case MPI_COMBINER_STRUCT: { // any mix of child types
    const int n = ints[0];
    ok = true;
    int have = -1; // `child` holds types[have]
    for (int i = 0; ok && i < n; ++i) {
      if (have < 0 || types[i] != types[have]) {
        child = flatten(types[i], cap);
        have = i;
      }
      ok = child.ok && add_block(r.runs, child, int64_t(addrs[i]), ints[1 + i]);
    }
    break;
  }
  case MPI_COMBINER_SUBARRAY: {
    // elements of the sub-block in array order, the fastest-varying dimension
    // taken a row at a time (MPI-3.1 4.1.3)
    const int n = ints[0];
    const int *sizes = &ints[1], *subs = &ints[1 + n], *starts = &ints[1 + 2 * n];
    const bool c_order = ints[1 + 3 * n] == MPI_ORDER_C;
    std::vector<int64_t> stride(size_t(n), 0), idx(size_t(n), 0);
    int64_t full = ce, rows = 1;
    for (int k = 0; k < n; ++k) {
      const int d = c_order ? n - 1 - k : k; // fastest first
      stride[size_t(d)] = full;
      full *= sizes[d];
    }
    const int fast = c_order ? n - 1 : 0;
    for (int d = 0; d < n; ++d)
      if (d != fast) rows *= subs[d];
    if (n < 1 || subs[fast] <= 0) rows = 0;
    for (int64_t row = 0; ok && row < rows; ++row) {
      int64_t off = int64_t(starts[fast]) * stride[size_t(fast)];
      for (int d = 0; d < n; ++d)
        if (d != fast) off += (starts[d] + idx[size_t(d)]) * stride[size_t(d)];
      ok = add_block(r.runs, child, off, subs[fast]);
      for (int k = 1; k < n; ++k) { // advance the next-fastest index first
        const int d = c_order ? n - 1 - k : k;
        if (++idx[size_t(d)] < subs[d]) break;
        idx[size_t(d)] = 0;
      }
    }
    break;
  }
  default:
    ok = false; // darray, F90 types, ...: library
    break;
  }

  for (int i = 0; i < nd; ++i) release_child(types[i]);
  r.ok = ok && !r.runs.over();
  return r;
}

} // namespace

std::unique_ptr<SegPacker> SegPacker::from_type(MPI_Datatype t, int64_t size, int64_t extent, int64_t maxSegs) {
  const Node n = flatten(t, maxSegs);
  if (!n.ok) {
    LOG_DEBUG("type " << t << (n.runs.over() ? " has more runs than the cap" : " has no segment list")
                      << "; library handles it");
    return nullptr;
  }
  seg::Table tab;
  if (!seg::build_table(n.runs.disp().data(), n.runs.len().data(), n.runs.size(), extent, maxSegs, &tab))
    return nullptr;
  // defensive: the runs must account for exactly the type's bytes
  if (tab.size != size || tab.disp.empty()) {
    LOG_WARN("segment list of type " << t << " has " << tab.size << " bytes, MPI says " << size << "; library path");
    return nullptr;
  }
  LOG_SPEW("type " << t << " -> " << tab.disp.size() << " runs, " << tab.size << " bytes, align " << tab.align);
  return std::make_unique<SegPacker>(std::move(tab));
}

SegPacker::~SegPacker() {}

void SegPacker::release_device() {
  std::lock_guard<std::mutex> g(mtx_);
  for (tempi_hip_seglist *s : dev_)
    if (s) tempi_hip_seglist_destroy(s);
  dev_.clear();
}

tempi_hip_seglist *SegPacker::device_table() const {
  int dev = 0;
  if (tempi_hip_get_device(&dev) != 0 || dev < 0) return nullptr;
  std::lock_guard<std::mutex> g(mtx_);
  if (dev_.size() <= size_t(dev)) dev_.resize(size_t(dev) + 1, nullptr);
  if (!dev_[size_t(dev)]) {
    tempi_hip_seglist *s = nullptr;
    if (tempi_hip_seglist_create(&s, tab_.disp.data(), tab_.len.data(), int64_t(tab_.disp.size()), tab_.extent) != 0)
      return nullptr;
    dev_[size_t(dev)] = s;
  }
  return dev_[size_t(dev)];
}

int SegPacker::launch(bool pack, char *packed, char *origin, int64_t count, void *stream,
                      Packer::Completion *done) const {
  if (count <= 0 || tab_.size == 0) return 0;
  const tempi_hip_seglist *s = device_table();
  if (!s) return 2; // (hipErrorOutOfMemory: the caller falls back to the library)
  const int64_t bytes = packed_bytes(count);
  if (pack) {
    counters.packs++;
    counters.irregular_packs++;
    counters.pack_bytes += uint64_t(bytes);
  } else {
    counters.unpacks++;
    counters.irregular_unpacks++;
    counters.unpack_bytes += uint64_t(bytes);
  }
  counters.launches++;
  if (done)
    return pack ? tempi_hip_pack_seglist_ticket(packed, origin, s, count, stream, &done->flag, &done->ticket)
                : tempi_hip_unpack_seglist_ticket(origin, packed, s, count, stream, &done->flag, &done->ticket);
  return pack ? tempi_hip_pack_seglist(packed, origin, s, count, stream)
              : tempi_hip_unpack_seglist(origin, packed, s, count, stream);
}

int SegPacker::pack_async(void *packed, const void *origin, int64_t count, void *stream) const {
  return launch(true, static_cast<char *>(packed), const_cast<char *>(static_cast<const char *>(origin)), count,
                stream, nullptr);
}

int SegPacker::unpack_async(void *origin, const void *packed, int64_t count, void *stream) const {
  return launch(false, const_cast<char *>(static_cast<const char *>(packed)), static_cast<char *>(origin), count,
                stream, nullptr);
}

int SegPacker::pack_ticket(void *packed, const void *origin, int64_t count, void *stream,
                           Packer::Completion *done) const {
  return launch(true, static_cast<char *>(packed), const_cast<char *>(static_cast<const char *>(origin)), count,
                stream, done);
}

int SegPacker::unpack_ticket(void *origin, const void *packed, int64_t count, void *stream,
                             Packer::Completion *done) const {
  return launch(false, const_cast<char *>(static_cast<const char *>(packed)), static_cast<char *>(origin), count,
                stream, done);
}

} // namespace tempi
