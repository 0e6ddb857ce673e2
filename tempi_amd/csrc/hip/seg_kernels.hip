// tempi_amd/csrc/hip/seg_kernels.hip -- segment-list gather / scatter for
// datatypes that are not one strided block (include/tempi_hip.h, "Irregular
// datatypes"), gfx950.
//
// The table of one element's runs lives in device memory as
//   pre[0 .. n]   exclusive prefix sums of the run lengths (pre[n] = size)
//   disp[0 .. n)  the runs' displacements from the MPI buffer address
// in MPI type-map order. The mapping is output-linear like the strided
// kernels': the packed stream is cut into tiles of kTile bytes, a workgroup
// owns a tile, and packed byte p belongs to element e = p / size at offset
// r = p % size, i.e. to run i with pre[i] <= r < pre[i + 1], at address
//   origin + e * extent + disp[i] + (r - pre[i])
// (64-bit arithmetic throughout). Accesses are words of W bytes, W chosen per
// call so that it divides every disp and len (hence every pre[i] and r), both
// addresses and -- for more than one element -- the extent: a word never
// straddles a run, so no lane reads or writes a byte outside the type map.
//
// Run lookup. A tile that stays inside one element finds its first and last
// run with two uniform binary searches over pre[] in global memory; a tile
// that crosses an element seam may meet any run, so its slice is the whole
// table. A slice of at most kLdsRuns runs (fewer when the whole table is
// smaller: the LDS is sized per launch, so that a table of a few long runs
// does not cost the copy its occupancy) is staged in LDS and every lane
// searches there (after trying the run its previous word was in: consecutive
// words of a lane are 4 KiB or less apart, so long runs rarely search at
// all). A larger slice -- thousands of tiny runs per tile -- is searched per
// lane in global memory; the table is read-mostly and small, so L2 and the
// Infinity Cache serve it.
#include <hip/hip_runtime.h>

#include "tempi_hip.h"

#include <cstdint>
#include <vector>

struct tempi_hip_seglist {
  int64_t *dev = nullptr; // pre[n + 1] then disp[n]
  int64_t n = 0, size = 0, extent = 0;
  uint64_t bits = 0; // OR of every disp and len: its low bits bound the word width
  int device = 0;
};

namespace {

constexpr int kThreads = 256;
constexpr int64_t kTile = 16384;  // packed bytes per workgroup
constexpr int kLdsRuns = 2048;    // most runs of a tile's slice staged in LDS (32 KiB of LDS)
constexpr int kUnroll = 4;        // words in flight per lane

// native vectors (HIP's uint2 / uint4 are structs: an array of them went to scratch)
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <int W> struct Word;
template <> struct Word<1> { typedef uint8_t T; };
template <> struct Word<2> { typedef uint16_t T; };
template <> struct Word<4> { typedef uint32_t T; };
template <> struct Word<8> { typedef u32x2 T; };
template <> struct Word<16> { typedef u32x4 T; };

struct SegArgs {
  const int64_t *pre;
  const int64_t *disp;
  int64_t n, size, extent;
  int64_t total; // packed bytes of the call
  char *packed;
  char *origin;
  int lds; // runs the launch's LDS holds: min(n, kLdsRuns)
};

// the largest i in [lo, hi] with pre[i] <= r (pre[lo] <= r is given)
template <typename I> __device__ __forceinline__ I find_run(const int64_t *pre, I lo, I hi, int64_t r) {
  while (lo < hi) {
    const I mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= r)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

template <int W, bool PACK> __global__ __launch_bounds__(kThreads) void seg_kernel(const SegArgs a) {
  typedef typename Word<W>::T T;
  HIP_DYNAMIC_SHARED(int64_t, sMem) // a.lds + 1 prefix sums, then a.lds displacements
  int64_t *const sPre = sMem;
  int64_t *const sDisp = sMem + a.lds + 1;

  const int64_t t0 = int64_t(blockIdx.x) * kTile;
  const int64_t t1 = t0 + kTile < a.total ? t0 + kTile : a.total;
  // the tile's slice of the table (uniform over the workgroup)
  const int64_t e0 = t0 / a.size, eLast = (t1 - 1) / a.size;
  int64_t i0 = 0, i1 = a.n - 1;
  if (e0 == eLast) {
    i0 = find_run<int64_t>(a.pre, 0, a.n - 1, t0 - e0 * a.size);
    i1 = find_run<int64_t>(a.pre, i0, a.n - 1, t1 - 1 - e0 * a.size);
  }
  const int m = i1 - i0 < a.lds ? int(i1 - i0 + 1) : 0; // 0: the slice does not fit, search global memory
  if (m) {
    // only the index is relative to the slice's first run: the prefix sums stay absolute
    for (int j = threadIdx.x; j <= m; j += kThreads) sPre[j] = a.pre[i0 + j];
    for (int j = threadIdx.x; j < m; j += kThreads) sDisp[j] = a.disp[i0 + j];
    __syncthreads();
  }

  constexpr int64_t kStep = int64_t(kThreads) * W;
  const int64_t stepE = kStep / a.size, stepR = kStep % a.size;
  int64_t p = t0 + int64_t(threadIdx.x) * W;
  int64_t e = p / a.size, r = p - e * a.size;
  int64_t cur = m ? 0 : i0; // the run of this lane's previous word
  while (p < t1) {
    T v[kUnroll];
    char *side[kUnroll]; // the strided side's address of each word
    int64_t pp[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      pp[u] = p;
      if (p < t1) {
        int64_t off;
        if (m) {
          int j = int(cur);
          if (!(sPre[j] <= r && r < sPre[j + 1])) j = find_run<int>(sPre, 0, m - 1, r);
          cur = j;
          off = sDisp[j] + (r - sPre[j]);
        } else {
          int64_t j = cur;
          if (!(a.pre[j] <= r && r < a.pre[j + 1])) j = find_run<int64_t>(a.pre, 0, a.n - 1, r);
          cur = j;
          off = a.disp[j] + (r - a.pre[j]);
        }
        side[u] = a.origin + e * a.extent + off;
        v[u] = PACK ? *reinterpret_cast<const T *>(side[u]) : *reinterpret_cast<const T *>(a.packed + p);
      }
      p += kStep;
      e += stepE;
      r += stepR;
      if (r >= a.size) {
        r -= a.size;
        e++;
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      if (pp[u] < t1) {
        if (PACK)
          *reinterpret_cast<T *>(a.packed + pp[u]) = v[u];
        else
          *reinterpret_cast<T *>(side[u]) = v[u];
      }
    }
  }
}

inline int width_of(const void *packed, const void *origin, const tempi_hip_seglist *s, int64_t count) {
  uint64_t bits = 16 | s->bits | uint64_t(reinterpret_cast<uintptr_t>(packed)) |
                  uint64_t(reinterpret_cast<uintptr_t>(origin));
  if (count > 1) bits |= uint64_t(s->extent);
  return int(bits & (~bits + 1)); // the lowest set bit: 1, 2, 4, 8 or 16
}

template <int W> int launch_w(bool pack, const SegArgs &a, uint32_t blocks, hipStream_t s) {
  const size_t lds = size_t(2 * a.lds + 1) * sizeof(int64_t);
  if (pack)
    hipLaunchKernelGGL((seg_kernel<W, true>), dim3(blocks), dim3(kThreads), lds, s, a);
  else
    hipLaunchKernelGGL((seg_kernel<W, false>), dim3(blocks), dim3(kThreads), lds, s, a);
  return int(hipGetLastError());
}

// 0 and *launched = false when there is nothing to do
int launch(bool pack, char *packed, char *origin, const tempi_hip_seglist *s, int64_t count, hipStream_t stream,
           bool *launched) {
  *launched = false;
  if (!s || !s->dev || s->n <= 0 || s->size <= 0) return int(hipErrorInvalidValue);
  if (count <= 0) return 0;
  if (count > INT64_MAX / s->size) return int(hipErrorInvalidValue);
  SegArgs a;
  a.pre = s->dev;
  a.disp = s->dev + s->n + 1;
  a.n = s->n;
  a.size = s->size;
  a.extent = s->extent;
  a.total = count * s->size;
  a.packed = packed;
  a.origin = origin;
  a.lds = int(s->n < kLdsRuns ? s->n : kLdsRuns);
  const int64_t blocks = (a.total + kTile - 1) / kTile;
  if (blocks > int64_t(0x7fffffff)) return int(hipErrorInvalidValue);
  int e;
  switch (width_of(packed, origin, s, count)) {
  case 16: e = launch_w<16>(pack, a, uint32_t(blocks), stream); break;
  case 8: e = launch_w<8>(pack, a, uint32_t(blocks), stream); break;
  case 4: e = launch_w<4>(pack, a, uint32_t(blocks), stream); break;
  case 2: e = launch_w<2>(pack, a, uint32_t(blocks), stream); break;
  default: e = launch_w<1>(pack, a, uint32_t(blocks), stream); break;
  }
  *launched = e == 0;
  return e;
}

int with_ticket(bool pack, char *packed, char *origin, const tempi_hip_seglist *s, int64_t count, void *stream,
                const uint32_t **flag, uint32_t *ticket) {
  *flag = nullptr;
  *ticket = 0;
  bool launched = false;
  const int e = launch(pack, packed, origin, s, count, static_cast<hipStream_t>(stream), &launched);
  if (e || !launched) return e;
  return tempi_hip_stream_ticket(stream, flag, ticket);
}

} // namespace

extern "C" {

int tempi_hip_seglist_create(tempi_hip_seglist **out, const int64_t *disp, const int64_t *len, int64_t nsegs,
                             int64_t extent) {
  if (!out) return int(hipErrorInvalidValue);
  *out = nullptr;
  if (!disp || !len || nsegs <= 0) return int(hipErrorInvalidValue);
  std::vector<int64_t> host(size_t(2 * nsegs + 1));
  uint64_t bits = 0;
  host[0] = 0;
  for (int64_t i = 0; i < nsegs; ++i) {
    if (len[i] <= 0) return int(hipErrorInvalidValue);
    host[size_t(i + 1)] = host[size_t(i)] + len[i];
    host[size_t(nsegs + 1 + i)] = disp[i];
    bits |= uint64_t(disp[i]) | uint64_t(len[i]);
  }
  tempi_hip_seglist *s = new tempi_hip_seglist;
  s->n = nsegs;
  s->size = host[size_t(nsegs)];
  s->extent = extent;
  s->bits = bits;
  hipError_t e = hipGetDevice(&s->device);
  void *d = nullptr;
  if (e == hipSuccess) e = hipMalloc(&d, host.size() * sizeof(int64_t));
  // a synchronous copy: the table is complete before any kernel can be launched on it
  if (e == hipSuccess) e = hipMemcpy(d, host.data(), host.size() * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (d) (void)hipFree(d);
    delete s;
    return int(e);
  }
  s->dev = static_cast<int64_t *>(d);
  *out = s;
  return 0;
}

int tempi_hip_seglist_destroy(tempi_hip_seglist *s) {
  if (!s) return 0;
  const hipError_t e = s->dev ? hipFree(s->dev) : hipSuccess;
  delete s;
  return int(e);
}

int tempi_hip_pack_seglist(void *packed, const void *origin, const tempi_hip_seglist *s, int64_t count,
                           void *stream) {
  bool launched;
  return launch(true, static_cast<char *>(packed), const_cast<char *>(static_cast<const char *>(origin)), s, count,
                static_cast<hipStream_t>(stream), &launched);
}

int tempi_hip_unpack_seglist(void *origin, const void *packed, const tempi_hip_seglist *s, int64_t count,
                             void *stream) {
  bool launched;
  return launch(false, const_cast<char *>(static_cast<const char *>(packed)), static_cast<char *>(origin), s, count,
                static_cast<hipStream_t>(stream), &launched);
}

int tempi_hip_pack_seglist_ticket(void *packed, const void *origin, const tempi_hip_seglist *s, int64_t count,
                                  void *stream, const uint32_t **flag, uint32_t *ticket) {
  return with_ticket(true, static_cast<char *>(packed), const_cast<char *>(static_cast<const char *>(origin)), s,
                     count, stream, flag, ticket);
}

int tempi_hip_unpack_seglist_ticket(void *origin, const void *packed, const tempi_hip_seglist *s, int64_t count,
                                    void *stream, const uint32_t **flag, uint32_t *ticket) {
  return with_ticket(false, const_cast<char *>(static_cast<const char *>(packed)), static_cast<char *>(origin), s,
                     count, stream, flag, ticket);
}

int tempi_hip_seglist_word_width(const void *packed, const void *origin, const tempi_hip_seglist *s,
                                 int64_t count) {
  return s ? width_of(packed, origin, s, count) : -1;
}

int64_t tempi_hip_seglist_tile_bytes(void) { return kTile; }
int64_t tempi_hip_seglist_lds_runs(void) { return kLdsRuns; }

} // extern "C"
