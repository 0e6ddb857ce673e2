// tempi_amd/csrc/core/seglist.hpp -- the packer of datatypes that are NOT one
// strided block (ragged or irregular (h)indexed, struct of several types, and
// anything built over them): the type map of one element flattened at commit
// into a segment list (seglist_core.hpp), gathered / scattered on the GPU by
// the segment-list kernels (hip/seg_kernels.hip).
//
// Opt-in (TEMPI_IRREGULAR / tempi_irregular_config, default off) and only for
// the synchronous MPI_Pack / MPI_Unpack: the strided descriptor, Packer and
// the transport never see it (such a type keeps desc.valid == false and a null
// TypeRecord::packer, so sends of it stay library-packed).
#pragma once

#include "packer.hpp"
#include "seglist_core.hpp"

#include <mpi.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

namespace tempi {

class SegPacker {
public:
  // Flatten committed type `t` (MPI_Type_get_envelope / _get_contents walk;
  // derived child handles are freed). nullptr when the type holds something the
  // walk leaves to the library (pair types, darray, F90 types), when its merged
  // run count passes `maxSegs`, or when the runs do not add up to `size`.
  static std::unique_ptr<SegPacker> from_type(MPI_Datatype t, int64_t size, int64_t extent, int64_t maxSegs);

  explicit SegPacker(seg::Table &&tab) : tab_(std::move(tab)) {}
  ~SegPacker(); // (frees nothing on the GPU: release_device does, while HIP is still up)

  int64_t packed_bytes(int64_t count) const { return tab_.size * count; }
  const seg::Table &table() const { return tab_; }

  // as Packer's: `origin` is the MPI buffer address as the GPU sees it
  int pack_async(void *packed, const void *origin, int64_t count, void *stream) const;
  int unpack_async(void *origin, const void *packed, int64_t count, void *stream) const;
  int pack_ticket(void *packed, const void *origin, int64_t count, void *stream, Packer::Completion *done) const;
  int unpack_ticket(void *origin, const void *packed, int64_t count, void *stream, Packer::Completion *done) const;

  // Free the device tables (MPI_Type_free, types_finalize). Safe without
  // waiting for anything: only the synchronous MPI_Pack / MPI_Unpack use a
  // table, and they complete before they return, so no kernel can still be
  // reading one when its type is freed.
  void release_device();

private:
  int launch(bool pack, char *packed, char *origin, int64_t count, void *stream, Packer::Completion *done) const;
  // the table on the current device, uploaded at the first call there
  tempi_hip_seglist *device_table() const;

  seg::Table tab_;
  mutable std::mutex mtx_;
  mutable std::vector<tempi_hip_seglist *> dev_; // by device ordinal
};

} // namespace tempi
