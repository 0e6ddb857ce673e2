"""GPU parity of MPI_Pack / MPI_Unpack of irregular datatypes through the
opt-in segment-list packer (core/seglist.cpp, hip/seg_kernels.hip), MI355X.

Oracles, as in test_pack_gpu.py: the committed MPICH goldens, the in-process
library MPI_Pack / MPI_Unpack on host copies, and oracle/typemap.c. Bit-exact
everywhere. Every successful GPU call is checked for the route it took:
packs / irregular_packs (or the unpack pair) advance by exactly one, the
library counters do not move, and the returned position is right.
"""
import ctypes

import numpy as np
import pytest

from oracle import pyoracle
from tests import golden_data as G
from tests import typezoo
from tests.irregular_cases import (RECIPES, STRUCT_EXTENT, STRUCT_RUNS, build_struct, gather, geometry, irregular,
                                   scatter)

pytestmark = pytest.mark.gpu

GOLDENS = ["zoo_hi", "zoo_hib", "hindexed_irregular", "struct_irregular"]


def _torch():
    import torch

    return torch


def to_np(t):
    return t.cpu().numpy()


def _hip():
    import tempi_amd

    H = ctypes.CDLL(tempi_amd.LIBTEMPI_HIP)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    H.tempi_hip_seglist_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64), i64, i64]
    H.tempi_hip_seglist_destroy.argtypes = [vp]
    H.tempi_hip_seglist_word_width.argtypes = [vp, vp, vp, i64]
    H.tempi_hip_seglist_tile_bytes.restype = i64
    H.tempi_hip_seglist_lds_runs.restype = i64
    return H


def gpu_pack(mpi, src_ptr, count, t, out_ptr, outsize, position, nbytes):
    """MPI_Pack that must take the segment-list kernels"""
    b = mpi.counters()
    pos = mpi.Pack(src_ptr, count, t, out_ptr, outsize, position)
    a = mpi.counters()
    assert a["packs"] == b["packs"] + 1 and a["irregular_packs"] == b["irregular_packs"] + 1
    assert a["lib_packs"] == b["lib_packs"] and a["lib_unpacks"] == b["lib_unpacks"]
    assert a["pack_bytes"] == b["pack_bytes"] + nbytes and a["launches"] == b["launches"] + 1
    assert pos == position + nbytes
    return pos


def gpu_unpack(mpi, in_ptr, insize, position, dst_ptr, count, t, nbytes):
    b = mpi.counters()
    pos = mpi.Unpack(in_ptr, insize, position, dst_ptr, count, t)
    a = mpi.counters()
    assert a["unpacks"] == b["unpacks"] + 1 and a["irregular_unpacks"] == b["irregular_unpacks"] + 1
    assert a["lib_packs"] == b["lib_packs"] and a["lib_unpacks"] == b["lib_unpacks"]
    assert a["unpack_bytes"] == b["unpack_bytes"] + nbytes and a["launches"] == b["launches"] + 1
    assert pos == position + nbytes
    return pos


def round_trip(mpi, gpu, t, runs, extent, count, seed=0, unpack=True):
    """pack on the GPU against numpy and the library; unpack into a random
    canvas against numpy and the library (bytes outside the type map survive)"""
    torch = _torch()
    origin, buflen = geometry(runs, extent, count)
    size = sum(n for _, n in runs) * count
    assert mpi.Pack_size(count, t) == size
    host = np.random.default_rng(seed).integers(0, 256, buflen, dtype=np.uint8)
    src = torch.from_numpy(host).to(gpu)
    out = torch.full((size + 16,), 0xA5, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    gpu_pack(mpi, src.data_ptr() + origin, count, t, out.data_ptr(), size, 0, size)
    got = to_np(out)
    assert (got[size:] == 0xA5).all()
    exp = gather(host, origin, runs, extent, count)
    assert np.array_equal(got[:size], exp)
    lib = np.zeros(size, dtype=np.uint8)
    assert mpi.Pack(host.ctypes.data + origin, count, t, lib.ctypes.data, size, 0) == size
    assert np.array_equal(got[:size], lib)
    if not unpack:
        return
    canvas = np.random.default_rng(seed + 99).integers(0, 256, buflen, dtype=np.uint8)
    dcanvas = torch.from_numpy(canvas).to(gpu)
    torch.cuda.synchronize()
    gpu_unpack(mpi, out.data_ptr(), size, 0, dcanvas.data_ptr() + origin, count, t, size)
    ref = canvas.copy()
    scatter(exp, ref, origin, runs, extent, count)
    libref = canvas.copy()
    assert mpi.Unpack(lib.ctypes.data, size, 0, libref.ctypes.data + origin, count, t) == size
    assert np.array_equal(ref, libref)
    assert np.array_equal(to_np(dcanvas), ref)


def hindexed(mpi, lens, disps):
    """a committed MPI_Type_create_hindexed over bytes and its runs (the
    caller picks displacements that do not merge)"""
    t = mpi.Type_commit(mpi.Type_create_hindexed(lens, disps, mpi.BYTE))
    runs = list(zip(disps, lens))
    assert mpi.type_segments(t)[0] == runs
    return t, runs, mpi.Type_get_extent(t)[1]


@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(mpi, gpu, name):
    torch = _torch()
    c = G.case(name)
    with irregular(mpi):
        t, temps, basic = typezoo.build(mpi, c["recipe"])
        try:
            src = (torch.arange(c["buflen"], dtype=torch.int64, device=gpu) & 0xFF).to(torch.uint8)
            out = torch.zeros(c["pack_size"], dtype=torch.uint8, device=gpu)
            torch.cuda.synchronize()
            pos = gpu_pack(mpi, src.data_ptr() + c["origin"], c["count"], t, out.data_ptr(), c["pack_size"], 0,
                           c["position"])
            G.check_packed(c, to_np(out[:pos]))
            dst = torch.zeros(c["buflen"], dtype=torch.uint8, device=gpu)
            torch.cuda.synchronize()
            upos = gpu_unpack(mpi, out.data_ptr(), c["pack_size"], 0, dst.data_ptr() + c["origin"], c["count"], t,
                              c["unpack_position"])
            assert upos == c["unpack_position"]
            G.check_unpacked(c, to_np(dst))
        finally:
            typezoo.free(mpi, t, temps, basic)


@pytest.mark.parametrize("recipe", RECIPES)
def test_recipes_vs_library_and_oracle(mpi, gpu, recipe):
    torch = _torch()
    tm = pyoracle.TypeMap(recipe)
    with irregular(mpi):
        t, temps, basic = typezoo.build(mpi, recipe)
        try:
            for count in (1, 2, 3):
                origin, buflen = tm.geometry(count)
                size = mpi.Pack_size(count, t)
                assert size == tm.size * count
                host = np.random.default_rng(count).integers(0, 256, buflen, dtype=np.uint8)
                src = torch.from_numpy(host).to(gpu)
                out = torch.zeros(size, dtype=torch.uint8, device=gpu)
                torch.cuda.synchronize()
                gpu_pack(mpi, src.data_ptr() + origin, count, t, out.data_ptr(), size, 0, size)
                lib = np.zeros(size, dtype=np.uint8)
                assert mpi.Pack(host.ctypes.data + origin, count, t, lib.ctypes.data, size, 0) == size
                got = to_np(out)
                assert np.array_equal(got, lib), (recipe, count)
                assert np.array_equal(got, tm.pack(host, origin, count)), (recipe, count)
                canvas = np.random.default_rng(count + 99).integers(0, 256, buflen, dtype=np.uint8)
                dcanvas = torch.from_numpy(canvas).to(gpu)
                torch.cuda.synchronize()
                gpu_unpack(mpi, out.data_ptr(), size, 0, dcanvas.data_ptr() + origin, count, t, size)
                exp = canvas.copy()
                mpi.Unpack(lib.ctypes.data, size, 0, exp.ctypes.data + origin, count, t)
                assert np.array_equal(to_np(dcanvas), exp), (recipe, count)
        finally:
            typezoo.free(mpi, t, temps, basic)


# one type per word width: every disp, len and the extent a multiple of W (and not of 2 W)
WIDTHS = {
    16: "resized(0,2064,hindexed([16,48,32,160],[0,64,256,1040],byte))",
    8: "indexed([1,2,3],[0,3,10],double)",   # extent 104
    4: "indexed([1,2,3],[0,3,10],int)",      # extent 52
    2: "indexed([1,2,3],[0,3,10],short)",    # extent 26
    1: "hindexed([3,1,7,5],[1,9,21,33],byte)",
}


def _seglist(H, runs, extent):
    n = len(runs)
    A = ctypes.c_int64 * n
    s = ctypes.c_void_p()
    assert H.tempi_hip_seglist_create(ctypes.byref(s), A(*[d for d, _ in runs]), A(*[ln for _, ln in runs]), n,
                                      extent) == 0
    return s


@pytest.mark.parametrize("w", sorted(WIDTHS))
def test_word_widths(mpi, gpu, w):
    torch = _torch()
    H = _hip()
    recipe = WIDTHS[w]
    tm = pyoracle.TypeMap(recipe)
    runs = tm.segments()
    with irregular(mpi):
        t, temps, basic = typezoo.build(mpi, recipe)
        try:
            assert mpi.type_segments(t) == (runs, tm.extent)
            round_trip(mpi, gpu, t, runs, tm.extent, 3, seed=w)
            # aligned buffers: the width is the type's own
            s = _seglist(H, runs, tm.extent)
            try:
                a = torch.zeros(64, dtype=torch.uint8, device=gpu)
                assert a.data_ptr() % 16 == 0
                assert H.tempi_hip_seglist_word_width(a.data_ptr(), a.data_ptr(), s, 3) == w
                # one element: the extent does not count
                assert H.tempi_hip_seglist_word_width(a.data_ptr(), a.data_ptr(), s, 1) == w
                assert H.tempi_hip_seglist_word_width(a.data_ptr() + 1, a.data_ptr(), s, 3) == 1
            finally:
                H.tempi_hip_seglist_destroy(s)
        finally:
            typezoo.free(mpi, t, temps, basic)


def test_extent_counts_only_for_several_elements(gpu):
    H = _hip()
    torch = _torch()
    s = _seglist(H, [(0, 16), (64, 32)], 100)  # runs 16-aligned, extent only 4-aligned
    try:
        a = torch.zeros(64, dtype=torch.uint8, device=gpu)
        assert H.tempi_hip_seglist_word_width(a.data_ptr(), a.data_ptr(), s, 1) == 16
        assert H.tempi_hip_seglist_word_width(a.data_ptr(), a.data_ptr(), s, 2) == 4
    finally:
        H.tempi_hip_seglist_destroy(s)


@pytest.mark.parametrize("prefix,shift,width", [(1, 0, 1), (3, 5, 1), (8, 0, 8), (16, 3, 1)])
def test_misaligned_position(mpi, gpu, prefix, shift, width):
    """the W = 16 type appended at odd positions in odd-aligned buffers: the
    word width drops, bytes before the position and after the end keep their
    fill"""
    torch = _torch()
    H = _hip()
    recipe = WIDTHS[16]
    tm = pyoracle.TypeMap(recipe)
    runs, count = tm.segments(), 3
    origin, buflen = tm.geometry(count)
    size = tm.size * count
    with irregular(mpi):
        t, temps, basic = typezoo.build(mpi, recipe)
        try:
            host = np.random.default_rng(prefix).integers(0, 256, buflen, dtype=np.uint8)
            src_raw = torch.zeros(buflen + 64, dtype=torch.uint8, device=gpu)
            src = src_raw[shift:shift + buflen]
            src.copy_(torch.from_numpy(host).to(gpu))
            base = torch.full((size + prefix + 64,), 0xA5, dtype=torch.uint8, device=gpu)
            assert src_raw.data_ptr() % 16 == 0 and base.data_ptr() % 16 == 0
            torch.cuda.synchronize()
            outp = base.data_ptr() + shift
            s = _seglist(H, runs, tm.extent)
            try:
                assert H.tempi_hip_seglist_word_width(outp + prefix, src.data_ptr() + origin, s, count) == width
            finally:
                H.tempi_hip_seglist_destroy(s)
            pos = gpu_pack(mpi, src.data_ptr() + origin, count, t, outp, prefix + size, prefix, size)
            got = to_np(base)
            assert (got[:shift + prefix] == 0xA5).all()
            assert (got[shift + pos:] == 0xA5).all()
            assert np.array_equal(got[shift + prefix:shift + pos], tm.pack(host, origin, count))
            # and back, into a canvas at the same misalignment
            canvas = np.random.default_rng(prefix + 7).integers(0, 256, buflen, dtype=np.uint8)
            dst_raw = torch.full((buflen + 64,), 0x3C, dtype=torch.uint8, device=gpu)
            dst_raw[shift:shift + buflen] = torch.from_numpy(canvas).to(gpu)
            torch.cuda.synchronize()
            gpu_unpack(mpi, outp, prefix + size, prefix, dst_raw.data_ptr() + shift + origin, count, t, size)
            ref = canvas.copy()
            tm.unpack(tm.pack(host, origin, count), ref, origin, count)
            back = to_np(dst_raw)
            assert np.array_equal(back[shift:shift + buflen], ref)
            assert (back[:shift] == 0x3C).all() and (back[shift + buflen:] == 0x3C).all()
        finally:
            typezoo.free(mpi, t, temps, basic)


def test_many_tiny_runs_take_the_global_lookup(mpi, gpu):
    """40,000 one-byte runs at 3 i + (i mod 2), count 2: every tile meets more
    runs than the LDS slice holds, and one tile crosses the element seam"""
    H = _hip()
    n = 40000
    assert H.tempi_hip_seglist_tile_bytes() > H.tempi_hip_seglist_lds_runs()  # one-byte runs per tile > LDS runs
    disps = [3 * i + (i % 2) for i in range(n)]
    with irregular(mpi):
        t = mpi.Type_commit(mpi.Type_create_hindexed_block(1, disps, mpi.BYTE))
        try:
            runs = [(d, 1) for d in disps]
            assert mpi.type_segments(t) == (runs, disps[-1] + 1)
            round_trip(mpi, gpu, t, runs, disps[-1] + 1, 2, seed=3)
        finally:
            mpi.Type_free(t)


def test_one_huge_run_among_tiny_ones(mpi, gpu):
    """{5 B, 1 MiB + 3 B, 7 B}, count 3: tiles deep inside one run (a one-run
    LDS slice), and element seams that fall mid-tile"""
    big = (1 << 20) + 3
    with irregular(mpi):
        t, runs, extent = hindexed(mpi, [5, big, 7], [0, 16, big + 32])
        try:
            round_trip(mpi, gpu, t, runs, extent, 3, seed=4)
        finally:
            mpi.Type_free(t)


@pytest.mark.parametrize("tiles", [1, 2])
def test_size_one_byte_short_of_the_tile(mpi, gpu, tiles):
    """the size is one byte less than a multiple of the kernel's tile, count
    4: every element seam lands one byte further from a tile boundary"""
    tile = _hip().tempi_hip_seglist_tile_bytes()
    size = tiles * tile - 1
    lens = [tile // 2 - 10, 9, size - (tile // 2 - 10) - 9]
    disps = [0, tile // 2, tile // 2 + 20]
    assert sum(lens) == size and all(n > 0 for n in lens)
    with irregular(mpi):
        t, runs, extent = hindexed(mpi, lens, disps)
        try:
            round_trip(mpi, gpu, t, runs, extent, 4, seed=tiles)
        finally:
            mpi.Type_free(t)


def test_out_of_order_and_negative(mpi, gpu):
    with irregular(mpi):
        t, runs, extent = hindexed(mpi, [4, 2, 6], [40, -16, 8])
        try:
            origin, _ = geometry(runs, extent, 2)
            assert origin == 16  # the MPI buffer address lies inside the allocation
            round_trip(mpi, gpu, t, runs, extent, 2, seed=6)
        finally:
            mpi.Type_free(t)


@pytest.mark.parametrize("lens,disps,extent,unpack", [
    ([6, 3], [0, 20], 4, False),  # elements overlap each other: a send type only
    ([2, 3], [0, 20], 8, True),   # elements interleave without overlapping
])
def test_extent_smaller_than_the_span(mpi, gpu, lens, disps, extent, unpack):
    with irregular(mpi):
        h = mpi.Type_create_hindexed(lens, disps, mpi.BYTE)
        t = mpi.Type_commit(mpi.Type_create_resized(h, 0, extent))
        try:
            runs = list(zip(disps, lens))
            assert mpi.type_segments(t) == (runs, extent)
            round_trip(mpi, gpu, t, runs, extent, 3, seed=8, unpack=unpack)
        finally:
            mpi.Type_free(t)
            mpi.Type_free(h)


def test_displacements_beyond_2_to_31(mpi, gpu):
    """runs 2 GiB and 3 GiB from the origin on a 3.5 GiB device buffer,
    checked with device-side slices only"""
    torch = _torch()
    lens = [24, 8, 40]
    disps = [0, (1 << 31) + 64, 3 * (1 << 30) + 8]
    with irregular(mpi):
        t, runs, extent = hindexed(mpi, lens, disps)
        buf = None
        try:
            buf = torch.empty(7 << 29, dtype=torch.uint8, device=gpu)
            g = torch.Generator(device=gpu).manual_seed(31)
            for d, n in runs:
                buf[d:d + n].random_(0, 256, generator=g)
            exp = torch.cat([buf[d:d + n] for d, n in runs]).clone()
            out = torch.full((72 + 16,), 0xA5, dtype=torch.uint8, device=gpu)
            torch.cuda.synchronize()
            gpu_pack(mpi, buf.data_ptr(), 1, t, out.data_ptr(), 72, 0, 72)
            assert torch.equal(out[:72], exp) and bool((out[72:] == 0xA5).all())
            # back: the runs and 8 guard bytes either side of each are rewritten first
            for d, n in runs:
                buf[max(d - 8, 0):d + n + 8] = 0x3C
            torch.cuda.synchronize()
            gpu_unpack(mpi, out.data_ptr(), 72, 0, buf.data_ptr(), 1, t, 72)
            p = 0
            for d, n in runs:
                assert torch.equal(buf[d:d + n], exp[p:p + n])
                assert bool((buf[max(d - 8, 0):d] == 0x3C).all()) and bool((buf[d + n:d + n + 8] == 0x3C).all())
                p += n
        finally:
            mpi.Type_free(t)
            del buf
            torch.cuda.empty_cache()


def test_multi_type_struct(mpi, gpu):
    with irregular(mpi):
        t, temps = build_struct(mpi)
        try:
            assert mpi.type_segments(t) == (STRUCT_RUNS, STRUCT_EXTENT)
            round_trip(mpi, gpu, t, STRUCT_RUNS, STRUCT_EXTENT, 5, seed=9)
        finally:
            for x in temps + [t]:
                mpi.Type_free(x)


@pytest.mark.parametrize("count,prefix", [(1, 0), (3, 13)])
def test_pageable_host_packed_side(mpi, gpu, count, prefix):
    """the packed bytes in a numpy buffer, both directions: staged through a
    pinned slab, no library pack"""
    torch = _torch()
    with irregular(mpi):
        t, runs, extent = hindexed(mpi, [5, 300, 7, 64], [3, 16, 1000, 2000])
        try:
            origin, buflen = geometry(runs, extent, count)
            size = sum(n for _, n in runs) * count
            host = np.random.default_rng(count).integers(0, 256, buflen, dtype=np.uint8)
            src = torch.from_numpy(host).to(gpu)
            out = np.full(prefix + size + 7, 0xA5, dtype=np.uint8)
            torch.cuda.synchronize()
            b = mpi.counters()
            pos = gpu_pack(mpi, src.data_ptr() + origin, count, t, out.ctypes.data, prefix + size, prefix, size)
            a = mpi.counters()
            assert a["staged_packs"] == b["staged_packs"] + 1
            exp = gather(host, origin, runs, extent, count)
            assert np.array_equal(out[prefix:pos], exp)
            assert (out[:prefix] == 0xA5).all() and (out[pos:] == 0xA5).all()
            dst = torch.full((buflen,), 0x3C, dtype=torch.uint8, device=gpu)
            torch.cuda.synchronize()
            gpu_unpack(mpi, out.ctypes.data, prefix + size, prefix, dst.data_ptr() + origin, count, t, size)
            assert mpi.counters()["staged_unpacks"] == a["staged_unpacks"] + 1
            ref = np.full(buflen, 0x3C, dtype=np.uint8)
            scatter(exp, ref, origin, runs, extent, count)
            assert np.array_equal(to_np(dst), ref)
        finally:
            mpi.Type_free(t)


PACK_COUNTERS = ("packs", "unpacks", "irregular_packs", "irregular_unpacks", "lib_packs", "lib_unpacks", "launches",
                 "pack_bytes", "unpack_bytes", "staged_packs", "staged_unpacks")


def test_truncation_is_an_error(mpi, gpu):
    """outsize / insize one byte short: the strided path's error class,
    nothing written past the position, no counter advanced"""
    torch = _torch()
    with irregular(mpi):
        t, runs, extent = hindexed(mpi, [3, 1, 4], [0, 9, 20])
        assert mpi.L.MPI_Comm_set_errhandler(mpi.COMM_WORLD, mpi.const("MPI_ERRORS_RETURN")) == 0
        try:
            src = torch.zeros(64, dtype=torch.uint8, device=gpu)
            out = torch.full((32,), 0xA5, dtype=torch.uint8, device=gpu)
            torch.cuda.synchronize()
            b = mpi.counters()
            rc, pos = mpi.Pack_rc(src.data_ptr(), 2, t, out.data_ptr(), 15, 0)
            assert rc == mpi.ERR_TRUNCATE and pos == 0
            rc, pos = mpi.Pack_rc(src.data_ptr(), 2, t, out.data_ptr(), 16, 1)
            assert rc == mpi.ERR_TRUNCATE and pos == 1
            p = ctypes.c_int(0)
            rc = mpi.L.MPI_Unpack(ctypes.c_void_p(out.data_ptr()), 15, ctypes.byref(p), ctypes.c_void_p(src.data_ptr()),
                                  2, mpi.h(t), mpi.h(mpi.COMM_WORLD))
            assert rc == mpi.ERR_TRUNCATE and p.value == 0
            a = mpi.counters()
            assert {k: a[k] for k in PACK_COUNTERS} == {k: b[k] for k in PACK_COUNTERS}
            assert bool((out == 0xA5).all()) and int(src.count_nonzero()) == 0
        finally:
            mpi.L.MPI_Comm_set_errhandler(mpi.COMM_WORLD, mpi.const("MPI_ERRORS_ARE_FATAL"))
            mpi.Type_free(t)


def _library_route(mpi, gpu, t, runs, extent):
    """pack + unpack of a device object that must go through the library"""
    torch = _torch()
    origin, buflen = geometry(runs, extent, 2)
    size = sum(n for _, n in runs) * 2
    host = np.random.default_rng(2).integers(0, 256, buflen, dtype=np.uint8)
    src = torch.from_numpy(host).to(gpu)
    out = torch.zeros(size, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    b = mpi.counters()
    assert mpi.Pack(src.data_ptr() + origin, 2, t, out.data_ptr(), size, 0) == size
    a = mpi.counters()
    assert a["lib_packs"] == b["lib_packs"] + 1 and a["irregular_packs"] == b["irregular_packs"]
    assert a["packs"] == b["packs"]
    exp = gather(host, origin, runs, extent, 2)
    assert np.array_equal(to_np(out), exp)
    dst = torch.full((buflen,), 0x3C, dtype=torch.uint8, device=gpu)
    torch.cuda.synchronize()
    assert mpi.Unpack(out.data_ptr(), size, 0, dst.data_ptr() + origin, 2, t) == size
    c = mpi.counters()
    assert c["lib_unpacks"] == a["lib_unpacks"] + 1 and c["irregular_unpacks"] == a["irregular_unpacks"]
    ref = np.full(buflen, 0x3C, dtype=np.uint8)
    scatter(exp, ref, origin, runs, extent, 2)
    assert np.array_equal(to_np(dst), ref)


def test_over_the_cap_goes_to_the_library(mpi, gpu):
    disps = [0, 3, 7, 12, 18, 25, 33, 42, 52]
    with irregular(mpi, True, 8):
        t = mpi.Type_commit(mpi.Type_create_hindexed_block(1, disps, mpi.BYTE))
        try:
            assert mpi.type_segments(t) is None
            _library_route(mpi, gpu, t, [(d, 1) for d in disps], 53)
        finally:
            mpi.Type_free(t)


def test_switched_off_after_commit_goes_to_the_library(mpi, gpu):
    with irregular(mpi):
        t, runs, extent = hindexed(mpi, [3, 1, 4], [0, 9, 20])
        try:
            round_trip(mpi, gpu, t, runs, extent, 2)
            assert mpi.irregular_config(False, 0) is True
            assert mpi.type_segments(t) is not None  # the list is kept, the route is not taken
            _library_route(mpi, gpu, t, runs, extent)
            mpi.irregular_config(True, 0)
            round_trip(mpi, gpu, t, runs, extent, 2)
        finally:
            mpi.Type_free(t)


def test_type_free_then_another_type(mpi, gpu):
    """MPI_Type_free of a used irregular type (its device table goes with it),
    then a different irregular type -- likely under the same handle"""
    with irregular(mpi):
        t, runs, extent = hindexed(mpi, [3, 1, 4], [0, 9, 20])
        round_trip(mpi, gpu, t, runs, extent, 2)
        mpi.Type_free(t)
        assert mpi.describe(t) is None and mpi.type_segments(t) is None
        t2, runs2, extent2 = hindexed(mpi, [8, 24, 16, 8], [64, 0, 128, 32])
        try:
            round_trip(mpi, gpu, t2, runs2, extent2, 3)
        finally:
            mpi.Type_free(t2)
