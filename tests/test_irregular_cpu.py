"""Host side of the opt-in segment-list packer (no GPU): the flattening of
irregular datatypes at MPI_Type_commit (core/seglist.cpp) against the oracle's
type map (oracle/typemap.c) and the library's own MPI_Pack, the default-off
contract, and the run cap.
"""
import numpy as np
import pytest

from oracle import pyoracle
from tests import golden_data as G
from tests import typezoo
from tests.irregular_cases import (RECIPES, STRUCT_EXTENT, STRUCT_RUNS, build_struct, gather, geometry, irregular)

GOLDENS = ["zoo_hi", "zoo_hib", "hindexed_irregular", "struct_irregular"]


def test_default_is_off(mpi):
    """with nothing set the type has no segment list and stays not-valid"""
    t, temps, basic = typezoo.build(mpi, "hindexed([3,1,4],[0,9,20],byte)")
    try:
        assert mpi.type_segments(t) is None
        assert not mpi.describe(t)["valid"]
    finally:
        typezoo.free(mpi, t, temps, basic)


def test_counters_end_with_the_irregular_pair(mpi):
    assert list(mpi.counters())[-2:] == ["irregular_packs", "irregular_unpacks"]


def _library_pack(mpi, t, host, origin, count):
    size = mpi.Pack_size(count, t)
    out = np.zeros(max(size, 1), dtype=np.uint8)
    pos = mpi.Pack(host.ctypes.data + origin, count, t, out.ctypes.data, size, 0)
    return out[:pos]


@pytest.mark.parametrize("recipe", [G.case(n)["recipe"] for n in GOLDENS] + RECIPES)
def test_segments_match_the_oracle_and_the_library(mpi, recipe):
    tm = pyoracle.TypeMap(recipe)
    with irregular(mpi):
        t, temps, basic = typezoo.build(mpi, recipe)
    try:
        d = mpi.describe(t)
        assert d is not None and not d["valid"], f"{recipe} is not irregular: {d}"
        seg = mpi.type_segments(t)
        assert seg is not None, recipe
        runs, extent = seg
        assert len(runs) > 0
        assert runs == tm.segments()
        assert extent == tm.extent == mpi.Type_get_extent(t)[1]
        for count in (1, 3):
            origin, buflen = tm.geometry(count)
            host = np.random.default_rng(count).integers(0, 256, buflen, dtype=np.uint8)
            lib = _library_pack(mpi, t, host, origin, count)
            assert lib.size == tm.size * count
            assert np.array_equal(gather(host, origin, runs, extent, count), lib), (recipe, count)
    finally:
        typezoo.free(mpi, t, temps, basic)


def test_multi_type_struct(mpi):
    with irregular(mpi):
        t, temps = build_struct(mpi)
    try:
        assert not mpi.describe(t)["valid"]
        assert mpi.type_segments(t) == (STRUCT_RUNS, STRUCT_EXTENT)
        origin, buflen = geometry(STRUCT_RUNS, STRUCT_EXTENT, 2)
        host = np.random.default_rng(5).integers(0, 256, buflen, dtype=np.uint8)
        lib = _library_pack(mpi, t, host, origin, 2)
        assert np.array_equal(gather(host, origin, STRUCT_RUNS, STRUCT_EXTENT, 2), lib)
    finally:
        for x in temps + [t]:
            mpi.Type_free(x)


def test_strided_types_have_no_segment_list(mpi):
    with irregular(mpi):
        t, temps, basic = typezoo.build(mpi, "vector(1024,512,1024,byte)")
    try:
        assert mpi.type_segments(t) is None
        assert mpi.describe(t)["valid"]
    finally:
        typezoo.free(mpi, t, temps, basic)


def test_types_committed_while_off_stay_with_the_library(mpi):
    t, temps, basic = typezoo.build(mpi, "hindexed([3,1,4],[0,9,20],byte)")
    try:
        with irregular(mpi):
            assert mpi.type_segments(t) is None
    finally:
        typezoo.free(mpi, t, temps, basic)


def test_config_returns_the_previous_state(mpi):
    prev = mpi.irregular_config(True)
    try:
        assert prev is False  # the default
        assert mpi.irregular_config(True) is True
        assert mpi.irregular_config(False) is True
        assert mpi.irregular_config(False) is False
    finally:
        mpi.irregular_config(prev)


NINE = [0, 3, 7, 12, 18, 25, 33, 42, 52]


@pytest.mark.parametrize("recipe,runs", [
    (f"hindexed_block(1,{NINE},byte)", None),                                 # 9 runs: over the cap
    (f"hindexed_block(1,{NINE[:8]},byte)", 8),                                # 8 runs: exactly at it
    ("hindexed_block(1,[0,1,10,11,20,21,30,31,40,41,50,51],byte)", 6),        # 12 blocks merging into 6 runs
    ("vector(3,1,2,hindexed([3,1,4],[0,9,20],byte))", None),                  # 3 x 3 runs through a child
])
def test_cap_counts_merged_runs(mpi, recipe, runs):
    recipe = recipe.replace(" ", "")
    with irregular(mpi, True, 8):
        t, temps, basic = typezoo.build(mpi, recipe)
    try:
        seg = mpi.type_segments(t)
        assert not mpi.describe(t)["valid"]
        if runs is None:
            assert seg is None
        else:
            assert len(seg[0]) == runs and seg[0] == pyoracle.TypeMap(recipe).segments()
    finally:
        typezoo.free(mpi, t, temps, basic)
    # the cap is back at its default: the 9-run type flattens again
    with irregular(mpi):
        t, temps, basic = typezoo.build(mpi, f"hindexed_block(1,{NINE},byte)".replace(" ", ""))
    try:
        assert len(mpi.type_segments(t)[0]) == 9
    finally:
        typezoo.free(mpi, t, temps, basic)
