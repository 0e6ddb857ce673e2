"""Shared by test_irregular_cpu.py and test_irregular_gpu.py: the fixed list of
irregular recipes (grammar: oracle/recipe.h), the multi-type struct, and the
helpers that turn the opt-in feature on for the length of a test.

Every recipe is irregular by construction: two of its block lengths differ,
or three of its displacements have unequal gaps (directly, or in a child), so
TEMPI's strided canonicaliser (core/types.cpp) rejects it.
"""
import contextlib

import numpy as np

DEFAULT_MAX_SEGS = 1 << 20

RAGGED = "hindexed([3,1,4],[0,9,20],byte)"

RECIPES = [
    RAGGED,                                                  # ragged hindexed
    "hindexed([2,2,2],[0,5,13],byte)",                       # equal blocks, unequal gaps
    "hindexed([5,3,7],[1,11,23],byte)",                      # odd displacements
    "indexed([1,2,3],[0,4,10],double)",                      # indexed over double, ragged
    "indexed([2,2,2],[0,3,9],double)",                       # indexed over double, unequal gaps
    "indexed([2,0,3],[0,5,9],int)",                          # a zero-length block in the middle
    "indexed_block(2,[0,3,9],int)",                          # indexed_block, unequal gaps
    "indexed_block(1,[0,5,6,20],double)",                    # ... two blocks that merge into one run
    "hindexed_block(3,[0,7,30],byte)",
    "hindexed([4,2,6],[40,-16,8],byte)",                     # negative and out of order
    "hindexed([1,1,1],[20,0,7],short)",                      # out of order
    f"vector(3,1,2,{RAGGED})",                               # vector over a ragged hindexed
    "vector(2,2,3,hindexed([2,5],[0,8],byte))",
    f"hvector(3,1,100,{RAGGED})",
    f"contig(3,{RAGGED})",
    "hindexed([2,1,3],[0,200,500],vector(3,2,5,byte))",      # ragged hindexed over a vector
    "indexed([1,3],[0,2],vector(2,1,3,int))",
    "struct([1,2,1],[0,16,64],double)",
    f"resized(0,64,{RAGGED})",                               # padded extent
    "resized(-8,40,hindexed([4,2,6],[24,-8,8],byte))",       # negative lower bound
    "hindexed([1,2],[0,100],subarray(C,[4,6],[2,3],[1,2],byte))",
    "struct([1,1,1],[0,40,100],subarray(C,[4,6],[2,3],[1,2],byte))",  # subarray in struct
    "subarray(F,[3,4],[2,2],[1,1],hindexed([1,2],[0,3],byte))",      # Fortran subarray of a ragged element
    f"dup({RAGGED})",
]

# {char x 3 @ 0, double x 2 @ 8, int x 1 @ 28, short x 5 @ 40}, resized to extent 64
STRUCT_RUNS = [(0, 3), (8, 16), (28, 4), (40, 10)]
STRUCT_EXTENT = 64


def build_struct(mpi):
    """the committed multi-type struct and the handles to free after it"""
    s = mpi.Type_create_struct([3, 2, 1, 5], [0, 8, 28, 40], [mpi.CHAR, mpi.DOUBLE, mpi.INT, mpi.SHORT])
    t = mpi.Type_commit(mpi.Type_create_resized(s, 0, STRUCT_EXTENT))
    return t, [s]


@contextlib.contextmanager
def irregular(mpi, on=True, max_segs=DEFAULT_MAX_SEGS):
    """the feature on (or off) inside the block; the previous state and the
    default cap are restored whatever happens"""
    prev = mpi.irregular_config(on, max_segs)
    try:
        yield
    finally:
        mpi.irregular_config(prev, DEFAULT_MAX_SEGS)


def gather(buf, origin, runs, extent, count):
    """numpy restatement of MPI_Pack by a segment list"""
    parts = [buf[origin + e * extent + d:origin + e * extent + d + n] for e in range(count) for d, n in runs]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def scatter(packed, buf, origin, runs, extent, count):
    """... and of MPI_Unpack (in place)"""
    p = 0
    for e in range(count):
        for d, n in runs:
            buf[origin + e * extent + d:origin + e * extent + d + n] = packed[p:p + n]
            p += n


def geometry(runs, extent, count):
    """(origin, buflen) of a buffer that holds `count` elements"""
    lo = min(d for d, _ in runs)
    hi = max(d + n for d, n in runs)
    span = (count - 1) * extent
    lo, hi = lo + min(span, 0), hi + max(span, 0)
    origin = -lo if lo < 0 else 0
    return origin, origin + max(hi, 1)
