#!/usr/bin/env python3
"""MPI_Pack / MPI_Unpack of irregular datatypes on device buffers: the opt-in
segment-list packer (TEMPI_IRREGULAR / tempi_irregular_config) against the
route these types take without it.

Feature OFF is the baseline: a type is then library-packed through host memory
(D2H of the touched span, the library's CPU pack, H2D of the result), which is
exactly what happens when the feature was never built. The same committed type
serves both sides -- it is committed with the feature on, and
tempi_irregular_config(0) sends later calls to the library -- and the two are
timed alternately, round by round, so that drift hits both alike.

One JSON line per shape: microseconds per call (median, min, p10, p90, max
over >= 20 timed calls after a warm-up, each call synchronous: MPI_Pack
returns when the bytes are there), GB/s of the touched bytes (packed bytes
read + written = 2 x packed) and that as a share of the ~6.3 TB/s the HBM
achieves. The packed bytes of both routes are compared before anything is
timed.

  python tools/irregular_bench.py [--reps 30] [--warmup 5] [--out FILE] [--shapes a,b,c,d,e]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_ACHIEVABLE_GBPS = 6300.0


def shape_runs(name, rng):
    """(description, [lens], [disps]) in bytes; runs never touch, so none merge"""
    if name == "a":  # 100,000 runs of 8-64 B, sorted random 8-aligned displacements inside 64 MiB
        n, cell = 100_000, 664
        lens = 8 * rng.integers(1, 9, n)
        offs = 8 * rng.integers(0, (cell - 64 - 8) // 8 + 1, n)
        return "100k runs of 8-64 B in 64 MiB", lens, np.arange(n) * cell + offs
    if name == "b":  # 64 runs of 0.5-2 MiB
        n, cell = 64, (2 << 20) + 64
        lens = 8 * rng.integers((1 << 19) // 8, (2 << 20) // 8 + 1, n)
        return "64 runs of 0.5-2 MiB", lens, np.arange(n) * cell
    if name == "c":  # 1,000,000 runs of 8 B, irregular strides (16 or 24 or 32 bytes apart)
        n = 1_000_000
        return "1M runs of 8 B, irregular strides", np.full(n, 8), np.arange(n) * 24 + 8 * rng.integers(0, 2, n)
    if name == "d":  # shape (a) with 1-7 byte runs at any displacement: one-byte words
        n, cell = 100_000, 664
        lens = rng.integers(1, 8, n)
        offs = rng.integers(0, cell - 8, n)
        return "100k runs of 1-7 B in 64 MiB", lens, np.arange(n) * cell + offs
    if name == "e":  # the small-call cost
        return "3 runs, 8 bytes", np.array([3, 1, 4]), np.array([0, 9, 20])
    raise ValueError(name)


def stats(us):
    q = statistics.quantiles(us, n=10)
    return {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "p10": round(q[0], 2),
            "p90": round(q[-1], 2), "max": round(max(us), 2), "n": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="on / off alternations the repetitions are split over")
    ap.add_argument("--shapes", default="a,b,c,d,e")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 timed repetitions"

    import torch

    import tempi_amd

    if not torch.cuda.is_available():
        sys.exit("irregular_bench needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    mpi = tempi_amd.get_mpi()
    mpi.Init()
    lines = []
    try:
        assert mpi.gpu_available()
        for name in args.shapes.split(","):
            rng = np.random.default_rng(ord(name))
            what, lens, disps = shape_runs(name, rng)
            lens, disps = [int(x) for x in lens], [int(x) for x in disps]
            mpi.irregular_config(True)
            t = mpi.Type_commit(mpi.Type_create_hindexed(lens, disps, mpi.BYTE))
            seg = mpi.type_segments(t)
            assert seg is not None and len(seg[0]) == len(lens), "the shape's runs merged or passed the cap"
            size = sum(lens)
            span = disps[-1] + lens[-1]
            src = torch.randint(0, 256, (span,), dtype=torch.uint8, device=dev)
            out = {True: torch.zeros(size, dtype=torch.uint8, device=dev),
                   False: torch.zeros(size, dtype=torch.uint8, device=dev)}
            back = torch.zeros(span, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def pack(on):
                mpi.Pack(src.data_ptr(), 1, t, out[on].data_ptr(), size, 0)

            def unpack(on):
                mpi.Unpack(out[True].data_ptr(), size, 0, back.data_ptr(), 1, t)

            # same bytes on both routes, and the route each side is meant to take
            c0 = mpi.counters()
            for on in (True, False):
                mpi.irregular_config(on)
                pack(on)
            c1 = mpi.counters()
            assert c1["irregular_packs"] == c0["irregular_packs"] + 1 and c1["lib_packs"] == c0["lib_packs"] + 1
            assert torch.equal(out[True], out[False]), f"shape {name}: GPU and library packs differ"
            for on in (True, False):
                mpi.irregular_config(on)
                back.zero_()
                torch.cuda.synchronize()
                unpack(on)
                assert torch.equal(back[disps[0]:disps[0] + lens[0]], out[True][:lens[0]])

            times = {(op, on): [] for op in ("pack", "unpack") for on in (True, False)}
            per_round = -(-args.reps // args.rounds)
            for rnd in range(args.rounds):
                for on in (True, False):
                    mpi.irregular_config(on)
                    for op, fn in (("pack", pack), ("unpack", unpack)):
                        for _ in range(args.warmup if rnd == 0 else 1):
                            fn(on)
                        for _ in range(per_round):
                            t0 = time.perf_counter()
                            fn(on)  # synchronous: returns when the bytes are there
                            times[(op, on)].append((time.perf_counter() - t0) * 1e6)
            rec = {"bench": "irregular", "shape": name, "what": what, "runs": len(lens), "packed_bytes": size,
                   "span_bytes": span, "word_width_bytes": 1 if name in "de" else 8}
            for op in ("pack", "unpack"):
                on_s, off_s = stats(times[(op, True)]), stats(times[(op, False)])
                gbps = 2 * size / (on_s["median"] * 1e-6) / 1e9
                rec[op] = {"on_us": on_s, "off_us": off_s,
                           "speedup_median": round(off_s["median"] / on_s["median"], 2),
                           "on_GBps_touched": round(gbps, 2),
                           "on_share_of_hbm_achievable": round(gbps / HBM_ACHIEVABLE_GBPS, 4)}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            mpi.irregular_config(False)
            mpi.Type_free(t)
            del src, out, back
    finally:
        mpi.irregular_config(False)
        mpi.Finalize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
