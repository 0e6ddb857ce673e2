"""bench.py's timed path on a small object: --steps sets the number of timed
steps, the line carries ms_per_step, and --dump-outputs writes what the last
step computed -- the packed buffer and the unpacked object -- checked here
against the source pattern (byte i = i & 0xFF), whole and sampled."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

# an odd row count, more than one block of the kernel; the object (ROWS * PITCH
# bytes) stays under bench.DUMP_SAMPLE, so that the "whole" case dumps all of it
ROWS, PITCH, BLOCK = 4093, 1024, 512


def _expected():
    src = (np.arange(ROWS * PITCH, dtype=np.int64) & 0xFF).astype(np.float32).reshape(ROWS, PITCH)
    unpacked = np.zeros_like(src)
    unpacked[:, :BLOCK] = src[:, :BLOCK]
    return src[:, :BLOCK].reshape(-1).copy(), unpacked.reshape(-1)


@pytest.mark.parametrize("sample", [None, 1 << 20], ids=["whole", "sampled"])
def test_plain_headline_and_dump(mpi, gpu, tmp_path, monkeypatch, sample):
    import torch

    if sample:
        monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", str(ROWS),
                                      "--pitch", str(PITCH), "--block", str(BLOCK), "--dump-outputs", str(tmp_path)])
    args = bench.parse()
    before = mpi.counters()
    rec = bench.headline(args, mpi, torch, 0, 1, None, gpu)
    line = bench.compact_line(rec)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["unit"] == "GB/s" and line["dtype"] == "u8"
    assert line["value"] == pytest.approx(4.0 * ROWS * BLOCK / (line["ms_per_step"] * 1e-3) / 1e9, rel=0.02)
    assert line["roofline"]["timed_launches"] == 6 and line["roofline"]["d2d_copy_GBps"] is None
    # reset_counters() in the headline: the counters hold the timed steps alone
    after = mpi.counters()
    assert (after["packs"], after["unpacks"]) == (3, 3), (before, after)
    exp_packed, exp_unpacked = _expected()
    for name, exp in (("packed", exp_packed), ("unpacked", exp_unpacked)):
        got = np.load(tmp_path / (name + ".npy"))
        idx = bench.dump_indices(exp.size)
        assert (idx is None) == (sample is None)
        assert got.dtype == np.float32 and np.array_equal(got, exp if idx is None else exp[idx]), name
