"""bench.py --dump-outputs: the last timed step's verdict codes as float32,
one file per rank, a fixed sample (in index order) above the size cap.  CPU
only: the codes are made up here."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402


def test_dump_writes_every_code_as_float32(tmp_path):
    codes = (np.arange(1000) % 5 - 3).astype(np.int8)
    bench.dump_outputs(str(tmp_path / "d"), codes, 0, 1)
    got = np.load(tmp_path / "d" / "verdicts.npy")
    assert got.dtype == np.float32 and np.array_equal(got, codes.astype(np.float32))
    bench.dump_outputs(str(tmp_path / "d"), codes, 1, 2)
    assert np.array_equal(np.load(tmp_path / "d" / "verdicts_rank1.npy"), got)


def test_dump_samples_a_large_output_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX", 256)
    codes = (np.arange(1000) % 7 - 3).astype(np.int8)
    bench.dump_outputs(str(tmp_path / "a"), codes, 0, 2)      # this rank's share: 128 codes
    bench.dump_outputs(str(tmp_path / "b"), codes, 0, 2)
    a, b = np.load(tmp_path / "a" / "verdicts_rank0.npy"), np.load(tmp_path / "b" / "verdicts_rank0.npy")
    assert a.shape == (128,) and np.array_equal(a, b)
    idx = np.sort(np.random.default_rng(0).choice(1000, 128, replace=False))
    assert np.array_equal(a, codes[idx].astype(np.float32))
