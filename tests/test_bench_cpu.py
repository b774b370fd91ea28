"""bench.py --dump-outputs: the table rows written as float64 are exact, ordered independently of hash-slot order,
and kept under the size cap."""
import os

import numpy as np

import bench
from trew_amd.capi import ROW_DTYPE


def random_rows(n, seed=1):
    rnd = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=ROW_DTYPE)
    rows["table"] = rnd.integers(0, 6, n)
    rows["k"] = rnd.integers(5, 65, n)
    rows["word_lo"] = rnd.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)  # bit 63 and bit 0 set
    rows["word_hi"] = rnd.integers(0, 1 << 40, n, dtype=np.uint64)
    rows["count"] = rnd.integers(1, 1 << 50, n, dtype=np.uint64)
    return rows


def test_dump_is_exact_and_sorted(tmp_path):
    rows = random_rows(5000)
    perm = np.random.default_rng(2).permutation(len(rows))
    bench.dump_outputs(str(tmp_path / "a"), rows)
    bench.dump_outputs(str(tmp_path / "b"), rows[perm])
    a = np.load(os.path.join(tmp_path, "a", "table_rows.npy"))
    b = np.load(os.path.join(tmp_path, "b", "table_rows.npy"))
    assert a.dtype == np.float64 and a.shape == (len(rows), 7)
    assert np.array_equal(a, b)
    u = a.astype(np.uint64)
    lo = u[:, 2] | (u[:, 3] << np.uint64(32))
    hi = u[:, 4] | (u[:, 5] << np.uint64(32))
    got = list(zip(u[:, 0].tolist(), u[:, 1].tolist(), hi.tolist(), lo.tolist(), u[:, 6].tolist()))
    want = sorted(zip(rows["table"].tolist(), rows["k"].tolist(), rows["word_hi"].tolist(), rows["word_lo"].tolist(),
                      rows["count"].tolist()))
    assert got == want


def test_dump_of_no_rows_and_over_the_cap(tmp_path, monkeypatch):
    bench.dump_outputs(str(tmp_path), np.zeros(0, dtype=ROW_DTYPE))
    assert np.load(os.path.join(tmp_path, "table_rows.npy")).shape == (0, 7)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * 7 * 8)
    rows = random_rows(1000)
    bench.dump_outputs(str(tmp_path), rows)
    a = np.load(os.path.join(tmp_path, "table_rows.npy"))
    bench.dump_outputs(str(tmp_path), rows[::-1])
    assert a.shape == (100, 7) and np.array_equal(a, np.load(os.path.join(tmp_path, "table_rows.npy")))
