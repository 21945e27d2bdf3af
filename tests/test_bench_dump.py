"""bench.py --dump-outputs: the arrays written for a result (host logic, CPU only)."""
import types

import numpy as np

import bench


def _result(n, rng):
    """A fetched result with 0..3 candidates per SOME query and pad bytes
    between the queries' records (layout, not answers)."""
    status = rng.choice(np.array([0, 1, 2, -1], dtype=np.int8), n)
    count = np.zeros(n, np.uint64)
    offset = np.zeros(n, np.uint64)
    pay, want = [], []
    for i in np.flatnonzero(status == 2):
        offset[i] = len(pay)
        count[i] = rng.integers(0, 4)
        for _ in range(int(count[i])):
            rows = sorted(rng.integers(0, 105, rng.integers(1, 6)).tolist())
            pay += [len(rows)] + rows
            want.append((i, [len(rows)] + rows))
        pay += [255] * int(rng.integers(0, 3))
    return types.SimpleNamespace(status=status, count=count, offset=offset,
                                 payload=np.array(pay, dtype=np.uint8)), want


def test_dump_small_result_is_complete(tmp_path):
    rng = np.random.default_rng(5)
    r, want = _result(500, rng)
    valid = rng.integers(0, 2, 2000).astype(np.int8)
    bench.dump_outputs(str(tmp_path), r, valid)
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("a7_valid", "a8_status", "a8_count", "a8_candidates")}
    assert got["a7_valid"].dtype == np.float32 and np.array_equal(got["a7_valid"], valid)
    assert got["a8_status"].dtype == np.float32 and np.array_equal(got["a8_status"], r.status)
    assert got["a8_count"].dtype == np.float64 and np.array_equal(got["a8_count"], r.count)
    assert got["a8_candidates"].dtype == np.float32
    assert got["a8_candidates"].tolist() == [x for _, rec in want for x in rec]


def test_dump_samples_large_arrays_the_same_way_each_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_QUERIES", 100)
    monkeypatch.setattr(bench, "DUMP_CAND_BYTES", 64)
    rng = np.random.default_rng(6)
    r, want = _result(1000, rng)
    valid = rng.integers(0, 2, 700).astype(np.int8)
    bench.dump_outputs(str(tmp_path / "a"), r, valid)
    bench.dump_outputs(str(tmp_path / "b"), r, valid, suffix="_rank1")
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("a7_valid", "a8_status", "a8_count", "a8_candidates")}
    for n, x in a.items():
        assert np.array_equal(x, np.load(tmp_path / "b" / f"{n}_rank1.npy")), n
    assert len(a["a7_valid"]) == len(a["a8_status"]) == len(a["a8_count"]) == 100
    # the sample is a subsequence of the queries: counts are those of the sampled SOME queries
    q = np.sort(np.random.default_rng(20240229).choice(1000, 100, replace=False))
    assert np.array_equal(a["a8_status"], r.status[q]) and np.array_equal(a["a8_count"], r.count[q])
    recs = [x for i, rec in want if i in set(q.tolist()) for x in rec]
    assert 0 < len(a["a8_candidates"]) <= 64 and a["a8_candidates"].tolist() == recs[:len(a["a8_candidates"])]
