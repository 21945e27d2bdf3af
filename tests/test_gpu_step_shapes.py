"""GPU tests of the fused step's grid shapes (through the C ABI):
sst_step_device -- is_valid over the peaks and the pair scan in one launch,
the scan's arguments passed as one struct and read again from the kernarg
segment after its tile loop -- against sst_is_valid_peaks_device +
sst_explain_batch_device on the same inputs, per query: status, count, the
exact candidate bytes, every is_valid byte; a sample through the per-query
accessor; and every query against the CPU oracle: status, count, and the byte
length and digest of its exact candidate list.

Query counts sit around the scan's tile rounds: fewer tiles than waves, one
full round of 64-query tiles over W waves, and the odd and even exits of the
two-tile unrolled loop, for W = 4096 (one 1024-lane scan workgroup per CU on
256 CUs, the step's grid) and W = 6144.  Peak counts sit around the is_valid
workgroups' 512 / 1024 peaks."""
import numpy as np
import pytest

import _digest
import _oracle as oracle
from conftest import load_golden
from spectrseqtools_amd import _native

pytestmark = pytest.mark.gpu

TOL, PREC = 1e-5, 1e-3
CANONICAL = (305042, 306026, 329053, 345048)
SHIFTS = np.array([0.0, 375.183, 537.119, 912.303])
W_STEP, W_WIDE = 4096, 6144
N_QUERIES = sorted({1, 63, 64, 65} | {64 * w + d for w in (W_STEP, W_WIDE) for d in (-1, 0, 1)} |
                   {k * w + 1 for w in (W_STEP, W_WIDE) for k in (128, 192)})
N_PEAKS = (1, 511, 512, 513, 1025)
N_VARIANT = 64 * W_STEP + 1


@pytest.fixture(scope="module")
def engine():
    return _native.get_engine(0)


@pytest.fixture(scope="module")
def rows():
    g = load_golden("alphabet.json")
    return sorted({r["tolerated_integer_masses"] for r in g["rows"]} | {0})


def _budgets(rows):
    is_mod = [m not in CANONICAL and m != 0 for m in rows]
    return is_mod, [round(20 * (0.5 if md else (1.0 if m else 0.0))) for m, md in zip(rows, is_mod)]


@pytest.fixture(scope="module")
def dev(engine, rows):
    t = _native.DeviceTable.build(rows, max(rows) * 35, 32, engine=engine)
    t.set_budgets(*_budgets(rows))
    return t


@pytest.fixture(scope="module")
def orc(rows):
    """The oracle's table and alphabet of `dev` (built once)."""
    return oracle.build_table(rows, max(rows) * 35, 32), oracle.Alphabet(rows, *_budgets(rows))


def check_vs_oracle(res, orc, masses, thr, mods, what):
    """All queries of a fetched result against the oracle's digests (16 threads)."""
    host, alph = orc
    A = 10 if mods is None else mods
    want = oracle.explain_digest_batch(host, 32, alph, masses, thr, A, TOL, nthreads=16)
    one = lambda i: oracle.explain_table(host, 32, alph, masses[i], None if thr is None else thr[i], TOL,
                                         int(np.broadcast_to(A, len(masses))[i]))[1]
    return _digest.assert_equals_oracle(res, want, one, _native, what)


def _queries(rng, rows, n, kind="mixed"):
    """Masses and thresholds: sums of one or two rows plus noise ("mixed":
    hits and misses on the pair list), "none": below the first reachable
    mass, "all": exact one-row masses with a wide threshold, "routed": some
    three-row sums (windows past the pair list: the routing block and the
    deferred class lists run)."""
    ints = np.array(rows[1:], dtype=np.int64)
    pick = lambda: ints[rng.integers(0, len(ints), n)]
    if kind == "none":
        return rng.uniform(0.2, 0.9, n), 1e-5 * rng.uniform(300, 2000, n)
    if kind == "all":
        return pick() * 1e-3, np.full(n, 0.02)
    m = pick() + np.where(rng.random(n) < 0.5, pick(), 0)
    if kind == "routed":
        m = m + np.where(rng.random(n) < 0.02, pick(), 0)
    return m * 1e-3 + rng.normal(0, 0.004, n), 1e-5 * rng.uniform(300, 14000, n)


def _candidate_bytes(res):
    """Per SOME query, in query order: the byte length of its candidate list
    and the lists' bytes, concatenated (the payload's layout taken out)."""
    qs = np.flatnonzero(res.status == _native.SST_SOME)
    beg = res.offset[qs].astype(np.int64)
    c = res.count[qs].astype(np.int64)
    pos = beg.copy()
    act = np.flatnonzero(c > 0)
    k = 0
    while len(act):
        pos[act] += 1 + res.payload[pos[act]].astype(np.int64)
        k += 1
        act = act[c[act] > k]
    ln = pos - beg
    idx = np.repeat(beg - (np.cumsum(ln) - ln), ln) + np.arange(int(ln.sum()))
    return ln, res.payload[idx]


def _check_step(engine, dev, orc, masses, thr, n_peaks, rng, mods=None, expect=None):
    """One step against the two separate calls and, every query, against the
    oracle; returns the step's result."""
    torch = pytest.importorskip("torch")
    n = len(masses)
    dev_t = torch.device("cuda", engine.device)
    obs = np.sort(rng.uniform(150.0, 9000.0, n_peaks))
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev_t)
    dm, dt, do, dmods = up(masses), up(thr), up(obs), up(mods)
    ptr = lambda t: None if t is None else t.data_ptr()
    out_a = torch.full((4 * n_peaks,), 9, dtype=torch.int8, device=dev_t)
    out_b = torch.full_like(out_a, 7)
    torch.cuda.synchronize()  # the engine queues on its own stream
    res = dev.step_device(do.data_ptr(), n_peaks, SHIFTS, out_a.data_ptr(), dm.data_ptr(), ptr(dt), n, TOL, PREC, 10,
                          d_mods=ptr(dmods))
    res.fetch_device()
    dev.is_valid_peaks_device(do.data_ptr(), n_peaks, SHIFTS, TOL, PREC, out_b.data_ptr())
    ref = dev.explain_device(dm.data_ptr(), ptr(dt), n, TOL, PREC, 10, d_mods=ptr(dmods))
    ref.fetch_device()
    engine.synchronize()
    assert np.array_equal(out_a.cpu().numpy(), out_b.cpu().numpy())
    assert np.array_equal(res.status, ref.status)
    counted = np.isin(res.status, (_native.SST_SOME, _native.SST_OVERFLOW))
    assert np.array_equal(res.count[counted], ref.count[counted])
    (ln_a, by_a), (ln_b, by_b) = _candidate_bytes(res), _candidate_bytes(ref)
    assert np.array_equal(ln_a, ln_b) and np.array_equal(by_a, by_b)
    some = np.flatnonzero(res.status == _native.SST_SOME)
    for i in some[rng.integers(0, len(some), min(len(some), 50))] if len(some) else ():
        assert res.candidates(int(i)) == ref.candidates(int(i)), i
    if expect == "none":
        assert not counted.any()
    if expect == "all":
        assert (res.status == _native.SST_SOME).all()
    ref.close()
    check_vs_oracle(res, orc, masses, thr, mods, f"step, n = {n}")
    return res


@pytest.mark.parametrize("n", N_QUERIES)
def test_step_query_counts(engine, dev, orc, rows, n):
    rng = np.random.default_rng(100 + n % 97)
    masses, thr = _queries(rng, rows, n)
    _check_step(engine, dev, orc, masses, thr, 513, rng).close()


@pytest.mark.parametrize("n_peaks", N_PEAKS)
@pytest.mark.parametrize("n", (65, 64 * W_STEP + 1))
def test_step_peak_counts(engine, dev, orc, rows, n, n_peaks):
    rng = np.random.default_rng(200 + n_peaks)
    masses, thr = _queries(rng, rows, n)
    _check_step(engine, dev, orc, masses, thr, n_peaks, rng).close()


@pytest.mark.parametrize("variant", ("no_thresholds", "per_query_mods", "mods_no_thresholds", "none", "all", "routed"))
def test_step_input_variants(engine, dev, orc, rows, variant):
    rng = np.random.default_rng(300)
    n = N_VARIANT if variant != "routed" else 64 * 65 + 1  # (routed: five workgroups; the deferred DFS is slow)
    kind = variant if variant in ("none", "all", "routed") else "mixed"
    masses, thr = _queries(rng, rows, n, kind)
    mods = rng.integers(0, 12, n).astype(np.int64) if "mods" in variant else None
    if "no_thresholds" in variant:
        thr = None
    res = _check_step(engine, dev, orc, masses, thr, 1025, rng, mods=mods, expect=kind)
    if variant == "routed":  # windows past the pair list were answered (three and more rows)
        some = np.flatnonzero(res.status == _native.SST_SOME)
        assert (res.payload[res.offset[some].astype(np.int64)] > 2).any()  # a first candidate's row count
    res.close()


def test_step_sample_vs_oracle(engine, dev, orc, rows):
    """A step's answers on a sample of its queries against the CPU oracle."""
    rng = np.random.default_rng(400)
    n = 64 * W_STEP + 65
    masses, thr = _queries(rng, rows, n)
    res = _check_step(engine, dev, orc, masses, thr, 513, rng)
    host, alph = orc
    for i in np.concatenate([rng.integers(0, n, 150), [0, 63, 64, n - 65, n - 64, n - 1]]):
        st, sols, n_empty, _ = oracle.explain_table(host, 32, alph, masses[i], thr[i], TOL, 10)
        want = _native.SST_OUT_OF_TABLE if st < 0 else (
            _native.SST_SOME if sols else (_native.SST_EMPTY if n_empty else _native.SST_NONE))
        assert int(res.status[i]) == want, i
        if sols:
            assert res.candidates(int(i)) == sols, i
    res.close()
