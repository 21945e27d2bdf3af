"""GPU tests of sst_table_certify (DeviceTable.certify, DynamicProgrammingTable
certify=True / .certify()): the device pass against the criterion's numpy
restatement (tests/_certify_model.py) on the reference's tiny tables, on
oracle-built tables of every compression, shape and last-column mask, on the
damaged and foreign tables a plain upload accepts, and the promotion itself --
a certified upload of the full 105-row table answers through the pair list,
the rows step, the length bound's fast path and the device pipeline exactly
as the table built by the engine does."""
import numpy as np
import pytest

import _certify_model as model
import _oracle as oracle
from conftest import load_golden
from spectrseqtools_amd import _native

pytestmark = pytest.mark.gpu
TOL, PREC = 1e-5, 1e-3


@pytest.fixture(scope="module")
def engine():
    return _native.get_engine(0)


def _probe(rng, ms, n, M):
    """Query masses: sums of up to three rows with jitter, and values over the whole table."""
    rows = np.array(ms[1:] if len(ms) > 1 else [1])
    sums = np.array([rows[rng.integers(0, len(rows), k)].sum() for k in rng.integers(1, 4, n)], dtype=np.float64)
    return np.concatenate([sums + rng.integers(-2, 3, n), rng.uniform(1, M + 5, n)]) * PREC


def _candidates(res):
    """Candidate lists of the queries that have one (SOME; an OVERFLOW / ABORTED query's count is no list)."""
    return [res.candidates(i) if res.status[i] == _native.SST_SOME else None for i in range(len(res.status))]


def _answers(dev, masses):
    thr = np.full(len(masses), 1.5 * PREC)
    res = dev.explain(masses, thr, TOL, PREC, -1)
    return dev.is_valid(masses, thr, TOL, PREC).tolist(), res.status.tolist(), _candidates(res)


# ---------------------------------------------------------------------------
# 1. the reference's tiny tables
# ---------------------------------------------------------------------------
def test_reference_tiny_tables(engine):
    rng = np.random.default_rng(11)
    seen = {True: 0, False: 0}
    for tiny in load_golden("tables.json")["tiny"]:
        C, ms = tiny["compression"], tiny["masses"]
        words = np.array(tiny["words"], dtype=model.DT[C])
        dev = _native.DeviceTable.upload(ms, words, C, engine=engine)
        masses = _probe(rng, ms, 40, words.shape[1] * C)
        before = _answers(dev, masses)
        want = model.certifiable(ms, C)
        assert dev.certify() is want, (ms, tiny["max_mass"], C)
        assert dev.certified is want
        assert _answers(dev, masses) == before
        built = _native.DeviceTable.build(ms, tiny["max_mass"], C, engine=engine)
        assert _answers(built, masses) == before
        assert np.array_equal(dev.pair_records(), built.pair_records() if want else [])
        seen[want] += 1
        dev.close()
        built.close()
    assert seen[True] >= 3 and seen[False] >= 3


# ---------------------------------------------------------------------------
# 2. shapes
# ---------------------------------------------------------------------------
def _alphabet(C, n_rows):
    # shift 0 (C, 2C), shift C - 1 (2C - 1), step 1 (C .. 2C - 1) and masses beyond every table here
    if n_rows == 1:
        return [0]
    if n_rows == 2:
        return [0, 2 * C - 1]
    small = [C + i for i in range(116)]  # every shift at C = 4 .. 32, steps 1 .. 29
    return [0] + small + [1025 * C, 1025 * C + 7, 4000 * C + C - 1]


@pytest.mark.parametrize("C", [4, 8, 16, 32])
def test_oracle_tables_of_every_shape_certify(engine, C):
    n = 0
    for n_rows in (1, 2, 120):
        ms = _alphabet(C, n_rows)
        assert len(ms) == n_rows and model.certifiable(ms, C)
        for n_cols in (1, 2, 257, 1025):
            # max_mass values sharing n_cols: one mask each; every mask at 257 columns and 2 rows
            top = n_cols * C - 1
            every = n_cols == 257 and n_rows == 2
            for max_mass in range(top - C + 1, top + 1) if every else (top, top - C // 2, top - C + 1):
                words = oracle.build_table(ms, max_mass, C)
                assert words.shape == (n_rows, n_cols)
                dev = _native.DeviceTable.upload(ms, words, C, engine=engine)
                assert not dev.certified
                assert dev.certify() is True and dev.certified, (ms, max_mass)
                assert dev.certify() is True  # nothing runs
                dev.close()
                n += 1
    assert n == 11 * 3 + C


def test_certified_small_table_matches_the_built_one(engine):
    ms, max_mass = [0, 40, 52, 70], 35 * 70
    built = _native.DeviceTable.build(ms, max_mass, 32, engine=engine)
    assert built.certified and len(built.pair_records()) > 0
    up = _native.DeviceTable.upload(ms, oracle.build_table(ms, max_mass, 32), 32, engine=engine)
    assert len(up.pair_records()) == 0
    rng = np.random.default_rng(5)
    masses = _probe(rng, ms, 300, max_mass)
    want = _answers(built, masses)
    assert _answers(up, masses) == want  # the bitset scan
    old = up.explain(masses, np.full(len(masses), 1.5 * PREC), TOL, PREC, -1)
    assert up.certify() is True
    assert np.array_equal(up.pair_records(), built.pair_records())
    assert up.scan_lds_hits() == built.scan_lds_hits()
    assert _answers(up, masses) == want  # the pair scan
    assert _candidates(old) == want[2]  # an earlier result stays readable
    again = _native.DeviceTable.upload(ms, built.download(), 32, engine=engine, certify=True)
    assert again.certified and np.array_equal(again.pair_records(), built.pair_records())
    for t in (built, up, again):
        t.close()


def test_result_created_before_certification_is_reused_after(engine):
    import torch

    ms, max_mass = [0, 40, 52, 70], 35 * 70
    built = _native.DeviceTable.build(ms, max_mass, 32, engine=engine)
    up = _native.DeviceTable.upload(ms, built.download(), 32, engine=engine)
    rng = np.random.default_rng(6)
    masses = _probe(rng, ms, 2000, max_mass)
    dm = torch.from_numpy(masses).cuda()
    dt = torch.full((len(masses),), 1.5 * PREC, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    want = built.explain_device(dm.data_ptr(), dt.data_ptr(), len(masses), TOL, PREC, -1).fetch_device()
    res = up.explain_device(dm.data_ptr(), dt.data_ptr(), len(masses), TOL, PREC, -1)
    res.fetch_device()
    assert up.certify() is True
    for r in (up.explain_device(dm.data_ptr(), dt.data_ptr(), len(masses), TOL, PREC, -1, reuse=res),
              up.explain_device(dm.data_ptr(), dt.data_ptr(), len(masses), TOL, PREC, -1)):
        r.fetch_device()
        assert np.array_equal(r.status, want.status)
        assert _candidates(r) == _candidates(want)
    built.close()
    up.close()


# ---------------------------------------------------------------------------
# 3. violations a plain upload accepts
# ---------------------------------------------------------------------------
MS, MAX_MASS, C3 = [0, 33, 47, 95, 20000], 300 * 32 - 5, 32  # 300 columns: two workgroups per row


def _cell_with_bit0(words, C, cell):
    """(row, col) of a word below the last row and column whose cell `cell` has bit0 set."""
    for r in range(1, words.shape[0] - 1):
        for c in range(1, words.shape[1] - 1):
            if (int(words[r, c]) >> (2 * (C - 1 - cell))) & 1:
                return r, c
    raise AssertionError("no such cell")


def _violations():
    good = oracle.build_table(MS, MAX_MASS, C3)
    assert good.shape == (5, 300) and model.first_violation(good, MS, C3) is None
    out = {"left bit at (1, 0)": (MS, model.flip_left(good, C3, 1, 0)[0], (1, 0)),
           "left bit at (last row, n_cols - 2)": (MS, model.flip_left(good, C3, 4, 298)[0], (4, 298)),
           "left bit in column 256": (MS, model.flip_left(good, C3, 2, 256)[0], (2, 256))}
    for cell in (0, C3 - 1):  # the first and the last cell of a word
        r, c = _cell_with_bit0(good, C3, cell)
        out[f"left bit of cell {cell} of a word"] = (MS, model.flip_left(good, C3, r, c, cell=cell)[0], (r, c))
    off = [0, 33, 48, 95, 20000]
    out["one mass off by one"] = (off, good, None)
    other = [0, 35, 47, 96, 20000]
    out["another alphabet's table"] = (MS, oracle.build_table(other, MAX_MASS, C3), None)
    lone = [0, 3 * C3 + 1, 3 * C3 + 2]  # nothing but mass 0 is reachable below 3C; mask k = 1
    sparse = oracle.build_table(lone, 3 * C3 - 2, C3)
    out["last-column bit outside the closure"] = (lone, model.stray_last_column_bit(sparse, lone, C3), (2, 2))
    return out


@pytest.fixture(scope="module")
def violations():
    return _violations()


@pytest.mark.parametrize("what", ["left bit at (1, 0)", "left bit at (last row, n_cols - 2)",
                                  "left bit in column 256", "left bit of cell 0 of a word",
                                  "left bit of cell 31 of a word", "one mass off by one",
                                  "another alphabet's table", "last-column bit outside the closure"])
def test_violation_is_reported_at_the_models_word(engine, violations, what):
    ms, words, at = violations[what]
    want = model.first_violation(words, ms, C3)
    assert want is not None and (at is None or want == at), (want, at)
    dev = _native.DeviceTable.upload(ms, words, C3, engine=engine)  # accepted today
    rng = np.random.default_rng(17)
    masses = _probe(rng, ms, 200, words.shape[1] * C3)
    before = _answers(dev, masses)
    with pytest.raises(_native.EngineError) as e:
        dev.certify()
    assert e.value.first_bad == want, (e.value.first_bad, want)
    lo = want[1] * C3
    assert f"row {want[0]}, column {want[1]} (masses {lo} to {lo + C3 - 1}" in str(e.value)
    assert not dev.certified and len(dev.pair_records()) == 0
    assert _answers(dev, masses) == before
    with pytest.raises(_native.EngineError):
        _native.DeviceTable.upload(ms, words, C3, engine=engine, certify=True)
    dev.close()


# ---------------------------------------------------------------------------
# 4. promotion at full size, 5. the device pipeline
# ---------------------------------------------------------------------------
def _dp(engine, max_len=20, **kw):
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation

    seq = SequenceInformation(max_len=max_len, su_mass=6500.0, obs_mass=6500.0, modification_rate=0.5)
    return DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                   precision=TOLERANCE, seq=seq, engine=engine, **kw)


@pytest.fixture(scope="module")
def built(engine):
    """The engine-built 105-row table."""
    dp = _dp(engine)
    assert dp.certified
    yield dp
    dp.close()


def _adopt(engine, built):
    """The same words adopted through the `table` setter."""
    dp = _dp(engine)
    dp.table = built.table
    assert not dp.certified and len(dp.device_table.pair_records()) == 0
    return dp


def _rows_step(dp, wl):
    import torch

    dev = torch.device("cuda", 0)
    do = torch.from_numpy(wl["obs"]).to(dev)
    dpo = torch.from_numpy(wl["peak_off"]).to(dev)
    ds = torch.from_numpy(wl["su_seq"]).to(dev)
    out7 = torch.full((4 * len(wl["obs"]),), 9, dtype=torch.int8, device=dev)
    torch.cuda.synchronize()
    A = round(dp.seq.modification_rate * dp.seq.max_len)
    res = dp.device_table.step_rows_device(do.data_ptr(), dpo.data_ptr(), len(wl["peak_off"]) - 1, len(wl["obs"]),
                                           ds.data_ptr(), wl["shifts"], wl["sides"], out7.data_ptr(),
                                           wl["max_weight"], dp.tolerance, dp.precision, A,
                                           int(len(wl["a8_mass"]) * 1.1) + 64)
    res.fetch_device()
    dp.device_table.engine.synchronize()
    return res, out7.cpu().numpy()


def _same_result(a, b):
    """Status, count and the candidate lists' bytes, query by query (the payload layout aside)."""
    from spectrseqtools_amd.parallel import canonical_digest

    return (np.array_equal(a.status, b.status) and np.array_equal(a.count, b.count) and
            canonical_digest(a.status, a.count, a.offset, a.payload) ==
            canonical_digest(b.status, b.count, b.offset, b.payload))


def test_full_table_promotion(engine, built):
    import bench
    import torch

    adopted = _adopt(engine, built)
    wl = bench.build_workload(400, 4242, built)
    with pytest.raises(_native.EngineError, match="no pair list"):
        _rows_step(adopted, wl)
    assert adopted.certify() is True and adopted.certified
    bt, at = built.device_table, adopted.device_table
    assert np.array_equal(at.pair_records(), bt.pair_records()) and len(at.pair_records()) > 0
    assert at.scan_lds_hits() == bt.scan_lds_hits()
    # 20 000 explain queries through the device path: the pair scan ran
    rng = np.random.default_rng(23)
    ms = np.array(bt.masses[1:])
    k = rng.integers(1, 4, 20000)
    masses = np.array([ms[rng.integers(0, len(ms), kk)].sum() for kk in k]) * PREC + rng.normal(0, 0.004, len(k))
    dm = torch.from_numpy(masses).cuda()
    dth = torch.from_numpy(1e-5 * rng.uniform(300, 14000, len(k))).cuda()
    torch.cuda.synchronize()
    A = round(built.seq.modification_rate * built.seq.max_len)
    got = at.explain_device(dm.data_ptr(), dth.data_ptr(), len(k), TOL, PREC, A)
    want = bt.explain_device(dm.data_ptr(), dth.data_ptr(), len(k), TOL, PREC, A)
    got.fetch_device()
    want.fetch_device()
    assert _same_result(got, want)
    assert got.pair_hits_device()[1] == want.pair_hits_device()[1]
    # the step's own queries (sliding-window differences: pair-class windows) are answered by the pair scan
    qm, qt = torch.from_numpy(wl["a8_mass"]).cuda(), torch.from_numpy(wl["a8_thr"]).cuda()
    torch.cuda.synchronize()
    got = at.explain_device(qm.data_ptr(), qt.data_ptr(), len(wl["a8_mass"]), TOL, PREC, A)
    want = bt.explain_device(qm.data_ptr(), qt.data_ptr(), len(wl["a8_mass"]), TOL, PREC, A)
    got.fetch_device()
    want.fetch_device()
    assert _same_result(got, want)
    assert got.pair_hits_device()[1] == want.pair_hits_device()[1] > 0
    # the step from the peaks
    r_got, a7_got = _rows_step(adopted, wl)
    r_want, a7_want = _rows_step(built, wl)
    assert np.array_equal(a7_got, a7_want) and np.array_equal(a7_got, wl["a7_valid"])
    assert r_got.n == r_want.n == len(wl["a8_mass"]) and _same_result(r_got, r_want)
    # the length bound (fast path and frontier are the closure's)
    su = rng.uniform(1500.0, 4000.0, 8)
    for d in ("lower", "upper"):
        g, gs = at.length_bound(su, su, TOL, PREC, 20, A, d)
        w, ws = bt.length_bound(su, su, TOL, PREC, 20, A, d)
        assert np.array_equal(g, w) and np.array_equal(gs, ws)
    adopted.close()


def test_pipeline_runs_on_a_certified_table(engine, built, tmp_path, monkeypatch):
    import _synth_cases as SC
    from spectrseqtools_amd import mass_table, pipeline_device as PD
    from spectrseqtools_amd.masses import build_breakage_dict

    v = SC.variant_inputs("full_ladders", n=8)
    bd = build_breakage_dict(*SC.TAGS)
    adopted = _adopt(engine, built)
    args = (v["obs"], v["offsets"], v["su_seq"], v["seq_mass"], bd)
    with pytest.raises(_native.EngineError, match="no pair list"):
        PD.run_batch(adopted, *args, max_len=v["max_len"])
    assert adopted.certify() is True
    want = PD.run_batch(built, *args, max_len=v["max_len"])
    got = PD.run_batch(adopted, *args, max_len=v["max_len"])
    assert len(got) == 8 and not got.default.all()
    assert got.equals(want)
    adopted.close()
    # the reference's own way to its table: the .npy cache
    monkeypatch.setattr(mass_table, "TABLE_DIR", str(tmp_path))
    cached = _dp(engine, use_cache=True, certify=True)
    assert cached.certified
    assert np.array_equal(cached.device_table.pair_records(), built.device_table.pair_records())
    cached.close()
