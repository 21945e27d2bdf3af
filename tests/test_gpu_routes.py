"""GPU tests of the explain engine's routes against the CPU oracle: windows on
every routing threshold and one group of windows per route (tests/
_route_cases.py; test_route_cases.py shows from the oracle alone that none is
vacuous).  Each case runs through sst_explain_batch on a built table (the
fused scan and its routing block), on an uploaded copy of the same words (no
pair list: k_bitset_scan, the expand kernel, the deferred classes) and
through sst_step_device, with and without the memo.  Every query's status,
count and exact candidate list (byte length and digest) must equal the
oracle's, and sst_result_stats must show that the route a group is meant for
ran at least as many queries as the group has queries with candidates."""
import numpy as np
import pytest

import _digest
import _route_cases as R
from spectrseqtools_amd import _native

pytestmark = pytest.mark.gpu

SHIFTS = np.array([0.0, 375.183])
MODES = ("explain", "uploaded", "step")


@pytest.fixture(scope="module")
def engine():
    return _native.get_engine(0)


@pytest.fixture(scope="module")
def device_tables(engine):
    """name -> {"explain" / "step": the built table, "uploaded": its words
    uploaded as they are (not certified: no pair list)}."""
    out = {}
    for name, t in R.tables().items():
        built = _native.DeviceTable.build(t.rows, t.max_mass, 32, engine=engine)
        built.set_budgets(t.is_mod, t.caps)
        up = _native.DeviceTable.upload(t.rows, built.download(), 32, engine=engine)
        up.set_budgets(t.is_mod, t.caps)
        assert built.certified and not up.certified
        assert len(built.pair_records()) > 0 and len(up.pair_records()) == 0
        out[name] = {"explain": built, "step": built, "uploaded": up}
    yield out
    for d in out.values():
        d["explain"].close(), d["uploaded"].close()


def _engine_budget(A):
    return np.inf if A == R.INF else int(A)


def run(engine, device_tables, case, mode, with_memo, cap=2 ** 32, sl=slice(None)):
    """The case's queries [sl] through one entry point -> the fetched result."""
    dev = device_tables[case.table.name][mode]
    mass, thr = case.mass[sl], case.thr[sl]
    per_query = not np.isscalar(case.A)
    if mode != "step":
        A = [_engine_budget(a) for a in case.A[sl]] if per_query else _engine_budget(case.A)
        return dev.explain(mass, thr, R.TOL, R.PREC, A, with_memo=with_memo, cap=cap)
    torch = pytest.importorskip("torch")
    dev_t = torch.device("cuda", engine.device)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev_t)
    obs = up(np.linspace(300.0, 2000.0, 65))
    valid = torch.full((len(SHIFTS) * 65,), 9, dtype=torch.int8, device=dev_t)
    dm, dt = up(mass), up(thr)
    dmods = up(case.A[sl]) if per_query else None  # (-1: no budget, as on the host path)
    torch.cuda.synchronize()  # the engine queues on its own stream
    res = dev.step_device(obs.data_ptr(), 65, SHIFTS, valid.data_ptr(), dm.data_ptr(), dt.data_ptr(), len(mass),
                          R.TOL, R.PREC, 0 if per_query else int(case.A), d_mods=None if dmods is None else dmods.data_ptr(),
                          with_memo=with_memo, cap=cap)
    res.fetch_device()
    engine.synchronize()
    return res


def check(case, res, mode, with_memo, cap=False, sl=slice(None)):
    want = tuple(a[sl] for a in case.answers(with_memo))
    base = sl.start or 0
    return _digest.assert_equals_oracle(res, want, lambda i: case.oracle_list(base + i, with_memo), _native,
                                        f"{case.name} {mode} memo={with_memo}", check_overflow=cap)


@pytest.mark.parametrize("with_memo", (True, False), ids=("memo", "nomemo"))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("table", tuple(R.tables()))
def test_threshold_windows(engine, device_tables, table, mode, with_memo):
    """Windows whose hi (and whose lo) is T-2 .. T+1 for each threshold T of
    the table, with the call's budget a scalar and (last case) per query."""
    cases = [c for c in R.threshold_cases() if c.table.name == table]
    assert len(cases) >= 3
    for case in cases:
        res = run(engine, device_tables, case, mode, with_memo)
        check(case, res, mode, with_memo)
        res.close()


def _route_counter(case, mode, with_memo):
    """The sst_result_stats counter a group's queries must show up in: its
    route on a table with the pair list; without one (uploaded) pair windows
    go to the shallow path; the exact class runs without the memo as no-memo."""
    route = case.route
    if route == R.PAIR and mode == "uploaded":
        route = R.SHALLOW
    if route == R.EXACT and not with_memo:
        route = R.NOMEMO
    return route


@pytest.mark.parametrize("with_memo", (True, False), ids=("memo", "nomemo"))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("group", [c.name for c in R.route_cases()])
def test_route_groups(engine, device_tables, group, mode, with_memo):
    case = next(c for c in R.route_cases() if c.name == group)
    res = run(engine, device_tables, case, mode, with_memo)
    stats = res.stats()
    print(f"route stats {group} {mode} memo={with_memo} n={case.n} some={case.n_some(with_memo)}: "
          f"{[int(x) for x in stats]}")
    check(case, res, mode, with_memo)
    res.close()
    if case.route is not None:
        assert int(stats[_route_counter(case, mode, with_memo)]) >= case.n_some(with_memo), (group, mode, stats)
    if mode == "uploaded":
        assert int(stats[R.PAIR]) == 0, stats


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("group", [c.name for c in R.route_cases() if c.route is not None])
def test_route_groups_overflow(engine, device_tables, group, mode):
    """cap_per_query of 1: queries with more candidates report OVERFLOW with
    the exact count, the others their list."""
    case = next(c for c in R.route_cases() if c.name == group)
    res = run(engine, device_tables, case, mode, True, cap=1)
    n_over = int((case.answers(True)[1] > 1).sum())
    assert (res.status == _native.SST_OVERFLOW).sum() == n_over
    check(case, res, mode, True, cap=1)
    res.close()
    if not group.startswith("canon"):
        assert n_over >= 5, group  # (the canonical table's windows hold one candidate)


@pytest.mark.parametrize("n", ("fit", "over", 130))
def test_rerun_after_region_overflow(engine, device_tables, n):
    """A first pass whose payload outgrows its regions is run again with
    larger ones (settle(): grow_for_retry): a re-run answers nothing from the
    fused scan, so the result reports no pair-path part, while a batch of the
    same n with narrow windows does.  n: the smallest number of the wide
    windows that the first pass's sizing cannot hold, three fewer (the fused
    scan answers them), and all of them (three tiles).  Every query equals the
    oracle either way."""
    torch = pytest.importorskip("torch")
    wide, narrow = R.rerun_case()
    n_fit, n_over = R.rerun_sizes()
    rerun = n != "fit"
    n = {"fit": n_fit, "over": n_over}.get(n, n)
    dev = device_tables["full_L20"]["explain"]
    dev_t = torch.device("cuda", engine.device)
    n_pair = {}
    for case in (narrow, wide):
        dm, dt = (torch.from_numpy(np.ascontiguousarray(x[:n])).to(dev_t) for x in (case.mass, case.thr))
        torch.cuda.synchronize()
        res = dev.explain_device(dm.data_ptr(), dt.data_ptr(), n, R.TOL, R.PREC, int(case.A))
        res.settle()
        n_pair[case.name] = res.pair_hits_device()[1]
        res.fetch_device()
        engine.synchronize()
        print(f"rerun {case.name} n={n}: pair hits {n_pair[case.name]}, stats {[int(x) for x in res.stats()]}")
        check(case, res, "explain_device", True, sl=slice(0, n))
        res.close()
    assert n_pair["rerun:narrow"] == n  # every narrow window has candidates (test_route_cases.py)
    assert n_pair["rerun:wide"] == (0 if rerun else n)
