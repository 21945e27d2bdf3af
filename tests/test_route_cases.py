"""CPU companion of test_gpu_routes.py: from the oracle alone, no case of
_route_cases.py is vacuous.  At each routing threshold the lists on its two
sides differ in the way the threshold implies, and every route group has
enough queries with candidates."""
import numpy as np
import pytest

import _route_cases as R


def _threshold_singles():
    """(table, what, T, A) of every threshold of every table."""
    return [(t, what, T, A) for t in R.tables().values() for what, T, A in R.thresholds(t)]


def _list(t, v, A, with_memo):
    """The oracle's list of the one-mass window [v, v]."""
    return R.Case("single", t, [v], [v], A, "threshold").oracle_list(0, with_memo)


def test_thresholds_are_the_engines():
    """The values the cases sit on: 3 and 4 w_min, (A + 1) w_min_mod and
    fast_limit_B + 1 = (cap + 1) w_min_mod of the three budget tables."""
    t = R.tables()
    assert [t[k].w_min for k in t] == [305042] * 5 and t["canon"].w_min_mod is None
    assert [(t[k].A, t[k].w_min_mod, t[k].fast_limit_B + 1) for k in ("full_L2", "full_L4", "full_L20", "small_L20")] == [
        (1, 308042, 2 * 308042), (2, 308042, 3 * 308042), (10, 308042, 11 * 308042), (10, 308042, 11 * 308042)]
    names = {k: [w for w, _, _ in R.thresholds(t[k])] for k in t}
    assert names["canon"] == ["3w_min", "4w_min"]
    assert names["full_L2"] == ["3w_min", "4w_min", "A0", "A1", "A2", "fast_limit_B+1"]
    assert names["full_L4"] == names["full_L2"]
    # 11 w_min_mod = 3.39 M: the full alphabet's lists there cannot be enumerated; the
    # five-row table's can (there the windows below the threshold are deep ones)
    assert names["full_L20"] == ["3w_min", "4w_min", "A0", "A1", "A2"]
    assert names["small_L20"] == ["3w_min", "4w_min", "A0", "A1", "A2", "A10", "fast_limit_B+1"]
    assert 11 * 308042 > 4 * 305042


@pytest.mark.parametrize("with_memo", (True, False))
def test_lists_differ_across_each_threshold(with_memo):
    n = 0
    for t, what, T, A in _threshold_singles():
        below, at = _list(t, T - 1, A, with_memo), _list(t, T, A, with_memo)
        if what in ("3w_min", "4w_min"):  # the first candidate of k rows: k times the lightest row
            k = int(what[0])
            assert (1,) * k in at, (t.name, what)
            assert all(len(s) < k for s in below) and all(len(s) <= k for s in at), (t.name, what)
            assert all(len(s) < k for s in _list(t, T - 2, A, with_memo)), (t.name, what)
        else:  # the first candidate a budget excludes: (A + 1) or (cap + 1) times the lightest modification
            r = t.rows.index(t.w_min_mod)
            k = T // t.w_min_mod
            assert k * t.w_min_mod == T and (k == A + 1 or (A == R.INF and k == t.caps[r] + 1)), (t.name, what)
            assert (r,) * k not in at, (t.name, what)
            free = R.unbudgeted(t)  # with no budget and caps of 20 the candidate is there
            assert (r,) * k in _list(free, T, R.INF, with_memo), (t.name, what)
            # and it is the budget that excludes it: everything below is within the budgets
            assert _list(t, T - 1, A, with_memo) == _list(free, T - 1, R.INF, with_memo), (t.name, what)
        n += 1
    assert n == 2 + 6 + 6 + 5 + 7


def test_threshold_cases_cover_both_sides():
    """Every threshold case has windows ending (and starting) at T-2 .. T+1 at
    three widths, its inputs quantise to them, and answers on both sides."""
    cases = R.threshold_cases()
    assert len(cases) == 2 + 6 + 6 + 5 + 7 + 5
    for c in cases:
        ths = R.thresholds(c.table)
        for k in np.unique(c.thresholds):
            T = ths[k][1]
            q = c.thresholds == k
            for d in (-2, -1, 0, 1):
                assert {int(x) for x in (c.hi - c.lo)[q & (c.hi == T + d)]} >= {0, 2, 8}, (c.name, T, d)
                assert {int(x) for x in (c.hi - c.lo)[q & (c.lo == T + d)]} >= {0, 2, 8}, (c.name, T, d)
        assert np.array_equal(np.rint(c.mass / R.PREC) - np.ceil(c.thr / R.PREC), c.lo), c.name
        assert np.array_equal(np.rint(c.mass / R.PREC) + np.ceil(c.thr / R.PREC), c.hi), c.name
        st = c.answers()[0]
        assert (st >= 0).all(), c.name
    # the per-query-budget cases hold every budget of their table's thresholds
    for c in cases:
        if c.name.endswith("per_query_budgets"):
            assert set(np.unique(c.A)) == {A for _, _, A in R.thresholds(c.table)}, c.name


def test_route_groups_are_not_vacuous():
    groups = {c.name: c for c in R.route_cases()}
    assert set(groups) == {f"full_L20:{g}" for g in ("pair", "shallow", "deep", "exact_A1", "exact_A2", "no_roots",
                                                     "zero")} | {
        f"canon:{g}" for g in ("pair", "shallow", "deep", "no_roots", "zero")}
    for name, c in groups.items():
        t, grp = c.table, name.split(":")[1]
        for memo in (True, False):
            st, cnt, nb, _ = c.answers(memo)
            assert (st >= 0).all() and (nb >= 0).all(), name
            if c.route is not None:  # at least half of a route group's queries have candidates
                assert c.n >= 40 and 2 * c.n_some(memo) >= c.n, (name, memo, c.n_some(memo), c.n)
        never = np.ones(c.n, bool) if t.w_min_mod is None else (
            (c.hi <= t.fast_limit_B) & ((c.A == R.INF) | (c.hi < (c.A + 1) * t.w_min_mod)))
        if grp == "pair":
            assert (never & (c.hi < 3 * t.w_min)).all()
        elif grp in ("shallow", "no_roots"):
            assert (never & (c.hi >= 3 * t.w_min) & (c.hi < 4 * t.w_min)).all()
            if grp == "shallow":  # three-row sums answer them
                assert sum(any(len(s) == 3 for s in c.oracle_list(i)) for i in range(c.n)) >= c.n // 2
            else:
                assert c.n == 64 and (c.answers()[0] == 0).all()
        elif grp == "deep":
            assert (never & (c.hi >= 4 * t.w_min)).all()
            assert sum(any(len(s) >= 5 for s in c.oracle_list(i)) for i in range(c.n)) >= c.n // 2
            if t.name == "canon":  # up to eight rows
                assert max(len(s) for i in range(c.n) for s in c.oracle_list(i)) == 8
        elif grp.startswith("exact"):
            assert not never.any()
            # budgets bind: with no budget most windows hold more candidates
            free = R.Case("free", t, c.lo, c.hi, R.INF, "route").answers()[1]
            assert ((free > c.answers()[1]).sum() >= c.n // 2), name
        elif grp == "zero":
            st, cnt, _, _ = c.answers()
            assert (c.lo <= 0).all() and (st == 1).all() and (cnt == 0).sum() >= 2 and (cnt > 0).sum() >= 4
    # the memo changes some of the exact groups' lists (the reference's memo
    # ignores the budgets left): both settings are worth running
    for g in ("exact_A1", "exact_A2"):
        c = groups[f"full_L20:{g}"]
        assert (c.answers(True)[3] != c.answers(False)[3]).sum() >= 5, g


def test_rerun_case_outgrows_a_region():
    """The wide windows' lists pass what a first pass holds at n_over queries
    and not at n_over - 1; n_fit queries fit with the engine's padding; the
    narrow windows all have candidates, a few bytes each."""
    wide, narrow = R.rerun_case()
    assert wide.n == narrow.n == 130 and (wide.hi < 3 * wide.table.w_min).all()
    nb = wide.answers()[2]
    n_fit, n_over = R.rerun_sizes()
    assert 1 <= n_fit < n_over <= 16
    assert nb[:n_over].sum() > R.FIRST_PASS_PAYLOAD >= nb[:n_over - 1].sum()
    assert (nb[:n_fit] + 2 + 16).sum() < R.FIRST_PASS_PAYLOAD
    assert narrow.answers()[2].max() < 64 and narrow.n_some() == narrow.n
