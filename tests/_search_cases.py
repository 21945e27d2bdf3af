"""The builders and comparisons of the bounded search's tests (final_program.
final_search_host, sst_final_search_device), shared by tests/
test_final_search_model.py (CPU) and tests/test_gpu_final_search.py.

Built on tests/_final_cases.py and tests/_robust_cases.py: a spectrum's "use"
holds 0 / 1 / 2 per fragment.  TEST INFRASTRUCTURE."""
import numpy as np

import _align_caps_cases as CC
import _align_cases as AC
import _final_cases as FC
import _robust_cases as RB

SEARCH_FIELDS = ("mode", "rounds", "nodes")


def host(specs, row_mass, row_cap, precision, max_combos=0, **kw):
    """final_search_host of a case: (FinalOutcome, RobustOutcome, SearchOutcome)."""
    from spectrseqtools_amd import final_program as FP

    o = AC.make_outcome(specs, row_mass)
    return FP.final_search_host(o, precision, CC.caps_of(specs, len(row_mass)), row_cap, use=RB.use3_array(specs),
                                max_combos=max_combos, **kw)


def truncated(pair, H, solved_only=True):
    """final_robust_host's fourteen arrays with gap and rgap replaced by min(., H + 1) where SOLVED."""
    fo, ro = pair
    want = [np.array(getattr(fo, k)) for k in FC.FIELDS] + [np.array(getattr(ro, k)) for k in RB.ROBUST_FIELDS]
    ok = fo.status == FC.SOLVED
    for k in (FC.FIELDS.index("gap"), 9 + RB.ROBUST_FIELDS.index("rgap")):
        want[k][ok] = np.minimum(want[k][ok], np.uint64(H + 1))
    return tuple(want)


def assert_equal17(got, want, what=""):
    """(FinalOutcome, RobustOutcome, SearchOutcome) against another such triple."""
    RB.assert_equal14(got[:2], want[:2], what)
    assert got[2].horizon == want[2].horizon, what
    for k in SEARCH_FIELDS:
        g, w = getattr(got[2], k), getattr(want[2], k)
        assert len(g) == len(w), (what, k)
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, k, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def ladder_spec(rm, precision, rng, L=24, n_free=20, rows_per=4, noise=3, spread=1, n_optional=0):
    """A planted ladder: L positions, n_free of them free over rows_per rows,
    a planted y, and per position a START pin of its prefix and an END pin of
    its suffix with +-noise units of noise and a range of ends of +-spread
    positions (END fragments: mn >= mx, final_program._ends).  n_optional
    fragments, every eighth one from the fourth, are optional.  Returns (spec, y)."""
    rows = list(range(1, len(rm)))
    free = sorted(rng.choice(L, size=n_free, replace=False).tolist())
    sets = [[rows[(3 * i) % len(rows)]] for i in range(L)]
    for p in free:
        sets[p] = sorted(rng.choice(rows, size=rows_per, replace=False).tolist())
    y = [int(rng.choice(s)) for s in sets]
    pre = np.concatenate([[0], np.cumsum([int(rm[r]) for r in y])])
    frags = []
    for p in range(L):
        lo, hi = max(0, p - spread), min(L - 1, p + spread)
        frags.append((FC.START, float(pre[p + 1] + rng.integers(-noise, noise + 1)) * precision, 100.0, lo, hi))
        frags.append((FC.END, float(pre[L] - pre[p] + rng.integers(-noise, noise + 1)) * precision, 100.0, hi, lo))
    use = [2 if j % 8 == 3 and j // 8 < n_optional else 1 for j in range(len(frags))]
    return FC.loose_spec(rm, sets, frags, use=use), y


def literal_objective(spec, rm, precision, y, kinds=(1,)):
    """obj(y) by the literal cost over the fragments whose use is in `kinds`."""
    L = spec["L"]
    use = RB.use3_of(spec)
    total = 0
    for j, (code, su, _, mn, mx) in enumerate(spec["frags"]):
        if use[j] not in kinds:
            continue
        q = FC.qfix(su, precision)
        total += min(abs(q - FC.FIX * sum(int(rm[y[i]]) for i in (range(l, r + 1) if l != 0xFF else ())))
                     for l, r in AC.admissible_intervals(code, mn, mx, L))
    return total


def offset_spec(rm, precision, offset_units, n_free=3):
    """n_free positions over two rows (a, b) and one START_END fragment that
    lies offset_units precision units above the largest reachable total: the
    optimum is offset_units * 65536 and every other objective lies above it by
    multiples of (mass b - mass a) * 65536.  Returns (spec, a, b)."""
    (a, b), = FC.distinct_pairs(rm, 1)
    lo, hi = sorted((a, b), key=lambda r: rm[r])
    top = n_free * int(rm[hi])
    frags = [(FC.START_END, float(top + offset_units) * precision, 100.0, 0, 0)]
    return FC.loose_spec(rm, [sorted([a, b])] * n_free, frags), lo, hi
