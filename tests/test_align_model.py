"""CPU tests of the alignment certificate's host model (alignment.align_host):
against the definition taken literally (tests/_align_cases.py: _set_x's loops
replayed, itertools.product over the position sets), the capacity rule, and
soundness against the full program with the modification caps restored."""
import itertools
import math

import numpy as np
import pytest

import _align_cases as AC
from spectrseqtools_amd import alignment

ALPHABETS = [[0, 3, 5], [0, 2, 9, 11], [0, 5, 6], [0, 4, 13, 31, 37], [0, 305, 306, 319, 320, 329, 345],
             [0, 7, 7, 9, 16, 23, 1]]  # (the last: equal masses in two rows, and 7 + 9 == 16)
TOL, PREC = 0.02, 0.5  # W = ceil(0.04 obs): 0 .. 3 for the cases' observed masses


def run_host(specs, row_mass, capacity=alignment.ALIGN_CAPACITY, tol=TOL, prec=PREC):
    return alignment.align_host(AC.make_outcome(specs, row_mass), tol, prec, capacity)


@pytest.mark.parametrize("k", range(len(ALPHABETS)))
def test_host_against_brute_force(k):
    """60 random spectra per alphabet (L 1 .. 6, alphabets of <= 6 rows,
    position sets of <= 3 rows): every output equals the brute force's.  With
    these limits no S has more than 3^6 = 729 sums, asserted from the brute
    force's own sets, so nothing may be OPEN."""
    row_mass = ALPHABETS[k]
    specs = AC.random_case(100 + k, row_mass, TOL, PREC, 60)
    st, al, nf, fi, biggest = AC.brute(specs, row_mass, TOL, PREC, alignment.ALIGN_CAPACITY)
    assert biggest <= 729 < alignment.ALIGN_CAPACITY
    got = run_host(specs, row_mass)
    AC.assert_equal(got, (st, al, nf, fi), row_mass)
    assert not (got.status == AC.OPEN).any()
    assert np.array_equal(got.frag_off, AC.make_outcome(specs, row_mass).frag_off)


def test_cases_cover_the_definition():
    """The random cases hold what the comparison is meant to exercise."""
    seen = {s: 0 for s in (AC.NONE, AC.FIT, AC.INFEASIBLE, AC.SKIPPED)}
    classes, empty_fit, mn_gt_mx, empty_mask = set(), 0, 0, 0
    for k, row_mass in enumerate(ALPHABETS):
        specs = AC.random_case(100 + k, row_mass, TOL, PREC, 60)
        st, _, nf, fi, _ = AC.brute(specs, row_mass, TOL, PREC, alignment.ALIGN_CAPACITY)
        for s in seen:
            seen[s] += int((st == s).sum())
        empty_fit += int((fi == 0xFFFF).sum())
        for sp in specs:
            empty_mask += sum(p == (0, 0) for p in sp["pos"])
            for code, _, _, mn, mx in sp["frags"]:
                classes.add((code >> 2) & 3)
                mn_gt_mx += mn > mx
    assert all(v >= 20 for v in seen.values()), seen
    assert classes == {0, 1, 2, 3} and empty_fit >= 5 and mn_gt_mx >= 50 and empty_mask >= 20


def test_empty_interval_and_default_spectrum():
    row_mass = [0, 3, 5]
    specs = [{"default": True},
             {"L": 2, "pos": [AC.mask([1]), AC.mask([2])], "alpha": AC.mask([1, 2]),
              "frags": [(AC.code_of(False, False), 0.4, 10.0, 0, 0),    # target 1 (0.8 -> 1), W 1: the empty interval, only
                        (AC.code_of(False, False), 1.5, 0.0, 0, 0),     # target 3, W 0: [0, 0]
                        (AC.code_of(True, True), 4.0, 0.0, 0, 0),       # target 8, W 0: [0, 1]
                        (AC.code_of(True, True), 4.5, 0.0, 0, 0)]}]     # target 9: no fit
    got = run_host(specs, row_mass)
    assert got.status.tolist() == [AC.FIT, AC.FIT, AC.FIT, AC.NONE]
    assert got.first.tolist() == [0xFFFF, 0x0000, 0x0001, 0xFFFE]
    assert got.n_fit.tolist() == [1, 1, 1, 0] and got.alignable.tolist() == [1, 1, 1, 0]
    assert len(got) == 2 and got.frag_off.tolist() == [0, 0, 4]


@pytest.mark.parametrize("capacity", [1, 2, 8])
def test_capacity_rule(capacity):
    """A small capacity gives OPEN exactly where the brute force's |S(l, r)|
    exceeds it (the brute force applies the rule to its own sets)."""
    n_open = 0
    for k, row_mass in enumerate(ALPHABETS):
        specs = AC.random_case(300 + k, row_mass, TOL, PREC, 40)
        st, al, nf, fi, biggest = AC.brute(specs, row_mass, TOL, PREC, capacity)
        AC.assert_equal(run_host(specs, row_mass, capacity), (st, al, nf, fi), (capacity, row_mass))
        n_open += int((st == AC.OPEN).sum())
    assert n_open >= 20


def test_take_and_concat():
    row_mass = ALPHABETS[1]
    specs = AC.random_case(7, row_mass, TOL, PREC, 9) + [{"default": True}]
    whole = run_host(specs, row_mass)
    parts = [run_host(specs[:4], row_mass), run_host(specs[4:], row_mass)]
    assert alignment.AlignOutcome.concat(parts).equals(whole)
    idx = [9, 3, 0, 7, 3]
    want = run_host([specs[i] for i in idx], row_mass)
    assert whole.take(idx).equals(want)
    assert abs(sum(whole.shares().values()) - 1.0) < 1e-12


def test_soundness_with_the_caps_restored():
    """Tiny instances (L <= 4, <= 4 rows): every y over all positions under the
    universal and the per-row caps (ceil(rate * L), linear_program.py:180-196)
    and every admissible x, the objective |su - sum of mass * precision| in
    floats as the reference computes it.  alignable == 0 implies the minimum
    exceeds tolerance * obs, or that nothing is feasible."""
    rng = np.random.default_rng(5)
    checked = dropped = 0
    for trial in range(150):
        row_mass = [0] + sorted(rng.choice(np.arange(3, 40), size=int(rng.integers(1, 5)), replace=False).tolist())
        n_rows = len(row_mass)
        is_mod = [False] + [bool(rng.random() < 0.5) for _ in row_mass[1:]]
        rate = [0.0] + [float(rng.choice([0.1, 0.34, 0.5, 1.0])) for _ in row_mass[1:]]
        universal = float(rng.choice([0.0, 0.25, 0.5, 1.0]))
        spec = AC.random_spectrum(rng, row_mass, TOL, PREC, max_len=4, max_alpha=4, max_set=3)
        L = spec["L"]
        got = run_host([spec], row_mass)
        sets = [[r for r in AC.rows_of(spec["alpha"] if not (p[0] | p[1]) else
                                       (p[0] & spec["alpha"][0], p[1] & spec["alpha"][1]), n_rows) if r]
                for p in spec["pos"]]
        ys = [y for y in itertools.product(*sets)
              if sum(is_mod[r] for r in y) <= math.ceil(universal * L)
              and all(y.count(r) <= math.ceil(rate[r] * L) for r in set(y))]
        for j, (code, su, obs, mn, mx) in enumerate(spec["frags"]):
            if got.alignable[j] or got.status[j] == AC.SKIPPED:
                continue
            dropped += 1
            best = math.inf
            for y in ys:
                for l, r in AC.admissible_intervals(code, mn, mx, L):
                    inside = range(l, r + 1) if l != 0xFF else ()
                    best = min(best, abs(su - sum(row_mass[y[i]] * PREC for i in inside)))
            assert best > TOL * obs, (trial, j, best, TOL * obs, spec)
            checked += bool(ys)
    assert dropped >= 100 and checked >= 50
