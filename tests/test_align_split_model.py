"""CPU tests of the two-list split of the alignment certificate's host model
(alignment.align_host(split=True)): against the brute force of
tests/_align_split_cases.py (the "exists m" definition over itertools.product
sets), the invariants that tie it to the base certificate, independence of
the sweep direction, and take / concat."""
import numpy as np
import pytest

import _align_cases as AC
import _align_split_cases as ASC
from spectrseqtools_amd import alignment

ALPHABETS = [[0, 3, 5], [0, 2, 9, 11], [0, 5, 6], [0, 4, 13, 31, 37], [0, 305, 306, 319, 320, 329, 345],
             [0, 7, 7, 9, 16, 23, 1]]  # (test_align_model.py's)
TOL, PREC = 0.02, 0.5
CAPACITIES = [3, 4, 6]
FIELDS = ("status", "alignable", "n_fit", "first")


def cases():
    return [(row_mass, AC.random_case(300 + k, row_mass, TOL, PREC, 40)) for k, row_mass in enumerate(ALPHABETS)]


def run_host(specs, row_mass, capacity=alignment.ALIGN_CAPACITY, split=True):
    return alignment.align_host(AC.make_outcome(specs, row_mass), TOL, PREC, capacity, split=split)


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_host_against_brute_force(capacity):
    """All four outputs equal the brute force's; the base-OPEN fragments end in
    each of FIT, OPEN and NONE at least 10 times."""
    ends = {AC.FIT: 0, AC.OPEN: 0, AC.NONE: 0}
    for row_mass, specs in cases():
        st, al, nf, fi, base = ASC.brute_split(specs, row_mass, TOL, PREC, capacity)
        AC.assert_equal(run_host(specs, row_mass, capacity), (st, al, nf, fi), (capacity, row_mass))
        for s in ends:
            ends[s] += int(((base == AC.OPEN) & (st == s)).sum())
        assert set(st[base == AC.OPEN].tolist()) <= set(ends)
    print("capacity", capacity, "base-OPEN fragments end FIT / OPEN / NONE:", ends[AC.FIT], ends[AC.OPEN], ends[AC.NONE])
    assert all(v >= 10 for v in ends.values()), ends


@pytest.mark.parametrize("capacity", CAPACITIES + [alignment.ALIGN_CAPACITY])
def test_invariants(capacity):
    """Fragments not OPEN at base keep all four outputs; a fragment the split
    decides has the status an unbounded capacity gives it; alignable never rises."""
    n_decided = 0
    for row_mass, specs in cases():
        base = run_host(specs, row_mass, capacity, split=False)
        got = run_host(specs, row_mass, capacity)
        exact = run_host(specs, row_mass, 10**9, split=False)
        assert np.array_equal(got.frag_off, base.frag_off)
        was_open = base.status == AC.OPEN
        for k in FIELDS:
            assert np.array_equal(getattr(got, k)[~was_open], getattr(base, k)[~was_open]), (capacity, row_mass, k)
        decided = was_open & (got.status != AC.OPEN)
        assert set(got.status[decided].tolist()) <= {AC.FIT, AC.NONE}
        assert np.array_equal(got.status[decided], exact.status[decided]), (capacity, row_mass)
        assert (got.alignable <= base.alignable).all()
        assert not (exact.status == AC.OPEN).any()
        n_decided += int(decided.sum())
    assert n_decided >= 50 or capacity == alignment.ALIGN_CAPACITY  # (nothing is OPEN at the default capacity here)


@pytest.mark.parametrize("capacity", CAPACITIES)
def test_direction_independence(capacity):
    """A mirrored spectrum (positions reversed, START and END swapped, mn / mx
    mapped) gives the same statuses and counts: the greedy cut from the left
    and from the right decide the same intervals."""
    n_open = 0
    for row_mass, specs in cases():
        got = run_host(specs, row_mass, capacity)
        mir = run_host([ASC.mirrored(s) for s in specs], row_mass, capacity)
        assert np.array_equal(got.status, mir.status), (capacity, row_mass)
        assert np.array_equal(got.n_fit, mir.n_fit) and np.array_equal(got.alignable, mir.alignable)
        n_open += int((run_host(specs, row_mass, capacity, split=False).status == AC.OPEN).sum())
    assert n_open >= 50


def test_take_and_concat():
    row_mass = ALPHABETS[1]
    specs = AC.random_case(301, row_mass, TOL, PREC, 9) + [{"default": True}]
    whole = run_host(specs, row_mass, 3)
    assert (whole.status != run_host(specs, row_mass, 3, split=False).status).any()
    parts = [run_host(specs[:4], row_mass, 3), run_host(specs[4:], row_mass, 3)]
    assert alignment.AlignOutcome.concat(parts).equals(whole)
    idx = [9, 3, 0, 7, 3]
    want = run_host([specs[i] for i in idx], row_mass, 3)
    assert whole.take(idx).equals(want)
    assert abs(sum(whole.shares().values()) - 1.0) < 1e-12
