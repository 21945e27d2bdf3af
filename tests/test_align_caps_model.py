"""CPU tests of the alignment certificate's host model under the universal
modification cap (alignment.align_host(caps=...), alignment.lp_caps): against
the definition taken literally (tests/_align_caps_cases.py: every y over all
positions within the cap), the split under caps against a brute force over
every cut and against its mirror image, the invariants that tie caps mode to
the uncapped certificate, and soundness against the full program with the
universal and the per-row caps restored."""
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
from spectrseqtools_amd import alignment

ALPHABETS = [[0, 3, 5], [0, 2, 9, 11], [0, 5, 6], [0, 4, 13, 31, 37], [0, 305, 306, 319, 320, 329, 345],
             [0, 7, 7, 9, 16, 23, 1]]  # (the last: equal masses in two rows, and 7 + 9 == 16)
TOL, PREC = 0.02, 0.5
FIELDS = ("status", "alignable", "n_fit", "first")
PER_ALPHABET = 70  # 420 spectra over the six alphabets


def cases():
    return [(rm, CC.random_caps_case(700 + k, rm, TOL, PREC, PER_ALPHABET)) for k, rm in enumerate(ALPHABETS)]


def host(specs, row_mass, capacity, caps=True, split=False):
    o = AC.make_outcome(specs, row_mass)
    return alignment.align_host(o, TOL, PREC, capacity, split=split,
                                caps=CC.caps_of(specs, len(row_mass)) if caps else None)


@pytest.mark.parametrize("capacity", [1024, 8, 4])
def test_host_against_brute_force_under_the_cap(capacity):
    """420 random spectra (L <= 6, sets of <= 3 rows), random row_mod, mod_cap =
    ceil(rate * L) for rate in {0, 0.1, 0.25, 0.5}: all four outputs equal the
    brute force's.  The cap must move something (floors from the issue)."""
    moved = {"fit_none": 0, "open_decided": 0, "infeasible": 0}
    for rm, specs in cases():
        got = host(specs, rm, capacity)
        AC.assert_equal(got, CC.brute_caps(specs, rm, TOL, PREC, capacity), (capacity, rm))
        plain = host(specs, rm, capacity, caps=False)
        moved["fit_none"] += int(((plain.status == AC.FIT) & (got.status == AC.NONE)).sum())
        moved["open_decided"] += int(((plain.status == AC.OPEN) & np.isin(got.status, (AC.FIT, AC.NONE))).sum())
        moved["infeasible"] += int(((plain.status != AC.INFEASIBLE) & (got.status == AC.INFEASIBLE)).sum())
    print("capacity", capacity, moved, flush=True)
    assert moved["infeasible"] >= 100, moved
    if capacity == 1024:
        assert moved["fit_none"] >= 30, moved
    if capacity == 4:
        assert moved["open_decided"] >= 50, moved


@pytest.mark.parametrize("capacity", [8, 4])
def test_split_under_caps_against_every_cut_and_the_mirror_image(capacity):
    """The greedy cut of align_host(split=True, caps=...) equals the brute force
    that tries every m on the capped sets; the mirrored spectrum (positions
    reversed, START and END swapped) gives the same status and n_fit."""
    n_open = n_decided = 0
    for rm, specs in cases():
        got = host(specs, rm, capacity, split=True)
        base = host(specs, rm, capacity)
        AC.assert_equal(got, CC.brute_caps(specs, rm, TOL, PREC, capacity, split=True), (capacity, rm))
        keep = base.status != AC.OPEN
        assert all(np.array_equal(getattr(got, k)[keep], getattr(base, k)[keep]) for k in FIELDS)
        n_open += int((~keep).sum())
        n_decided += int((~keep & (got.status != AC.OPEN)).sum())
        mir = host([CC.mirrored(s) for s in specs], rm, capacity, split=True)
        assert np.array_equal(mir.status, got.status) and np.array_equal(mir.n_fit, got.n_fit)
    assert n_open >= 50 and n_decided >= 20, (n_open, n_decided)


def test_invariants():
    """mod_cap >= L or row_mod == 0 reproduces the uncapped outcome bit for
    bit; the cap never makes a fragment alignable; an uncapped NONE stays NONE."""
    for capacity in (1024, 4):
        for rm, specs in cases():
            o = AC.make_outcome(specs, rm)
            row_mod, mod_cap = CC.caps_of(specs, len(rm))
            for split in (False, True):
                plain = alignment.align_host(o, TOL, PREC, capacity, split=split)
                loose = alignment.align_host(o, TOL, PREC, capacity, split=split, caps=(row_mod, o.seq_len))
                zero = alignment.align_host(o, TOL, PREC, capacity, split=split,
                                            caps=(np.zeros_like(row_mod), np.zeros_like(mod_cap)))
                assert plain.equals(loose) and plain.equals(zero)
                got = alignment.align_host(o, TOL, PREC, capacity, split=split, caps=(row_mod, mod_cap))
                assert (got.alignable <= plain.alignable).all()
                assert np.isin(got.status[plain.status == AC.NONE], (AC.NONE, AC.INFEASIBLE)).all()
                # an interval that is closed uncapped is closed capped: nothing newly OPEN
                assert not ((got.status == AC.OPEN) & ~np.isin(plain.status, (AC.OPEN, AC.FIT))).any()


def test_soundness_with_every_cap_restored():
    """Tiny instances: every y over all positions under the universal and the
    per-row caps (ceil(rate * L), linear_program.py:180-196) and every
    admissible x, the objective in floats as the reference computes it.
    alignable == 0 under caps (base and split) implies the minimum exceeds
    tolerance * obs, or that nothing is feasible."""
    rng = np.random.default_rng(5)
    checked = dropped = by_cap = 0
    for trial in range(260):
        row_mass = [0] + sorted(rng.choice(np.arange(3, 40), size=int(rng.integers(1, 5)), replace=False).tolist())
        n_rows = len(row_mass)
        is_mod = [False] + [bool(rng.random() < 0.5) for _ in row_mass[1:]]
        rate = [0.0] + [float(rng.choice([0.1, 0.34, 0.5, 1.0])) for _ in row_mass[1:]]
        universal = float(rng.choice([0.0, 0.1, 0.25, 0.5, 1.0]))
        spec = AC.random_spectrum(rng, row_mass, TOL, PREC, max_len=4, max_alpha=4, max_set=3)
        L = spec["L"]
        o = AC.make_outcome([spec], row_mass)
        caps = (np.array(is_mod, dtype=np.uint8), np.array([math.ceil(universal * L)], dtype=np.int32))
        capacity = int(rng.choice([1024, 4, 2]))
        plain = alignment.align_host(o, TOL, PREC, capacity, split=True)
        got = alignment.align_host(o, TOL, PREC, capacity, split=True, caps=caps)
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
            by_cap += int(plain.alignable[j])
            best = math.inf
            for y in ys:
                for l, r in AC.admissible_intervals(code, mn, mx, L):
                    inside = range(l, r + 1) if l != 0xFF else ()
                    best = min(best, abs(su - sum(row_mass[y[i]] * PREC for i in inside)))
            assert best > TOL * obs, (trial, j, best, TOL * obs, spec)
            checked += bool(ys)
    assert dropped >= 100 and checked >= 50 and by_cap >= 20, (dropped, checked, by_cap)


def test_the_minimum_mass_row_may_be_the_modified_one():
    """Positions {m, c} with w_m < w_c: the smallest sum is the one that pays."""
    row_mass, row_mod = [0, 3, 5], np.array([0, 1, 0], dtype=np.uint8)
    both = AC.mask([1, 2])
    frag = lambda t: (AC.code_of(True, True), t * PREC, 0.0, 0, 0)  # noqa: E731  ([0, L - 1] only, W = 0)
    spec = {"L": 3, "pos": [both] * 3, "alpha": both, "frags": [frag(t) for t in (9, 11, 13, 15)]}
    o = AC.make_outcome([spec], row_mass)
    for cap, want in ((0, [0, 0, 0, 1]), (1, [0, 0, 1, 1]), (2, [0, 1, 1, 1]), (3, [1, 1, 1, 1])):
        got = alignment.align_host(o, TOL, PREC, caps=(row_mod, np.array([cap], dtype=np.int32)))
        assert got.alignable.tolist() == want, cap
        s = dict(spec, row_mod=row_mod, mod_cap=cap)
        AC.assert_equal(got, CC.brute_caps([s], row_mass, TOL, PREC, 1024), cap)


def test_lp_caps():
    """row_mod follows the row's FIRST name (linear_program.py:186 tests the
    name the y variable carries), not "any name"; mod_cap = ceil(rate * L)."""
    names = [[""], ["A", "m6A"], ["m1A", "A"], ["G"], ["m7G"]]
    any_name = [any(n and n not in ("A", "C", "G", "U") for n in ns) for ns in names]
    outcome = SimpleNamespace(row_names=[ns[0] for ns in names], seq_len=np.array([0, 1, 7, 10, 20, 253]))
    for rate, want in ((0.05, [0, 1, 1, 1, 1, 13]), (0.1, [0, 1, 1, 1, 2, 26]), (0.5, [0, 1, 4, 5, 10, 127]),
                       (0.0, [0] * 6), (1.0, [0, 1, 7, 10, 20, 253])):
        dp = SimpleNamespace(seq=SimpleNamespace(modification_rate=rate))
        row_mod, mod_cap = alignment.lp_caps(dp, outcome)
        assert row_mod.dtype == np.uint8 and mod_cap.dtype == np.int32
        assert row_mod.tolist() == [0, 0, 1, 0, 1] and any_name[1] and not row_mod[1]
        assert mod_cap.tolist() == want == [int(np.ceil(rate * L)) for L in outcome.seq_len]
    # 0.07 * 100 is 7.000000000000001 in f64: the reference's ceil gives 8, and so does lp_caps
    dp = SimpleNamespace(seq=SimpleNamespace(modification_rate=0.07))
    o100 = SimpleNamespace(row_names=outcome.row_names, seq_len=np.array([100]))
    assert alignment.lp_caps(dp, o100)[1].tolist() == [int(np.ceil(0.07 * 100))]
    with pytest.raises(ValueError):
        alignment.align_host(AC.make_outcome([], [0, 3]), TOL, PREC, caps=(np.zeros(3, np.uint8), np.zeros(0, np.int32)))
