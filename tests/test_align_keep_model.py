"""CPU tests of the alignment certificate's keep mode (alignment.align_host(
keep=...), alignment.lp_row_caps, alignment.lp_decisions): the host model
against the definition taken literally (tests/_align_keep_cases.py), soundness
and completeness against the full program with the universal and the per-row
caps restored (every y and x enumerated), the edges of the inner window and of
the row-free test, and AlignOutcome with and without the new fields."""
import itertools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
from spectrseqtools_amd import alignment

ALPHABETS = [[0, 3, 5], [0, 2, 9, 11], [0, 5, 6], [0, 4, 13, 31, 37], [0, 305, 306, 319, 320, 329, 345],
             [0, 7, 7, 9, 16, 23, 1]]  # (the last: equal masses in two rows, and 7 + 9 == 16)
TOL, PREC = 0.02, 0.5
PER_ALPHABET = 70  # 420 spectra over the six alphabets
BIG = [0, 30011, 41017, 52021, 63029, 74051, 85061]  # masses far above every W of the edge cases


def cases():
    return [(rm,) + KC.random_keep_case(900 + k, rm, TOL, PREC, PER_ALPHABET) for k, rm in enumerate(ALPHABETS)]


def host(specs, row_mass, row_cap, capacity=1024, split=False, tol=TOL, prec=PREC):
    o = AC.make_outcome(specs, row_mass)
    return alignment.align_host(o, tol, prec, capacity, split=split, caps=CC.caps_of(specs, len(row_mass)), keep=row_cap)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("capacity", [1024, 4, 2])
def test_host_against_brute_force(capacity, split):
    """420 random spectra (L <= 6, sets of <= 3 rows), random row_mod, mod_cap
    and per-row rates from {0.1, 0.34, 0.5, 1.0}: all seven arrays equal the
    brute force's; the four base outputs equal the run without keep."""
    kept = free = gated = from_split = 0
    for rm, specs, row_cap in cases():
        got = host(specs, rm, row_cap, capacity, split)
        KC.assert_equal7(got, KC.brute_keep(specs, rm, row_cap, TOL, PREC, capacity, split), (capacity, split, rm))
        o = AC.make_outcome(specs, rm)
        plain = alignment.align_host(o, TOL, PREC, capacity, split=split, caps=CC.caps_of(specs, len(rm)))
        assert plain.keep is None and all(np.array_equal(getattr(got, k), getattr(plain, k)) for k in plain.FRAGMENT_FIELDS)
        assert (got.status[got.keep == 1] == AC.FIT).all()
        loose = host(specs, rm, KC.loose_row_cap(len(rm)), capacity, split)
        assert (got.keep <= loose.keep).all()
        kept += int(got.keep.sum())
        free += int(got.spec_free.sum())
        gated += int(((loose.keep == 1) & (got.keep == 0)).sum())
        if split:
            base = host(specs, rm, row_cap, capacity, False)
            from_split += int(((base.status == AC.OPEN) & (got.keep == 1)).sum())
            same = base.status != AC.OPEN
            assert np.array_equal(got.keep[same], base.keep[same]) and np.array_equal(got.keep_first[same], base.keep_first[same])
    print("capacity", capacity, "split", split, "kept", kept, "row-free spectra", free, "gated", gated, "kept by the split",
          from_split, flush=True)
    # (floors against a vacuous pass only: about half of what these seeds give; the split's keeps have a test of their own)
    assert kept >= 60 and 50 <= free <= 370 and gated >= 45, (kept, free, gated)


def test_split_keeps_from_split_closed_intervals():
    """Capacity 4, positions {a, b, c} x 2 (b modified, mod_cap = 1): [0, 1] has
    five capped sums (open) and splits into two closed halves of three.  START_END
    fragments around a + b (one modified row: within the budget) and around
    2 b (over it): base-OPEN, then kept iff a pair within the budget lies
    within W_in -- against the brute force, with every outcome present."""
    a, b, c = 1, 2, 4  # (no two of the six pair sums within 2 W of each other)
    row_mod = np.array([0, 0, 1] + [0] * (len(BIG) - 3), dtype=np.uint8)
    both = AC.mask([a, b, c])
    wide, exact = 4.4 * PREC / TOL, 4.0 * PREC / TOL  # W = 5, W_in = 3; W = 4, W_in = 3
    frags = [(AC.code_of(True, True), (base + s) * PREC, obs, 0, 0)
             for base in (BIG[a] + BIG[b], 2 * BIG[b], 2 * BIG[a]) for s in range(-6, 7) for obs in (wide, exact)]
    spec = {"L": 2, "pos": [both, both], "alpha": both, "row_mod": row_mod, "mod_cap": 1,
            "frags": sorted(frags, key=lambda f: f[1])}
    specs = [spec, CC.mirrored(spec), dict(spec, mod_cap=2)]
    row_cap = KC.loose_row_cap(len(BIG))
    base = host(specs, BIG, row_cap, 4)
    got = host(specs, BIG, row_cap, 4, split=True)
    KC.assert_equal7(base, KC.brute_keep(specs, BIG, row_cap, TOL, PREC, 4), "base")
    KC.assert_equal7(got, KC.brute_keep(specs, BIG, row_cap, TOL, PREC, 4, split=True), "split")
    nf = len(frags)
    assert np.isin(base.status, (AC.OPEN, AC.NONE)).all() and (base.status == AC.OPEN).sum() >= 3 * (nf - 4)
    assert not base.keep.any() and got.spec_free.tolist() == [1, 1, 1]
    assert np.array_equal(got.keep[:nf], got.keep[nf:2 * nf]) and np.array_equal(got.status[:nf], got.status[nf:2 * nf])
    tight, free_budget = got.keep[:nf], got.keep[2 * nf:]
    band = (got.status[:nf] == AC.FIT) & (tight == 0)            # a pair fits W, none fits W_in
    over = (tight == 0) & (free_budget == 1)                     # fits inside only with both modified rows
    # per base and observed mass: |s| <= 3 inside (7 values); |s| in {4, 5} / {4} in the band
    assert tight.sum() == 2 * 14 and band.sum() == 2 * 6 and over.sum() == 14, (tight.sum(), band.sum(), over.sum())
    assert (got.keep_first[:nf][tight == 1] == 1).all() and (got.keep_first[:nf][tight == 0] == 0xFFFE).all()


def enumerate_program(spec, row_mass, is_mod, rate, universal):
    """Every y over all positions under the universal and the per-row caps
    (ceil(rate * L), linear_program.py:180-196)."""
    L, n_rows = spec["L"], len(row_mass)
    sets = [[r for r in AC.rows_of(spec["alpha"] if not (p[0] | p[1]) else
                                   (p[0] & spec["alpha"][0], p[1] & spec["alpha"][1]), n_rows) if r]
            for p in spec["pos"]]
    return [y for y in itertools.product(*sets)
            if sum(is_mod[r] for r in y) <= math.ceil(universal * L)
            and all(y.count(r) <= math.ceil(rate[r] * L) for r in set(y))]


def tiny_instance(rng):
    row_mass = [0] + sorted(rng.choice(np.arange(3, 40), size=int(rng.integers(1, 5)), replace=False).tolist())
    is_mod = [False] + [bool(rng.random() < 0.5) for _ in row_mass[1:]]
    rate = [0.0] + [float(rng.choice(KC.RATES)) for _ in row_mass[1:]]
    universal = float(rng.choice([0.1, 0.25, 0.5, 1.0]))
    spec = AC.random_spectrum(rng, row_mass, TOL, PREC, max_len=4, max_alpha=4, max_set=3)
    spec["frags"] = [KC.widened(f, rng, TOL, PREC) if rng.random() < 0.5 else f for f in spec["frags"]]
    spec["row_mod"], spec["mod_cap"] = np.array(is_mod, dtype=np.uint8), math.ceil(universal * spec["L"])
    return row_mass, is_mod, rate, universal, spec


def test_soundness_with_every_cap_restored():
    """Tiny instances: every y under the universal and the per-row caps and
    every admissible x, the objective in floats as the reference computes it.
    keep == 1 (base and split, capacities 1024, 4, 2) implies the minimum is <=
    tolerance * obs.  The gate is exercised: fragments whose S_E holds an inner
    fit that no per-row-feasible y reaches exist, and every one has keep == 0."""
    rng = np.random.default_rng(11)
    kept = gated = not_free = 0
    for trial in range(400):
        row_mass, is_mod, rate, universal, spec = tiny_instance(rng)
        L, n_rows = spec["L"], len(row_mass)
        capacity = int(rng.choice([1024, 4, 2]))
        row_cap = KC.row_cap_table(rate)
        got = host([spec], row_mass, row_cap, capacity, split=True)
        loose = host([spec], row_mass, KC.loose_row_cap(n_rows), capacity, split=True)  # S_E alone, no row test
        ys = enumerate_program(spec, row_mass, is_mod, rate, universal)
        not_free += int(got.status[0] not in (AC.INFEASIBLE,) and not got.spec_free[0])
        for j, (code, su, obs, mn, mx) in enumerate(spec["frags"]):
            if not (got.keep[j] or loose.keep[j]):
                continue
            ivs = AC.admissible_intervals(code, mn, mx, L)
            sums = [sum(row_mass[y[i]] for i in (range(l, r + 1) if l != 0xFF else ())) for y in ys for l, r in ivs]
            if got.keep[j]:
                kept += 1
                best = min((abs(su - s * PREC) for s in sums), default=math.inf)
                assert best <= TOL * obs, (trial, j, best, TOL * obs, spec)
            else:  # S_E holds an inner fit; does a y within every cap reach one?
                w_in, target = KC.inner_w(obs, TOL, PREC), round(su / PREC)
                if not any(abs(s - target) <= w_in for s in sums):
                    gated += 1  # the fragments the gate exists for: keep == 0 (this branch)
    print("kept", kept, "gated", gated, "spectra not row-free", not_free, flush=True)
    assert kept >= 150 and gated >= 15 and not_free >= 60, (kept, gated, not_free)


def test_completeness_where_everything_is_closed():
    """Row-free spectra at capacity 1024 (every interval of these tiny spectra
    is closed): keep == 1 iff some y within every cap and some admissible x has
    |s - target| <= W_in; keep_first is the smallest such interval."""
    rng = np.random.default_rng(12)
    n_free = n_keep = n_not = 0
    for trial in range(400):
        row_mass, is_mod, rate, universal, spec = tiny_instance(rng)
        L = spec["L"]
        got = host([spec], row_mass, KC.row_cap_table(rate), 1024)
        if not got.spec_free[0]:
            assert not got.keep.any()
            continue
        n_free += 1
        assert not (got.status == AC.OPEN).any()
        ys = enumerate_program(spec, row_mass, is_mod, rate, universal)
        for j, (code, su, obs, mn, mx) in enumerate(spec["frags"]):
            if got.status[j] == AC.SKIPPED:
                assert not got.keep[j]
                continue
            w_in, target = KC.inner_w(obs, TOL, PREC), round(su / PREC)
            fits = [(l, r) for l, r in AC.admissible_intervals(code, mn, mx, L)
                    if any(abs(sum(row_mass[y[i]] for i in (range(l, r + 1) if l != 0xFF else ())) - target) <= w_in
                           for y in ys)]
            assert bool(got.keep[j]) == bool(fits), (trial, j, spec)
            assert int(got.keep_first[j]) == (min(fits)[0] << 8 | min(fits)[1] if fits else 0xFFFE), (trial, j)
            n_keep += bool(fits)
            n_not += not fits
    assert n_free >= 100 and n_keep >= 150 and n_not >= 150, (n_free, n_keep, n_not)


def test_window_edges():
    """Sums at target +- W_in and +- (W_in + 1), +- W and +- (W + 1); q an exact
    integer (W - W_in == 1) and just above one (2); q < 1, q = 0, q not finite
    and q so large that W and W_in are both clamped."""
    tol, prec = 1e-5, 1e-3  # (q = 0.01 obs up to the rounding of the two f64 operations)
    spec, notes = KC.window_edge_spec(BIG, (1, 2), tol, prec)
    spec["row_mod"], spec["mod_cap"] = np.zeros(len(BIG), np.uint8), 0
    got = host([spec], BIG, KC.loose_row_cap(len(BIG)), tol=tol, prec=prec)
    assert got.spec_free.tolist() == [1]
    seen = set()
    for j, (kind, d, w, w_in) in enumerate(notes):
        if kind == "huge":
            want_fit, want_keep = True, True
        elif kind == "inf":
            want_fit, want_keep = True, False
        else:
            want_fit, want_keep = w >= 0 and abs(d) <= w, w_in >= 0 and abs(d) <= w_in
        assert (got.status[j] == AC.FIT) == want_fit and bool(got.keep[j]) == want_keep, (j, kind, d, w, w_in)
        assert (got.keep_first[j] != 0xFFFE) == want_keep
        seen.add((kind, want_fit, want_keep))
    for kind in ("integer", "above"):
        assert {(kind, True, True), (kind, True, False), (kind, False, False)} <= seen  # inside, in the band, outside
    assert ("below_one", True, False) in seen and ("zero", True, False) in seen and ("nan", False, False) in seen
    assert ("below_one", True, True) not in seen and ("zero", True, True) not in seen
    kinds = KC.observed_masses(tol, prec)
    assert [alignment.inner_window(kinds[k], tol, prec) for k in ("below_one", "zero", "inf", "nan")] == [-1] * 4
    assert alignment.inner_window(kinds["huge"], tol, prec) == 1 << 61 == alignment.quantise(0.0, kinds["huge"], tol, prec)[1]
    for k in ("integer", "above"):
        assert alignment.inner_window(kinds[k], tol, prec) == KC.inner_w(kinds[k], tol, prec) >= 2


def test_row_cap_edges():
    """row_cap == n_r is free and n_r - 1 is not (an unmodified row); row_cap ==
    mod_cap is free and mod_cap - 1 is not (a modified row with n_r > row_cap)."""
    unmod, mod = (1, 2, 3, 4), (5, 6)
    row_mod = np.zeros(len(BIG), np.uint8)
    row_mod[list(mod)] = 1
    specs, want_free = KC.row_edge_specs(BIG, unmod, mod, TOL, PREC)
    for s in specs:
        s["row_mod"] = row_mod
    row_cap = KC.row_edge_caps(len(BIG), unmod, mod)
    got = host(specs, BIG, row_cap)
    assert got.spec_free.tolist() == want_free
    KC.assert_equal7(got, KC.brute_keep(specs, BIG, row_cap, TOL, PREC, 1024), "row edges")
    per = got.keep.reshape(4, 3)
    assert (got.status == AC.FIT).all() and per[[0, 2]].all() and not per[[1, 3]].any()
    loose = host(specs, BIG, KC.loose_row_cap(len(BIG)))
    assert loose.spec_free.tolist() == [1] * 4 and loose.keep.all()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("capacity", [1024, 2])
def test_limit_kinds_against_brute_force(capacity, split):
    """The kinds of input the GPU tests of a workgroup's later spectra and of
    the row-count edges hold the kernels to this model on, here the model
    against the brute force: L == 0 (the empty interval alone; START_END is
    admissible for it, a terminal fragment is SKIPPED); su that is negative or
    at the edge of the final program's fixed-point range, in every class; and a
    65-row table with free positions over rows 63 | 64, modified rows from 64
    on and every alphabet and constrained position with all bits from 65 to
    127 set."""
    import _final_cases as FC

    zero, _, _ = FC.zero_length_specs(BIG, PREC)
    values, _ = FC.su_value_specs(BIG, PREC, values=FC.SU_INSIDE)
    specs = zero + values
    row_cap = KC.loose_row_cap(len(BIG))
    got = host(specs, BIG, row_cap, capacity, split)
    KC.assert_equal7(got, KC.brute_keep(specs, BIG, row_cap, TOL, PREC, capacity, split), ("zero, su", capacity, split))
    first = got.first[:4].tolist()
    assert first[2] == 0xFFFF and got.status[:4].tolist() == [AC.FIT, AC.FIT, AC.FIT, AC.FIT]  # (W = 4 around 0)
    assert got.status[12] == AC.SKIPPED and got.spec_free[:4].tolist() == [1, 1, 1, 1]
    rm, specs, row_cap = FC.row_edge_case(65, PREC, np.random.default_rng(8))
    got = host(specs, rm, row_cap, capacity, split)
    KC.assert_equal7(got, KC.brute_keep(specs, rm, row_cap, TOL, PREC, capacity, split), ("65 rows", capacity, split))
    assert got.spec_free.tolist() == [1, 1, 1, 1, 1, 0, 0, 1] and got.keep.sum() >= 10


def test_lp_row_caps():
    """row_cap[L * n_rows + r] = int(np.ceil(rate * L)) with the rate of the row
    that holds row r's FIRST name; a name in two rows is a ValueError."""
    names = [[""], ["A", "m6A"], ["m1A", "Am"], ["G"], ["m7G"]]
    rates = [0.0, 1.0, 0.07, 0.34, 0.5]
    masses = [SimpleNamespace(names=ns, modification_rate=rt) for ns, rt in zip(names, rates)]
    outcome = SimpleNamespace(row_names=[ns[0] for ns in names])
    dp = SimpleNamespace(masses=masses)
    t = alignment.lp_row_caps(dp, outcome)
    assert t.dtype == np.int32 and t.shape == (254 * 5,)
    for L in range(254):
        for r in range(5):
            assert t[L * 5 + r] == int(np.ceil(rates[r] * L)), (L, r)
    assert t[100 * 5 + 2] == 8  # 0.07 * 100 is 7.000000000000001 in f64: the reference's ceil gives 8
    # the rate follows the row that holds the first name, wherever that row is; a name no row holds is unconstrained
    swapped = SimpleNamespace(masses=[masses[0], masses[2], masses[1], masses[3]])
    t2 = alignment.lp_row_caps(swapped, outcome)
    assert t2[10 * 5 + 1] == 10 and t2[10 * 5 + 2] == 1 and t2[10 * 5 + 4] == 10
    twice = SimpleNamespace(masses=masses + [SimpleNamespace(names=["Gm", "A"], modification_rate=0.1)])
    with pytest.raises(ValueError, match="two rows"):
        alignment.lp_row_caps(twice, outcome)
    o = AC.make_outcome([], [0, 3])
    with pytest.raises(ValueError):
        alignment.align_host(o, TOL, PREC, keep=KC.loose_row_cap(2))  # keep requires caps
    with pytest.raises(ValueError):
        alignment.align_host(o, TOL, PREC, caps=(np.zeros(2, np.uint8), np.zeros(0, np.int32)), keep=np.zeros(7, np.int32))


def test_lp_decisions_and_outcomes_without_keep():
    """lp_decisions: 0 DROP, 1 KEEP, 2 SOLVE.  An AlignOutcome without the new
    fields behaves as before under equals, take and concat; with them they are
    carried."""
    rm, specs, row_cap = cases()[3]
    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    plain = alignment.align_host(o, TOL, PREC, caps=caps)
    kept = alignment.align_host(o, TOL, PREC, caps=caps, keep=row_cap)
    d = alignment.lp_decisions(kept)
    assert d.dtype == np.uint8 and set(d.tolist()) == {0, 1, 2}
    assert np.array_equal(d == 0, kept.alignable == 0) and np.array_equal(d == 1, kept.keep == 1)
    assert np.array_equal(alignment.lp_decisions(plain), np.where(plain.alignable == 0, 0, 2))
    assert (alignment.LP_DROP, alignment.LP_KEEP, alignment.LP_SOLVE) == (0, 1, 2)

    assert plain.keep is None and plain.keep_first is None and plain.spec_free is None
    idx = np.array([5, 0, 17, 5])
    n = np.diff(o.frag_off)
    for al in (plain, kept):
        part = al.take(idx)
        assert part.has_keep == al.has_keep and len(part) == 4 and np.array_equal(np.diff(part.frag_off), n[idx])
        whole = alignment.AlignOutcome.concat([al.take(np.arange(0, 30)), al.take(np.arange(30, len(al)))])
        assert whole.equals(al) and al.equals(whole) and whole.has_keep == al.has_keep
        for k in al.FRAGMENT_FIELDS:
            assert np.array_equal(getattr(part, k)[:n[5]], getattr(al, k)[o.frag_off[5]:o.frag_off[6]])
    part = kept.take(idx)
    assert np.array_equal(part.spec_free, kept.spec_free[idx])
    assert np.array_equal(part.keep[:n[5]], kept.keep[o.frag_off[5]:o.frag_off[6]])
    assert not plain.equals(kept) and not kept.equals(plain)
    other = alignment.align_host(o, TOL, PREC, caps=caps, keep=KC.loose_row_cap(len(rm)))
    assert not kept.equals(other) and kept.take(idx).equals(part)
    with pytest.raises(ValueError):
        alignment.AlignOutcome.concat([plain, kept])
    with pytest.raises(ValueError):
        alignment.AlignOutcome(frag_off=plain.frag_off, status=plain.status, alignable=plain.alignable, n_fit=plain.n_fit,
                               first=plain.first, keep=kept.keep)
