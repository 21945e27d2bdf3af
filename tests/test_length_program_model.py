"""CPU tests of the length program's host model (length_program.py): the
shapes against the fixture recorded from the reference's own _set_x, the model
against the definition taken literally (tests/_length_cases.py), the claim
behind LENGTH_TAKE in exact fractions, length_decisions' branches, the
validation against the mirror's, and the plumbing."""
import ctypes
import gzip
import itertools
import json
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import _length_cases as LC
from spectrseqtools_amd import _native
from spectrseqtools_amd import length_program as LP

ALPHABETS = [[0, 3, 5], [0, 2, 9, 11], [0, 5, 6], [0, 4, 13, 31, 37], [0, 305, 306, 319, 320, 329, 345],
             [0, 7, 7, 9, 16, 23, 1]]  # (tests/_final_cases.py's users' alphabets; the last is not ascending:
#                                          validation reads masses by row order, so its su_mass is drawn freely)
PREC = 0.125  # (an eighth: the small alphabets' masses are then below MAX_VARIANCE and most lengths are valid)
PER_ALPHABET = 60  # 360 spectra over the six alphabets
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "length_program_setx.json.gz")


def cases():
    return [(rm,) + LC.random_case(4100 + k, rm, PREC, PER_ALPHABET) for k, rm in enumerate(ALPHABETS)]


def test_status_constants():
    assert (LP.LEN_INVALID, LP.LEN_RAISES, LP.LEN_NOT_MODELLED, LP.LEN_INFEASIBLE, LP.LEN_NOT_FREE, LP.LEN_TOO_LARGE,
            LP.LEN_SOLVED) == (LC.INVALID, LC.RAISES, LC.NOT_MODELLED, LC.INFEASIBLE, LC.NOT_FREE, LC.TOO_LARGE,
                               LC.SOLVED)
    assert (LP.LENGTH_NONE, LP.LENGTH_JACCARD, LP.LENGTH_TAKE, LP.LENGTH_SOLVE) == (0, 1, 2, 3) and LP.FIX == LC.FIX
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "sst.h")).read()
    for name, value in (("INVALID", 0), ("RAISES", 1), ("NOT_MODELLED", 2), ("INFEASIBLE", 3), ("NOT_FREE", 4),
                        ("TOO_LARGE", 5), ("SOLVED", 6)):
        assert f"#define SST_LEN_{name} {value}\n" in header
    assert "#define SST_K_LENGTH_PROGRAM 30 " in header and _native.K_LENGTH_PROGRAM == 30 < _native.K_COUNT
    assert _native.KERNEL_NAMES[30] == "k_length_program"


def test_shapes_against_the_reference_fixture():
    """Every c in 1..6, raw (min_end, max_end) in [0, 8]^2, three classes: the
    simulated pattern, the RAISES condition, and the closed-form shape (its runs
    against every run that agrees with the recorded pattern) equal what the
    reference's own determine_lp_score / _set_x left."""
    g = json.load(gzip.open(GOLDEN))
    assert g["lengths"] == list(range(1, 7)) and g["ends"] == list(range(9))
    cls_of = {"START": 1, "END": 2, "START_END": 3}
    code_of = {"START": LC.START, "END": LC.END, "START_END": LC.START_END}
    seen = {}
    for name in g["classes"]:
        for ci, c in enumerate(g["lengths"]):
            for a in g["ends"]:
                for b in g["ends"]:
                    rec = g["patterns"][name][ci][a][b]
                    x = LP.setx_pattern(cls_of[name], a, b, c)
                    rule = LP.shape_rule(cls_of[name], a, b, c)
                    what = (name, c, a, b)
                    assert LC.replay_set_x(code_of[name], a, b, c) == x, what
                    if rec is None:
                        assert x is None and rule == LP.RULE_RAISES, what
                        seen["RAISES"] = seen.get("RAISES", 0) + 1
                        continue
                    assert x == [None if ch == "." else int(ch) for ch in rec], what
                    assert rule != LP.RULE_RAISES and LP.pattern_shape(x) == rule, what
                    runs = LP.pattern_runs(x)
                    assert runs == LC.runs_of(x), what
                    if rule == LP.RULE_NOT_MODELLED:
                        assert not LC.modelled(runs, c), what
                        seen["NOT_MODELLED"] = seen.get("NOT_MODELLED", 0) + 1
                    else:
                        assert LC.modelled(runs, c) and runs == LP.shape_runs(*rule, c), (what, rule, runs)
                        seen[rule[0]] = seen.get(rule[0], 0) + 1
    print("fixture", seen, flush=True)
    assert all(seen.get(k, 0) >= 10 for k in ("RAISES", "NOT_MODELLED", LP.SHAPE_EMPTY, LP.SHAPE_PREFIX,
                                               LP.SHAPE_SUFFIX, LP.SHAPE_WHOLE)), seen


def test_shape_rule_beyond_the_fixture():
    """The closed form against the simulation where the fixture does not reach: c = 0, negative and far ends."""
    for cls, c, a, b in itertools.product((1, 2, 3), (0, 1, 2, 5), range(-9, 10), range(-9, 10)):
        x = LP.setx_pattern(cls, a, b, c)
        rule = LP.shape_rule(cls, a, b, c)
        assert (x is None) == (rule == LP.RULE_RAISES), (cls, c, a, b)
        if x is not None and c >= 1:
            assert LP.pattern_shape(x) == rule, (cls, c, a, b)
    assert LP.shape_rule(1, 2 ** 31 - 1, 2 ** 31 - 1, 253) == LP.RULE_RAISES
    assert LP.shape_rule(2, -2 ** 31, -2 ** 31, 253) == LP.RULE_RAISES == LP.shape_rule(2, 2 ** 31 - 1, 0, 253)
    assert LP.setx_pattern(2, 2 ** 31 - 1, 0, 253) is None and LP.setx_pattern(1, 2 ** 31 - 1, 5, 253) is None


@pytest.mark.parametrize("max_combos", [1 << 20, 6])
def test_host_against_brute_force(max_combos):
    """360 random spectra (M <= 6, sets of <= 3 rows, up to 4 candidates, wild
    ends in a fifth of them): status, combos, n_feas and best of every candidate
    equal the brute force's.  At max_combos = 6 some SOLVED candidates become
    TOO_LARGE and nothing else changes."""
    n = {k: 0 for k in range(7)}
    total = 0
    for rm, specs, row_mod, rate, rates in cases():
        caps = LC.caps_of(specs, len(rm), row_mod, rate, rates)
        got, valid = LC.host(specs, rm, caps, PREC, max_combos)
        cand = [c for s in specs for c in LC.candidates_of(s)]
        assert got.cand_len.tolist() == cand and got.cand_off[-1] == len(cand)
        LC.assert_equal4(got, LC.brute(specs, valid, rm, caps, PREC, max_combos), (max_combos, rm))
        for st in got.status.tolist():
            n[st] += 1
        total += len(cand)
    print("max_combos", max_combos, "candidates", total, "statuses", n, flush=True)
    assert all(n[k] > 0 for k in n if k != LC.TOO_LARGE), n  # every status occurs
    if max_combos == 6:
        assert n[LC.TOO_LARGE] >= 20, n
    else:
        assert 2 * n[LC.SOLVED] >= total and n[LC.TOO_LARGE] == 0, (n, total)  # at least half are SOLVED


def test_too_large_occurs_with_every_other_status():
    """Every status in one run (max_combos = 6)."""
    n = set()
    for rm, specs, row_mod, rate, rates in cases():
        caps = LC.caps_of(specs, len(rm), row_mod, rate, rates)
        n |= set(LC.host(specs, rm, caps, PREC, 6)[0].status.tolist())
    assert n == set(range(7)), n


def test_valid_equals_the_mirror():
    """length_valid against SkeletonBuilder.validate_sequence_length_by_mass of the
    mirror on the slices select_sequence_length_with_lp passes, name sets and all."""
    from spectrseqtools_amd.skeleton_building import SkeletonBuilder

    yes = no = 0
    for rm, specs, *_ in cases()[:5]:  # (rows ascending by mass, as a table's are)
        cases_ = LC.make_cases(specs, rm)
        got = LP.length_valid(cases_, PREC)
        names = cases_.row_names
        nuc = {names[r]: rm[r] * PREC for r in range(1, len(rm))}
        k = 0
        for s in specs:
            start = [{names[r] for r in p} for p in s["start"]]
            end = [{names[r] for r in p} for p in s["end"]]
            shim = SimpleNamespace(dp_table=SimpleNamespace(seq=SimpleNamespace(su_mass=s["su_mass"])))
            for c in LC.candidates_of(s):
                want = SkeletonBuilder.validate_sequence_length_by_mass(shim, start[:c], end[len(end) - c:], nuc)
                assert bool(got[k]) == bool(want), (s, c)
                yes, no, k = yes + bool(want), no + (not want), k + 1
    assert yes >= 100 and no >= 30, (yes, no)


def exact_optimum(spec, c, rm, row_mod, mod_cap, prec):
    """min over the feasible y and every run of sum |su / prec - S| in fractions (per-row caps loose)."""
    sets = LC.position_rows(spec, c, len(rm))
    runs = [LC.runs_of(LC.replay_set_x(code, mn, mx, c)) for code, _, mn, mx in spec["frags"]]
    best = None
    for y in itertools.product(*sets):
        if sum(int(row_mod[r]) for r in y) > mod_cap:
            continue
        obj = sum(min(abs(Fraction(su) / Fraction(prec) - (sum(rm[y[i]] for i in range(r[0], r[1] + 1)) if r else 0))
                      for r in rr) for (_, su, _, _), rr in zip(spec["frags"], runs))
        best = obj if best is None or obj < best else best
    return best


def test_best_and_take_in_exact_arithmetic():
    """On tiny instances: best / 65536 is within n 2^-16 units of the exact
    optimum, and wherever the decision is TAKE the exact argmin over the
    candidates the reference can choose is c*, and unique."""
    solved = taken = 0
    for k, rm in enumerate(ALPHABETS[:5]):
        specs, row_mod, rate, _ = LC.random_case(5200 + k, rm, PREC, 40, max_M=5, max_rows=2)
        caps = LC.caps_of(specs, len(rm), row_mod, rate)
        got, valid = LC.host(specs, rm, caps, PREC)
        decision, length = LP.length_decisions(got)
        for g, s in enumerate(specs):
            ks = range(int(got.cand_off[g]), int(got.cand_off[g + 1]))
            exact = {}
            for kk in ks:
                if got.status[kk] != LC.SOLVED:
                    continue
                c, n = int(got.cand_len[kk]), len(s["frags"])
                exact[c] = exact_optimum(s, c, rm, row_mod, int(caps[1][kk]), PREC)
                assert abs(Fraction(int(got.best[kk]), LC.FIX) - exact[c]) <= Fraction(n, LC.FIX), (g, c)
                solved += 1
            if decision[g] == LP.LENGTH_TAKE:
                assert all(got.status[kk] in (LC.INVALID, LC.RAISES, LC.SOLVED) for kk in ks)
                low = min(exact.values())
                assert [c for c, v in exact.items() if v == low] == [int(length[g])], (g, exact, length[g])
                taken += 1
            else:
                assert length[g] == -1
    print("solved", solved, "TAKE", taken, flush=True)
    assert solved >= 150 and taken >= 40, (solved, taken)


def outcome_of(statuses, bests, n_frag=3, lower=2, max_len=9, lb_status=0, undecided=0):
    n = len(statuses)
    return LP.LengthOutcome(cand_off=[0, n], cand_len=np.arange(lower, lower + n), status=statuses,
                            combos=np.ones(n), n_feas=np.ones(n), best=bests, max_len=[max_len], lower=[lower],
                            upper=[lower + n - 1], lb_status=[lb_status], n_frag=[n_frag], undecided=[undecided])


def test_length_decisions_branches():
    I, R, N, F, NF, TL, S = range(7)  # noqa: E741
    d = lambda *a, **k: tuple(int(x[0]) for x in LP.length_decisions(outcome_of(*a, **k)))  # noqa: E731
    half = LC.FIX // 2
    assert d([S, S], [100, 100 + half]) == (LP.LENGTH_TAKE, 2)
    assert d([S, S], [100, 100 + half - 1]) == (LP.LENGTH_SOLVE, -1)
    assert d([S, S, I, R], [100 + half, 100, 0, 0]) == (LP.LENGTH_TAKE, 3)
    assert d([S], [7]) == (LP.LENGTH_TAKE, 2)
    assert d([S, S], [5, 5]) == (LP.LENGTH_SOLVE, -1)  # a tie
    assert d([], []) == (LP.LENGTH_JACCARD, -1)  # lower > upper: no candidates
    assert d([I, R, I], [0, 0, 0]) == (LP.LENGTH_JACCARD, -1)
    for other in (N, F, NF, TL):
        assert d([S, other], [5, 0]) == (LP.LENGTH_SOLVE, -1)
        assert d([I, other], [0, 0]) == (LP.LENGTH_SOLVE, -1)
    assert d([S, S], [5, 1 << 40], lb_status=-3) == (LP.LENGTH_NONE, -1)
    assert d([S, S], [5, 1 << 40], max_len=2) == (LP.LENGTH_NONE, -1)  # upper = 3 > max_len
    assert d([S, S], [5, 1 << 40], max_len=3) == (LP.LENGTH_TAKE, 2)
    assert d([S, S], [5, 1 << 40], undecided=1) == (LP.LENGTH_SOLVE, -1)
    # the rounding margin alone (min_gap_units = 0): 2 n + 1 units decide, 2 n do not
    zero = lambda *a, **k: tuple(int(x[0]) for x in LP.length_decisions(outcome_of(*a, **k), 0.0))  # noqa: E731
    assert zero([S, S], [50, 50 + 2 * 3 + 1], n_frag=3) == (LP.LENGTH_TAKE, 2)
    assert zero([S, S], [50, 50 + 2 * 3], n_frag=3) == (LP.LENGTH_SOLVE, -1)
    assert zero([S, S], [50 + 2 * 20000 + 1, 50], n_frag=20000) == (LP.LENGTH_TAKE, 3)
    assert d([S, S], [50 + 2 * 20000 + 1, 50], n_frag=20000) == (LP.LENGTH_TAKE, 3)  # 2 n + 1 above half a unit
    assert d([S, S], [50 + 2 * 20000, 50], n_frag=20000) == (LP.LENGTH_SOLVE, -1)


def test_cases_and_outcome_take_concat():
    rm = ALPHABETS[3]
    specs, row_mod, rate, rates = LC.random_case(77, rm, PREC, 12)
    cases_ = LC.make_cases(specs, rm)
    caps = LC.caps_of(specs, len(rm), row_mod, rate, rates)
    lo, valid = LC.host(specs, rm, caps, PREC)
    idx = [5, 0, 11, 5]
    sub = cases_.take(idx)
    want = LC.make_cases([specs[i] for i in idx], rm)
    for k in LP.LengthCases._DTYPES:
        assert np.array_equal(getattr(sub, k), getattr(want, k)), k
    sub_specs = [specs[i] for i in idx]
    sub_caps = LC.caps_of(sub_specs, len(rm), row_mod, rate, rates)
    assert lo.take(idx).equals(LC.host(sub_specs, rm, sub_caps, PREC)[0])
    parts = [cases_.take([i]) for i in range(len(specs))]
    back = LP.LengthCases.concat(parts)
    assert all(np.array_equal(getattr(back, k), getattr(cases_, k)) for k in LP.LengthCases._DTYPES)
    assert LP.LengthOutcome.concat([lo.take([i]) for i in range(len(specs))]).equals(lo)
    blank = LP.LengthOutcome.concat([lo, LP.LengthOutcome.not_computed(2)])
    assert len(blank) == len(lo) + 2 and LP.length_decisions(blank)[0][-2:].tolist() == [LP.LENGTH_SOLVE] * 2
    assert abs(sum(lo.shares().values()) - 1.0) < 1e-12
    with pytest.raises(ValueError):
        LP.length_program_host(cases_, PREC, valid, caps, max_combos=0)
    with pytest.raises(ValueError):
        LP.length_program_host(cases_, PREC, valid[:-1], caps)


def test_ctypes_mirror_matches_header_struct():
    """_native.LengthProgramArgs is the header's sst_length_program_args, field by field."""
    from test_boundary import SCALARS, header_functions, header_struct_fields

    want = [(f, ctypes.c_void_p if pointer else SCALARS[base])
            for f, base, pointer, _ in header_struct_fields("sst_length_program_args")]
    assert [(n, t) for n, t, *_ in _native.LengthProgramArgs._fields_] == want
    assert [n for n, _ in want[-4:]] == ["status", "combos", "n_feas", "best"] and want[0][0] == "n_spec"
    assert ctypes.sizeof(_native.LengthProgramArgs) == 8 * len(want)
    assert "sst_length_program_device" in header_functions() and "sst_length_program_device" in _native.EXPORTS
