"""CPU tests of the final program's host model (final_program.final_host,
final_use, final_decisions, FinalOutcome): the model against the definition
taken literally (tests/_final_cases.py: itertools.product over every y, every
admissible interval, Python ints), the claim behind FINAL_TAKE against the full
program with the per-row caps restored in exact fractions, and the plumbing."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
import _final_cases as FC
from spectrseqtools_amd import alignment
from spectrseqtools_amd import final_program as FP
from test_align_keep_model import ALPHABETS, PREC, TOL, enumerate_program

PER_ALPHABET = 70  # 420 spectra over the six alphabets


def cases():
    return [(rm,) + FC.random_final_case(1900 + k, rm, TOL, PREC, PER_ALPHABET) for k, rm in enumerate(ALPHABETS)]


def test_status_constants():
    assert (FP.FINAL_NONE, FP.FINAL_SOLVED, FP.FINAL_TOO_LARGE, FP.FINAL_INFEASIBLE, FP.FINAL_SKIPPED, FP.FINAL_NOT_FREE,
            FP.FINAL_UNDECIDED) == (FC.NONE, FC.SOLVED, FC.TOO_LARGE, FC.INFEASIBLE, FC.SKIPPED, FC.NOT_FREE, FC.UNDECIDED)
    assert FP.FINAL_MAX_COMBOS == 1 << 22 and FP.FINAL_DEFAULT_COMBOS == 1 << 20 and FP.FIX == FC.FIX


@pytest.mark.parametrize("max_combos", [1 << 20, 12])
def test_host_against_brute_force(max_combos):
    """420 random spectra (L <= 6, sets of <= 3 rows, rows of equal mass in the
    last alphabet), random row_mod, mod_cap, per-row rates and use masks: all
    nine arrays equal the brute force's.  At max_combos = 12 some of the SOLVED
    spectra become TOO_LARGE and nothing else changes."""
    n = {k: 0 for k in range(6)}
    unique = tied = bound = masked = big = 0
    for rm, specs, row_cap in cases():
        got = FC.host(specs, rm, row_cap, PREC, max_combos)
        FC.assert_equal9(got, FC.brute_final(specs, rm, row_cap, PREC, max_combos), (max_combos, rm))
        for st in got.status.tolist():
            n[st] += 1
        solved = got.status == FC.SOLVED
        unique += int((got.n_opt[solved] == 1).sum())
        tied += int((got.n_opt[solved] > 1).sum())
        bound += int((got.n_feas[solved] < got.combos[solved]).sum())
        masked += sum(1 for s, ok in zip(specs, solved) if ok and s.get("use") is not None and not all(s["use"]))
        big = max(big, int(got.combos[solved].max(initial=0)))
    print("max_combos", max_combos, "statuses", n, "unique", unique, "tied", tied, "cap binds", bound, "masked", masked,
          "largest combos", big, flush=True)
    # (floors against a vacuous pass only: about half of what the brute force gives for this generator)
    if max_combos == 12:
        assert n[FC.TOO_LARGE] >= 24 and n[FC.SOLVED] >= 95 and big <= 12, n
    else:
        assert n[FC.SOLVED] >= 115 and unique >= 85 and tied >= 25 and bound >= 12 and masked >= 25 and big >= 80, n
        assert n[FC.SKIPPED] >= 5 and n[FC.INFEASIBLE] >= 40 and n[FC.NOT_FREE] >= 45 and n[FC.TOO_LARGE] == 0, n


def test_edge_builders_against_brute_force():
    """The edge cases the GPU tests run at full size, here at a size the brute
    force can enumerate: the tie across passes (two optima, the lower index
    wins), pinned prefixes, the classes with ranges of ends, mn > mx, the empty
    interval, fragments out of su order, a use mask that takes out a fragment
    the model skips."""
    rm = [0, 30011, 41017, 52021, 63029, 74051, 85061]
    rng = np.random.default_rng(5)
    row_cap = KC.loose_row_cap(len(rm))
    tie, a, b = FC.tie_across_passes(rm, PREC, high=1, low=3, x=5)
    pinned, y = FC.pinned_binary_spec(rm, 6, [1, 0, 1, 1, 0, 1], PREC)
    sets = [[1, 2], [3], [2, 4, 5], [1, 6], [3]]
    mixed = FC.loose_spec(rm, sets, FC.random_frags(rng, rm, sets, 44, PREC))
    assert any(f[3] > f[4] for f in mixed["frags"]) and mixed["frags"] != sorted(mixed["frags"], key=lambda f: f[1])
    bad_end = (FC.START, 30011 * PREC, 100.0, 7, 7)
    unused_bad = FC.loose_spec(rm, sets, mixed["frags"][:6] + [bad_end], use=[1] * 6 + [0])
    used_bad = FC.loose_spec(rm, sets, mixed["frags"][:6] + [bad_end])
    specs = [tie, pinned, mixed, unused_bad, used_bad]
    got = FC.host(specs, rm, row_cap, PREC)
    FC.assert_equal9(got, FC.brute_final(specs, rm, row_cap, PREC, 1 << 20), "edges")
    assert got.status.tolist() == [FC.SOLVED] * 4 + [FC.SKIPPED]
    assert got.n_opt[0] == 2 and got.best[0] == 0 and a < b == a + 8
    digits = [int(r == 2) for r in got.seq[:6]]  # (the pair is rows 1 and 2)
    assert int("".join(map(str, digits)), 2) == a
    assert got.n_opt[1] == 1 and got.best[1] == 0 and got.seq[6:12].tolist() == y and got.gap[1] > 0
    assert (got.iv[got.frag_off[2]:got.frag_off[3]] == 0xFFFF).any()  # the empty interval as a minimiser
    assert got.iv[got.frag_off[4] - 1] == 0xFFFE and (got.iv[got.frag_off[3]:got.frag_off[4] - 1] != 0xFFFE).all()


def exact_program(spec, row_mass, is_mod, rate, universal, used):
    """{y: the exact objective} over the full program (the universal and the
    per-row caps, every admissible x), in fractions of a mass unit."""
    L = spec["L"]
    prec = Fraction(PREC)
    out = {}
    for y in enumerate_program(spec, row_mass, is_mod, rate, universal):
        total = Fraction(0)
        for j in used:
            code, su, _, mn, mx = spec["frags"][j]
            total += min(abs(Fraction(su) - prec * sum(row_mass[y[i]] for i in (range(l, r + 1) if l != 0xFF else ())))
                         for l, r in AC.admissible_intervals(code, mn, mx, L))
        out[y] = total
    return out


def test_take_is_the_exact_unique_optimum():
    """Tiny instances with every cap restored, every y and x enumerated in
    fractions.Fraction: best is within n_used fixed-point units of the exact
    optimum for every SOLVED spectrum; wherever final_decisions says TAKE the
    exact argmin is unique and equals seq."""
    rng = np.random.default_rng(21)
    solved = taken = not_taken = 0
    for trial in range(500):
        row_mass = [0] + sorted(rng.choice(np.arange(3, 40), size=int(rng.integers(1, 5)), replace=True).tolist())
        is_mod = [False] + [bool(rng.random() < 0.5) for _ in row_mass[1:]]
        rate = [0.0] + [float(rng.choice(KC.RATES + (1.0, 1.0))) for _ in row_mass[1:]]
        universal = float(rng.choice([0.25, 0.5, 1.0]))
        spec = AC.random_spectrum(rng, row_mass, TOL, PREC, max_len=4, max_alpha=4, max_set=3)
        L = spec["L"]
        spec["frags"] = [(c, su + float(rng.choice([0.0, 1e-7, -3e-6])), obs, min(max(mn, 0), L - 1), min(max(mx, 0), L - 1))
                         for c, su, obs, mn, mx in spec["frags"]]
        spec["row_mod"], spec["mod_cap"] = np.array(is_mod, dtype=np.uint8), math.ceil(universal * L)
        if trial % 3 == 0:
            spec["use"] = [int(rng.random() < 0.7) for _ in spec["frags"]]
        fo = FC.host([spec], row_mass, KC.row_cap_table(rate), PREC)
        if fo.status[0] != FC.SOLVED:
            continue
        solved += 1
        used = [j for j, u in enumerate(FC.use_of(spec)) if u]
        assert fo.n_used().tolist() == [len(used)]
        exact = exact_program(spec, row_mass, is_mod, rate, universal, used)
        assert len(exact) == int(fo.n_feas[0])  # row-free: the program's y are the cap-feasible y
        opt = min(exact.values())
        assert abs(int(fo.best[0]) - opt * FC.FIX / Fraction(PREC)) <= len(used), (trial, fo.best[0], opt)
        if FP.final_decisions(fo)[0] == FP.FINAL_TAKE:
            taken += 1
            argmin = [y for y, v in exact.items() if v == opt]
            assert argmin == [tuple(fo.seq.tolist())], (trial, argmin, fo.seq)
        else:
            not_taken += 1
    print("solved", solved, "TAKE", taken, "SOLVE", not_taken, flush=True)
    assert solved >= 130 and taken >= 115 and not_taken >= 14, (solved, taken, not_taken)


def test_final_decisions_thresholds():
    """TAKE iff SOLVED, n_opt == 1 and gap >= max(2 n_used + 1, min_gap_units * 65536)."""
    S = 6
    off = np.arange(S + 1) * 3
    iv = np.full(3 * S, 0xFFFE, np.uint16)
    iv[:15] = 0  # three used fragments each; the last spectrum: none
    fo = FP.FinalOutcome(frag_off=off, pos_off=np.zeros(S + 1, np.int64), status=[1, 1, 1, 2, 1, 1],
                         combos=np.ones(S), n_feas=np.ones(S), best=np.zeros(S), n_opt=[1, 1, 2, 1, 1, 1],
                         gap=[32768, 32767, 1 << 40, 1 << 40, FP.NO_GAP, 1], seq=np.zeros(0), iv=iv, sum=np.zeros(3 * S))
    assert fo.n_used().tolist() == [3, 3, 3, 3, 3, 0]
    assert FP.final_decisions(fo).tolist() == [1, 0, 0, 0, 1, 0]
    assert FP.final_decisions(fo, min_gap_units=0.0).tolist() == [1, 1, 0, 0, 1, 1]
    fo.gap[:2] = [7, 6]
    assert FP.final_decisions(fo, min_gap_units=0.0).tolist()[:2] == [1, 0]  # 2 n_used + 1 = 7


def test_final_use_and_outcome_plumbing():
    """final_use: use = the KEEP fragments, undecided = the spectra that hold an
    LP_SOLVE fragment; undecided spectra get FINAL_UNDECIDED and nothing else;
    FinalOutcome take / concat / equals; sequence_names."""
    rm, specs, row_cap = cases()[3]
    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    al = alignment.align_host(o, TOL, PREC, caps=caps, keep=row_cap)
    use, undecided = FP.final_use(al)
    dec = alignment.lp_decisions(al)
    assert use.dtype == np.uint8 and np.array_equal(use == 1, dec == alignment.LP_KEEP)
    assert undecided.dtype == bool and len(undecided) == len(o)
    for g in range(len(o)):
        assert undecided[g] == (dec[o.frag_off[g]:o.frag_off[g + 1]] == alignment.LP_SOLVE).any()
    assert 5 <= undecided.sum() < len(o) and use.any()
    with pytest.raises(ValueError, match="keep mode"):
        FP.final_use(alignment.align_host(o, TOL, PREC, caps=caps))

    fo = FP.final_host(o, PREC, caps, row_cap, use=use, undecided=undecided)
    free = FP.final_host(o, PREC, caps, row_cap, use=use)
    assert (fo.status[undecided] == FP.FINAL_UNDECIDED).all() and not (fo.status[~undecided] == FP.FINAL_UNDECIDED).any()
    assert fo.take(np.flatnonzero(~undecided)).equals(free.take(np.flatnonzero(~undecided)))
    blank = FP.FinalOutcome.blank(o.take(np.flatnonzero(undecided)), FP.FINAL_UNDECIDED)
    assert fo.take(np.flatnonzero(undecided)).equals(blank) and (blank.gap == FP.NO_GAP).all()
    assert abs(sum(fo.shares().values()) - 1.0) < 1e-12 and fo.shares()["UNDECIDED"] == undecided.mean()

    idx = np.array([5, 0, 17, 5])
    part = free.take(idx)
    assert len(part) == 4 and np.array_equal(np.diff(part.frag_off), np.diff(o.frag_off)[idx])
    assert np.array_equal(np.diff(part.pos_off), np.diff(o.pos_off)[idx])
    assert np.array_equal(part.seq[:part.pos_off[1]], free.seq[o.pos_off[5]:o.pos_off[6]])
    assert np.array_equal(part.iv[:part.frag_off[1]], free.iv[o.frag_off[5]:o.frag_off[6]])
    whole = FP.FinalOutcome.concat([free.take(np.arange(0, 30)), free.take(np.arange(30, len(free)))])
    assert whole.equals(free) and free.equals(whole) and not free.equals(fo)
    with pytest.raises(ValueError):
        FP.FinalOutcome.concat([])
    with pytest.raises(ValueError):
        FP.FinalOutcome(frag_off=free.frag_off, pos_off=free.pos_off, status=free.status[:-1], combos=free.combos,
                        n_feas=free.n_feas, best=free.best, n_opt=free.n_opt, gap=free.gap, seq=free.seq, iv=free.iv,
                        sum=free.sum)
    g = int(np.flatnonzero(free.status == FP.FINAL_SOLVED)[0])
    names = FP.sequence_names(free, o, g)
    assert names == [o.row_names[r] for r in free.seq[o.pos_off[g]:o.pos_off[g + 1]]] and len(names) == o.seq_len[g]
    with pytest.raises(ValueError, match="not SOLVED"):
        FP.sequence_names(free, o, int(np.flatnonzero(free.status != FP.FINAL_SOLVED)[0]))
    for bad in (0, (1 << 22) + 1):
        with pytest.raises(ValueError, match="max_combos"):
            FP.final_host(o, PREC, caps, row_cap, max_combos=bad)
    with pytest.raises(ValueError):
        FP.final_host(o, PREC, caps, row_cap, use=np.ones(3))


def test_limit_kinds_against_brute_force():
    """The kinds of input tests/test_gpu_final_limits.py holds the kernel to the
    host model on, here the host model against the brute force at a size it
    enumerates: L == 0; su that is not finite, at the fixed-point range's edge
    and negative, used and unused, in every class; 1100 fragments with the
    middle 512 out of use, over 8 assignments; 16384 and 16385 used fragments
    over 2 assignments."""
    rm = [0, 30011, 41017, 52021, 63029, 74051, 85061]
    rng = np.random.default_rng(6)
    zero, zero_want, objective = FC.zero_length_specs(rm, PREC)
    values, su_want = FC.su_value_specs(rm, PREC)
    masked = FC.chunk_mask_spec(rm, [[1, 2], [3, 4], [5, 6]], 1100, PREC, rng)
    edge, a, b = FC.n_used_specs(rm, PREC)
    specs = zero + values + [masked, dict(masked, use=None)] + edge
    got = FC.host(specs, rm, KC.loose_row_cap(len(rm)), PREC)
    FC.assert_equal9(got, FC.brute_final(specs, rm, KC.loose_row_cap(len(rm)), PREC, 1 << 20), "limit kinds")
    assert got.status.tolist() == zero_want + su_want + [FC.SOLVED] * 3 + [FC.SKIPPED]
    assert got.best[:2].tolist() == [objective] * 2 and (got.iv[:8] == 0xFFFF).all() and got.combos[:4].tolist() == [1, 1, 0, 1]
    at = len(zero) + len(values)
    assert got.combos[at] == 8 and got.best[at] < got.best[at + 1] and got.n_used()[at:].tolist() == [588, 1100, 16384, 0]
    assert got.gap[at + 2] == 16384 * FC.FIX * abs(rm[b] - rm[a]) and got.combos[at + 2] == 2


def test_bits_above_the_row_count_against_brute_force():
    """A 65-row table, free positions over rows 63 | 64 (the two words of a
    mask), modified rows from 64 on, every alphabet and constrained position
    with all bits from 65 to 127 set, and bit 0 of the alphabet: the rows that
    do not exist are in no A_i."""
    rm, specs, row_cap = FC.row_edge_case(65, PREC, np.random.default_rng(7))
    got = FC.host(specs, rm, row_cap, PREC)
    FC.assert_equal9(got, FC.brute_final(specs, rm, row_cap, PREC, 1 << 20), "65 rows")
    assert got.combos.tolist() == [8, 8, 8, 8, 18, 0, 8, 8] and got.status[4:7].tolist() == [FC.SOLVED, FC.INFEASIBLE, FC.NOT_FREE]
    assert all(s["alpha"][1] >> 63 and s["alpha"][0] & 1 for s in specs) and got.n_feas[1] < got.combos[1]


def test_model_limits():
    """|u| >= 2^32, a u that is not finite and an out-of-range end make the
    spectrum SKIPPED only where the fragment is used; combos saturates."""
    rm = [0, 30011, 41017]
    row_cap = KC.loose_row_cap(3)
    sets = [[1, 2], [1]]
    ok = (FC.START_END, (30011 + 41017) * PREC, 100.0, 0, 0)
    specs = []
    for su in (2.0 ** 32 * PREC, -2.0 ** 32 * PREC, math.inf, math.nan, (2.0 ** 32 - 1) * PREC):
        specs.append(FC.loose_spec(rm, sets, [ok, (FC.INTERNAL, su, 100.0, 0, 0)]))
        specs.append(FC.loose_spec(rm, sets, [ok, (FC.INTERNAL, su, 100.0, 0, 0)], use=[1, 0]))
    wide = FC.loose_spec(rm, [[1, 2]] * 70, [ok])  # 2^70 assignments
    specs.append(wide)
    got = FC.host(specs, rm, row_cap, PREC)
    FC.assert_equal9(got, FC.brute_final(specs, rm, row_cap, PREC, 1 << 20), "limits")
    assert got.status.tolist() == [FC.SKIPPED, FC.SOLVED] * 4 + [FC.SOLVED, FC.SOLVED, FC.TOO_LARGE]
    assert got.combos[-1] == np.uint64(FC.NO_GAP) and got.combos[0] == 0 and got.combos[1] == 2
