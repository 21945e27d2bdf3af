"""CPU tests of the robust final program's host model (final_program.
final_robust_host, robust_decisions, RobustOutcome, final_use(optional=True)):
the model against the definition taken literally (tests/_robust_cases.py), the
identity behind it against every subset of the optional fragments through
final_host, the claim behind FINAL_TAKE against the full program in exact
fractions for every subset, and the plumbing."""
import math

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
import _final_cases as FC
import _robust_cases as RB
from spectrseqtools_amd import alignment
from spectrseqtools_amd import final_program as FP
from test_align_keep_model import ALPHABETS, PREC, TOL
from test_final_model import exact_program

PER_ALPHABET = 70  # 420 spectra over the six alphabets


def random_cases():
    return [(rm,) + RB.random_robust_case(3100 + k, rm, TOL, PREC, PER_ALPHABET) for k, rm in enumerate(ALPHABETS)]


@pytest.mark.parametrize("max_combos", [1 << 20, 12])
def test_host_against_brute_force(max_combos):
    """420 random spectra with a random 0 / 1 / 2 use per fragment: all
    fourteen arrays equal the brute force's, at the default max_combos and at 12."""
    solved = with_optional = copied = lower = tied = 0
    for rm, specs, row_cap in random_cases():
        fo, ro = RB.host(specs, rm, row_cap, PREC, max_combos)
        RB.assert_equal14((fo, ro), RB.brute_robust(specs, rm, row_cap, PREC, max_combos), (max_combos, rm))
        ok = fo.status == FC.SOLVED
        solved += int(ok.sum())
        with_optional += int((ro.n_optional[ok] > 0).sum())
        copied += int((ro.n_optional[ok] == 0).sum())
        lower += int((ro.rbest[ok] < fo.best[ok] + ro.cstar[ok]).sum())
        tied += int(((ro.rn_opt[ok] > 1) & (ro.n_optional[ok] > 0)).sum())
        assert (ro.rbest[ok] <= fo.best[ok] + ro.cstar[ok]).all()  # cap(y*) = best + cstar is one of the caps
        assert not ro.n_optional[~ok].any() and (ro.rgap[~ok] == FP.NO_GAP).all() and not ro.rbest[~ok].any()
    print("max_combos", max_combos, "solved", solved, "with optional", with_optional, "without", copied,
          "rbest < best + cstar", lower, "rn_opt > 1", tied, flush=True)
    # (floors against a vacuous pass only: about half of what this generator gives)
    if max_combos == 12:
        assert solved >= 60 and with_optional >= 35, (solved, with_optional)
    else:
        assert solved >= 75 and with_optional >= 45 and copied >= 15 and lower >= 8 and tied >= 10


def test_identity_against_all_subsets():
    """420 spectra with 15 % of the fragments optional, at most 6 each: for
    every SOLVED spectrum robust_decisions says TAKE iff for every one of the
    2^|O| subsets final_host with that subset used gives n_opt == 1, the same
    seq and gap >= need (need over n_used + n_optional)."""
    robust = fragile = moved = checked = 0
    for k, rm in enumerate(ALPHABETS):
        specs, row_cap = RB.sparse_optional_case(5100 + k, rm, TOL, PREC, PER_ALPHABET)
        o = AC.make_outcome(specs, rm)
        row_mod, mod_cap = CC.caps_of(specs, len(rm))
        use = RB.use3_array(specs)
        fo, ro = FP.final_robust_host(o, PREC, (row_mod, mod_cap), row_cap, use=use)
        dec = FP.robust_decisions(fo, ro)
        for g in np.flatnonzero((fo.status == FC.SOLVED) & (ro.n_optional > 0)).tolist():
            assert ro.n_optional[g] <= 6
            one = o.take([g])
            u = use[o.frag_off[g]:o.frag_off[g + 1]]
            seq = fo.seq[o.pos_off[g]:o.pos_off[g + 1]]
            need = max(2 * int(np.count_nonzero(u)) + 1, FP.FIX // 2)
            solve = lambda mask: FP.final_host(one, PREC, (row_mod, mod_cap[g:g + 1]), row_cap,  # noqa: E731
                                               use=mask.astype(np.uint8))
            every = True
            for t in RB.subsets(np.flatnonzero(u == 2).tolist()):
                mask = u == 1
                mask[list(t)] = True
                f = solve(mask)
                assert f.status[0] == FC.SOLVED
                every = every and f.n_opt[0] == 1 and np.array_equal(f.seq, seq) and int(f.gap[0]) >= need
            assert (dec[g] == FP.FINAL_TAKE) == every, (k, g)
            checked += 1
            robust += int(every)
            fragile += int(FP.final_decisions(solve(u == 1))[0] == FP.FINAL_TAKE and not every)
            moved += int(not np.array_equal(solve(u != 0).seq, seq))
    print("with optional", checked, "TAKE", robust, "TAKE on R alone only", fragile, "another argmin over R + O", moved,
          flush=True)
    assert robust >= 40 and fragile >= 10 and moved >= 15, (checked, robust, fragile, moved)


def test_take_is_the_exact_unique_optimum_of_every_subset():
    """Tiny instances with every cap restored, every y and x enumerated in
    fractions.Fraction: wherever robust_decisions says TAKE, for every subset T
    of the optional fragments the exact argmin over the required ones and T is
    unique and equals seq."""
    rng = np.random.default_rng(23)
    solved = taken = taken_optional = not_taken = 0
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
        use = [int(rng.choice([0, 1, 1, 1, 2])) for _ in spec["frags"]]
        while use.count(2) > 4:
            use[use.index(2)] = 1
        spec["use"] = use
        fo, ro = RB.host([spec], row_mass, KC.row_cap_table(rate), PREC)
        if fo.status[0] != FC.SOLVED:
            continue
        solved += 1
        required = [j for j, u in enumerate(use) if u == 1]
        optional = [j for j, u in enumerate(use) if u == 2]
        assert fo.n_used().tolist() == [len(required) + len(optional)] and ro.n_optional[0] == len(optional)
        if FP.robust_decisions(fo, ro)[0] != FP.FINAL_TAKE:
            not_taken += 1
            continue
        taken += 1
        taken_optional += bool(optional)
        for t in RB.subsets(optional):
            exact = exact_program(spec, row_mass, is_mod, rate, universal, required + list(t))
            opt = min(exact.values())
            argmin = [y for y, v in exact.items() if v == opt]
            assert argmin == [tuple(fo.seq.tolist())], (trial, t, argmin, fo.seq)
    print("solved", solved, "TAKE", taken, "of them with optional fragments", taken_optional, "SOLVE", not_taken, flush=True)
    assert solved >= 130 and taken_optional >= 40 and not_taken >= 14, (solved, taken, taken_optional, not_taken)


def test_ctypes_mirror_matches_header_struct():
    """_native.FinalRobustArgs is the header's sst_final_robust_args: the
    sst_final_args struct by value, then five pointers of the header's names."""
    import ctypes

    from spectrseqtools_amd import _native
    from test_boundary import header_functions, header_struct_fields

    fields = header_struct_fields("sst_final_robust_args")
    assert fields[0] == ("base", "sst_final_args", False, None) and all(pointer for _, _, pointer, _ in fields[1:])
    want = [("base", _native.FinalArgs)] + [(name, ctypes.c_void_p) for name, _, _, _ in fields[1:]]
    assert [(n, t) for n, t, *_ in _native.FinalRobustArgs._fields_] == want
    assert [n for n, _ in want[1:]] == list(RB.ROBUST_FIELDS)
    assert ctypes.sizeof(_native.FinalRobustArgs) == ctypes.sizeof(_native.FinalArgs) + 5 * ctypes.sizeof(ctypes.c_void_p)
    assert "sst_final_robust_device" in header_functions() and "sst_final_robust_device" in _native.EXPORTS


def test_robust_decisions_thresholds():
    """TAKE iff SOLVED, rbest == best + cstar, rn_opt == 1 and rgap >= max(2 (n_used + n_optional) + 1,
    min_gap_units * 65536)."""
    S = 7
    off = np.arange(S + 1) * 3
    iv = np.zeros(3 * S, np.uint16)  # three fragments with an interval each: required and optional together
    fo = FP.FinalOutcome(frag_off=off, pos_off=np.zeros(S + 1, np.int64), status=[1, 1, 1, 1, 2, 1, 1],
                         combos=np.ones(S), n_feas=np.ones(S), best=np.full(S, 10), n_opt=np.ones(S),
                         gap=np.full(S, 1 << 40), seq=np.zeros(0), iv=iv, sum=np.zeros(3 * S))
    ro = FP.RobustOutcome(n_optional=np.ones(S), cstar=np.full(S, 5), rbest=[15, 15, 14, 15, 15, 15, 15],
                          rn_opt=[1, 1, 1, 2, 1, 1, 1], rgap=[32768, 32767, 1 << 40, 1 << 40, 1 << 40, FP.NO_GAP, 7])
    assert FP.robust_decisions(fo, ro).tolist() == [1, 0, 0, 0, 0, 1, 0]
    assert FP.robust_decisions(fo, ro, min_gap_units=0.0).tolist() == [1, 1, 0, 0, 0, 1, 1]
    ro.rgap[6] = 6  # 2 * 3 + 1 = 7
    assert FP.robust_decisions(fo, ro, min_gap_units=0.0)[6] == FP.FINAL_SOLVE


def test_no_optional_fragment_is_the_base_program():
    """With use in {0, 1} the FinalOutcome is final_host's, the robust outputs
    are (0, 0, best, n_opt, gap) on SOLVED spectra, and robust_decisions is
    final_decisions; use values other than 0 and 2 count as 1; final_host itself
    still maps every non-zero use to 1."""
    rm = ALPHABETS[3]
    specs, row_cap = FC.random_final_case(1903, rm, TOL, PREC, PER_ALPHABET)
    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    use = FC.use_array(specs)
    base = FP.final_host(o, PREC, caps, row_cap, use=use)
    fo, ro = FP.final_robust_host(o, PREC, caps, row_cap, use=use)
    assert fo.equals(base)
    ok = fo.status == FC.SOLVED
    assert ok.sum() >= 15 and not ro.n_optional.any() and not ro.cstar.any()
    assert np.array_equal(ro.rbest, fo.best) and np.array_equal(ro.rn_opt, fo.n_opt) and np.array_equal(ro.rgap, fo.gap)
    assert np.array_equal(FP.robust_decisions(fo, ro), FP.final_decisions(fo))
    assert np.array_equal(FP.robust_decisions(fo, ro, 0.0), FP.final_decisions(fo, 0.0))
    odd, _ = FP.final_robust_host(o, PREC, caps, row_cap, use=use * 7)
    assert odd.equals(base)
    assert FP.final_host(o, PREC, caps, row_cap, use=use * 2).equals(base)
    none, ro_none = FP.final_robust_host(o, PREC, caps, row_cap)
    assert none.equals(FP.final_host(o, PREC, caps, row_cap)) and not ro_none.n_optional.any()


def test_final_use_optional_and_outcome_plumbing():
    """final_use(optional=True): 1 at the KEEP fragments, 2 at the SOLVE ones,
    nothing undecided, and the default call unchanged; RobustOutcome take /
    concat / blank / equals; argument errors."""
    rm = ALPHABETS[3]
    specs, row_cap = FC.random_final_case(1903, rm, TOL, PREC, PER_ALPHABET)
    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    al = alignment.align_host(o, TOL, PREC, caps=caps, keep=row_cap)
    dec = alignment.lp_decisions(al)
    use, undecided = FP.final_use(al, optional=True)
    assert use.dtype == np.uint8 and undecided.dtype == bool and len(undecided) == len(o) and not undecided.any()
    assert np.array_equal(use == 1, dec == alignment.LP_KEEP) and np.array_equal(use == 2, dec == alignment.LP_SOLVE)
    assert (use == 2).sum() >= 5
    plain_use, plain_undecided = FP.final_use(al)
    again_use, again_undecided = FP.final_use(al, optional=False)
    assert np.array_equal(plain_use, again_use) and np.array_equal(plain_undecided, again_undecided)
    assert np.array_equal(plain_use, (use == 1).astype(np.uint8)) and plain_undecided.sum() >= 5
    with pytest.raises(ValueError, match="keep mode"):
        FP.final_use(alignment.align_host(o, TOL, PREC, caps=caps), optional=True)

    fo, ro = FP.final_robust_host(o, PREC, caps, row_cap, use=use)
    assert len(ro) == len(o) and not (fo.status == FP.FINAL_UNDECIDED).any()
    decided = np.flatnonzero(~plain_undecided)  # no LP_SOLVE fragment: the fo of the plain call
    assert fo.take(decided).equals(FP.final_host(o, PREC, caps, row_cap, use=plain_use).take(decided))
    idx = np.array([5, 0, 17, 5])
    part = ro.take(idx)
    assert len(part) == 4 and all(np.array_equal(getattr(part, k), getattr(ro, k)[idx]) for k in RB.ROBUST_FIELDS)
    whole = FP.RobustOutcome.concat([ro.take(np.arange(0, 30)), ro.take(np.arange(30, len(ro)))])
    assert whole.equals(ro) and ro.equals(whole)
    blank = FP.RobustOutcome.blank(o)
    assert len(blank) == len(o) and (blank.rgap == FP.NO_GAP).all() and not blank.rbest.any() and not blank.equals(ro)
    assert blank.take(np.flatnonzero(fo.status != FC.SOLVED)).equals(ro.take(np.flatnonzero(fo.status != FC.SOLVED)))
    with pytest.raises(ValueError):
        FP.RobustOutcome.concat([])
    with pytest.raises(ValueError):
        FP.RobustOutcome(n_optional=ro.n_optional[:-1], cstar=ro.cstar, rbest=ro.rbest, rn_opt=ro.rn_opt, rgap=ro.rgap)
    for bad in (0, (1 << 22) + 1):
        with pytest.raises(ValueError, match="max_combos"):
            FP.final_robust_host(o, PREC, caps, row_cap, max_combos=bad)
    with pytest.raises(ValueError):
        FP.final_robust_host(o, PREC, caps, row_cap, use=np.ones(3))
