"""CPU tests of the bounded search's host model (final_program.
final_search_host, SearchOutcome; include/sst.h, sst_final_search_device): the
search against the enumeration (final_robust_host, which
tests/test_final_robust_model.py holds to the brute force) with gap and rgap
truncated at the horizon, the bound against its definition taken literally,
the width limit, the widening rounds by hand-computed thresholds, and spectra
the enumeration cannot reach."""
import itertools

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
import _final_cases as FC
import _robust_cases as RB
import _search_cases as SC
from spectrseqtools_amd import final_program as FP
from test_align_keep_model import ALPHABETS, PREC, TOL
from test_final_robust_model import random_cases

FIX = FC.FIX


@pytest.fixture(scope="module")
def cases():
    """The 420 spectra of the robust model test with final_robust_host's result (computed once, left unchanged)."""
    return [(rm, specs, row_cap, RB.host(specs, rm, row_cap, PREC)) for rm, specs, row_cap in random_cases()]


@pytest.mark.parametrize("H", [1 << 17, 0, 300])
def test_search_against_the_enumeration(cases, H):
    """max_combos = 0: every modelled spectrum is searched.  All fourteen
    arrays equal final_robust_host's with gap and rgap replaced by min(., H + 1)
    -- n_feas included: the count over modified rows against the enumeration's."""
    solved = with_optional = cut = infeasible = 0
    for rm, specs, row_cap, ref in cases:
        assert not (ref[0].status == FC.TOO_LARGE).any()
        fo, ro, so = SC.host(specs, rm, row_cap, PREC, 0, horizon=H)
        RB.assert_equal14((fo, ro), SC.truncated(ref, H), (H, rm))
        ok = fo.status == FC.SOLVED
        assert (so.mode[ok] == FP.SEARCH_SEARCHED).all() and (so.rounds[ok] >= 1).all() and so.horizon == H
        assert not so.mode[~ok].any() and not so.rounds[~ok].any() and not so.nodes[~ok].any()
        solved += int(ok.sum())
        with_optional += int((ro.n_optional[ok] > 0).sum())
        cut += int((ref[0].gap[ok] > np.uint64(H + 1)).sum())
        infeasible += int(((fo.status == FC.INFEASIBLE) & (fo.combos > 0)).sum())
    print("H", H, "solved", solved, "with optional", with_optional, "gap cut at H + 1", cut, "n_feas == 0", infeasible,
          flush=True)
    # (floors against a vacuous pass only: about half of what this generator gives)
    assert solved >= 110 and with_optional >= 55 and cut >= 50, (solved, with_optional, cut)


def test_mixed_paths(cases):
    """max_combos = 12: the enumerated spectra equal final_robust_host at 12
    byte for byte, the searched ones its result at the default, truncated
    where SOLVED and as it is where not (n_feas == 0); mode tells the two apart."""
    enumerated = searched = unsolved = 0
    for rm, specs, row_cap, ref in cases:
        small = RB.host(specs, rm, row_cap, PREC, 12)
        fo, ro, so = SC.host(specs, rm, row_cap, PREC, 12)
        ok = fo.status == FC.SOLVED
        by_mode = np.where(ok, np.where(fo.combos <= 12, FP.SEARCH_ENUMERATED, FP.SEARCH_SEARCHED), 0)
        assert np.array_equal(so.mode, by_mode)
        one = np.flatnonzero(so.mode != FP.SEARCH_SEARCHED)  # enumerated, or not solved on either path
        two = np.flatnonzero(so.mode == FP.SEARCH_SEARCHED)
        above = small[0].status[one] == FC.TOO_LARGE
        keep, rest = one[~above], one[above]  # rest: searched and not SOLVED (no sweep overflows at these sizes)
        assert fo.take(keep).equals(small[0].take(keep)) and ro.take(keep).equals(small[1].take(keep))
        assert (fo.status[rest] == FC.INFEASIBLE).all()
        assert fo.take(rest).equals(ref[0].take(rest)) and ro.take(rest).equals(ref[1].take(rest))
        unsolved += len(rest)
        want = SC.truncated((ref[0].take(two), ref[1].take(two)), so.horizon)
        RB.assert_equal14((fo.take(two), ro.take(two)), want, "searched")
        assert not so.rounds[one].any() and not so.nodes[one].any()
        enumerated += int((so.mode == FP.SEARCH_ENUMERATED).sum())
        searched += len(two)
    # (floors against a vacuous pass only: about half of what this generator gives)
    print("enumerated", enumerated, "searched and SOLVED", searched, "searched and INFEASIBLE", unsolved, flush=True)
    assert enumerated >= 95 and searched >= 18, (enumerated, searched)


def _small_search(spec, rm):
    """(_Search, sets, use, outcome) of one small modelled spectrum."""
    o = AC.make_outcome([spec], rm)
    row_mod, mod_cap = CC.caps_of([spec], len(rm))
    use = RB.use3_array([spec])
    on = np.flatnonzero(use)
    cls = (o.frag_code[on].astype(np.int64) >> 2) & 3
    q = np.array([FC.qfix(su, PREC) for su in o.frag_su[on]], dtype=np.int64)
    sets = CC.position_rows(spec, len(rm))
    s = FP._Search(spec["L"], sets, rm, row_mod, int(mod_cap[0]), cls, q, o.frag_min_end[on].astype(np.int64),
                   o.frag_max_end[on].astype(np.int64), use[on] == 2, 1 << 16)
    return s, sets, on, q


def test_the_bound_taken_literally():
    """On small spectra (L <= 6), for every node: lb equals a brute force over
    the admissible intervals (_align_cases.admissible_intervals), is at most
    the objective of every feasible leaf below it (itertools.product), does not
    exceed any child's, and equals obj at a leaf -- for the required bound and
    for the capped one with optional fragments."""
    checked = capped = 0
    for k, rm in enumerate(ALPHABETS):
        specs, row_cap = RB.random_robust_case(3100 + k, rm, TOL, PREC, 70)
        ref = RB.host(specs, rm, row_cap, PREC)
        for g, spec in enumerate(specs):
            if ref[0].status[g] != FC.SOLVED or spec["L"] > 6 or ref[0].combos[g] > 300:
                continue
            s, sets, on, q = _small_search(spec, rm)
            L = spec["L"]
            frags = [spec["frags"][j] for j in on]
            ivs = [AC.admissible_intervals(f[0], f[3], f[4], L) for f in frags]
            mass = lambda r: int(rm[r])  # noqa: E731
            y_star = ref[0].seq[AC.make_outcome(specs, rm).pos_off[g]:][:L].tolist()

            def cost(y, j):
                return min(abs(int(q[j]) - FIX * sum(mass(y[i]) for i in (range(l, r + 1) if l != 0xFF else ())))
                           for l, r in ivs[j])

            c_star = [cost(y_star, j) for j in range(len(frags))]

            def literal(fixed, with_cap):
                """lb of the node that fixes `fixed` at the first free positions, by the definition"""
                row_at = dict(zip(s.free, fixed))
                lo = [mass(row_at[p]) if p in row_at else min(mass(r) for r in sets[p]) for p in range(L)]
                hi = [mass(row_at[p]) if p in row_at else max(mass(r) for r in sets[p]) for p in range(L)]
                total = 0
                for j in range(len(frags)):
                    if s.optional[j] and not with_cap:
                        continue
                    d = min(abs(int(q[j])) if l == 0xFF else
                            max(0, FIX * sum(lo[l:r + 1]) - int(q[j]), int(q[j]) - FIX * sum(hi[l:r + 1])) for l, r in ivs[j])
                    total += min(d, c_star[j]) if s.optional[j] else d
                return total

            def leaf_objective(y, with_cap):
                return sum((min(cost(y, j), c_star[j]) if s.optional[j] else cost(y, j)) for j in range(len(frags))
                           if with_cap or not s.optional[j])

            feasible = [y for y in itertools.product(*sets)
                        if sum(int(spec["row_mod"][r]) for r in y) <= spec["mod_cap"]]
            for with_cap in (False, True) if s.optional.any() else (False,):
                cap = np.where(s.optional, np.array(c_star, dtype=np.int64), np.iinfo(np.int64).max) if with_cap else None
                lb_of = {}
                for d in range(len(s.free) + 1):
                    nodes = list(itertools.product(*[sets[p] for p in s.free[:d]]))
                    got = s.bound(np.array(nodes, dtype=np.int64).reshape(len(nodes), d), cap)
                    for node, lb in zip(nodes, got.tolist()):
                        assert lb == literal(node, with_cap), (k, g, node, with_cap)
                        below = [leaf_objective(y, with_cap) for y in feasible
                                 if all(y[p] == r for p, r in zip(s.free, node))]
                        assert not below or lb <= min(below), (k, g, node)
                        if d:
                            assert lb_of[node[:-1]] <= lb, (k, g, node)
                        if d == len(s.free):
                            y = [dict(zip(s.free, node)).get(p, sets[p][0]) for p in range(L)]
                            assert lb == leaf_objective(y, with_cap), (k, g, node)
                        lb_of[node] = lb
                        checked += 1
                capped += with_cap
    print("nodes checked", checked, "spectra with the capped bound", capped, flush=True)
    assert checked >= 2000 and capped >= 20, (checked, capped)


def test_width(cases):
    """A max_width that some level of some spectrum exceeds by one: exactly the
    spectra with a wider level become TOO_LARGE, nothing else changes; a level
    of exactly max_width is no overflow."""
    hit = exact = 0
    for rm, specs, row_cap, _ in cases:
        full = SC.host(specs, rm, row_cap, PREC, 0)
        widths = set(full[2].widest.tolist())
        W = next((w for w in sorted(widths) if w >= 2 and w + 1 in widths), None)
        if W is None:
            continue
        fo, ro, so = SC.host(specs, rm, row_cap, PREC, 0, max_width=W)
        over = full[2].widest > W
        assert (fo.status[over] == FC.TOO_LARGE).all() and not so.mode[over].any() and not so.nodes[over].any()
        assert (ro.rgap[over] == FP.NO_GAP).all() and not fo.n_feas[over].any() and (fo.combos[over] > 0).all()
        same = np.flatnonzero(~over)
        SC.assert_equal17(tuple(x.take(same) for x in (fo, ro, so)), tuple(x.take(same) for x in full), W)
        hit += int((full[2].widest == W + 1).sum())
        exact += int((full[2].widest == W).sum())
    assert hit >= 3 and exact >= 3, (hit, exact)


@pytest.mark.parametrize("H_units,offset,rounds,nodes", [(1, 20, 4, 3), (8, 30, 3, 6), (8, 20, 2, 3)])
def test_widening_rounds(H_units, offset, rounds, nodes):
    """One START_END fragment `offset` precision units above the largest
    reachable total over three positions of two rows: best = offset * 65536, and
    only the path of upper rows stays within any threshold below best + (mass
    difference) * 65536.  H = 65536, offset 20 (best above 16 H): the thresholds
    1, 4, 16 units keep no node, 64 keeps the path (4 sweeps, 3 nodes), and
    21 <= 64 asks for no further sweep.  H = 8 units, offset 30: 8 keeps
    nothing, 32 the path, and 30 + 8 > 32 forces the sweep at 38 (3 sweeps, 6
    nodes).  H = 8 units, offset 20: 8, then 32 >= 28 (2 sweeps, 3 nodes)."""
    rm = FC.synthetic_masses(12)
    spec, lo, hi = SC.offset_spec(rm, PREC, offset)
    assert (rm[hi] - rm[lo]) > 64
    H = H_units * FIX
    fo, ro, so = SC.host([spec], rm, KC.loose_row_cap(len(rm)), PREC, 0, horizon=H)
    assert fo.status.tolist() == [FC.SOLVED] and fo.best.tolist() == [offset * FIX] and fo.seq.tolist() == [hi] * 3
    assert so.rounds.tolist() == [rounds] and so.nodes.tolist() == [nodes] and so.mode.tolist() == [2]
    assert fo.gap.tolist() == [H + 1] and fo.n_opt.tolist() == [1] and fo.n_feas.tolist() == [8]


def test_beyond_the_enumeration():
    """Planted ladders of 2^40 and 2^44 assignments (24 positions, 20 and 22
    free over 4 rows, START and END pins with ranges of ends and +-3 units of
    noise), one with optional fragments: SOLVED; best is the objective of seq by
    the literal cost; every y that differs from seq in one position has an
    objective of at least best + gap."""
    rm = FC.synthetic_masses(40)
    rng = np.random.default_rng(606)
    specs = [SC.ladder_spec(rm, PREC, rng, n_free=20)[0], SC.ladder_spec(rm, PREC, rng, n_free=22, spread=2)[0],
             SC.ladder_spec(rm, PREC, rng, n_free=20, n_optional=6)[0]]
    fo, ro, so = SC.host(specs, rm, KC.loose_row_cap(len(rm)), PREC)
    o = AC.make_outcome(specs, rm)
    print("rounds", so.rounds.tolist(), "nodes", so.nodes.tolist(), "widest", so.widest.tolist(), flush=True)
    assert fo.status.tolist() == [FC.SOLVED] * 3 and so.mode.tolist() == [2] * 3
    assert fo.combos.tolist() == [1 << 40, 1 << 44, 1 << 40] and fo.n_feas.tolist() == fo.combos.tolist()
    assert ro.n_optional.tolist() == [0, 0, 6]
    for g, spec in enumerate(specs):
        seq = fo.seq[o.pos_off[g]:o.pos_off[g + 1]].tolist()
        best, gap = int(fo.best[g]), int(fo.gap[g])
        assert best == SC.literal_objective(spec, rm, PREC, seq) and fo.n_opt[g] == 1 and gap >= 1
        for p, rows in enumerate(CC.position_rows(spec, len(rm))):
            for r in rows:
                if r != seq[p]:
                    assert SC.literal_objective(spec, rm, PREC, seq[:p] + [r] + seq[p + 1:]) >= best + gap, (g, p, r)
    assert ro.rbest[2] <= fo.best[2] + ro.cstar[2]


def test_a_spectrum_at_the_enumeration_limit():
    """One spectrum of exactly 2^22 assignments, the most final_host takes (about
    8 s of enumeration here): the search equals it, gap truncated."""
    rm = FC.synthetic_masses(40)
    spec, _ = SC.ladder_spec(rm, PREC, np.random.default_rng(607), L=12, n_free=11, spread=1)
    row_cap = KC.loose_row_cap(len(rm))
    want = FC.host([spec], rm, row_cap, PREC, max_combos=1 << 22)
    fo, ro, so = SC.host([spec], rm, row_cap, PREC)
    assert want.status.tolist() == [FC.SOLVED] and want.combos.tolist() == [1 << 22] and so.mode.tolist() == [2]
    want.gap[:] = np.minimum(want.gap, np.uint64(so.horizon + 1))
    FC.assert_equal9(fo, want, "2^22")
