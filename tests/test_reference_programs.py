"""The host models of the stages that replace a solver call, held to the
REFERENCE's own programs: tests/golden/make_program_golden.py builds
LinearProgramInstance unmodified behind an exact enumeration and records what a
completed solve returns in filter_with_lp, in the last evaluate and in
select_sequence_length_with_lp (program_*.json.gz).  Here align_host /
lp_decisions, final_host / final_robust_host / final_search_host with their
decisions, and length_program_host / length_decisions run on the same inputs,
with the caps read from the table by alignment.lp_caps / lp_row_caps, and every
claim they make is compared with the record (tests/_program_checks.py).  The
replays of _set_x the models are built on are compared with the recorded raise /
no-raise outcome on the whole (min_end, max_end) grid.
tests/test_gpu_reference_programs.py does the same with the kernels."""
import pytest

import _align_cases as AC
import _program_checks as PK


@pytest.fixture(scope="module")
def filt():
    return PK.Family("program_filter.json.gz")


@pytest.fixture(scope="module")
def fin():
    return PK.Family("program_final.json.gz")


@pytest.fixture(scope="module")
def lng():
    return PK.Family("program_length.json.gz")


def test_fixtures_cover_what_they_should(filt, fin, lng):
    """Two thirds of each family carry no tag; the filter grid is whole; the
    float coefficients move no objective by a fixed-point unit."""
    for fam, tags in ((filt, [r["tags"] for s in filt.specs for r in s["records"]]), (fin, [s["tags"] for s in fin.specs]),
                      (lng, [s["tags"] for s in lng.specs])):
        assert 3 * sum(not t for t in tags) >= 2 * len(tags) and len(tags) >= 48
        assert PK.float_effect_is_small(fam)
    for cls in ("START", "END"):
        grid, = [s for s in filt.specs if s.get("grid") == cls]
        assert sorted((f[3], f[4]) for f in grid["frags"]) == [(a, b) for a in range(-1, 5) for b in range(-1, 5)]
    raised = {r["raised"] for s in filt.specs for r in s["records"]}
    assert raised == {None, "IndexError", "KeyError"}
    assert any(r["no_y"] for s in filt.specs for r in s["records"])
    assert {len(s["cands"]) for s in lng.specs} == {1, 2, 3}
    assert any(c["raised"] for s in lng.specs for c in s["cands"]) and any(s["chosen"] == -1 for s in lng.specs)
    assert any(len(r["subset"]) == 2 for s in fin.specs for r in s["subsets"])


def test_replay_set_x_raises_where_the_reference_does(filt):
    """_align_cases.replay_set_x on the whole grid at L == 3: an IndexError
    exactly where the constructor raised, and where it does not raise and an
    end lies outside [0, L - 1] the layer's rule says SKIPPED."""
    n = 0
    for s in filt.specs:
        if not s.get("grid"):
            continue
        for (code, _, _, mn, mx), rec in zip(s["frags"], s["records"]):
            try:
                x = AC.replay_set_x(code, mn, mx, s["L"])
            except IndexError:
                x = None
            assert (x is None) == (rec["raised"] == "IndexError"), (s["grid"], mn, mx, rec)
            assert ("ends" in rec["tags"]) == (not (0 <= mn < s["L"] and 0 <= mx < s["L"]))
            n += 1
    assert n == 72


def test_setx_pattern_raises_where_the_reference_does(lng):
    """length_program.setx_pattern and shape_rule per fragment and candidate:
    a candidate's constructor raised iff some fragment's pattern does."""
    from spectrseqtools_amd import length_program as LP

    n = 0
    for s in lng.specs:
        for c in s["cands"]:
            pats = [LP.setx_pattern((f[0] >> 2) & 3, f[2], f[3], c["c"]) for f in s["frags"]]
            rules = [LP.shape_rule((f[0] >> 2) & 3, f[2], f[3], c["c"]) for f in s["frags"]]
            assert any(p is None for p in pats) == c["raised"] == any(r == LP.RULE_RAISES for r in rules), (s["note"], c)
            n += c["raised"]
    assert n >= 3


@pytest.mark.parametrize("variant", PK.ALIGN_VARIANTS, ids=lambda v: "-".join(k for k, on in v.items() if on) or "plain")
def test_align_host_against_filter_with_lp(filt, variant):
    """alignable == 0 and DROP => removed, KEEP => kept, INFEASIBLE <=> no y,
    SKIPPED <=> an end outside; in keep mode every untagged fragment is decided."""
    from spectrseqtools_amd import alignment

    clean = 0
    for (rates, seq_rate), specs in filt.batches:
        dp = filt.table(rates, seq_rate)
        o = filt.outcome(specs)
        caps, row_cap = PK.caps_of(dp, o)
        al = alignment.align_host(o, filt.tolerance, filt.precision, split=variant["split"],
                                  caps=caps if variant["caps"] else None, keep=row_cap if variant["keep"] else None)
        clean += PK.check_filter(specs, al, alignment.lp_decisions(al), variant, (rates, seq_rate))
    assert clean >= 300


@pytest.mark.parametrize("model,optional", [("final", "none"), ("final", "all"), ("robust", "robust"), ("search", "robust")])
def test_final_host_against_evaluate(fin, model, optional):
    """SOLVED => best within (n_used + 1) fixed-point units of the exact optimum,
    INFEASIBLE <=> infeasible, TAKE => the unique minimiser's names (robust: of
    every subset of the optional fragments), every untagged spectrum TAKE.
    final_host takes no optional fragments: it runs without them and with
    them as required ones, each against that subset's record."""
    from spectrseqtools_amd import final_program as FP

    clean = 0
    for (rates, seq_rate), specs in fin.batches:
        dp = fin.table(rates, seq_rate)
        o = fin.outcome(specs)
        caps, row_cap = PK.caps_of(dp, o)
        use = PK.final_use(specs, optional)
        if model == "final":
            fo = FP.final_host(o, fin.precision, caps, row_cap, use=use)
            dec = FP.final_decisions(fo)
        else:
            if model == "robust":
                fo, ro = FP.final_robust_host(o, fin.precision, caps, row_cap, use=use)
            else:
                fo, ro, so = FP.final_search_host(o, fin.precision, caps, row_cap, use=use, max_combos=0)
                assert set(so.mode[fo.status == PK.F_SOLVED].tolist()) <= {FP.SEARCH_SEARCHED}
            dec = FP.robust_decisions(fo, ro)
        clean += PK.check_final(fin, specs, o, fo, dec, optional, (model, rates, seq_rate), ro_decisions=model != "final")
    assert clean >= 48


def test_length_program_host_against_the_selection_loop(lng):
    """Per candidate INVALID / RAISES as recorded and best within the bound;
    TAKE => the recorded length, NONE / JACCARD <=> -1, every untagged spectrum decided."""
    from spectrseqtools_amd import length_program as LP

    clean = 0
    for (rates, seq_rate), specs in lng.batches:
        dp = lng.table(rates, seq_rate)
        cases = lng.cases(specs)
        lo = LP.length_program_host(cases, lng.precision, LP.length_valid(cases, lng.precision), LP.length_caps(dp, cases))
        decision, length = LP.length_decisions(lo)
        clean += PK.check_length(lng, specs, lo, decision, length, (rates, seq_rate))
    assert clean >= 32
