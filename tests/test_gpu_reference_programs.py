"""GPU tests that hold the kernels which replace a solver call to the
REFERENCE's own programs (tests/golden/make_program_golden.py: program_filter /
program_final / program_length.json.gz, every instance of
LinearProgramInstance solved exactly): align_device in its six variants
against what filter_with_lp did with each fragment, final_device /
final_robust_device / final_search_device against what the last evaluate
returned, length_program_device against select_sequence_length_with_lp's loop.
The device results are compared with the recorded results directly
(tests/_program_checks.py), never through the host models; each family is a few
batches of tiny spectra on one table built over the fixture's masses."""

import pytest

import _program_checks as PK
from _align_gpu import engine  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_table(engine):
    """One table over the fixtures' row masses (the three families share them)."""
    from spectrseqtools_amd import _native

    rm = PK.Family("program_filter.json.gz").row_mass
    assert rm == PK.Family("program_final.json.gz").row_mass == PK.Family("program_length.json.gz").row_mass
    table = _native.DeviceTable.build(rm, max(rm) * 4, 32, engine=engine)
    try:
        yield table
    finally:
        table.close()


@pytest.mark.parametrize("variant", PK.ALIGN_VARIANTS, ids=lambda v: "-".join(k for k, on in v.items() if on) or "plain")
def test_align_device_against_filter_with_lp(device_table, variant):
    """alignable == 0 and DROP => removed, KEEP => kept, INFEASIBLE <=> no y,
    SKIPPED <=> an end outside; in keep mode every untagged fragment is decided."""
    from spectrseqtools_amd import alignment

    filt = PK.Family("program_filter.json.gz")
    clean = 0
    for (rates, seq_rate), specs in filt.batches:
        dp = filt.table(rates, seq_rate, device_table)
        al = alignment.align_device(dp, filt.outcome(specs), **variant)
        assert al.has_keep == variant["keep"]
        clean += PK.check_filter(specs, al, alignment.lp_decisions(al), variant, (rates, seq_rate))
    assert clean >= 300


@pytest.mark.parametrize("kernel,optional", [("final", "none"), ("final", "all"), ("robust", "robust"), ("search", "robust")])
def test_final_device_against_evaluate(device_table, kernel, optional):
    """SOLVED => best within (n_used + 1) fixed-point units of the exact optimum,
    INFEASIBLE <=> infeasible, TAKE => the unique minimiser's names (robust and
    search: of every subset of the optional fragments), every untagged spectrum
    TAKE.  The search runs with max_combos == 0: every spectrum is searched."""
    from spectrseqtools_amd import final_program as FP

    fin = PK.Family("program_final.json.gz")
    clean = 0
    for (rates, seq_rate), specs in fin.batches:
        dp = fin.table(rates, seq_rate, device_table)
        o = fin.outcome(specs)
        use = PK.final_use(specs, optional)
        if kernel == "final":
            fo = FP.final_device(dp, o, use=use)
            dec = FP.final_decisions(fo)
        else:
            if kernel == "robust":
                fo, ro = FP.final_robust_device(dp, o, use=use)
            else:
                fo, ro, so = FP.final_search_device(dp, o, use=use, max_combos=0)
                assert set(so.mode[fo.status == PK.F_SOLVED].tolist()) <= {FP.SEARCH_SEARCHED}
            dec = FP.robust_decisions(fo, ro)
        clean += PK.check_final(fin, specs, o, fo, dec, optional, (kernel, rates, seq_rate), ro_decisions=kernel != "final")
    assert clean >= 48


def test_length_program_device_against_the_selection_loop(device_table):
    """Per candidate INVALID / RAISES as recorded and best within the bound;
    TAKE => the recorded length, NONE / JACCARD <=> -1, every untagged spectrum decided."""
    from spectrseqtools_amd import length_program as LP

    lng = PK.Family("program_length.json.gz")
    clean = 0
    for (rates, seq_rate), specs in lng.batches:
        dp = lng.table(rates, seq_rate, device_table)
        lo = LP.length_program_device(dp, lng.cases(specs))
        decision, length = LP.length_decisions(lo)
        clean += PK.check_length(lng, specs, lo, decision, length, (rates, seq_rate))
    assert clean >= 32
