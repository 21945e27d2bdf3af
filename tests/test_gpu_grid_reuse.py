"""GPU tests of a workgroup's later spectra: the alignment certificate's
kernels (k_align_windows_caps, k_align_windows_keep, k_align_split,
k_align_split_caps, k_align_split_keep; grid 2 x CUs) and k_final_program
(grid 3 x CUs) run one spectrum per workgroup on a persistent grid, so a launch
has to hold several times the grid's spectra before any workgroup resets its
per-spectrum state (the flags, the counters n_forced, row_bad, n_used, have_pos,
the final program's D columns and digit table) or leaves a spectrum early and
goes on to the next.

One base set of B = 199 distinct spectra of every kind (tests/_reuse_cases.py),
the host models once on it, then a launch of 4 * 3 * CUs + 37 spectra gathered
from the base by idx[i] = (i * step) % B: B is prime and unrelated to the grid,
so the spectra one workgroup sees are different base spectra in a varying
order.  The device equals the host model's result gathered by the same idx, in
every array, and the same for the launch reversed: nothing in a spectrum's
result depends on its neighbours."""
from types import SimpleNamespace

import numpy as np
import pytest

import _align_cases as AC
import _align_caps_cases as CC
import _align_keep_cases as KC
import _final_cases as FC
import _reuse_cases as RC
from _align_gpu import FIELDS, K, engine, full_table  # noqa: F401

pytestmark = pytest.mark.gpu
SMALL_COMBOS = 12


@pytest.fixture(scope="module")
def base(full_table, K):  # noqa: F811
    """The base set, its outcome and every host model on it, computed once."""
    from spectrseqtools_amd import alignment, final_program as FP

    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    specs, row_cap = RC.base_set(rm, dp.tolerance, dp.precision)
    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    use = FC.use_array(specs)
    ah = lambda **kw: alignment.align_host(o, dp.tolerance, dp.precision, K, **kw)  # noqa: E731
    fh = lambda mc: FP.final_host(o, dp.precision, caps, row_cap, use=use, max_combos=mc)  # noqa: E731
    return SimpleNamespace(
        specs=specs, rm=rm, o=o, caps=caps, row_cap=row_cap, use=use,
        plain_split=ah(split=True), caps_base=ah(caps=caps), caps_split=ah(caps=caps, split=True),
        keep_base=ah(caps=caps, keep=row_cap), keep_split=ah(caps=caps, keep=row_cap, split=True),
        final=fh(FP.FINAL_DEFAULT_COMBOS), final_small=fh(SMALL_COMBOS))


@pytest.fixture(scope="module")
def launch(engine):  # noqa: F811
    """The compute units of the engine's device, the launch's size and its gather."""
    import torch

    cus = int(torch.cuda.get_device_properties(engine.device).multi_processor_count)
    n = 4 * 3 * cus + 37
    print("compute units", cus, "spectra per launch", n, "align grid", 2 * cus, "final grid", 3 * cus, flush=True)
    assert cus > 0 and n > 4 * (3 * cus) and n > 4 * (2 * cus)
    return SimpleNamespace(cus=cus, n=n, idx=RC.launch_index(n))


def gathered(base, idx):
    """(outcome, caps, use) of the launch that holds base spectra idx, in that order."""
    from spectrseqtools_amd.pipeline_device import _segments

    src, _ = _segments(base.o.frag_off, idx)
    return base.o.take(idx), (base.caps[0], base.caps[1][idx]), base.use[src]


def align(dp, base, idx, want, what, split=False, caps=False, keep=False):
    from spectrseqtools_amd import alignment

    o, caps_n, _ = gathered(base, idx)
    dev = alignment.align_device(dp, o, split=split, caps=caps_n if caps else False,
                                 keep=base.row_cap if keep else False)
    assert np.array_equal(dev.frag_off, o.frag_off) and len(dev) == len(idx)
    want = want.take(idx)
    if keep:
        KC.same7(dev, want, what)
    else:
        assert dev.keep is None
        AC.assert_equal(dev, tuple(getattr(want, k) for k in FIELDS), what)


def final(dp, base, idx, want, what, max_combos):
    from spectrseqtools_amd import final_program as FP

    o, caps_n, use_n = gathered(base, idx)
    got = FP.final_device(dp, o, use=use_n, max_combos=max_combos, caps=caps_n, row_cap=base.row_cap)
    assert np.array_equal(got.frag_off, o.frag_off) and np.array_equal(got.pos_off, o.pos_off)
    FC.assert_equal9(got, want.take(idx), what)


def test_base_set_holds_every_kind(base, launch):
    """Every kind of spectrum is in the base set (floors against a vacuous
    pass), and every base spectrum is in the launch at least four times per
    grid's worth."""
    from spectrseqtools_amd import final_program as FP

    specs, o = base.specs, base.o
    at = RC.kinds(specs, len(base.rm))
    kinds = {k: len(v) for k, v in at.items()}
    spec_of = np.repeat(np.arange(len(specs)), np.diff(o.frag_off))
    per_spec = lambda mask: np.bincount(spec_of[mask], minlength=len(specs))  # noqa: E731
    kb, ks, fin, small = base.keep_base, base.keep_split, base.final, base.final_small
    has_frags = np.diff(o.frag_off) > 0
    open_specs = per_spec(base.caps_base.status == AC.OPEN) > 0
    solved = fin.status == FC.SOLVED
    kinds.update(
        row_free=int(kb.spec_free.sum()), not_row_free=int((has_frags & (kb.spec_free == 0)).sum()),
        final_not_free=int((fin.status == FC.NOT_FREE).sum()), final_skipped=int((fin.status == FC.SKIPPED).sum()),
        final_infeasible=int((fin.status == FC.INFEASIBLE).sum()), final_solved=int(solved.sum()),
        too_large_default=int((fin.status == FC.TOO_LARGE).sum()), too_large_small=int((small.status == FC.TOO_LARGE).sum()),
        align_infeasible=int((per_spec(kb.status == AC.INFEASIBLE) > 0).sum()),
        align_skipped_fragments=int((kb.status == AC.SKIPPED).sum()),
        open_spectra=int(open_specs.sum()), open_fragments=int((base.caps_base.status == AC.OPEN).sum()),
        plain_open_fragments=int((base.plain_split.status == AC.OPEN).sum()),
        open_next_to_none=int((open_specs[1:-1] & ~open_specs[:-2] & ~open_specs[2:]).sum()),
        decided_by_split=int(((base.caps_base.status == AC.OPEN) & (base.caps_split.status != AC.OPEN)).sum()),
        combos_4096=int((solved & (fin.combos == 4096)).sum()), combos_1=int((solved & (fin.combos == 1)).sum()),
        combos_below_256=int((solved & (fin.combos > 1) & (fin.combos < 256)).sum()),
        cap_binds=int((solved & (fin.n_feas < fin.combos)).sum()),
        kept=int(kb.keep.sum()), kept_by_split=int(ks.keep.sum() - kb.keep.sum()),
        fit_not_kept=int(((kb.status == AC.FIT) & (kb.keep == 0) & (kb.spec_free[spec_of] == 1)).sum()),
        misses=int((kb.status == AC.NONE).sum()), fragments=int(o.frag_off[-1]), positions=int(o.pos_off[-1]))
    print("base set", RC.B, "step", RC.STEP, "kinds", kinds, flush=True)
    floors = dict(default=3, empty=3, n_pos=3, bad_end=5, empty_set=10, forced=4, no_cap=2, L0=3, L1=6, L253=1, chunk=1, used_limit=1,
                  row_free=60, not_row_free=25, final_not_free=10, final_skipped=8, final_infeasible=15, final_solved=60,
                  too_large_default=4, too_large_small=10, align_infeasible=15, align_skipped_fragments=10, open_spectra=2,
                  open_fragments=20, plain_open_fragments=14, open_next_to_none=2, decided_by_split=5, combos_4096=2,
                  combos_1=3, combos_below_256=30, cap_binds=3, kept=40, kept_by_split=1, fit_not_kept=10, misses=100)
    # (floors against a vacuous pass only: what is built by hand in full, of the random part about half of what it gives)
    short = {k: (kinds[k], v) for k, v in floors.items() if kinds[k] < v}
    assert not short, short
    assert (fin.status[at["no_cap"]] == FC.INFEASIBLE).all() and (fin.status[at["used_limit"]] == FC.SOLVED).all()
    assert FP.FINAL_DEFAULT_COMBOS > 4096 > SMALL_COMBOS
    assert np.gcd(RC.STEP, RC.B) == 1 and np.bincount(launch.idx, minlength=RC.B).min() >= 4 * 3 * launch.cus // RC.B


def test_align_caps_base_and_split(full_table, base, launch):  # noqa: F811
    """k_align_windows_caps, then k_align_split_caps over it: four arrays each."""
    align(full_table, base, launch.idx, base.caps_base, "caps", caps=True)
    align(full_table, base, launch.idx, base.caps_split, "caps split", caps=True, split=True)


def test_align_keep_base_and_split(full_table, base, launch):  # noqa: F811
    """k_align_windows_keep, then k_align_split_keep over it: seven arrays each."""
    align(full_table, base, launch.idx, base.keep_base, "keep", caps=True, keep=True)
    align(full_table, base, launch.idx, base.keep_split, "keep split", caps=True, keep=True, split=True)


def test_plain_split(full_table, base, launch):  # noqa: F811
    """k_align_split over k_align_windows: four arrays."""
    align(full_table, base, launch.idx, base.plain_split, "plain split", split=True)


@pytest.mark.parametrize("small", [False, True])
def test_final_program(full_table, base, launch, small):  # noqa: F811
    """k_final_program at the default max_combos and at 12 (TOO_LARGE among the rest): nine arrays."""
    from spectrseqtools_amd import final_program as FP

    if small:
        final(full_table, base, launch.idx, base.final_small, "max_combos 12", SMALL_COMBOS)
    else:
        final(full_table, base, launch.idx, base.final, "default max_combos", FP.FINAL_DEFAULT_COMBOS)


def test_reversed_launch(full_table, base, launch):  # noqa: F811
    """The same batch in reverse order through the keep-mode split and the
    final program: every spectrum's result is what it was."""
    from spectrseqtools_amd import final_program as FP

    back = launch.idx[::-1].copy()
    assert not np.array_equal(back, launch.idx)
    align(full_table, base, back, base.keep_split, "keep split, reversed", caps=True, keep=True, split=True)
    final(full_table, base, back, base.final, "final, reversed", FP.FINAL_DEFAULT_COMBOS)
