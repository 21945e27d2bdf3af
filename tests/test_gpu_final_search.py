"""GPU tests of the bounded search (sst_final_search_device: k_final_robust,
k_final_search_list and k_final_search in csrc/sst_final.hip;
final_program.final_search_device, run_batch(align_search=True)): the device
result equals final_program.final_search_host in all seventeen arrays -- which
tests/test_final_search_model.py holds to the enumeration and to the
definition -- on random spectra, on a batch that takes both paths, and on the
smallest shapes at which the sweep can go wrong."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
import _final_cases as FC
import _robust_cases as RB
import _search_cases as SC
from _align_gpu import engine, full_table  # noqa: F401
from conftest import load_golden
from test_gpu_final import CHUNK, WG, device_args, masses_of

pytestmark = pytest.mark.gpu

PREC = 0.001


def run(dp, specs, rm, row_cap=None, max_combos=0, what="", **kw):
    """(outcome, FinalOutcome, RobustOutcome, SearchOutcome, the host's SearchOutcome) of a case on the device;
    asserts it equal to the host model in all seventeen arrays."""
    from spectrseqtools_amd import final_program as FP

    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    row_cap = KC.loose_row_cap(len(rm)) if row_cap is None else row_cap
    use = RB.use3_array(specs)
    want = FP.final_search_host(o, dp.precision, caps, row_cap, use=use, max_combos=max_combos, **kw)
    got = FP.final_search_device(dp, o, use=use, max_combos=max_combos, caps=caps, row_cap=row_cap, **kw)
    assert np.array_equal(got[0].frag_off, o.frag_off) and np.array_equal(got[0].pos_off, o.pos_off)
    SC.assert_equal17(got, want, what)
    return (o,) + got + (want[2],)


@pytest.fixture(scope="module")
def synth_table(engine):  # noqa: F811
    """A table of 120 rows over _final_cases.synthetic_masses: rows 100 .. 119 count as modified in the cases below."""
    from spectrseqtools_amd import _native

    rm = FC.synthetic_masses(120)
    table = _native.DeviceTable.build(rm, max(rm) * 4, 32, engine=engine)
    yield SimpleNamespace(masses=[SimpleNamespace(mass=m) for m in rm], device_table=table, precision=PREC,
                          tolerance=1e-5)
    table.close()


ROW_MOD = np.array([0] * 100 + [1] * 20, dtype=np.uint8)
ZERO = (FC.INTERNAL, 0.0, 100.0, 0, 0)  # lb_j == 0 at every node: every live-feasible node survives


def test_random_spectra_all_searched(full_table):  # noqa: F811
    """200 random spectra with a random 0 / 1 / 2 use per fragment over the
    real masses, default spectra among them, at max_combos = 0: every modelled
    spectrum is searched, at the default horizon, at 0 and at a width of 3."""
    from spectrseqtools_amd import final_program as FP

    dp = full_table
    rm = masses_of(dp)
    specs, row_cap = RB.random_robust_case(77, rm, dp.tolerance, dp.precision, 200)
    for at in (3, 100, 199):
        specs.insert(at, {"default": True})
    _, fo, ro, so, _ = run(dp, specs, rm, row_cap, what="H default")
    ok = fo.status == FC.SOLVED
    assert set(fo.status.tolist()) == {FC.NONE, FC.SOLVED, FC.INFEASIBLE, FC.SKIPPED, FC.NOT_FREE}
    assert (so.mode[ok] == FP.SEARCH_SEARCHED).all() and ok.sum() >= 60 and (ro.n_optional[ok] > 0).sum() >= 30
    run(dp, specs, rm, row_cap, what="H 0", horizon=0)
    _, narrow, _, _, _ = run(dp, specs, rm, row_cap, what="width 3", max_width=3)
    assert (narrow.status == FC.TOO_LARGE).sum() >= 10 and (narrow.status == FC.SOLVED).sum() >= 30


def test_mixed_batch(full_table):  # noqa: F811
    """max_combos = 16: both paths in one call; the enumerated spectra also
    equal sst_final_robust_device byte for byte, and two identical calls give
    identical arrays."""
    from spectrseqtools_amd import final_program as FP

    dp = full_table
    rm = masses_of(dp)
    specs, row_cap = RB.random_robust_case(79, rm, dp.tolerance, dp.precision, 200)
    o, fo, ro, so, _ = run(dp, specs, rm, row_cap, 16, "mixed")
    caps, use = CC.caps_of(specs, len(rm)), RB.use3_array(specs)
    r_fo, r_ro = FP.final_robust_device(dp, o, use=use, max_combos=16, caps=caps, row_cap=row_cap)
    one = np.flatnonzero(so.mode == FP.SEARCH_ENUMERATED)
    assert np.array_equal(one, np.flatnonzero(r_fo.status == FC.SOLVED))
    for k in FC.FIELDS:
        assert getattr(fo.take(one), k).tobytes() == getattr(r_fo.take(one), k).tobytes(), k
    assert ro.take(one).equals(r_ro.take(one))
    # (floors against a vacuous pass only: half of what this generator gives)
    assert len(one) >= 50 and (so.mode == FP.SEARCH_SEARCHED).sum() >= 7
    again = FP.final_search_device(dp, o, use=use, max_combos=16, caps=caps, row_cap=row_cap)
    assert all(x.equals(y) for x, y in zip(again, (fo, ro, so)))


def _level_spec(rm, n_unmod, n_mod, tail=()):
    """Position 0: one unmodified and three modified rows; position 1: n_unmod
    unmodified and n_mod modified rows; mod_cap 1 and one fragment of lb 0: the
    second level holds 4 n_unmod + n_mod nodes (255 = 4 * 63 + 3, 256 = 4 * 64,
    257 = 4 * 64 + 1).  tail: further positions' rows."""
    sets = [[1, 100, 101, 102], list(range(2, 2 + n_unmod)) + list(range(103, 103 + n_mod))] + [list(t) for t in tail]
    return FC.loose_spec(rm, sets, [ZERO], mod_cap=1, row_mod=ROW_MOD)


def test_levels_around_a_workgroup_and_the_width(synth_table):
    """A level of 255, 256 and 257 survivors (one round of a 256-lane workgroup
    and one more), read back as parents by a further level; at max_width = 256
    the level of 256 is no overflow and the one of 257 is TOO_LARGE."""
    dp = synth_table
    rm = masses_of(dp)
    shapes = [(63, 3), (64, 0), (64, 1)]
    specs = [_level_spec(rm, u, m) for u, m in shapes] + [_level_spec(rm, u, m, tail=[(70, 71, 104)]) for u, m in shapes]
    _, fo, _, so, host = run(dp, specs, rm, what="levels")
    # (the tail adds two unmodified rows and a modified one: 3 children of a node without a modified row, 2 of the others)
    assert host.widest.tolist() == [255, 256, 257] + [9 * u + 2 * m for u, m in shapes]
    assert fo.status.tolist() == [FC.SOLVED] * 6 and fo.n_feas.tolist() == host.widest.tolist()
    assert so.nodes[:3].tolist() == [4 + 255, 4 + 256, 4 + 257] and so.rounds.tolist() == [1] * 6 and WG == 256
    _, fo, _, so, _ = run(dp, specs[:3], rm, what="width 256", max_width=256)
    assert fo.status.tolist() == [FC.SOLVED, FC.SOLVED, FC.TOO_LARGE] and so.nodes.tolist() == [259, 260, 0]
    assert fo.combos.tolist() == [4 * 66, 4 * 64, 4 * 65]


def test_free_position_limits(synth_table):
    """48 free positions are searched, 49 are TOO_LARGE; one free position of
    all 119 rows of the largest table (SST_MAX_ROWS = 120: a set has no more)."""
    dp = synth_table
    rm = masses_of(dp)
    rng = np.random.default_rng(11)
    specs = [FC.pinned_binary_spec(rm, n, rng.integers(0, 2, n).tolist(), dp.precision)[0] for n in (48, 49)]
    wide = [list(range(1, 120)), [5], [7, 9]]
    specs.append(FC.loose_spec(rm, wide, FC.random_frags(rng, rm, wide, 9, dp.precision)))
    _, fo, _, so, _ = run(dp, specs, rm, what="free positions")
    assert fo.status.tolist() == [FC.SOLVED, FC.TOO_LARGE, FC.SOLVED] and fo.combos.tolist() == [1 << 48, 1 << 49, 238]
    assert fo.n_feas.tolist() == [1 << 48, 0, 238] and so.mode.tolist() == [2, 0, 2] and fo.n_opt[0] == 1


def test_lengths_and_chunks(full_table):  # noqa: F811
    """L of 0, 1 and 253; 513 and 1025 fragments with optional ones at the
    records' chunk borders (the search holds 256 records at a time); optional
    fragments with cap(y) < cap(y*); every class of optional fragment."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(98)
    zero, want, _ = FC.zero_length_specs(rm, dp.precision)
    zero = [RB.mark(s, (0, 2)) for s in zero[:2]] + [RB.mark(zero[2], (4,)), RB.mark(zero[3], (1,), unused=(4,))]
    ones = [RB.every_third_optional(FC.loose_spec(rm, sets, FC.random_frags(rng, rm, sets, 9, dp.precision)))
            for sets in ([[5]], [[1, 2]], [[3, 4, 6]])]
    lng = RB.every_third_optional(FC.long_spec(rm, dp.precision, rng, n_frags=16, free_at=(0, 126, 252)))
    chunks = RB.chunk_border_specs(rm, dp.precision, rng, CHUNK)
    pulls, _, _ = RB.pull_specs(rm, dp.precision)
    kinds = RB.class_specs(rm, dp.precision, rng)
    o, fo, ro, so, _ = run(dp, zero + ones + [lng] + chunks + pulls + kinds, rm, what="lengths")
    n = len(zero) + len(ones) + 1
    assert fo.status[:n].tolist() == want + [FC.SOLVED] * 4 and fo.combos[n - 1] == 27
    assert so.mode[:n].tolist() == [2, 2, 0, 2] + [2] * 4 and so.nodes[:2].tolist() == [0, 0]
    assert fo.status[n:].tolist() == [FC.SOLVED] * (len(chunks) + len(pulls) + len(kinds))
    assert np.diff(o.frag_off)[n:n + 6].tolist() == [CHUNK + 1] * 3 + [2 * CHUNK + 1] * 3
    at = n + len(chunks)
    assert ro.rbest[at] < fo.best[at] + ro.cstar[at]  # cap(y) < cap(y*)


@pytest.mark.parametrize("n_rows", [64, 65, 120])
def test_row_count_edges(engine, n_rows):  # noqa: F811
    """Tables of 64, 65 and 120 rows with bits set for rows that do not exist, every third used fragment optional."""
    from spectrseqtools_amd import _native

    rm, specs, row_cap = FC.row_edge_case(n_rows, PREC, np.random.default_rng(95))
    specs = [RB.every_third_optional(s) for s in specs]
    table = _native.DeviceTable.build(rm, max(rm) * 4, 32, engine=engine)
    dp = SimpleNamespace(masses=[SimpleNamespace(mass=m) for m in rm], device_table=table, precision=PREC, tolerance=1e-5)
    try:
        _, fo, ro, so, _ = run(dp, specs, rm, row_cap)
        assert fo.status[:2].tolist() == [FC.SOLVED] * 2 and fo.status[5] == FC.INFEASIBLE and fo.status[6] == FC.NOT_FREE
        assert (ro.n_optional[:2] > 0).all() and so.mode[:2].tolist() == [2, 2]
    finally:
        table.close()


def test_mod_cap_binds_through_unavoidable_rows(synth_table):
    """One modified one-row position and two free positions of modified rows
    only: at mod_cap 3 the two mixed positions before them must both take their
    unmodified row (a child with a modified row is not live-feasible), at 4 one
    of them may, at 2 nothing is feasible."""
    dp = synth_table
    rm = masses_of(dp)
    sets = [[1, 100], [2, 101], [102, 103], [104, 105], [106]]
    rng = np.random.default_rng(12)
    frags = FC.random_frags(rng, rm, sets, 10, dp.precision) + [ZERO]
    specs = [FC.loose_spec(rm, sets, frags, mod_cap=c, row_mod=ROW_MOD) for c in (3, 4, 2, 5)]
    _, fo, _, so, host = run(dp, specs, rm, what="mod_cap")
    assert fo.status.tolist() == [FC.SOLVED, FC.SOLVED, FC.INFEASIBLE, FC.SOLVED] and fo.n_feas.tolist() == [4, 12, 0, 16]
    assert fo.seq[:2].tolist() == [1, 2] and fo.combos.tolist() == [16] * 4


@pytest.mark.parametrize("H_units,offset,rounds,nodes", [(1, 20, 4, 3), (8, 30, 3, 6), (8, 20, 2, 3)])
def test_widening_rounds(synth_table, H_units, offset, rounds, nodes):
    """The hand-computed thresholds of tests/test_final_search_model.py::test_widening_rounds on the device."""
    dp = synth_table
    rm = masses_of(dp)
    spec, lo, hi = SC.offset_spec(rm, dp.precision, offset)
    _, fo, _, so, _ = run(dp, [spec], rm, horizon=H_units * FC.FIX)
    assert fo.best.tolist() == [offset * FC.FIX] and so.rounds.tolist() == [rounds] and so.nodes.tolist() == [nodes]


def test_planted_ladders(synth_table):
    """Planted ladders of 2^40 and 2^44 assignments, one with optional fragments: SOLVED, far beyond the enumeration."""
    dp = synth_table
    rm = masses_of(dp)
    rng = np.random.default_rng(606)
    specs = [SC.ladder_spec(rm, dp.precision, rng, n_free=20)[0], SC.ladder_spec(rm, dp.precision, rng, n_free=22, spread=2)[0],
             SC.ladder_spec(rm, dp.precision, rng, n_free=20, n_optional=6)[0]]
    _, fo, ro, so, _ = run(dp, specs, rm, what="ladders")
    assert fo.status.tolist() == [FC.SOLVED] * 3 and fo.combos.tolist() == [1 << 40, 1 << 44, 1 << 40]
    assert ro.n_optional.tolist() == [0, 0, 6] and (so.rounds >= 2).all()


def test_later_spectra_of_a_workgroup(full_table, engine):  # noqa: F811
    """n = 4 * 2 * CUs + 37 spectra gathered from 61 base spectra that alternate
    between the two paths, between spectra with and without optional fragments
    and between the statuses, forward and reversed: every search workgroup
    (two per CU) runs several spectra, and a spectrum's result is what it is
    alone.  The reversed run fails if any per-spectrum state (the optional
    count, the cstar accumulator, P*, the frontier) survives the spectrum loop."""
    import torch

    from spectrseqtools_amd import final_program as FP
    from spectrseqtools_amd.pipeline_device import _segments

    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(99)
    specs, row_cap = RB.random_robust_case(4243, rm, dp.tolerance, dp.precision, 48)
    row_mod = specs[0]["row_mod"]
    hand = [RB.chunk_border_specs(rm, dp.precision, rng, CHUNK)[5], RB.robust_tie(rm, dp.precision)[0]] + \
        RB.pull_specs(rm, dp.precision)[0] + RB.class_specs(rm, dp.precision, rng)[-3:] + \
        [FC.loose_spec(rm, [[1, 2], [3, 4]], FC.random_frags(rng, rm, [[1, 2], [3, 4]], 7, dp.precision))] * 3
    hand = [dict(s, row_mod=row_mod, mod_cap=s["L"]) for s in hand]
    base = [s for pair in zip(specs[:len(hand)], hand) for s in pair] + specs[len(hand):]
    base.insert(9, {"default": True})
    o = AC.make_outcome(base, rm)
    caps = CC.caps_of(base, len(rm))
    use = RB.use3_array(base)
    want = FP.final_search_host(o, dp.precision, caps, row_cap, use=use, max_combos=2)
    ok = want[0].status == FC.SOLVED
    two = want[2].mode == FP.SEARCH_SEARCHED
    # (floors against a vacuous base set only: 10 and 9 searched spectra with and without optional fragments, 15 enumerated)
    assert ((want[1].n_optional > 0) & two).sum() >= 5 and ((want[1].n_optional == 0) & two).sum() >= 4
    assert (ok & ~two).sum() >= 7 and len(set(want[0].status.tolist())) >= 4

    cus = int(torch.cuda.get_device_properties(engine.device).multi_processor_count)
    n = 4 * 2 * cus + 37
    idx = (np.arange(n, dtype=np.int64) * 23) % len(base)
    for order in (idx, idx[::-1].copy()):
        src, _ = _segments(o.frag_off, order)
        got = FP.final_search_device(dp, o.take(order), use=use[src], max_combos=2, caps=(caps[0], caps[1][order]),
                                     row_cap=row_cap)
        SC.assert_equal17(got, tuple(x.take(order) for x in want), "later spectra")


def test_entry_point_contract(full_table):  # noqa: F811
    """SST_E_ARG with a message for a NULL struct, a NULL member with n_spec >
    0 (the three new pointers included), max_width of 0 or above the limit,
    horizon above 2^62 and max_combos above the limit; max_combos = 0 and n_spec
    == 0 are SST_OK; the raw call over poisoned outputs equals
    final_search_device; the limit, the profile id and sst_ctx_trim."""
    import torch

    from spectrseqtools_amd import _native
    from spectrseqtools_amd import final_program as FP

    OK, E_ARG = 0, -1  # SST_OK, SST_E_ARG
    dp = full_table
    eng = dp.device_table.engine
    lib, handle = eng._lib, dp.device_table.handle
    rm = masses_of(dp)
    specs, _ = FC.random_final_case(78, rm, dp.tolerance, dp.precision, 60)
    for s in specs:
        s["use"], s["row_mod"], s["mod_cap"] = None, np.zeros(len(rm), np.uint8), s["L"]
    specs.append({"default": True})
    o = AC.make_outcome(specs, rm)
    base, ins, outs = device_args(dp, o, max_combos=8)
    dev = torch.device("cuda", eng.device)
    S = len(o)
    more = [torch.zeros(S, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64, torch.int32, torch.int64,
                                                            torch.uint8, torch.int32, torch.int64)]
    a = _native.FinalSearchArgs()
    a.robust.base = base
    r = a.robust
    r.n_optional, r.cstar, r.rbest, r.rn_opt, r.rgap, a.mode, a.rounds, a.nodes = (x.data_ptr() for x in more)
    a.horizon, a.max_width = 1 << 17, 1 << 12
    fn = lib.sst_final_search_device
    assert lib.sst_final_search_max_width() == FP.SEARCH_MAX_WIDTH == 1 << 16
    results = []
    for fill in (0x5A, 0xC3):
        for x in outs + more:
            x.view(dtype=torch.uint8).fill_(fill)
        eng.synchronize()
        eng.check(fn(handle, ctypes.byref(a)), "final search")
        eng.synchronize()
        results.append([x.cpu().numpy().copy() for x in outs + more])
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    want = FP.final_search_device(dp, o, max_combos=8, caps=(np.zeros(len(rm), np.uint8), o.seq_len.astype(np.int32)),
                                  row_cap=KC.loose_row_cap(len(rm)))
    dts = (np.uint8, np.uint64, np.uint64, np.uint64, np.uint32, np.uint64, np.uint8, np.uint16, np.uint32,
           np.uint32, np.uint64, np.uint64, np.uint32, np.uint64, np.uint8, np.uint32, np.uint64)
    raw = [x.view(dt) for x, dt in zip(results[0], dts)]
    RB.assert_equal14(want[:2], tuple(raw[:14]), "raw call")
    assert all(np.array_equal(getattr(want[2], k), x) for k, x in zip(SC.SEARCH_FIELDS, raw[14:]))
    assert set(want[2].mode.tolist()) == {0, 1, 2}

    assert fn(None, ctypes.byref(a)) == E_ARG
    assert fn(handle, None) == E_ARG
    with pytest.raises(_native.EngineError, match="NULL sst_final_search_args"):
        eng.check(E_ARG, "final search")
    empty = _native.FinalSearchArgs()
    empty.robust.base.n_spec, empty.robust.base.prec, empty.max_width = 0, dp.precision, 1
    assert fn(handle, ctypes.byref(empty)) == OK  # nothing to do, no array is read; max_combos == 0
    empty.robust.base.n_spec = 1
    assert fn(handle, ctypes.byref(empty)) == E_ARG
    with pytest.raises(_native.EngineError, match="NULL member of sst_final_args"):
        eng.check(E_ARG, "final search")
    for name in RB.ROBUST_FIELDS + SC.SEARCH_FIELDS:
        holder = a.robust if name in RB.ROBUST_FIELDS else a
        keep = getattr(holder, name)
        setattr(holder, name, None)
        assert fn(handle, ctypes.byref(a)) == E_ARG, name
        with pytest.raises(_native.EngineError, match="NULL member of sst_final_search_args"):
            eng.check(E_ARG, "final search")
        setattr(holder, name, keep)
    for bad in (0, (1 << 16) + 1):
        a.max_width = bad
        assert fn(handle, ctypes.byref(a)) == E_ARG
        with pytest.raises(_native.EngineError, match="max_width"):
            eng.check(E_ARG, "final search")
    a.max_width = 1 << 12
    a.horizon = (1 << 62) + 1
    assert fn(handle, ctypes.byref(a)) == E_ARG
    with pytest.raises(_native.EngineError, match="horizon"):
        eng.check(E_ARG, "final search")
    a.horizon = 1 << 62
    assert fn(handle, ctypes.byref(a)) == OK
    a.horizon = 1 << 17
    a.robust.base.max_combos = (1 << 22) + 1
    assert fn(handle, ctypes.byref(a)) == E_ARG
    with pytest.raises(_native.EngineError, match="max_combos"):
        eng.check(E_ARG, "final search")
    a.robust.base.max_combos = 0
    assert fn(handle, ctypes.byref(a)) == OK
    assert lib.sst_final_robust_device(handle, ctypes.byref(a.robust)) == E_ARG  # 0 here and only here
    assert _native.K_FINAL_SEARCH == 29 < _native.K_COUNT and _native.KERNEL_NAMES[29] == "k_final_search"
    eng.synchronize()
    eng.profile(True)
    eng.check(fn(handle, ctypes.byref(a)), "final search")
    prof = eng.profile_read()
    eng.profile(False)
    assert prof[_native.K_FINAL_SEARCH][1] == 1 and prof[_native.K_FINAL_ROBUST][1] == 1 and _native.K_FINAL not in prof
    eng.trim()  # the workspace goes back; the next call allocates it again
    eng.check(fn(handle, ctypes.byref(a)), "final search")
    eng.synchronize()


def test_run_batch_align_search(engine):  # noqa: F811
    """run_batch(align_search=True) on the synthetic spectra at
    final_max_combos = 4 (both paths), the largest spectrum that has fragments
    forced onto the mirror route: the three outcomes equal final_search_host
    over the whole outcome; the first two results are align_robust's."""
    import _synth_cases as SY
    from spectrseqtools_amd import alignment, final_program as FP, pipeline_device as PD
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE, build_breakage_dict

    n = min(48, len(load_golden("synth_stages.json.gz")["noise_free_exact"]["spectra"]))
    d = SY.variant_inputs("noise_free_exact", n=n)
    offsets = d["offsets"][:n + 1]
    seq = SequenceInformation(max_len=20, su_mass=float(d["su_seq"][0]), obs_mass=float(d["seq_mass"][0]),
                              modification_rate=d["mod_rate"])
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq, engine=engine)
    try:
        peaks = np.diff(offsets)
        kw = dict(max_len=d["max_len"][:n], trim=False)
        args = (dp, d["obs"][:offsets[n]], offsets, d["su_seq"][:n], d["seq_mass"][:n], build_breakage_dict(*SY.TAGS))
        plain = PD.run_batch(*args, **kw)
        live = np.flatnonzero(~plain.default & (np.diff(plain.frag_off) > 0))
        g = int(live[np.argmax(peaks[live])])
        kw["limits"] = PD.DeviceLimits(max_peaks=int(peaks[g]) - 1)
        out, al, fo, ro, so = PD.run_batch(*args, align_search=True, final_max_combos=4, **kw)
        out_r, al_r, fo_r, ro_r = PD.run_batch(*args, align_robust=True, final_max_combos=4, **kw)
        assert out.equals(out_r) and al.equals(al_r)
        routed = np.flatnonzero(out.route == PD.ROUTE_MIRROR)
        assert g in routed and len(routed) < len(out)
        use, _ = FP.final_use(al, optional=True)
        want = FP.final_search_host(out, dp.precision, alignment.lp_caps(dp, out), alignment.lp_row_caps(dp, out), use=use,
                                    max_combos=4)
        SC.assert_equal17((fo, ro, so), want, "run_batch")
        one = np.flatnonzero(fo_r.status == FC.SOLVED)
        assert fo.take(one).equals(fo_r.take(one)) and ro.take(one).equals(ro_r.take(one))
        assert (so.mode[one] == FP.SEARCH_ENUMERATED).all()
        print("spectra", len(out), "enumerated", len(one), "searched and SOLVED", int((so.mode == 2).sum()),
              "TOO_LARGE before", int((fo_r.status == FC.TOO_LARGE).sum()), "after", int((fo.status == FC.TOO_LARGE).sum()),
              flush=True)
        assert (so.mode == FP.SEARCH_SEARCHED).sum() >= 1
    finally:
        dp.close()
        engine.trim()
        PD.release_length_buffer()
