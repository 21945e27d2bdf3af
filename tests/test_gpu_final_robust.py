"""GPU tests of the robust final program (sst_final_robust_device:
k_final_robust in csrc/sst_final.hip; final_program.final_robust_device,
run_batch(align_robust=True)): the device result equals
final_program.final_robust_host in all fourteen arrays -- which
tests/test_final_robust_model.py holds to the brute force -- on random small
spectra with every status in one launch, against the base entry point where no
fragment is optional, and on the smallest shapes at which the second, capped
enumeration can go wrong."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
import _final_cases as FC
import _robust_cases as RB
from _align_gpu import engine, full_table  # noqa: F401
from conftest import load_golden
from test_gpu_final import CHUNK, WG, device_args, masses_of

pytestmark = pytest.mark.gpu


def run(dp, specs, rm, row_cap=None, max_combos=1 << 20, what=""):
    """(outcome, FinalOutcome, RobustOutcome) of a case on the device; asserts it equal to the host model in all
    fourteen arrays."""
    from spectrseqtools_amd import final_program as FP

    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    row_cap = KC.loose_row_cap(len(rm)) if row_cap is None else row_cap
    use = RB.use3_array(specs)
    want = FP.final_robust_host(o, dp.precision, caps, row_cap, use=use, max_combos=max_combos)
    got = FP.final_robust_device(dp, o, use=use, max_combos=max_combos, caps=caps, row_cap=row_cap)
    assert np.array_equal(got[0].frag_off, o.frag_off) and np.array_equal(got[0].pos_off, o.pos_off)
    RB.assert_equal14(got, want, what)
    return (o,) + got


def test_random_small_spectra(full_table):  # noqa: F811
    """200 random spectra with a random 0 / 1 / 2 use per fragment over the
    real masses, default spectra among them: at max_combos = 12 every status
    shares one launch; at the default nothing is TOO_LARGE."""
    dp = full_table
    rm = masses_of(dp)
    specs, row_cap = RB.random_robust_case(77, rm, dp.tolerance, dp.precision, 200)
    for at in (3, 100, 199):
        specs.insert(at, {"default": True})
    _, small, _ = run(dp, specs, rm, row_cap, 12, "max_combos 12")
    assert set(small.status.tolist()) == {FC.NONE, FC.SOLVED, FC.TOO_LARGE, FC.INFEASIBLE, FC.SKIPPED, FC.NOT_FREE}
    _, fo, ro = run(dp, specs, rm, row_cap, what="default max_combos")
    ok = fo.status == FC.SOLVED
    lower = int((ro.rbest[ok] < fo.best[ok] + ro.cstar[ok]).sum())
    print("solved", int(ok.sum()), "with optional", int((ro.n_optional > 0).sum()), "rbest < best + cstar", lower,
          "rn_opt > 1", int((ro.rn_opt[ok] > 1).sum()), flush=True)
    assert ok.sum() >= 60 and (ro.n_optional[ok] > 0).sum() >= 30 and (ro.n_optional[ok] == 0).sum() >= 15
    assert lower >= 5 and ((ro.rn_opt[ok] == 1) & (ro.n_optional[ok] > 0)).sum() >= 15


def test_base_entry_point(full_table):  # noqa: F811
    """With use in {0, 1} only the nine outputs equal sst_final_program_device's
    byte for byte and the five new ones are (0, 0, best, n_opt, gap); a use
    value other than 0, 1, 2 is required."""
    from spectrseqtools_amd import final_program as FP

    dp = full_table
    rm = masses_of(dp)
    specs, row_cap = FC.random_final_case(78, rm, dp.tolerance, dp.precision, 240)
    specs.insert(17, {"default": True})
    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    use = FC.use_array(specs)
    for max_combos in (12, 1 << 20):
        base = FP.final_device(dp, o, use=use, max_combos=max_combos, caps=caps, row_cap=row_cap)
        for u in (use, use * 3):
            fo, ro = FP.final_robust_device(dp, o, use=u, max_combos=max_combos, caps=caps, row_cap=row_cap)
            for k in FC.FIELDS:
                assert getattr(fo, k).tobytes() == getattr(base, k).tobytes(), (max_combos, k)
            assert not ro.n_optional.any() and not ro.cstar.any()
            assert np.array_equal(ro.rbest, base.best) and np.array_equal(ro.rn_opt, base.n_opt)
            assert np.array_equal(ro.rgap, base.gap)
            assert np.array_equal(FP.robust_decisions(fo, ro), FP.final_decisions(base))
    assert (base.status == FC.SOLVED).sum() >= 60 and (use == 0).sum() >= 100


def test_optional_records_at_chunk_borders(full_table):  # noqa: F811
    """513 and 1025 fragments with optional ones at 0, 511, 512, 1024 and last,
    over 1, 256 and 258 assignments: one pass and several passes of the
    workgroup each meet one chunk of records and several."""
    dp = full_table
    rm = masses_of(dp)
    specs = RB.chunk_border_specs(rm, dp.precision, np.random.default_rng(96), CHUNK)
    o, fo, ro = run(dp, specs, rm)
    assert fo.status.tolist() == [FC.SOLVED] * 6 and fo.combos.tolist() == [1, 256, 258] * 2
    assert np.diff(o.frag_off).tolist() == [CHUNK + 1] * 3 + [2 * CHUNK + 1] * 3 and 256 == WG < 258
    assert ro.n_optional.tolist() == [3, 3, 3, 4, 4, 4]  # (the last record is the one at 512 / at 1024)
    assert (ro.cstar > 0).all() and (fo.iv != 0xFFFE).all()
    assert ro.rbest[0] == fo.best[0] + ro.cstar[0] and ro.rn_opt[0] == 1 and ro.rgap[0] == FC.NO_GAP  # one y


def test_ties_and_pulls(full_table):  # noqa: F811
    """A robust tie across passes: y* alone is optimal over the required
    fragments, a second y in a later pass and a lower lane has the same cap
    (rn_opt == 2).  One position of two rows: an optional fragment that pulls
    the optimum away (rbest < best + cstar), one whose own best y differs by a
    small cost (robust), by a large cost (a tie), and one with c* == 0."""
    from spectrseqtools_amd import final_program as FP

    dp = full_table
    rm = masses_of(dp)
    ties = [RB.robust_tie(rm, dp.precision, x=x) for x in (5, 127, 64)]
    pulls, p, q = RB.pull_specs(rm, dp.precision)
    o, fo, ro = run(dp, [t[0] for t in ties] + pulls, rm)
    assert fo.status.tolist() == [FC.SOLVED] * 7 and fo.combos.tolist() == [4096] * 3 + [2] * 4
    for k, (_, a, b) in enumerate(ties):
        assert a // WG < b // WG and a % WG > b % WG
        seq = fo.seq[12 * k:12 * k + 12].tolist()
        assert int("".join(str(int(r == FC.distinct_pairs(rm, 1)[0][1])) for r in seq), 2) == a
    assert fo.n_opt[:3].tolist() == [1] * 3 and ro.rn_opt[:3].tolist() == [2] * 3 and ro.n_optional[:3].tolist() == [1] * 3
    assert (ro.rbest[:3] == fo.best[:3] + ro.cstar[:3]).all() and (ro.cstar[:3] > 0).all()
    d = abs(rm[p] - rm[q]) * FC.FIX
    assert fo.seq[36:].tolist() == [p] * 4 and fo.n_opt[3:].tolist() == [1] * 4
    assert ro.rbest[3] < fo.best[3] + ro.cstar[3] and ro.cstar[3] == d
    assert ro.rbest[4] == fo.best[4] + ro.cstar[4] and ro.rn_opt[4] == 1 and ro.rgap[4] == d - 2 * FC.FIX
    assert ro.rbest[5] == d == ro.cstar[5] and ro.rn_opt[5] == 2
    assert ro.cstar[6] == 0 and (ro.rbest[6], ro.rn_opt[6], ro.rgap[6]) == (fo.best[6], fo.n_opt[6], fo.gap[6])
    assert FP.robust_decisions(fo, ro).tolist() == [0, 0, 0, 0, 1, 0, 1]


def test_optional_fragment_kinds(full_table):  # noqa: F811
    """An optional fragment of every class: internal with q <= 0 (the empty
    interval), terminal with mn > mx, terminal with a range of ends, START_END,
    internal of positive mass, and all together.  An optional fragment outside
    the fixed-point range or with an end outside [0, L - 1]: SKIPPED; unused: SOLVED."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(97)
    kinds = RB.class_specs(rm, dp.precision, rng)
    bad, want = RB.unmodelled_optional_specs(rm, dp.precision, rng)
    o, fo, ro = run(dp, kinds + bad, rm)
    n = len(kinds)
    assert fo.status.tolist() == [FC.SOLVED] * n + want and ro.n_optional[:n].tolist() == [1] * (n - 1) + [n - 1]
    last = fo.iv[o.frag_off[1:n] - 1]  # the optional fragment of each of the first n - 1 spectra
    assert last[0] == last[1] == 0xFFFF and (last != 0xFFFE).all() and fo.sum[o.frag_off[1] - 1] == 0
    assert ro.n_optional[n:].tolist() == [0, 8] * (len(bad) // 2) and (ro.rgap[n::2] == FC.NO_GAP).all()


def test_limits_with_optional_fragments(full_table):  # noqa: F811
    """Required + optional = 16384 is SOLVED, 16385 is SKIPPED; L == 0 and
    L == 1; L = 253 with optional fragments of every class."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(98)
    edge, a, b = FC.n_used_specs(rm, dp.precision)
    edge = [RB.every_third_optional(s) for s in edge]
    zero, want, _ = FC.zero_length_specs(rm, dp.precision)
    zero = [RB.mark(s, (0, 2)) for s in zero[:2]] + [RB.mark(zero[2], (4,)), RB.mark(zero[3], (1,), unused=(4,))]
    ones = [RB.every_third_optional(FC.loose_spec(rm, sets, FC.random_frags(rng, rm, sets, 9, dp.precision)))
            for sets in ([[5]], [[1, 2]], [[3, 4, 6]])]
    lng = RB.every_third_optional(FC.long_spec(rm, dp.precision, rng, n_frags=40))
    o, fo, ro = run(dp, edge + zero + ones + [lng], rm)
    assert fo.status.tolist() == [FC.SOLVED, FC.SKIPPED] + want + [FC.SOLVED] * 4
    assert ro.n_optional.tolist() == [16384 // 3, 0, 2, 2, 0, 1, 3, 3, 3, 13] and fo.combos[-1] == 243
    assert (fo.iv[:16390] != 0xFFFE).sum() == 16384 and fo.seq[0] == b and ro.cstar[0] == 0
    assert ro.rgap[0] == (16384 - 16384 // 3) * FC.FIX * abs(rm[b] - rm[a])  # the optional ones are capped at c* == 0


@pytest.mark.parametrize("n_rows", [64, 65, 120])
def test_row_count_edges(engine, n_rows):  # noqa: F811
    """Tables of 64, 65 and 120 rows with bits set for rows that do not exist, every third used fragment optional."""
    from spectrseqtools_amd import _native

    rm, specs, row_cap = FC.row_edge_case(n_rows, 0.001, np.random.default_rng(95))
    specs = [RB.every_third_optional(s) for s in specs]
    table = _native.DeviceTable.build(rm, max(rm) * 4, 32, engine=engine)
    dp = SimpleNamespace(masses=[SimpleNamespace(mass=m) for m in rm], device_table=table, precision=0.001, tolerance=1e-5)
    try:
        o, fo, ro = run(dp, specs, rm, row_cap)
        assert fo.status[:2].tolist() == [FC.SOLVED] * 2 and fo.status[5] == FC.INFEASIBLE and fo.status[6] == FC.NOT_FREE
        assert (ro.n_optional[:2] > 0).all() and not ro.n_optional[5:7].any()
    finally:
        table.close()


def test_22_free_positions_with_an_optional_fragment(full_table):  # noqa: F811
    """2^22 assignments, enumerated twice: the optional fragment pins the last
    prefix sum to the other row, and the pinned y stays the cap's unique optimum."""
    dp = full_table
    rm = masses_of(dp)
    pairs = FC.distinct_pairs(rm, 22)
    spec, y = FC.pinned_binary_spec(rm, 22, [1] * 22, dp.precision, pairs=pairs)
    other = sum(int(rm[r]) for r in y[:21]) + int(rm[pairs[21][0]])
    spec = RB.mark(dict(spec, frags=spec["frags"] + [(FC.START, float(other) * dp.precision, 100.0, 21, 21)]), (22,))
    o, fo, ro = run(dp, [spec], rm, max_combos=1 << 22)
    d = abs(rm[pairs[21][0]] - rm[pairs[21][1]]) * FC.FIX
    assert fo.status.tolist() == [FC.SOLVED] and fo.n_feas.tolist() == [1 << 22] and fo.seq.tolist() == y
    assert ro.n_optional.tolist() == [1] and ro.cstar.tolist() == [d] and ro.rbest.tolist() == [d]
    assert ro.rn_opt.tolist() == [2] and fo.n_opt.tolist() == [1]  # (the other row: the pin's d against the cap's d)


def test_later_spectra_of_a_workgroup(full_table, engine):  # noqa: F811
    """n = 4 * 3 * CUs + 37 spectra gathered from 61 base spectra that alternate
    between spectra with and without optional fragments and between the
    statuses, forward and reversed: every workgroup runs several spectra, and a
    spectrum's result is what it is alone.  A P* left from the previous spectrum
    would change cstar and the caps; an optional count or a cstar accumulator
    that is not reset inside the spectrum loop carries over into the next
    spectrum's n_optional (and sends a spectrum without optional fragments
    through the second enumeration) or cstar."""
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
    assert len(base) == 61
    o = AC.make_outcome(base, rm)
    caps = CC.caps_of(base, len(rm))
    use = RB.use3_array(base)
    want = FP.final_robust_host(o, dp.precision, caps, row_cap, use=use, max_combos=1 << 12)
    ok = want[0].status == FC.SOLVED
    # (floors against a vacuous base set only: 19 and 15 SOLVED spectra with and without optional fragments)
    assert ((want[1].n_optional > 0) & ok).sum() >= 12 and ((want[1].n_optional == 0) & ok).sum() >= 8
    assert len(set(want[0].status.tolist())) >= 5 and (want[1].cstar > 0).sum() >= 10

    cus = int(torch.cuda.get_device_properties(engine.device).multi_processor_count)
    n = 4 * 3 * cus + 37
    idx = (np.arange(n, dtype=np.int64) * 23) % len(base)
    for order in (idx, idx[::-1].copy()):
        src, _ = _segments(o.frag_off, order)
        got = FP.final_robust_device(dp, o.take(order), use=use[src], max_combos=1 << 12,
                                     caps=(caps[0], caps[1][order]), row_cap=row_cap)
        RB.assert_equal14(got, (want[0].take(order), want[1].take(order)), "later spectra")


def test_entry_point_contract(full_table):  # noqa: F811
    """A second identical call over poisoned outputs gives identical arrays
    (every element is written) and equals final_robust_device (frag_use NULL:
    all required).  SST_E_ARG with a message for a NULL struct, a NULL member
    with n_spec > 0 (the five new pointers included), max_combos of 0 or above
    the limit and a bad prec; n_spec == 0 is SST_OK; the profile id."""
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
    base, ins, outs = device_args(dp, o)
    dev = torch.device("cuda", eng.device)
    S = len(o)
    r_outs = [torch.zeros(S, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int64, torch.int32,
                                                               torch.int64)]
    a = _native.FinalRobustArgs()
    a.base = base
    a.n_optional, a.cstar, a.rbest, a.rn_opt, a.rgap = (x.data_ptr() for x in r_outs)
    fn = lib.sst_final_robust_device
    call = lambda: eng.check(fn(handle, ctypes.byref(a)), "final robust")  # noqa: E731
    results = []
    for fill in (0x5A, 0xC3):
        for x in outs + r_outs:
            x.view(dtype=torch.uint8).fill_(fill)
        eng.synchronize()
        call()
        eng.synchronize()
        results.append([x.cpu().numpy().copy() for x in outs + r_outs])
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    want = FP.final_robust_device(dp, o, caps=(np.zeros(len(rm), np.uint8), o.seq_len.astype(np.int32)),
                                  row_cap=KC.loose_row_cap(len(rm)))
    dts = (np.uint8, np.uint64, np.uint64, np.uint64, np.uint32, np.uint64, np.uint8, np.uint16, np.uint32,
           np.uint32, np.uint64, np.uint64, np.uint32, np.uint64)
    RB.assert_equal14(want, tuple(x.view(dt) for x, dt in zip(results[0], dts)), "raw call")
    assert (want[0].status == FC.SOLVED).sum() >= 20 and want[0].status[-1] == FC.NONE

    assert fn(None, ctypes.byref(a)) == E_ARG
    assert fn(handle, None) == E_ARG
    with pytest.raises(_native.EngineError, match="NULL sst_final_robust_args"):
        eng.check(E_ARG, "final robust")
    empty = _native.FinalRobustArgs()
    empty.base.n_spec, empty.base.prec, empty.base.max_combos = 0, dp.precision, 1
    assert fn(handle, ctypes.byref(empty)) == OK  # nothing to do, no array is read
    empty.base.n_spec = 1
    assert fn(handle, ctypes.byref(empty)) == E_ARG
    with pytest.raises(_native.EngineError, match="NULL member of sst_final_args"):
        eng.check(E_ARG, "final robust")
    for name, _ in _native.FinalArgs._fields_:
        if name in ("n_spec", "prec", "max_combos", "frag_use"):
            continue
        keep = getattr(a.base, name)
        setattr(a.base, name, None)
        assert fn(handle, ctypes.byref(a)) == E_ARG, name
        setattr(a.base, name, keep)
    for name in RB.ROBUST_FIELDS:
        keep = getattr(a, name)
        setattr(a, name, None)
        assert fn(handle, ctypes.byref(a)) == E_ARG, name
        with pytest.raises(_native.EngineError, match="NULL member of sst_final_robust_args"):
            eng.check(E_ARG, "final robust")
        setattr(a, name, keep)
    for bad in (0, (1 << 22) + 1):
        a.base.max_combos = bad
        assert fn(handle, ctypes.byref(a)) == E_ARG
        with pytest.raises(_native.EngineError, match="max_combos"):
            eng.check(E_ARG, "final robust")
    a.base.max_combos = 1 << 22
    assert fn(handle, ctypes.byref(a)) == OK
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        a.base.prec = bad
        assert fn(handle, ctypes.byref(a)) == E_ARG
        with pytest.raises(_native.EngineError, match="prec"):
            eng.check(E_ARG, "final robust")
    a.base.n_spec = -1
    assert fn(handle, ctypes.byref(a)) == E_ARG
    assert _native.K_FINAL_ROBUST == 28 < _native.K_COUNT and _native.KERNEL_NAMES[28] == "k_final_robust"
    eng.synchronize()
    eng.profile(True)
    a.base.n_spec, a.base.prec = S, float(dp.precision)
    call()
    prof = eng.profile_read()
    eng.profile(False)
    assert prof[_native.K_FINAL_ROBUST][1] == 1 and prof[_native.K_FINAL_ROBUST][0] > 0 and _native.K_FINAL not in prof


def test_run_batch_align_robust(engine):  # noqa: F811
    """run_batch(align_robust=True) on the synthetic spectra, the largest
    spectrum that has fragments forced onto the mirror route: fo / ro equal
    final_robust_host over the whole outcome, nothing is UNDECIDED, spectra
    without an LP_SOLVE fragment have the fo of align_final=True, and the
    existing options return what they did."""
    import _synth_cases as SC
    from spectrseqtools_amd import alignment, final_program as FP, pipeline_device as PD
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE, build_breakage_dict

    n = min(48, len(load_golden("synth_stages.json.gz")["noise_free_exact"]["spectra"]))
    d = SC.variant_inputs("noise_free_exact", n=n)
    offsets = d["offsets"][:n + 1]
    seq = SequenceInformation(max_len=20, su_mass=float(d["su_seq"][0]), obs_mass=float(d["seq_mass"][0]),
                              modification_rate=d["mod_rate"])
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq, engine=engine)
    try:
        peaks = np.diff(offsets)
        kw = dict(max_len=d["max_len"][:n], trim=False)
        args = (dp, d["obs"][:offsets[n]], offsets, d["su_seq"][:n], d["seq_mass"][:n], build_breakage_dict(*SC.TAGS))
        plain = PD.run_batch(*args, **kw)
        live = np.flatnonzero(~plain.default & (np.diff(plain.frag_off) > 0))
        g = int(live[np.argmax(peaks[live])])
        kw["limits"] = PD.DeviceLimits(max_peaks=int(peaks[g]) - 1)
        out, al, fo, ro = PD.run_batch(*args, align_robust=True, **kw)
        out_f, al_f, fo_f = PD.run_batch(*args, align_final=True, **kw)
        out_k, al_k = PD.run_batch(*args, align_keep=True, align_split=True, **kw)
        assert out.equals(out_f) and al.equals(al_f) and out_f.equals(out_k) and al_f.equals(al_k)
        assert out.equals(plain, ignore=("route", "reason")) and PD.run_batch(*args, **kw).equals(out)
        routed = np.flatnonzero(out.route == PD.ROUTE_MIRROR)
        assert g in routed and len(routed) < len(out)
        use, undecided = FP.final_use(al, optional=True)
        host_args = (out, dp.precision, alignment.lp_caps(dp, out), alignment.lp_row_caps(dp, out))
        want = FP.final_robust_host(*host_args, use=use)
        RB.assert_equal14((fo, ro), want, "run_batch")
        for x in (int(routed[0]), int(live[0])):  # ... and spectrum by spectrum: a routed one, a device one
            RB.assert_equal14((fo.take([x]), ro.take([x])), (want[0].take([x]), want[1].take([x])), x)
        assert not undecided.any() and not (fo.status == FP.FINAL_UNDECIDED).any() and len(ro) == len(out)
        plain_use, was_undecided = FP.final_use(al)
        assert fo_f.equals(FP.final_host(*host_args, use=plain_use, undecided=was_undecided))  # (as before)
        decided = np.flatnonzero(~was_undecided)
        assert fo.take(decided).equals(fo_f.take(decided)) and not ro.n_optional[decided].any()
        assert np.array_equal(FP.robust_decisions(fo, ro)[decided], FP.final_decisions(fo_f)[decided])
        dec = FP.robust_decisions(fo, ro)
        print("spectra", len(out), "formerly undecided", int(was_undecided.sum()), "of them TAKE",
              int(dec[was_undecided].sum()), "TAKE", float(dec.mean()), flush=True)
    finally:
        dp.close()
        engine.trim()
        PD.release_length_buffer()
