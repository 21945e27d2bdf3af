"""GPU tests of the final program (sst_final_program_device: k_final_program in
csrc/sst_final.hip; final_program.final_device, run_batch(align_final=True)): the
device result equals final_program.final_host in all nine arrays -- which
tests/test_final_model.py holds to the brute force -- on random small spectra
over the real masses with every status in one launch, at the edges of
max_combos and of the modification cap, on rows of equal mass, across passes of
the workgroup and chunks of fragment records, at L = 253, and through
run_batch."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
import _final_cases as FC
from _align_gpu import engine, full_table  # noqa: F401
from conftest import load_golden

pytestmark = pytest.mark.gpu
WG = 256      # lanes of a workgroup: assignments per pass
CHUNK = 512   # fragment records the kernel holds at a time


def masses_of(dp):
    return [int(m.mass) for m in dp.masses]


def run(dp, specs, rm, row_cap=None, max_combos=1 << 20, what=""):
    """(outcome, device result) of a case; asserts the device equal to the host model in all nine arrays."""
    from spectrseqtools_amd import final_program as FP

    o = AC.make_outcome(specs, rm)
    caps = CC.caps_of(specs, len(rm))
    row_cap = KC.loose_row_cap(len(rm)) if row_cap is None else row_cap
    use = FC.use_array(specs)
    want = FP.final_host(o, dp.precision, caps, row_cap, use=use, max_combos=max_combos)
    got = FP.final_device(dp, o, use=use, max_combos=max_combos, caps=caps, row_cap=row_cap)
    assert np.array_equal(got.frag_off, o.frag_off) and np.array_equal(got.pos_off, o.pos_off)
    FC.assert_equal9(got, want, what)
    return o, got


def test_random_small_spectra(full_table):
    """360 random spectra (L <= 6, sets of <= 3 rows) over the real masses, a
    random row_mod, mixed mod_cap and row caps, use masks, default spectra: at
    max_combos = 12 every status shares one launch; at the default nothing is
    TOO_LARGE."""
    dp = full_table
    rm = masses_of(dp)
    specs, row_cap = FC.random_final_case(77, rm, dp.tolerance, dp.precision, 360)
    for at in (3, 100, 359):
        specs.insert(at, {"default": True})
    _, small = run(dp, specs, rm, row_cap, 12, "max_combos 12")
    assert set(small.status.tolist()) == {FC.NONE, FC.SOLVED, FC.TOO_LARGE, FC.INFEASIBLE, FC.SKIPPED, FC.NOT_FREE}
    _, got = run(dp, specs, rm, row_cap, what="default max_combos")
    n = np.bincount(got.status, minlength=6)
    solved = got.status == FC.SOLVED
    print("statuses", n.tolist(), "unique", int((got.n_opt[solved] == 1).sum()), "cap binds",
          int((got.n_feas[solved] < got.combos[solved]).sum()), flush=True)
    assert n[FC.NONE] == 3 and n[FC.TOO_LARGE] == 0 and n[FC.SOLVED] >= 100 and n[FC.NOT_FREE] >= 30
    assert n[FC.SKIPPED] >= 5 and n[FC.INFEASIBLE] >= 20 and (got.n_feas[solved] < got.combos[solved]).sum() >= 5
    assert (got.combos[solved] > 12).sum() >= 10 and (got.iv[got.iv != 0xFFFE] == 0xFFFF).any()


def test_max_combos_edge_and_cap_binding(full_table):
    """combos == max_combos is SOLVED, max_combos + 1 would not be needed:
    combos == max_combos + 1 is TOO_LARGE (16 and 4096 assignments).  The
    modification cap binding: n_feas < combos, and n_feas == 0 (INFEASIBLE with
    its combos reported)."""
    dp = full_table
    rm = masses_of(dp)
    pairs = FC.distinct_pairs(rm, 3)
    small, _ = FC.pinned_binary_spec(rm, 4, [1, 0, 0, 1], dp.precision, pairs=pairs)
    large, _ = FC.pinned_binary_spec(rm, 12, [0, 1] * 6, dp.precision, pairs=pairs)
    for spec, combos in ((small, 16), (large, 4096)):
        _, at = run(dp, [spec], rm, max_combos=combos)
        _, below = run(dp, [spec], rm, max_combos=combos - 1)
        assert at.status.tolist() == [FC.SOLVED] and below.status.tolist() == [FC.TOO_LARGE]
        assert at.combos.tolist() == below.combos.tolist() == [combos] and at.n_feas.tolist() == [combos]
        assert at.n_opt.tolist() == [1] and at.best.tolist() == [0] and below.n_feas.tolist() == [0]
    # every upper row modified: a y is feasible iff it has at most mod_cap upper rows
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[b for _, b in pairs]] = 1
    capped = [dict(small, row_mod=row_mod, mod_cap=c) for c in (4, 2, 1, 0, -1)]  # (the pinned y has two upper rows)
    forced = FC.loose_spec(rm, [[pairs[0][1]], list(pairs[1])], small["frags"][:2], mod_cap=0, row_mod=row_mod)
    _, got = run(dp, capped + [forced], rm)
    assert got.status.tolist() == [FC.SOLVED] * 4 + [FC.INFEASIBLE] * 2
    assert got.n_feas.tolist() == [16, 11, 5, 1, 0, 0] and got.combos.tolist() == [16] * 5 + [2]
    assert got.best[:2].tolist() == [0, 0] and (got.best[2:4] > 0).all()


def test_equal_mass_rows(engine):
    """A table with two rows of one mass: n_opt == 2, gap counts the next
    distinct objective, and the lower row wins."""
    from spectrseqtools_amd import _native

    rm = [0, 305041, 329052, 305041, 345047, 329052]
    table = _native.DeviceTable.build(rm, max(rm) * 4, 32, engine=engine)
    dp = SimpleNamespace(masses=[SimpleNamespace(mass=m) for m in rm], device_table=table, precision=0.001, tolerance=1e-5)
    try:
        total = (rm[1] + rm[2] + rm[4]) * dp.precision
        one = FC.loose_spec(rm, [[1, 3], [2], [4]], [(FC.START_END, total, 100.0, 0, 0)])
        two = FC.loose_spec(rm, [[3, 1, 4], [5, 2], [4]], [(FC.START_END, total, 100.0, 0, 0),
                                                            (FC.START, rm[1] * dp.precision, 100.0, 0, 0)])
        _, got = run(dp, [one, two], rm)
        assert got.status.tolist() == [FC.SOLVED] * 2 and got.n_opt.tolist() == [2, 4] and got.best.tolist() == [0, 0]
        assert got.seq.tolist() == [1, 2, 4, 1, 2, 4] and got.gap[0] == FC.NO_GAP
        assert got.gap[1] == 2 * FC.FIX * (rm[4] - rm[1])  # row 4 at position 0: both fragments off by the difference
    finally:
        table.close()


def test_more_than_one_pass(full_table):
    """4096 and 4374 assignments (16 and 18 passes of the workgroup), at most 12
    fragments: the unique optimum has its last free position at its last row, so
    its index is odd / = 2 mod 3 and sits in a late pass.  And a tie of two
    optima whose first index sits in an earlier pass but a higher lane than the
    second: the lower index wins, whatever order the lanes are reduced in."""
    dp = full_table
    rm = masses_of(dp)
    pairs = FC.distinct_pairs(rm, 4)
    digits = [1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1]
    binary, y2 = FC.pinned_binary_spec(rm, 12, digits, dp.precision, pairs=pairs)
    rows = [r for r in range(1, len(rm))]
    triples = [[rows[3 * i], rows[3 * i + 1], rows[3 * i + 2]] for i in range(8)]
    assert all(len({rm[r] for r in t}) == 3 for t in triples)
    sets = triples[:7] + [triples[7][:2]]
    d3 = [2, 0, 1, 2, 2, 0, 1, 1]
    y3 = [s[d] for s, d in zip(sets, d3)]
    ternary = FC.loose_spec(rm, sets, FC.prefix_pins(rm, sets, y3, range(8), dp.precision))
    ties = [FC.tie_across_passes(rm, dp.precision, x=x) for x in (5, 127, 64)]
    _, got = run(dp, [binary, ternary] + [t[0] for t in ties], rm)
    assert got.status.tolist() == [FC.SOLVED] * 5 and got.combos.tolist() == [4096, 4374, 4096, 4096, 4096]
    assert got.n_opt.tolist() == [1, 1, 2, 2, 2] and got.best.tolist() == [0] * 5
    assert len(binary["frags"]) == 12 and len(ternary["frags"]) == 8
    assert got.seq[:12].tolist() == y2 and got.seq[12:20].tolist() == y3
    assert int("".join(map(str, digits)), 2) // WG == 13 and digits[-1] == 1 and d3[-1] == 1
    p, q = FC.distinct_pairs(rm, 1)[0]
    for k, (_, a, b) in enumerate(ties):
        seq = got.seq[20 + 12 * k:32 + 12 * k].tolist()
        assert int("".join(str(int(r == q)) for r in seq), 2) == a
        assert a < b and a // WG < b // WG and a % WG > b % WG, (a, b)


def test_long_skeleton_and_fragment_chunks(full_table):
    """L = 253 with five free positions of three rows (243 assignments, the
    two-pointer sweep over 254 prefix sums, ranges of ends); 900 fragments (two
    chunks of records) at 16 assignments with a use mask; fragments out of su
    order, mn > mx, the END class, the empty interval as a minimiser; 6561
    assignments under 40 noisy fragments (a lane sees 26 objectives and stops
    summing those above its two smallest)."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(91)
    lng = FC.long_spec(rm, dp.precision, rng, n_frags=40)
    sets = [[1, 2], [3], [2, 4], [1, 6], [3, 5], [4]]
    many = FC.loose_spec(rm, sets, FC.random_frags(rng, rm, sets, 900, dp.precision),
                         use=[int(i % 7 != 3) for i in range(900)])
    assert len(many["frags"]) > CHUNK and [f[1] for f in many["frags"]] != sorted(f[1] for f in many["frags"])
    assert any(f[3] > f[4] for f in many["frags"]) and any(f[0] == FC.END for f in many["frags"])
    rows = list(range(1, 25))
    wide_sets = [rows[3 * i:3 * i + 3] for i in range(8)]  # 6561 assignments, 26 passes, 40 fragments of every class
    wide = FC.loose_spec(rm, wide_sets, FC.random_frags(rng, rm, wide_sets, 40, dp.precision, noise=400))
    o, got = run(dp, [lng, many, dict(many, use=None), wide], rm)
    assert got.status.tolist() == [FC.SOLVED] * 4 and got.combos.tolist() == [243, 16, 16, 6561]
    assert got.best[3] > 0 and got.gap[3] != FC.NO_GAP
    iv = got.iv[o.frag_off[1]:o.frag_off[2]]
    assert (iv == 0xFFFE).sum() == sum(1 for i in range(900) if i % 7 == 3) and (iv == 0xFFFF).sum() >= 10
    assert (iv[CHUNK:] != 0xFFFE).sum() >= 300 and got.best[1] < got.best[2]
    end = np.array([f[0] == FC.END for f in many["frags"]]) & (iv != 0xFFFE)
    assert end.sum() >= 100 and ((iv[end] & 0xFF) == 5).all()
    assert len(set((got.iv[:o.frag_off[1]] >> 8).tolist())) >= 8  # intervals from many left ends of the long skeleton


def test_used_and_unused_unmodelled_fragments(full_table):
    """A terminal fragment with an end outside [0, L - 1], and one whose mass
    is outside the fixed-point range: used, the spectrum is SKIPPED; unused, it
    is SOLVED with iv == 0xFFFE there.  A spectrum with every fragment unused is
    SOLVED at objective 0 with every feasible y optimal."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(92)
    sets = [[1, 2], [3], [2, 4, 5]]
    frags = FC.random_frags(rng, rm, sets, 8, dp.precision)
    bad_end = (FC.END, rm[4] * dp.precision, 100.0, 3, 0)
    bad_mass = (FC.INTERNAL, 2.0 ** 32 * dp.precision, 100.0, 0, 0)
    specs = []
    for bad in (bad_end, bad_mass):
        specs += [FC.loose_spec(rm, sets, frags + [bad]), FC.loose_spec(rm, sets, frags + [bad], use=[1] * 8 + [0])]
    specs.append(FC.loose_spec(rm, sets, frags, use=[0] * 8))
    o, got = run(dp, specs, rm)
    assert got.status.tolist() == [FC.SKIPPED, FC.SOLVED, FC.SKIPPED, FC.SOLVED, FC.SOLVED]
    assert got.iv[o.frag_off[2] - 1] == 0xFFFE and (got.iv[o.frag_off[1]:o.frag_off[2] - 1] != 0xFFFE).all()
    assert got.n_opt[4] == 6 and got.best[4] == 0 and got.gap[4] == FC.NO_GAP and got.seq[-3:].tolist() == [1, 3, 2]


def device_args(dp, o, max_combos=1 << 20):
    """sst_final_args over device copies of an outcome (every fragment used, loose caps), and the tensors."""
    import torch

    from spectrseqtools_amd import _native

    dev = torch.device("cuda", dp.device_table.engine.device)
    up = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt).reshape(-1), device=dev)  # noqa: E731
    n_rows, S, nf, n_pos = len(o.row_mass), len(o), int(o.frag_off[-1]), int(o.pos_off[-1])
    ins = [up(o.seq_len, np.int32), up(o.pos_off, np.int64), up(o.skeleton.view(np.int64), np.int64),
           up(o.alpha.view(np.int64), np.int64), up(o.frag_off, np.int64), up(o.frag_code, np.uint8),
           up(o.frag_su, np.float64), up(o.frag_min_end, np.int32), up(o.frag_max_end, np.int32),
           up(np.zeros(n_rows), np.uint8), up(o.seq_len, np.int32), up(KC.loose_row_cap(n_rows), np.int32)]
    outs = [torch.zeros(n, dtype=dt, device=dev) for n, dt in (
        (S, torch.uint8), (S, torch.int64), (S, torch.int64), (S, torch.int64), (S, torch.int32), (S, torch.int64),
        (n_pos, torch.uint8), (nf, torch.int16), (nf, torch.int32))]
    a = _native.FinalArgs()
    a.n_spec = S
    (a.seq_len, a.pos_off, a.skeleton, a.alpha, a.frag_off, a.frag_code, a.frag_su, a.frag_min_end, a.frag_max_end,
     a.row_mod, a.mod_cap, a.row_cap) = (x.data_ptr() for x in ins)
    a.frag_use = None
    a.prec, a.max_combos = float(dp.precision), max_combos
    a.status, a.combos, a.n_feas, a.best, a.n_opt, a.gap, a.seq, a.iv, a.sum = (x.data_ptr() for x in outs)
    torch.cuda.synchronize(dev)
    return a, ins, outs


def test_identical_calls_and_entry_point_contract(full_table):
    """A second identical call gives identical arrays, over poisoned outputs
    (every element is written), and equals final_device (frag_use NULL: all).
    SST_E_ARG with a message for a NULL struct, a NULL member with n_spec > 0,
    max_combos of 0 or above the limit and a bad prec; n_spec == 0 is SST_OK; the
    limit and the profile id."""
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
    a, ins, outs = device_args(dp, o)
    call = lambda: eng.check(lib.sst_final_program_device(handle, ctypes.byref(a)), "final")  # noqa: E731
    results = []
    for fill in (0x5A, 0xC3):
        for x in outs:
            x.view(dtype=outs[0].dtype).fill_(fill)
        eng.synchronize()
        call()
        eng.synchronize()
        results.append([x.cpu().numpy().copy() for x in outs])
    assert all(np.array_equal(x, y) for x, y in zip(*results))
    want = FP.final_device(dp, o, caps=(np.zeros(len(rm), np.uint8), o.seq_len.astype(np.int32)),
                           row_cap=KC.loose_row_cap(len(rm)))
    dts = (np.uint8, np.uint64, np.uint64, np.uint64, np.uint32, np.uint64, np.uint8, np.uint16, np.uint32)
    FC.assert_equal9(want, tuple(x.view(dt) for x, dt in zip(results[0], dts)), "raw call")
    assert (want.status == FC.SOLVED).sum() >= 20 and want.status[-1] == FC.NONE

    fn = lib.sst_final_program_device
    assert int(lib.sst_final_max_combos()) == FP.FINAL_MAX_COMBOS == 1 << 22
    assert fn(None, ctypes.byref(a)) == E_ARG
    assert fn(handle, None) == E_ARG
    with pytest.raises(_native.EngineError, match="NULL sst_final_args"):
        eng.check(E_ARG, "final")
    empty = _native.FinalArgs()
    empty.n_spec, empty.prec, empty.max_combos = 0, dp.precision, 1
    assert fn(handle, ctypes.byref(empty)) == OK  # nothing to do, no array is read
    empty.n_spec = 1
    assert fn(handle, ctypes.byref(empty)) == E_ARG
    with pytest.raises(_native.EngineError, match="NULL member of sst_final_args"):
        eng.check(E_ARG, "final")
    for name, _ in _native.FinalArgs._fields_:
        if name in ("n_spec", "prec", "max_combos", "frag_use"):
            continue
        keep = getattr(a, name)
        setattr(a, name, None)
        assert fn(handle, ctypes.byref(a)) == E_ARG, name
        setattr(a, name, keep)
    for bad in (0, (1 << 22) + 1):
        a.max_combos = bad
        assert fn(handle, ctypes.byref(a)) == E_ARG
        with pytest.raises(_native.EngineError, match="max_combos"):
            eng.check(E_ARG, "final")
    a.max_combos = 1 << 22
    assert fn(handle, ctypes.byref(a)) == OK
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        a.prec = bad
        assert fn(handle, ctypes.byref(a)) == E_ARG
        with pytest.raises(_native.EngineError, match="prec"):
            eng.check(E_ARG, "final")
    a.n_spec = -1
    assert fn(handle, ctypes.byref(a)) == E_ARG
    assert _native.K_FINAL == 27 < _native.K_COUNT and _native.KERNEL_NAMES[27] == "k_final_program"
    eng.synchronize()
    eng.profile(True)
    a.n_spec, a.prec = len(o), float(dp.precision)
    call()
    prof = eng.profile_read()
    eng.profile(False)
    assert prof[_native.K_FINAL][1] == 1 and prof[_native.K_FINAL][0] > 0


def test_run_batch_align_final(engine):
    """run_batch(align_final=True) on the synthetic spectra, the largest
    spectrum that has fragments forced onto the mirror route: the FinalOutcome
    equals final_host over the whole outcome with final_use of the certificate;
    the other two outputs equal the run with align_keep and align_split."""
    import _synth_cases as SC
    from spectrseqtools_amd import alignment, final_program as FP, pipeline_device as PD
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE, build_breakage_dict

    n = len(load_golden("synth_stages.json.gz")["noise_free_exact"]["spectra"])
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
        out, al, fo = PD.run_batch(*args, align_final=True, **kw)
        out_k, al_k = PD.run_batch(*args, align_keep=True, align_split=True, **kw)
        assert out.equals(out_k) and al.equals(al_k) and out.equals(plain, ignore=("route", "reason"))
        routed = np.flatnonzero(out.route == PD.ROUTE_MIRROR)
        assert g in routed and len(routed) < len(out)
        use, undecided = FP.final_use(al)
        want = FP.final_host(out, dp.precision, alignment.lp_caps(dp, out), alignment.lp_row_caps(dp, out), use=use,
                             undecided=undecided)
        FC.assert_equal9(fo, want, "run_batch")
        for x in (int(routed[0]), int(live[0])):  # ... and spectrum by spectrum: a routed one, a device one
            FC.assert_equal9(fo.take([x]), want.take([x]), x)
        assert (fo.status[undecided] == FP.FINAL_UNDECIDED).all() and (fo.status[plain.default] == FP.FINAL_NONE).all()
        _, _, fo_small = PD.run_batch(*args, align_final=True, final_max_combos=2, **kw)
        assert fo_small.equals(FP.final_host(out, dp.precision, alignment.lp_caps(dp, out), alignment.lp_row_caps(dp, out),
                                             use=use, undecided=undecided, max_combos=2))
        dec = FP.final_decisions(fo)
        print("shares", {k: round(v, 3) for k, v in fo.shares().items() if v}, "TAKE", float(dec.mean()), flush=True)
        solved = np.flatnonzero(fo.status == FP.FINAL_SOLVED)
        if len(solved):
            names = FP.sequence_names(fo, out, int(solved[0]))
            assert len(names) == out.seq_len[solved[0]] and all(nm in out.row_names for nm in names)
    finally:
        dp.close()
        engine.trim()
        PD.release_length_buffer()
