"""GPU tests of the length program (sst_length_program_device: k_length_program
in csrc/sst_length_program.hip; length_program.length_program_device,
run_batch(length_program=True)): every output array equals
length_program.length_program_host's -- which tests/test_length_program_model.py
holds to the brute force -- on random small spectra, at the edges of the
candidate lengths, of max_combos, of the shapes and of the fixed-point limits,
on tables of 64, 65 and 120 rows, across passes of the workgroup and chunks of
fragment records, on a workgroup's later candidates, and through run_batch."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import _length_cases as LC
from _align_gpu import engine, full_table  # noqa: F401
from conftest import load_golden

pytestmark = pytest.mark.gpu
PREC = 0.001
E_ARG = -1  # SST_E_ARG


def table_of(engine, n_rows):
    """A table of n_rows rows of ascending distinct masses, dressed as the fields length_program_device reads."""
    from spectrseqtools_amd import _native

    rm = [0] + [300000 + 1009 * i for i in range(1, n_rows)]
    table = _native.DeviceTable.build(rm, max(rm) * 4, 32, engine=engine)
    return SimpleNamespace(masses=[SimpleNamespace(mass=m) for m in rm], device_table=table, precision=PREC,
                           tolerance=1e-5), rm


@pytest.fixture(scope="module")
def small_table(engine):
    dp, rm = table_of(engine, 8)
    yield dp, rm
    dp.device_table.close()


def run(dp, specs, rm, row_mod, rate, rates=None, max_combos=1 << 20, what=""):
    """(cases, valid, caps, device result) of a case; asserts the device equal to the host model in every array."""
    from spectrseqtools_amd import length_program as LP

    cases = LC.make_cases(specs, rm)
    caps = LC.caps_of(specs, len(rm), row_mod, rate, rates)
    valid = LP.length_valid(cases, dp.precision)
    want = LP.length_program_host(cases, dp.precision, valid, caps, max_combos=max_combos)
    got = LP.length_program_device(dp, cases, max_combos=max_combos, valid=valid, caps=caps)
    for k in ("cand_off", "cand_len") + LP.LengthOutcome.SPECTRUM_FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k)
    LC.assert_equal4(got, want, what)
    return cases, valid, caps, got


def test_random_small_spectra(small_table):
    """400 random spectra, M <= 12, at most 4 candidates each, sets of <= 3 rows:
    at max_combos = 64 every status shares one launch."""
    dp, rm = small_table
    specs, row_mod, rate, rates = LC.random_case(31, rm, dp.precision, 400, max_M=12)
    assert max(s["M"] for s in specs) == 12 and max(len(LC.candidates_of(s)) for s in specs) == 4
    *_, got = run(dp, specs, rm, row_mod, rate, rates, 64, "random, max_combos 64")
    n = np.bincount(got.status, minlength=7)
    print("statuses", n.tolist(), flush=True)
    assert (n > 0).all() and n[LC.SOLVED] >= 200, n


EDGES = ("lengths_1_M_253", "no_candidates_and_above_M", "combos_at_max", "combos_above_max", "one_lane",
         "mod_cap_binds", "mod_cap_no_feasible", "empty_A_i", "not_free", "shape_boundaries", "513_fragments",
         "fixed_point_limit")
WANT = {"lengths_1_M_253": [LC.SOLVED] * 3, "combos_at_max": [LC.SOLVED], "combos_above_max": [LC.TOO_LARGE],
        "one_lane": [LC.SOLVED], "mod_cap_binds": [LC.SOLVED], "mod_cap_no_feasible": [LC.INFEASIBLE],
        "empty_A_i": [LC.INFEASIBLE], "not_free": [LC.NOT_FREE], "513_fragments": [LC.SOLVED],
        "no_candidates_and_above_M": [LC.SOLVED, LC.SOLVED, LC.NOT_MODELLED, LC.NOT_MODELLED, LC.NOT_MODELLED,
                                      LC.SOLVED],
        "fixed_point_limit": [LC.SOLVED, LC.SOLVED] + [LC.NOT_MODELLED] * 3}


@pytest.mark.parametrize("name", EDGES)
def test_edge_cases(small_table, name):
    """c of 1, M and 253 with lower == upper; lower > upper and raised bounds (no
    candidates), a candidate above M and one below 1; combos == max_combos and
    max_combos + 1; one lane; mod_cap binding and with n_feas == 0; an empty A_i;
    NOT_FREE; each shape and each RAISES condition at its boundary (mn = c - 1
    and c, mx = c and c + 1, the wrapped END range and its last index, mn > mx);
    513 fragments; fragments at the fixed-point limit."""
    dp, rm = small_table
    specs, row_mod, rate, rates, max_combos = LC.edge_cases(rm, dp.precision)[name]
    *_, got = run(dp, specs, rm, row_mod, rate, rates, max_combos, name)
    if name in WANT:
        assert got.status.tolist() == WANT[name], (name, got.status.tolist())
    if name == "lengths_1_M_253":
        assert got.cand_len.tolist() == [253, 1, 4] and got.combos.tolist() == [12, 2, 4] and not got.best.any()
    if name == "mod_cap_binds":
        assert got.combos.tolist() == [8] and got.n_feas.tolist() == [4]
    if name == "mod_cap_no_feasible":
        assert got.combos.tolist() == [8] and got.n_feas.tolist() == [0]
    if name == "shape_boundaries":
        st = dict(zip(("start_mn_c-1", "start_mn_c", "start_mx_over", "start_mn_gt_mx", "start_empty",
                       "start_empty_wrap", "start_raises_wrap", "start_no_ones", "end_mx_c", "end_mx_c+1",
                       "end_mn_gt_mx", "end_wrapped", "end_wrapped_last", "end_raises_wrap", "end_empty",
                       "end_no_ones", "end_range", "internal", "whole"), got.status.tolist()))
        raises = {k for k, v in st.items() if v == LC.RAISES}
        assert raises == {"start_mn_c", "start_raises_wrap", "end_mx_c+1", "end_raises_wrap"}, st
        assert {k for k, v in st.items() if v == LC.NOT_MODELLED} == {"start_no_ones", "end_no_ones", "internal"}, st
        assert all(v == LC.SOLVED for k, v in st.items() if k not in raises | {"start_no_ones", "end_no_ones",
                                                                                "internal"}), st


@pytest.mark.parametrize("n_rows", [64, 65, 120])
def test_table_sizes(engine, n_rows):
    """Tables of 64, 65 and 120 rows: position sets over the highest rows (both
    mask words), modified high rows, and 255, 256 and 258 assignments (257 is
    prime: no product of radices) -- one short of a pass, a full pass, a second
    pass."""
    dp, rm = table_of(engine, n_rows)
    try:
        top = n_rows - 1
        row_mod = np.zeros(n_rows, np.uint8)
        row_mod[top] = row_mod[top - 4] = 1
        high = [[1, top], [top - 3, top - 2, top - 1, top], [2], [top - 4, top]]
        specs = [LC.solved_spec(rm, high, dp.precision),
                 LC.solved_spec(rm, LC.free_positions(rm, [3, 5, 17], fixed=1), dp.precision),
                 LC.solved_spec(rm, LC.free_positions(rm, [2] * 8), dp.precision),
                 LC.solved_spec(rm, LC.free_positions(rm, [2, 3, 43], fixed=2), dp.precision),
                 LC.solved_spec(rm, [list(range(1, n_rows))[-min(n_rows - 1, 127):], [top]], dp.precision)]
        *_, got = run(dp, specs, rm, row_mod, 0.5, None, 1 << 20, n_rows)
        assert got.status.tolist() == [LC.SOLVED] * 5
        assert got.combos.tolist() == [16, 255, 256, 258, min(n_rows - 1, 127)]
        assert got.n_feas[[0, 4]].tolist() == [14, got.combos[4] - 2] and got.n_feas[1:4].tolist() == [255, 256, 258]
        assert not got.best[1:4].any() and got.best[0] > 0  # (the pinned y of the first holds two modified rows)
    finally:
        dp.device_table.close()


def test_later_candidates_forward_and_reversed(small_table):
    """More candidates than the grid has workgroups: a workgroup's second and
    later candidates carry no state over (every status in the batch, spectra
    forward and reversed)."""
    dp, rm = small_table
    specs, row_mod, rate, rates = LC.random_case(47, rm, dp.precision, 2200, max_M=6)
    import torch

    n_cu = torch.cuda.get_device_properties(dp.device_table.engine.device).multi_processor_count
    *_, fwd = run(dp, specs, rm, row_mod, rate, rates, 32, "forward")
    assert len(fwd.status) > 2 * 3 * n_cu and (np.bincount(fwd.status, minlength=7) > 0).all()
    *_, rev = run(dp, specs[::-1], rm, row_mod, rate, rates, 32, "reversed")
    assert rev.take(np.arange(len(specs))[::-1]).equals(fwd)


def raw_args(dp, cases, valid, caps, max_combos):
    """sst_length_program_args over device copies, and the tensors (inputs, outputs)."""
    import torch

    from spectrseqtools_amd import _native

    dev = torch.device("cuda", dp.device_table.engine.device)
    up = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt).reshape(-1), device=dev)  # noqa: E731
    cand_off, cand_len = cases.candidates()
    keep = [up(cases.max_len, np.int32), up(cases.skel_off, np.int64), up(cases.skeleton.view(np.int64), np.int64),
            up(cases.alpha.view(np.int64), np.int64), up(cases.frag_off, np.int64), up(cases.frag_code, np.uint8),
            up(cases.frag_su, np.float64), up(cases.frag_min_end, np.int32), up(cases.frag_max_end, np.int32),
            up(cand_off, np.int64), up(cand_len, np.int32), up(valid, np.uint8), up(caps[1], np.int32),
            up(caps[0], np.uint8), up(caps[2], np.int32)]
    n = len(cand_len)
    outs = [torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)] + \
        [torch.full((n,), 0x5A5A5A5A, dtype=torch.int64, device=dev) for _ in range(3)]
    a = _native.LengthProgramArgs()
    a.n_spec, a.n_cand = len(cases), n
    (a.max_len, a.skel_off, a.skeleton, a.alpha, a.frag_off, a.frag_code, a.frag_su, a.frag_min_end, a.frag_max_end,
     a.cand_off, a.cand_len, a.valid, a.mod_cap, a.row_mod, a.row_cap) = (x.data_ptr() for x in keep)
    a.prec, a.max_combos = float(dp.precision), int(max_combos)
    a.status, a.combos, a.n_feas, a.best = (x.data_ptr() for x in outs)
    torch.cuda.synchronize(dev)
    return a, keep, outs


def test_same_call_twice_and_argument_errors(small_table):
    """The same call twice into the same buffers gives the same arrays, every
    element written; the argument errors come with a message and launch
    nothing."""
    from spectrseqtools_amd import _native, length_program as LP

    dp, rm = small_table
    eng = dp.device_table.engine
    specs, row_mod, rate, rates = LC.random_case(53, rm, dp.precision, 60, max_M=8)
    cases, valid, caps, want = run(dp, specs, rm, row_mod, rate, rates, 64, "twice")
    a, keep, outs = raw_args(dp, cases, valid, caps, 64)
    call = lambda x: eng._lib.sst_length_program_device(dp.device_table.handle, x)  # noqa: E731
    results = []
    for _ in range(2):
        assert call(ctypes.byref(a)) == 0
        eng.synchronize()
        results.append([x.cpu().numpy().copy() for x in outs])
    for k, (x, y) in enumerate(zip(*results)):
        assert np.array_equal(x, y), k
    got = results[1]
    assert np.array_equal(got[0], want.status) and np.array_equal(got[1].view(np.uint64), want.combos)
    assert np.array_equal(got[2].view(np.uint64), want.n_feas) and np.array_equal(got[3].view(np.uint64), want.best)

    def refused(**change):
        b = _native.LengthProgramArgs.from_buffer_copy(a)
        for k, v in change.items():
            setattr(b, k, v)
        rc = call(ctypes.byref(b))
        assert rc == E_ARG, (change, rc)
        return eng._lib.sst_last_error(eng.handle).decode()

    assert call(None) == E_ARG
    assert "max_combos" in refused(max_combos=0) and "max_combos" in refused(max_combos=(1 << 22) + 1)
    for prec in (0.0, -1.0, float("nan"), float("inf")):
        assert "prec" in refused(prec=prec)
    for name, _ in _native.LengthProgramArgs._fields_:
        if name not in ("n_spec", "n_cand", "prec", "max_combos"):
            assert "NULL member" in refused(**{name: None}), name
    assert "n_cand" in refused(n_cand=-1) and "n_spec" in refused(n_spec=-1)
    b = _native.LengthProgramArgs.from_buffer_copy(a)
    b.n_spec = 0
    for k, _ in _native.LengthProgramArgs._fields_[2:]:
        if k not in ("prec", "max_combos"):
            setattr(b, k, None)
    assert call(ctypes.byref(b)) == 0  # n_spec == 0 is SST_OK
    with pytest.raises(ValueError):
        LP.length_program_device(dp, cases, max_combos=0, valid=valid, caps=caps)
    for x, y in zip(outs, results[1]):  # the refused calls wrote nothing
        assert np.array_equal(x.cpu().numpy(), y)


def test_row_mass_limits(engine):
    """A row mass of 2^32 / 253 or more is refused, as by the align calls."""
    from spectrseqtools_amd import _native

    rm = [0, 305042, (1 << 32) // 253]
    table = _native.DeviceTable.build(rm, max(rm) * 2, 32, engine=engine)
    dp = SimpleNamespace(masses=[SimpleNamespace(mass=m) for m in rm], device_table=table, precision=PREC, tolerance=1e-5)
    try:
        spec = LC.solved_spec([0, 305042, 306026], [[1]], PREC)
        cases = LC.make_cases([spec], [0, 305042, 306026])
        caps = LC.caps_of([spec], 3, np.zeros(3, np.uint8), 1.0)
        a, keep, outs = raw_args(dp, cases, np.ones(1, np.uint8), caps, 16)
        assert engine._lib.sst_length_program_device(table.handle, ctypes.byref(a)) == E_ARG
    finally:
        table.close()


def test_run_batch_length_program(engine):
    """run_batch(length_program=True) on the synthetic spectra, one spectrum
    forced onto the mirror route: the first result equals the plain run_batch's
    field by field, the LengthOutcome of the device's spectra equals
    length_program_host on the same cases, the routed spectrum is undecided."""
    import _synth_cases as SC
    from spectrseqtools_amd import length_program as LP, pipeline_device as PD
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
        record = {}
        combos = 1 << 12
        out, lo = PD.run_batch(*args, length_program=True, length_max_combos=combos, record=record, **kw)
        assert out.equals(PD.run_batch(*args, **kw)) and out.equals(plain, ignore=("route", "reason"))
        assert len(lo) == len(out) and lo.undecided[g] == 1 and lo.cand_off[g] == lo.cand_off[g + 1]
        cases, d_idx = record["length_cases"], record["device_index"]
        assert lo.undecided.sum() == len(out) - len(d_idx)
        valid = LP.length_valid(cases, dp.precision)
        want = LP.length_program_host(cases, dp.precision, valid, LP.length_caps(dp, cases), max_combos=combos)
        dev = lo.take(d_idx)
        for k in ("cand_off", "cand_len") + LP.LengthOutcome.SPECTRUM_FIELDS:
            assert np.array_equal(getattr(dev, k), getattr(want, k)), k
        LC.assert_equal4(dev, want, "run_batch")
        n_st = np.bincount(lo.status, minlength=7)
        decision, length = LP.length_decisions(lo)
        print("candidates", len(lo.status), "statuses", n_st.tolist(), "decisions",
              np.bincount(decision, minlength=4).tolist(), "TAKE != Jaccard",
              int(((decision == LP.LENGTH_TAKE) & (length != out.seq_len)).sum()), flush=True)
        assert len(lo.status) >= len(d_idx) and decision[g] == LP.LENGTH_SOLVE
        # the kept rows of length_cases are the walk's: per spectrum what skeleton_frames shows
        assert (np.diff(cases.frag_off) > 0).any() and (cases.lower[cases.lb_status == 0] >= 0).all()
        # with the other results: the LengthOutcome comes last and nothing before it changes
        out2, al2, lo2 = PD.run_batch(*args, align=True, length_program=True, length_max_combos=combos, **kw)
        out3, al3 = PD.run_batch(*args, align=True, **kw)
        assert out2.equals(out3) and al2.equals(al3) and lo2.equals(lo)
    finally:
        dp.close()
