"""GPU tests of the alignment certificate's two-list split
(sst_align_split_device, k_align_split in csrc/sst_align.hip;
alignment.align_device(split=True), run_batch(align_split=True)): the device
result equals alignment.align_host(..., K, split=True) in all four outputs --
on runs of unconstrained positions over the real row masses, on spectra that
mix constrained and unconstrained positions, at the capacity's edge of the
second list, at the window's edges, and through run_batch."""
import itertools
import math

import numpy as np
import pytest

import _align_cases as AC
import _align_gpu as AG
import _align_split_cases as ASC
from _align_gpu import (CHUNK, FIELDS, OBS_W, K, device_args, edge_positions, engine, full_table,  # noqa: F401
                        prefix_counts, window_frags)
from conftest import load_golden

pytestmark = pytest.mark.gpu
def run(dp, specs, rm, K):
    """(outcome, device split, host split at capacity K, device base) of a
    case; asserts the device split equal to the host's in all four outputs."""
    from spectrseqtools_amd import alignment

    o, dev, host = AG.run(dp, specs, rm, K, split=True)
    return o, dev, host, alignment.align_device(dp, o)


def assert_rest_untouched(dev, base):
    """Fragments not OPEN at base are bit-identical to the base call's."""
    keep = base.status != AC.OPEN
    for k in FIELDS:
        assert np.array_equal(getattr(dev, k)[keep], getattr(base, k)[keep]), k
    assert (dev.alignable <= base.alignable).all()


def run_counts(masses, n):
    """Distinct sums of runs of 1 .. n positions that each take any of `masses`."""
    out, sums = [], np.zeros(1, np.int64)
    for _ in range(n):
        sums = np.unique(np.add.outer(sums, np.array(sorted(set(masses)), dtype=np.int64)))
        out.append(len(sums))
    return out


def test_run_lengths_on_real_masses(full_table, K):
    """L = 14 unconstrained positions over rows 1 .. 8 of the full table: runs
    of <= 6 positions are closed, 7 .. 12 split-closed, 13 and 14 undecided
    (recounted here).  One spectrum with more base-OPEN fragments than a chunk
    holds, one with its fragments out of su order."""
    from spectrseqtools_amd import alignment

    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    alpha = AC.mask(range(1, 9))
    counts = run_counts(rm[1:9], 8)
    assert counts == [8, 33, 98, 238, 503, 958, 1683, 2773], counts
    closed = max(n for n in range(1, 9) if counts[n - 1] <= K)
    assert closed == 6 and 14 > 2 * closed  # 7 .. 12 positions split into two closed runs, 13 and 14 do not
    rng = np.random.default_rng(11)
    spec = {"L": 14, "pos": [(0, 0)] * 14, "alpha": alpha}
    sets = AC.position_masses(spec, rm)
    spec["frags"] = window_frags(rng, sets, 560, range(7, 15), dp.precision)
    part = [spec["frags"][i] for i in rng.permutation(len(spec["frags"]))[:150]]
    assert any(a[1] > b[1] for a, b in zip(part, part[1:]))
    specs = [spec, dict(spec, frags=part)]
    o, dev, host, base = run(dp, specs, rm, K)
    was_open = base.status == AC.OPEN
    assert int(was_open[:len(spec["frags"])].sum()) > CHUNK
    ends = {s: int(((dev.status == s) & was_open).sum()) for s in (AC.FIT, AC.NONE, AC.OPEN)}
    print("base-OPEN", int(was_open.sum()), "end FIT / NONE / OPEN", ends, flush=True)
    assert all(ends.values()) and sum(ends.values()) == int(was_open.sum())
    assert_rest_untouched(dev, base)
    exact = alignment.align_host(o, dp.tolerance, dp.precision, 10**9)
    decided = was_open & (dev.status != AC.OPEN)
    assert np.array_equal(dev.status[decided], exact.status[decided])
    w_seen = {math.ceil(dp.tolerance * f[2] / dp.precision) for f, d in zip(spec["frags"], decided) if d}
    assert w_seen == {0, 1, 30}


def test_mixed_spectra(full_table, K):
    """Constrained positions (1 .. 3 rows) between unconstrained runs on a
    20-row alphabet, in one batch with a spectrum without an OPEN fragment, an
    INFEASIBLE one, one with SKIPPED fragments (mn out of range) and L = 1."""
    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    rows = list(range(1, 21))
    alpha = AC.mask(rows)
    assert [c > K for c in run_counts([rm[r] for r in rows], 4)] == [False, False, False, True]
    rng = np.random.default_rng(12)

    def positions(L):
        pos = []
        while len(pos) < L:
            pos += [(0, 0)] * int(rng.integers(2, 6))
            pos += [AC.mask(rng.choice(rows, size=int(rng.integers(1, 4)), replace=False).tolist())
                    for _ in range(int(rng.integers(1, 3)))]
        return pos[:L]

    def spectrum(pos, n, lengths):
        sp = {"L": len(pos), "pos": pos, "alpha": alpha}
        sp["frags"] = window_frags(rng, AC.position_masses(sp, rm), n, lengths, dp.precision)
        return sp

    specs = [spectrum(positions(L), 40, range(3, L + 1)) for L in (9, 12, 16, 11, 14, 7)]
    n_mixed = len(specs)
    no_open = spectrum([AC.mask([int(r)]) for r in rng.choice(rows, size=10)], 24, range(1, 11))
    infeasible = spectrum(positions(8), 12, range(3, 9))
    infeasible["pos"][3] = AC.mask([30])  # a row outside the alphabet: A_3 is empty
    skipped = spectrum(positions(10), 24, range(4, 11))
    skipped["frags"] = [(c, su, obs, 10 if (c >> 2) & 3 == 1 else mn, mx) for c, su, obs, mn, mx in skipped["frags"]]
    one = spectrum([(0, 0)], 8, range(1, 2))
    specs += [no_open, infeasible, skipped, one]
    o, dev, host, base = run(dp, specs, rm, K)
    f = o.frag_off
    at = lambda i: slice(int(f[i]), int(f[i + 1]))  # noqa: E731
    assert not (base.status[at(n_mixed)] == AC.OPEN).any() and not (base.status[at(n_mixed + 3)] == AC.OPEN).any()
    assert (dev.status[at(n_mixed + 1)] == AC.INFEASIBLE).all()
    sk = dev.status[at(n_mixed + 2)]
    assert (sk == AC.SKIPPED).sum() >= 4 and (base.status[at(n_mixed + 2)] == AC.OPEN).any()
    was_open = base.status == AC.OPEN
    ends = {s: int(((dev.status == s) & was_open).sum()) for s in (AC.FIT, AC.NONE, AC.OPEN)}
    print("base-OPEN", int(was_open.sum()), "end FIT / NONE / OPEN", ends, flush=True)
    assert all(ends.values())
    assert set(dev.status.tolist()) == {AC.NONE, AC.FIT, AC.OPEN, AC.INFEASIBLE, AC.SKIPPED}
    assert_rest_untouched(dev, base)


def test_capacity_edge_of_the_second_list(full_table, K):
    """Both halves with exactly K sums: decided; K + 1 in the second half:
    undecided (K and K + 1 counted here), forward and, on the mirrored
    spectrum, through the END class's backward sweep."""
    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    alpha = AC.mask(range(1, len(rm)))
    half, more, d = edge_positions(rm, K)
    pos = half + half + [more]  # [0, n - 1]: K sums; + the next position: open; [n, 2 n - 1]: K sums; + more: K + 1
    n, L = len(half), 2 * len(half) + 1
    assert L <= 253 and d >= 3
    sets = AC.position_masses({"pos": pos, "alpha": alpha}, rm)
    first, _ = prefix_counts(sets[:n + 1])
    second, _ = prefix_counts(sets[n:])
    assert first[n - 1] == K and first[n] > K and second[n - 1] == K and second[n] == K + 1
    lo = lambda r: sum(min(m) for m in sets[:r + 1])  # noqa: E731
    start, prec = AC.code_of(True, False), dp.precision
    r1, r2 = 2 * n - 1, 2 * n
    frags = [(start, (lo(r1) + K * d) * prec, 0.0, r1, r1),            # [0, r1] only: K and K sums, a sum of both: FIT
             (start, (lo(r1) + K * d + 1) * prec, 0.0, r1, r1),        # between two sums: NONE
             (start, (lo(r2) + K * d) * prec, 0.0, r2, r2),            # [0, r2] only: the second half has K + 1: OPEN
             (AC.code_of(True, True), (lo(r2) + K * d + 1) * prec, 0.0, 0, 0),  # the same interval: OPEN
             (start, (lo(r2) + 4 * K * d) * prec, 0.0, r2, r2)]        # beyond HI: NONE at base already
    want = [AC.FIT, AC.NONE, AC.OPEN, AC.OPEN, AC.NONE]
    spec = {"L": L, "pos": pos, "alpha": alpha, "frags": sorted(frags, key=lambda f: f[1])}
    order = np.argsort(np.argsort([f[1] for f in frags]))
    o, dev, host, base = run(dp, [spec, ASC.mirrored(spec)], rm, K)
    nf = len(frags)
    assert base.status[order].tolist() == [AC.OPEN] * 4 + [AC.NONE]
    for side in (0, nf):  # the spectrum, then its mirror image (END fragments, the backward sweep)
        assert dev.status[side + order].tolist() == want, side
        assert dev.n_fit[side + order].tolist() == [1, 0, 0, 0, 0]
    assert dev.first[order[0]] == r1 and dev.first[nf + order[0]] == (L - 1 - r1) << 8 | (L - 1)
    assert ((o.frag_code[nf:] >> 2) & 3).tolist().count(2) == 4
    assert_rest_untouched(dev, base)


def test_window_edges(full_table, K):
    """First half K sums (step d), second half one position of two rows D
    apart, D beyond the first half's span: every sum is a + b of one pair only.
    a_last + b_first and a_first + b_last sit exactly at target - W and at
    target + W (FIT); one unit further out nothing fits (NONE)."""
    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    alpha = AC.mask(range(1, len(rm)))
    half, _, d = edge_positions(rm, K)
    span = (K - 1) * d
    rows = range(1, len(rm))
    D, two = min((rm[b] - rm[a], (a, b)) for a in rows for b in rows if rm[b] - rm[a] > span + 64)
    pos = half + [AC.mask(two)]
    n, L = len(half), len(half) + 1
    sets = AC.position_masses({"pos": pos, "alpha": alpha}, rm)
    counts, sums = prefix_counts(sets)
    assert counts[n - 1] == K and counts[n] == 2 * K and d > 2 * 4 + 1
    LO = int(sums[0])
    s1, s2 = LO + span, LO + D  # a_last + b_first, a_first + b_last: neighbours in S(0, n), D - span apart
    assert sums[K - 1] == s1 and sums[K] == s2 and sums[K - 2] == s1 - d and sums[K + 1] == s2 + d
    start, prec = AC.code_of(True, False), dp.precision
    frags, want = [], []
    for w in (1, 4):
        for s in (s1, s2):
            for t, fits in ((s + w, True), (s - w, True), (s + w + 1, False), (s - w - 1, False)):
                frags.append((start, t * prec, OBS_W[w], n, n))  # [0, n] only
                want.append(AC.FIT if fits else AC.NONE)
    spec = {"L": L, "pos": pos, "alpha": alpha, "frags": sorted(frags, key=lambda f: f[1])}
    order = np.argsort(np.argsort([f[1] for f in frags], kind="stable"), kind="stable")
    o, dev, host, base = run(dp, [spec, ASC.mirrored(spec)], rm, K)
    nf = len(frags)
    assert (base.status == AC.OPEN).all()
    for side in (0, nf):
        assert dev.status[side + order].tolist() == want, side
    assert dev.n_fit.max() == 1


def test_entry_point_contract(full_table, K):
    """The base call's argument errors also come from the split call; the
    split on its own output changes nothing."""
    import ctypes

    from spectrseqtools_amd import _native, alignment

    OK, E_ARG = 0, -1  # SST_OK, SST_E_ARG
    dp = full_table
    eng = dp.device_table.engine
    lib, handle = eng._lib, dp.device_table.handle
    a = _native.AlignArgs()
    a.n_spec, a.tol, a.prec = 0, dp.tolerance, dp.precision
    assert lib.sst_align_split_device(handle, ctypes.byref(a)) == OK
    a.n_spec = 1
    assert lib.sst_align_split_device(handle, ctypes.byref(a)) == E_ARG
    a.n_spec, a.prec = 0, 0.0
    assert lib.sst_align_split_device(handle, ctypes.byref(a)) == E_ARG
    a.n_spec, a.prec = -1, dp.precision
    assert lib.sst_align_split_device(handle, ctypes.byref(a)) == E_ARG
    assert lib.sst_align_split_device(None, ctypes.byref(a)) == E_ARG
    assert _native.K_ALIGN_SPLIT == 22 < _native.K_COUNT and _native.KERNEL_NAMES[22] == "k_align_split"

    rm = [int(m.mass) for m in dp.masses]
    rng = np.random.default_rng(13)
    spec = {"L": 14, "pos": [(0, 0)] * 14, "alpha": AC.mask(range(1, 9))}
    spec["frags"] = window_frags(rng, AC.position_masses(spec, rm), 60, range(7, 15), dp.precision)
    o = AC.make_outcome([spec], rm)
    args, keep, outs = device_args(dp, o)
    eng.check(lib.sst_align_windows_device(handle, ctypes.byref(args)), "sst_align_windows_device")
    eng.check(lib.sst_align_split_device(handle, ctypes.byref(args)), "sst_align_split_device")
    eng.synchronize()
    once = [x.cpu().numpy().copy() for x in outs]
    eng.check(lib.sst_align_split_device(handle, ctypes.byref(args)), "sst_align_split_device")
    eng.synchronize()
    twice = [x.cpu().numpy() for x in outs]
    assert all(np.array_equal(x, y) for x, y in zip(once, twice))
    host = alignment.align_host(o, dp.tolerance, dp.precision, K, split=True)
    assert np.array_equal(once[0], host.status) and np.array_equal(once[2].view(np.uint32), host.n_fit)
    assert (host.status == AC.OPEN).any() and (host.status == AC.FIT).any()


def test_run_batch_align_split(engine, K):
    """run_batch(align_split=True) on the synthetic reference spectra, the
    largest spectrum that has fragments forced onto the mirror route (as
    test_gpu_align.py's test_run_batch_align): align_device(split=True) on the
    device's spectra, align_host(split=True) on the routed ones;
    run_batch(align=True) is unchanged."""
    import _synth_cases as SC
    from spectrseqtools_amd import alignment, pipeline_device as PD
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
        g = int(live[np.argmax(peaks[live])])  # onto the mirror route: the largest spectrum that has fragments
        kw["limits"] = PD.DeviceLimits(max_peaks=int(peaks[g]) - 1)
        out_a, al_a = PD.run_batch(*args, align=True, **kw)
        out, al = PD.run_batch(*args, align_split=True, **kw)
        assert out.equals(out_a) and out.equals(plain, ignore=("route", "reason"))
        routed = np.flatnonzero(out.route == PD.ROUTE_MIRROR)
        on_dev = np.flatnonzero(out.route != PD.ROUTE_MIRROR)
        assert g in routed and len(on_dev) >= 10
        assert al_a.equals(alignment.align_host(out, dp.tolerance, dp.precision, K))
        assert al.take(on_dev).equals(alignment.align_device(dp, out.take(on_dev), split=True))
        assert al.take(routed).equals(alignment.align_host(out.take(routed), dp.tolerance, dp.precision, K, split=True))
        assert al.equals(alignment.align_host(out, dp.tolerance, dp.precision, K, split=True))
        assert len(al.status) == int(out.frag_off[-1]) > 100
        print("status shares: base", al_a.shares(), "split", al.shares(), flush=True)
        keep = al_a.status != AC.OPEN
        assert all(np.array_equal(getattr(al, k)[keep], getattr(al_a, k)[keep]) for k in FIELDS)
    finally:
        dp.close()
        engine.trim()  # (trim=False kept the frontier's workspace and the reach buffer between the calls)
        PD.release_length_buffer()
