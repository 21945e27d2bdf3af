"""GPU tests of the alignment certificate (sst_align_windows_device,
csrc/sst_align.hip; alignment.align_device, run_batch(align=True)): the
device result equals alignment.align_host at the device's capacity in all four
outputs -- on random spectra over the small alphabets of tables.json (also
against the brute force of tests/_align_cases.py), on a batch of shapes chosen
to stress the kernel, on the full alphabet at the capacity's edge, and through
run_batch on the synthetic reference spectra."""
import types

import numpy as np
import pytest

import _align_cases as AC
import _align_gpu as AG
from _align_gpu import CHUNK, K, engine, full_table  # noqa: F401
from conftest import load_golden

pytestmark = pytest.mark.gpu
TOL, PREC = 0.02, 0.5  # the small alphabets' (W = ceil(0.04 obs))
WAVES = 4              # waves of a k_align_windows workgroup


@pytest.fixture(scope="module")
def small_tables(engine):
    """One built table per distinct small alphabet of tables.json, dressed as
    the DynamicProgrammingTable fields align_device reads."""
    from spectrseqtools_amd import _native

    out, seen = [], set()
    for tiny in load_golden("tables.json")["tiny"]:
        ms = tuple(tiny["masses"])
        if ms in seen or tiny["compression"] != 32:
            continue
        seen.add(ms)
        dev = _native.DeviceTable.build(list(ms), tiny["max_mass"], 32, engine=engine)
        out.append(types.SimpleNamespace(device_table=dev, masses=[types.SimpleNamespace(mass=m) for m in ms],
                                         tolerance=TOL, precision=PREC, row_mass=list(ms)))
    assert len(out) == 6
    yield out
    for t in out:
        t.device_table.close()


def both(dp, specs, row_mass, K):
    """(device, host at capacity K) certificates of a case; asserts them equal."""
    _, dev, host = AG.run(dp, specs, row_mass, K)
    return dev, host


def test_random_spectra(small_tables, K):
    """64 random spectra per small alphabet, as the CPU test's; the brute
    force agrees too (no S here has more than 729 sums)."""
    statuses = set()
    for k, dp in enumerate(small_tables):
        specs = AC.random_case(100 + k, dp.row_mass, TOL, PREC, 64)
        dev, _ = both(dp, specs, dp.row_mass, K)
        st, al, nf, fi, biggest = AC.brute(specs, dp.row_mass, TOL, PREC, K)
        assert biggest <= 729
        AC.assert_equal(dev, (st, al, nf, fi), ("brute", dp.row_mass))
        statuses |= set(dev.status.tolist())
    assert statuses == {AC.NONE, AC.FIT, AC.INFEASIBLE, AC.SKIPPED}


def _ladder(rng, sets_mass, n, W_of, classes=(0, 1, 2, 3), L=None):
    """n fragments around sums of random windows of the positions' masses."""
    L = len(sets_mass) if L is None else L
    frags = []
    for i in range(n):
        cls = classes[i % len(classes)]
        start, end = bool(cls & 1), bool(cls & 2)
        l = 0 if start else int(rng.integers(0, L))
        r = L - 1 if end else int(rng.integers(l, min(L, l + 12)))
        true = sum(int(rng.choice(m)) for m in sets_mass[l:r + 1])
        obs = float(rng.choice([0.0, 3.0, 40.0]))
        su = (true + int(rng.integers(-2, 3)) * (W_of(obs) + 1) // 2) * PREC
        mn, mx = (r, r) if start and not end else (l, l) if end and not start else (0, 0)
        if i % 7 == 3:
            mn, mx = max(0, mn - 2), min(L - 1, mx + 2)
        frags.append((AC.code_of(start, end), su, obs, mn, mx))
    return sorted(frags, key=lambda f: f[1])


def test_stress_shapes(small_tables, K):
    """One batch on the alphabet [0, 4, 13, 31, 37]: L = 1; L one more than a
    workgroup's waves (a wave takes a second left end); a spectrum without
    fragments; a default spectrum; 1 and 65 fragments; more fragments than one
    chunk, and the same out of su order; twelve positions {a, b} (13 sums, stays
    closed); L = 253 of one-row positions; W = 0; more spectra than the grid
    has workgroups.  Then the first spectrum alone (a batch with S = 1)."""
    import math

    dp = [t for t in small_tables if t.row_mass == [0, 4, 13, 31, 37]][0]
    rm = dp.row_mass
    rng = np.random.default_rng(3)
    W_of = lambda obs: math.ceil(TOL * obs / PREC)  # noqa: E731
    alpha = AC.mask([1, 2, 3, 4])
    masses = lambda pos: AC.position_masses({"pos": pos, "alpha": alpha}, rm)  # noqa: E731

    def spectrum(pos, n, **kw):
        return {"L": len(pos), "pos": pos, "alpha": alpha, "frags": _ladder(rng, masses(pos), n, W_of, **kw)}

    any_pos = lambda n: [AC.mask(rng.choice([1, 2, 3, 4], size=int(rng.integers(1, 3)), replace=False).tolist())  # noqa: E731
                         for _ in range(n)]
    specs = [spectrum(any_pos(1), 6),                                   # L = 1
             spectrum(any_pos(WAVES + 1), 12),                          # a second left end for wave 0
             {"L": 3, "pos": any_pos(3), "alpha": alpha, "frags": []},  # no fragments
             {"default": True},
             spectrum(any_pos(7), 1, classes=(0,)),
             spectrum(any_pos(9), 65)]
    big = spectrum(any_pos(10), CHUNK + 17)                             # two chunks
    shuffled = dict(big, frags=[big["frags"][i] for i in rng.permutation(len(big["frags"]))])
    twelve = spectrum([AC.mask([1, 2])] * 12, 40)                       # S(0, 11) = 12 * 4 + 9 k, k = 0 .. 12
    assert len({sum(c) for c in __import__("itertools").product(*masses(twelve["pos"]))}) == 13
    long_one = spectrum([AC.mask([int(r)]) for r in rng.integers(1, 5, 253)], 30)
    w_zero = spectrum(any_pos(6), 24)
    w_zero["frags"] = sorted([(c, su, 0.0, mn, mx) for c, su, _, mn, mx in w_zero["frags"]], key=lambda f: f[1])
    specs += [big, shuffled, twelve, long_one, w_zero]
    specs += [spectrum(any_pos(int(rng.integers(1, 5))), 3) for _ in range(600)]  # > 2 workgroups per CU x 256 CUs
    dev, host = both(dp, specs, rm, K)
    assert not (dev.status == AC.OPEN).any()  # (twelve {a, b} positions included)
    assert (dev.status == AC.FIT).sum() > 400 and (dev.status == AC.NONE).sum() > 200
    f = AC.make_outcome(specs, rm).frag_off
    twelve_at, long_at = slice(f[8], f[9]), slice(f[9], f[10])
    print("twelve n_fit", dev.n_fit[twelve_at].tolist(), "long status", dev.status[long_at].tolist(), flush=True)
    assert (dev.status[long_at] == AC.FIT).sum() >= 10 and (dev.n_fit[twelve_at] > 1).any()
    fits = dev.first[long_at][dev.status[long_at] == AC.FIT]
    assert (fits >> 8).max() > 100  # a fit found from a far left end of the 253 positions
    one, _ = both(dp, specs[:1], rm, K)
    assert np.array_equal(one.status, dev.status[:f[1]])


def capacity_edge_positions(row_mass, K):
    """Position sets on the full alphabet whose prefix sums number exactly K at
    one prefix and K + 1 at the next: with d the smallest difference of two row
    masses, pairs of rows k * d apart (k <= the steps so far + 1) keep S an
    arithmetic progression of step d, lengthened by k per position."""
    rows = range(1, len(row_mass))
    d = min(abs(row_mass[a] - row_mass[b]) for a in rows for b in rows if row_mass[a] != row_mass[b])
    pair = {}
    for a in rows:
        for b in rows:
            if row_mass[b] > row_mass[a] and (row_mass[b] - row_mass[a]) % d == 0:
                pair.setdefault((row_mass[b] - row_mass[a]) // d, (a, b))
    pos, steps = [], 0
    while steps < K:  # K - 1 steps: K sums; one more step: K + 1
        k = max(k for k in pair if k <= min(steps + 1, max(1, K - 1 - steps)))
        pos.append(AC.mask(pair[k]))
        steps += k
    assert steps == K and pair[1]
    return pos


def test_capacity_edge_and_open(full_table, K):
    """On the full alphabet: a prefix with exactly K sums stays closed, the
    next (K + 1 sums, by the test's own count) is open; three unconstrained
    positions are open."""
    from spectrseqtools_amd.masses import TOLERANCE

    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    alpha = AC.mask(range(1, len(rm)))
    pos = capacity_edge_positions(rm, K)
    L = len(pos)
    assert L <= 253
    sets = AC.position_masses({"pos": pos, "alpha": alpha}, rm)
    count, sums = [], np.zeros(1, np.int64)
    for m in sets:
        sums = np.unique(np.add.outer(sums, np.array(m, dtype=np.int64)))
        count.append(len(sums))
    assert count[-2] == K and count[-1] == K + 1, count[-3:]
    lo = [sum(min(m) for m in sets[:r + 1]) for r in range(L)]
    mid = lambda r: (lo[r] + (count[r] // 2) * (sums[1] - sums[0])) * TOLERANCE  # noqa: E731 a sum of S(0, r)
    start = AC.code_of(True, False)
    frags = [(start, mid(L - 2), 500.0, L - 2, L - 2),                # [0, L - 2] only: K sums, closed, fits
             (start, mid(L - 1), 500.0, L - 1, L - 1),                # [0, L - 1] only: K + 1 sums, open
             (AC.code_of(True, True), mid(L - 1), 500.0, 0, 0),       # the same interval
             (start, mid(L - 1) + 1e6, 500.0, L - 1, L - 1)]          # beyond HI: NONE although open
    edge = {"L": L, "pos": pos, "alpha": alpha, "frags": sorted(frags, key=lambda f: f[1])}
    three = {"L": 3, "pos": [(0, 0)] * 3, "alpha": alpha,
             "frags": [(AC.code_of(True, True), 3 * 330.0, 990.0, 0, 0),   # inside [LO, HI] of [0, 2]
                       (AC.code_of(False, False), 320.0, 320.0, 0, 0),     # one position holds it
                       (AC.code_of(False, False), 3 * 330.0, 990.0, 0, 0)]}
    assert len({a + b + c for a in rm[1:] for b in rm[1:] for c in rm[1:]}) > K
    dev, _ = both(dp, [edge, three], rm, K)
    order = np.argsort(np.argsort([f[1] for f in frags]))  # where each of `frags` went
    assert dev.status[order].tolist() == [AC.FIT, AC.OPEN, AC.OPEN, AC.NONE]
    assert dev.first[order[0]] == L - 2 and dev.n_fit[order].tolist() == [1, 0, 0, 0]
    assert dev.status[4] == AC.OPEN and dev.status[5] in (AC.FIT, AC.NONE) and dev.status[6] in (AC.FIT, AC.OPEN)


def test_arguments(small_tables):
    """NULL arrays and a non-positive precision are SST_E_ARG; no spectra is fine."""
    import ctypes

    from spectrseqtools_amd import _native

    OK, E_ARG = 0, -1  # SST_OK, SST_E_ARG
    dp = small_tables[0]
    lib = dp.device_table.engine._lib
    a = _native.AlignArgs()
    a.n_spec, a.tol, a.prec = 0, TOL, PREC
    assert lib.sst_align_windows_device(dp.device_table.handle, ctypes.byref(a)) == OK
    a.n_spec = 1
    assert lib.sst_align_windows_device(dp.device_table.handle, ctypes.byref(a)) == E_ARG
    a.n_spec, a.prec = 0, 0.0
    assert lib.sst_align_windows_device(dp.device_table.handle, ctypes.byref(a)) == E_ARG
    a.n_spec, a.prec = -1, PREC
    assert lib.sst_align_windows_device(dp.device_table.handle, ctypes.byref(a)) == E_ARG


def test_run_batch_align(engine, K):
    """run_batch(align=True) on the synthetic reference spectra
    (synth_stages.json.gz's noise_free_exact inputs), the largest spectrum
    that has fragments (and any larger one) forced onto the mirror route
    through `limits`: the BatchOutcome is that of the default call, the
    AlignOutcome align_host's on it."""
    import time

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
        t0 = time.perf_counter()
        plain = PD.run_batch(*args, **kw)
        t1 = time.perf_counter()
        live = np.flatnonzero(~plain.default & (np.diff(plain.frag_off) > 0))
        assert isinstance(plain, PD.BatchOutcome) and len(live) >= 10 and not plain.route.any()
        g = int(live[np.argmax(peaks[live])])  # onto the mirror route: the largest spectrum that has fragments
        kw["limits"] = PD.DeviceLimits(max_peaks=int(peaks[g]) - 1)
        base = PD.run_batch(*args, **kw)
        t2 = time.perf_counter()
        out, al = PD.run_batch(*args, align=True, **kw)
        print(f"run_batch {t1 - t0:.2f} s, one routed {t2 - t1:.2f} s, with align {time.perf_counter() - t2:.2f} s", flush=True)
        assert out.equals(base) and base.equals(plain, ignore=("route", "reason"))
        routed = np.flatnonzero(out.route == PD.ROUTE_MIRROR)
        assert g in routed and routed.tolist() == np.flatnonzero(peaks >= peaks[g]).tolist()
        host = alignment.align_host(out, dp.tolerance, dp.precision, K)
        assert al.equals(host) and len(al.status) == int(out.frag_off[-1]) > 100
        print("status shares:", al.shares(), flush=True)
        assert (al.status == AC.FIT).any()
    finally:
        dp.close()
        engine.trim()  # (trim=False kept the frontier's workspace and the reach buffer between the calls)
        PD.release_length_buffer()
