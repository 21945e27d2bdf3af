"""GPU tests of the alignment certificate's keep mode (sst_align_windows_keep_device,
sst_align_split_keep_device: k_align_windows_keep and k_align_split_keep in
csrc/sst_align.hip; alignment.align_device(keep=), run_batch(align_keep=True)):
the device result equals alignment.align_host(..., keep=...) in all seven arrays
-- on random small spectra over the real masses, at the edges of the inner window
and of the row-free test, across a record chunk, on INFEASIBLE and SKIPPED
spectra, in the split at the capacity's edge and under the budget, and through
run_batch; the caps and plain entry points are untouched."""
import ctypes
import math

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
from _align_gpu import (FIELDS, OBS_W, K, device_args, edge_positions, engine, full_table,  # noqa: F401
                        window_frags)
from conftest import load_golden
from test_gpu_align_caps import capped_counts, far_pairs, rows_in, run_lo

pytestmark = pytest.mark.gpu
START = AC.code_of(True, False)
OBS_IN = 350.0  # W = 4, W_in = 2 on the full table (q = 3.5)


def run(dp, specs, rm, K, caps, row_cap, split=False):
    """(outcome, device, host) of a case in keep mode; asserts the device equal
    to the host model at capacity K in all seven arrays."""
    from spectrseqtools_amd import alignment

    o = AC.make_outcome(specs, rm)
    host = alignment.align_host(o, dp.tolerance, dp.precision, K, split=split, caps=caps, keep=row_cap)
    dev = alignment.align_device(dp, o, split=split, caps=caps, keep=row_cap)
    assert np.array_equal(dev.frag_off, o.frag_off)
    KC.same7(dev, host, ("split", split))
    assert (dev.status[dev.keep == 1] == AC.FIT).all()
    return o, dev, host


def masses_of(dp):
    rm = [int(m.mass) for m in dp.masses]
    assert math.ceil(dp.tolerance * OBS_IN / dp.precision) == 4 and KC.inner_w(OBS_IN, dp.tolerance, dp.precision) == 2
    return rm


def test_random_small_spectra(full_table, K):
    """350 random spectra (L <= 6, sets of <= 3 rows) over the real masses, a
    random row_mod, mixed mod_cap (-1: INFEASIBLE) and per-row rates: base and
    split equal the host model, which the CPU tests hold to the brute force.
    Row-free and not row-free spectra share the launch."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(23)
    row_mod = (rng.random(len(rm)) < 0.5).astype(np.uint8)
    row_mod[0] = 0
    rates = [0.0] + [1.0 if rng.random() < 0.6 else float(rng.choice(KC.RATES)) for _ in rm[1:]]
    row_cap = KC.row_cap_table(rates)
    specs, caps = [], []
    for i in range(350):
        s = AC.random_spectrum(rng, rm, dp.tolerance, dp.precision)
        s["frags"] = [KC.widened(f, rng, dp.tolerance, dp.precision) if rng.random() < 0.5 else f for f in s["frags"]]
        specs.append(s)
        caps.append([math.ceil(0.5 * s["L"]), s["L"], 1, -1, math.ceil(0.25 * s["L"])][i % 5])
    mod_cap = np.array(caps, dtype=np.int32)
    o, dev, host = run(dp, specs, rm, K, (row_mod, mod_cap), row_cap)
    run(dp, specs, rm, K, (row_mod, mod_cap), row_cap, split=True)
    spec_of = np.repeat(np.arange(len(specs)), np.diff(o.frag_off))
    print("kept", int(dev.keep.sum()), "of", len(dev.keep), "row-free", int(dev.spec_free.sum()), flush=True)
    assert dev.keep.sum() >= 40 and 60 <= dev.spec_free.sum() <= 250
    assert not dev.keep[dev.spec_free[spec_of] == 0].any()
    bad = np.isin(dev.status, (AC.INFEASIBLE, AC.SKIPPED))
    assert bad.sum() >= 100 and not dev.keep[bad].any() and (dev.keep_first[bad] == 0xFFFE).all()
    assert not dev.spec_free[np.unique(spec_of[dev.status == AC.INFEASIBLE])].any()
    assert {AC.NONE, AC.FIT, AC.INFEASIBLE, AC.SKIPPED} <= set(dev.status.tolist())


def test_window_and_row_edges(full_table, K):
    """One launch: sums at target +- W_in, +- (W_in + 1), +- W, +- (W + 1) for q
    an exact integer, just above one, below 1, zero, not finite and clamped; and
    the four row-cap edges (row_cap == n_r, n_r - 1 on an unmodified row;
    == mod_cap, mod_cap - 1 on a modified one)."""
    dp = full_table
    rm = masses_of(dp)
    kinds = KC.observed_masses(dp.tolerance, dp.precision)
    assert "above" in kinds and "integer" in kinds
    unmod, mod = (1, 2, 4, 5), (7, 9)
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[list(mod)] = 1
    edge, notes = KC.window_edge_spec(rm, (1, 2), dp.tolerance, dp.precision)
    edge["mod_cap"] = 0
    rows, want_free = KC.row_edge_specs(rm, unmod, mod, dp.tolerance, dp.precision)
    specs = [edge] + rows
    row_cap = KC.row_edge_caps(len(rm), unmod, mod)
    caps = (row_mod, np.array([s["mod_cap"] for s in specs], dtype=np.int32))
    for split in (False, True):
        o, dev, host = run(dp, specs, rm, K, caps, row_cap, split=split)
        assert dev.spec_free.tolist() == [1] + want_free
        for j, (kind, d, w, w_in) in enumerate(notes):
            if kind == "huge":
                want_fit, want_keep = True, True
            elif kind == "inf":
                want_fit, want_keep = True, False
            else:
                want_fit, want_keep = w >= 0 and abs(d) <= w, w_in >= 0 and abs(d) <= w_in
            assert (dev.status[j] == AC.FIT) == want_fit and bool(dev.keep[j]) == want_keep, (j, kind, d, w, w_in)
        per = dev.keep[len(notes):].reshape(4, 3)
        assert per[[0, 2]].all() and not per[[1, 3]].any() and (dev.status[len(notes):] == AC.FIT).all()
    assert {(n[2] - n[3]) for n in notes if n[0] in ("integer", "above")} == {1, 2}


def mixed_case(dp, rm, seed, n, lengths=range(1, 15)):
    """14 unconstrained positions over rows 1 .. 8 (closed up to 6 positions,
    split-closed up to 12), half of the rows modified; n fragments, W in {0, 1,
    4, 30}."""
    rng = np.random.default_rng(seed)
    spec = {"L": 14, "pos": [(0, 0)] * 14, "alpha": AC.mask(range(1, 9))}
    spec["frags"] = window_frags(rng, AC.position_masses(spec, rm), n, lengths, dp.precision, ws=(0, 1, 4, 30))
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[2, 3, 5, 8]] = 1
    return spec, row_mod


def test_more_fragments_than_a_chunk(full_table, K):
    """A spectrum of 900 fragments (chunks of 384 records) beside one that is
    not row-free and a default one: keeps in every chunk, base and split."""
    dp = full_table
    rm = masses_of(dp)
    spec, row_mod = mixed_case(dp, rm, 33, 900, lengths=range(1, 9))  # (mostly closed intervals)
    small, _ = mixed_case(dp, rm, 34, 40)
    specs = [spec, {"default": True}, small]
    row_cap = KC.loose_row_cap(len(rm)).reshape(254, -1)
    row_cap[14, 1] = 13  # row 1 is in all 14 position sets and unmodified ...
    caps = (row_mod, np.array([14, 0, 14], dtype=np.int32))
    tight = row_cap.reshape(-1).copy()
    row_cap[14, 1] = 14
    for split in (False, True):
        o, dev, _ = run(dp, specs, rm, K, caps, row_cap.reshape(-1), split=split)
        assert dev.spec_free.tolist() == [1, 0, 1]
        kept = dev.keep[:900]
        assert kept[:384].sum() >= 50 and kept[384:].sum() >= 20, kept.sum()  # (the last chunk: whole-skeleton sums, open)
        _, none, _ = run(dp, specs, rm, K, caps, tight, split=split)  # ... so 13 is n_r - 1: nothing is kept
        assert none.spec_free.tolist() == [0, 0, 0] and not none.keep.any()
        assert all(np.array_equal(getattr(none, k), getattr(dev, k)) for k in FIELDS)
    base = run(dp, specs, rm, K, caps, row_cap.reshape(-1))[1]
    was_open = base.status == AC.OPEN
    assert was_open.sum() >= 20 and dev.keep[was_open].sum() >= 1  # (dev: the split's) keeps from split-closed intervals


def test_unmodelled_and_infeasible_spectra(full_table, K):
    """SKIPPED spectra (positions that do not number seq_len, L > 253) and
    INFEASIBLE ones (F > mod_cap, an empty A_i) keep nothing and are not
    row-free, whatever the row caps; a modelled spectrum beside them is."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(41)
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[2, 3, 5, 8]] = 1
    alpha = AC.mask(range(1, 9))
    good = {"L": 6, "pos": [(0, 0)] * 6, "alpha": alpha}
    good["frags"] = window_frags(rng, AC.position_masses(good, rm), 24, range(1, 7), dp.precision, ws=(4, 30))
    short = dict(good, pos=[(0, 0)] * 4)                       # pos_off[g + 1] - pos_off[g] != seq_len
    long_ = dict(good, L=254, pos=[AC.mask([1])] * 254)        # L > 253
    empty = dict(good, pos=[(0, 0)] * 5 + [AC.mask([20])])     # an empty A_i
    specs = [short, good, long_, dict(good), empty]
    nf = len(good["frags"])
    row_cap = KC.loose_row_cap(len(rm))
    for split in (False, True):
        o, dev, _ = run(dp, specs, rm, K, (row_mod, np.array([6, -1, 6, 6, 6], dtype=np.int32)), row_cap, split=split)
        st = dev.status.reshape(5, nf)
        assert (st[[0, 2]] == AC.SKIPPED).all() and (st[[1, 4]] == AC.INFEASIBLE).all()
        assert dev.spec_free.tolist() == [0, 0, 0, 1, 0]
        kept = dev.keep.reshape(5, nf)
        assert not kept[[0, 1, 2, 4]].any() and kept[3].sum() >= 5
        assert (dev.keep_first.reshape(5, nf)[[0, 1, 2, 4]] == 0xFFFE).all()


def test_second_list_at_the_capacity_edge(full_table, K):
    """E = 0, a {c, m} position inside each half (the construction of
    test_gpu_align_caps.py): the first half has exactly K capped sums, the
    second exactly K at r1 (split-closed: kept where a pair lies within W_in)
    and K + 1 at r2 (undecided: OPEN, never kept).  Forward and, mirrored,
    through the END class's backward sweep."""
    dp = full_table
    rm = masses_of(dp)
    run_pos, more, d = edge_positions(rm, K)
    assert d > 2 * 4 + 1
    span = (K - 1) * d
    (a1, a2, _), (b1, b2, _) = far_pairs(rm, rows_in(run_pos + [more], len(rm)), span + 64, 2)
    mA, cA = sorted((a1, a2), key=lambda r: rm[r])
    cB, mB = sorted((b1, b2), key=lambda r: rm[r])
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[mA, mB]] = 1
    pos = [AC.mask([cA, mA])] + run_pos + run_pos[:1] + [AC.mask([cB, mB])] + run_pos[1:] + [more]
    spec = {"L": len(pos), "pos": pos, "alpha": AC.mask(range(1, len(rm)))}
    nA = 1 + len(run_pos)
    first = capped_counts(spec, rm, row_mod, 0)
    second = capped_counts(dict(spec, pos=pos[nA:]), rm, row_mod, 0)
    assert first[nA - 1] == K and first[nA] > K and second[nA - 1] == K and second[nA] == K + 1, (first, second)
    lo, prec = 2 * run_lo(run_pos, rm), dp.precision
    r1, r2 = 2 * nA - 1, 2 * nA
    t = lambda a, b, j: (rm[a] + rm[b] + lo + j * d)  # noqa: E731
    deltas = list(range(-5, 6))
    frags = [(START, (t(cA, cB, K) + s) * prec, OBS_IN, r1, r1) for s in deltas]            # W = 4, W_in = 2
    frags += [(START, (t(mA, cB, K + 3) + s) * prec, OBS_IN, r1, r1) for s in (0, 1)]       # needs a modified row: NONE
    frags += [(START, (t(cA, cB, K) + run_lo([more], rm) + s) * prec, OBS_IN, r2, r2) for s in (0, 3)]  # K + 1: OPEN
    want_st = [AC.FIT if abs(s) <= 4 else AC.NONE for s in deltas] + [AC.NONE] * 2 + [AC.OPEN] * 2
    want_keep = [int(abs(s) <= 2) for s in deltas] + [0] * 4
    order = np.argsort(np.argsort([f[1] for f in frags], kind="stable"), kind="stable")
    spec["frags"] = sorted(frags, key=lambda f: f[1])
    caps = (row_mod, np.array([0, 0], dtype=np.int32))
    specs = [spec, CC.mirrored(spec)]
    row_cap = KC.loose_row_cap(len(rm))
    _, base, _ = run(dp, specs, rm, K, caps, row_cap)
    assert (base.status == AC.OPEN).all() and not base.keep.any() and base.spec_free.tolist() == [1, 1]
    _, dev, _ = run(dp, specs, rm, K, caps, row_cap, split=True)
    nf = len(frags)
    for side in (0, nf):
        assert dev.status[side + order].tolist() == want_st, (side, dev.status.tolist())
        assert dev.keep[side + order].tolist() == want_keep, (side, dev.keep.tolist())
    assert (dev.keep_first[:nf][dev.keep[:nf] == 1] == r1).all()  # l = 0
    # not row-free (cA appears in the first position only, but row_cap says never): the status stays, nothing is kept
    tight = row_cap.reshape(254, -1).copy()
    tight[spec["L"], cA] = 0
    _, gated, _ = run(dp, specs, rm, K, caps, tight.reshape(-1), split=True)
    assert not gated.keep.any() and np.array_equal(gated.status, dev.status) and gated.spec_free.tolist() == [0, 0]


def test_split_budget_and_inner_window(full_table, K):
    """E = 1 (the construction of test_gpu_align_caps.py's
    test_split_tries_every_b_in_the_window): first half {c1, m1} + a run of K / 2
    sums, second half one position {m2, c2}.  Targets around m1 + x + m2 (over
    budget) and m1 + x + c2 (within), W = 4 and W_in = 2: pairs that fit W but
    not W_in are FIT and not kept; a pair that fits inside only with both
    modified rows is not kept at mod_cap 1 and kept at mod_cap 2."""
    dp = full_table
    rm = masses_of(dp)
    run_pos, more, d = edge_positions(rm, K // 2)
    span = (K // 2 - 1) * d
    used = rows_in(run_pos, len(rm))
    free = [r for r in range(1, len(rm)) if r not in used]
    delta, m2, c2 = min((rm[b] - rm[a], a, b) for a in free for b in free if 0 < rm[b] - rm[a] <= 30
                        and (rm[b] - rm[a]) % d)
    (p, q, D), = far_pairs(rm, used | {m2, c2}, 2 * span + 128, 1)
    c1, m1 = sorted((p, q), key=lambda r: rm[r])
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[m1, m2]] = 1
    pos = [AC.mask([c1, m1])] + run_pos + [AC.mask([m2, c2])]
    spec = {"L": len(pos), "pos": pos, "alpha": AC.mask(range(1, len(rm)))}
    counts = capped_counts(spec, rm, row_mod, 1)
    L = len(pos)
    assert counts[L - 2] == K and counts[L - 1] > K, counts
    lo, prec = run_lo(run_pos, rm), dp.precision
    both = rm[m1] + lo + 20 * d + rm[m2]
    frags = [(START, (both + s) * prec, OBS_IN, L - 1, L - 1) for s in range(-d, d + 1)]
    frags += [(START, (rm[c1] + lo + 20 * d + rm[m2] + s) * prec, OBS_IN, L - 1, L - 1) for s in range(-5, 6)]
    spec["frags"] = sorted(frags, key=lambda f: f[1])
    specs = [spec, CC.mirrored(spec), dict(spec), CC.mirrored(spec)]
    caps = (row_mod, np.array([1, 1, 2, 2], dtype=np.int32))
    row_cap = KC.loose_row_cap(len(rm))
    _, base, _ = run(dp, specs, rm, K, caps, row_cap)
    nf = len(frags)
    assert (base.status[:2 * nf] == AC.OPEN).all() and not base.keep.any()
    _, dev, _ = run(dp, specs, rm, K, caps, row_cap, split=True)
    st, kept = dev.status.reshape(4, nf), dev.keep.reshape(4, nf)
    assert np.array_equal(kept[0], kept[1]) and np.array_equal(st[0], st[1]) and np.array_equal(kept[2], kept[3])
    band = (st[0] == AC.FIT) & (kept[0] == 0)    # a pair within the budget fits W, none fits W_in
    over = (kept[0] == 0) & (kept[2] == 1)       # fits inside only with e_a + e_b > E
    print("kept", int(kept[0].sum()), "band", int(band.sum()), "over budget", int(over.sum()), flush=True)
    assert kept[0].sum() >= 10 and band.sum() >= 4 and over.sum() >= 3 and (kept[0] <= kept[2]).all()
    assert ((st[0] == AC.FIT) & over).any()      # ... while another pair fits W: FIT, and still not kept


def test_untouched_paths(full_table, K):
    """The four base outputs of the keep entry points equal the caps entry
    points' on the same inputs, base and split; the four old entry points give
    what the host model gives; the keep split leaves every fragment that was
    not base-OPEN bit for bit and is idempotent."""
    import torch

    from spectrseqtools_amd import _native, alignment

    dp = full_table
    eng = dp.device_table.engine
    lib, handle = eng._lib, dp.device_table.handle
    rm = masses_of(dp)
    spec, row_mod = mixed_case(dp, rm, 31, 120)
    specs = [spec, dict(spec), dict(spec)]
    caps = (row_mod, np.array([2, 5, 14], dtype=np.int32))
    row_cap = KC.loose_row_cap(len(rm))
    o, base, _ = run(dp, specs, rm, K, caps, row_cap)
    _, dev, _ = run(dp, specs, rm, K, caps, row_cap, split=True)
    same = base.status != AC.OPEN
    assert (~same).sum() >= 20 and dev.keep[~same].any() and base.keep.any()
    assert all(np.array_equal(getattr(dev, k)[same], getattr(base, k)[same]) for k in FIELDS + ("keep", "keep_first"))
    for split, kept in ((False, base), (True, dev)):
        capped = alignment.align_device(dp, o, split=split, caps=caps)
        assert capped.keep is None and all(np.array_equal(getattr(capped, k), getattr(kept, k)) for k in FIELDS)
        assert capped.equals(alignment.align_host(o, dp.tolerance, dp.precision, K, split=split, caps=caps))
        plain = alignment.align_device(dp, o, split=split)
        assert plain.equals(alignment.align_host(o, dp.tolerance, dp.precision, K, split=split))

    args, keep_t, outs = device_args(dp, o)
    dev_t = torch.device("cuda", eng.device)
    nf = int(o.frag_off[-1])
    cm = [torch.as_tensor(caps[0], device=dev_t), torch.as_tensor(caps[1], device=dev_t), torch.as_tensor(row_cap, device=dev_t)]
    ko = [torch.zeros(nf, dtype=torch.uint8, device=dev_t), torch.zeros(nf, dtype=torch.int16, device=dev_t),
          torch.zeros(len(o), dtype=torch.uint8, device=dev_t)]
    c = _native.AlignCaps(cm[0].data_ptr(), cm[1].data_ptr())
    kp = _native.AlignKeep(cm[2].data_ptr(), *(x.data_ptr() for x in ko))
    torch.cuda.synchronize(dev_t)
    call = lambda fn: eng.check(fn(handle, ctypes.byref(args), ctypes.byref(c), ctypes.byref(kp)), "keep")  # noqa: E731
    call(lib.sst_align_windows_keep_device)
    call(lib.sst_align_split_keep_device)
    eng.synchronize()
    once = [x.cpu().numpy().copy() for x in outs + ko]
    call(lib.sst_align_split_keep_device)
    eng.synchronize()
    twice = [x.cpu().numpy() for x in outs + ko]
    assert all(np.array_equal(x, y) for x, y in zip(once, twice))
    assert np.array_equal(once[0], dev.status) and np.array_equal(once[4], dev.keep)
    assert np.array_equal(once[5].view(np.uint16), dev.keep_first) and np.array_equal(once[6], dev.spec_free)


def test_entry_point_contract(full_table, K):
    """SST_E_ARG with a message for a NULL keep struct or, with n_spec > 0, a
    NULL member; the caps calls' errors; n_spec == 0 is SST_OK; the profile ids."""
    import torch

    from spectrseqtools_amd import _native

    OK, E_ARG = 0, -1  # SST_OK, SST_E_ARG
    dp = full_table
    eng = dp.device_table.engine
    lib, handle = eng._lib, dp.device_table.handle
    rm = masses_of(dp)
    spec, row_mod = mixed_case(dp, rm, 32, 60)
    o = AC.make_outcome([spec], rm)
    args, keep_t, outs = device_args(dp, o)
    dev_t = torch.device("cuda", eng.device)
    nf = int(o.frag_off[-1])
    cm = [torch.as_tensor(row_mod, device=dev_t), torch.as_tensor(np.array([3], dtype=np.int32), device=dev_t)]
    kt = [torch.as_tensor(KC.loose_row_cap(len(rm)), device=dev_t), torch.zeros(nf, dtype=torch.uint8, device=dev_t),
          torch.zeros(nf, dtype=torch.int16, device=dev_t), torch.zeros(1, dtype=torch.uint8, device=dev_t)]
    ptrs = [x.data_ptr() for x in kt]
    good_caps = _native.AlignCaps(cm[0].data_ptr(), cm[1].data_ptr())
    torch.cuda.synchronize(dev_t)
    for fn in (lib.sst_align_windows_keep_device, lib.sst_align_split_keep_device):
        a = _native.AlignArgs()
        a.n_spec, a.tol, a.prec = 0, dp.tolerance, dp.precision
        c, kp = _native.AlignCaps(None, None), _native.AlignKeep(None, None, None, None)
        assert fn(handle, ctypes.byref(a), ctypes.byref(c), ctypes.byref(kp)) == OK       # nothing to do
        assert fn(handle, ctypes.byref(a), ctypes.byref(c), None) == E_ARG
        with pytest.raises(_native.EngineError, match="NULL sst_align_keep"):
            eng.check(E_ARG, "keep")
        assert fn(handle, ctypes.byref(a), None, ctypes.byref(kp)) == E_ARG
        assert fn(None, ctypes.byref(a), ctypes.byref(c), ctypes.byref(kp)) == E_ARG
        assert fn(None, ctypes.byref(a), ctypes.byref(c), None) == E_ARG
        a.n_spec = 1
        assert fn(handle, ctypes.byref(a), ctypes.byref(c), ctypes.byref(kp)) == E_ARG    # NULL arrays
        a.n_spec, a.prec = 0, 0.0
        assert fn(handle, ctypes.byref(a), ctypes.byref(c), ctypes.byref(kp)) == E_ARG
        for i in range(4):
            kp = _native.AlignKeep(*[None if j == i else p for j, p in enumerate(ptrs)])
            assert fn(handle, ctypes.byref(args), ctypes.byref(good_caps), ctypes.byref(kp)) == E_ARG
            with pytest.raises(_native.EngineError, match="member of sst_align_keep"):
                eng.check(E_ARG, "keep")
        kp = _native.AlignKeep(*ptrs)
        assert fn(handle, ctypes.byref(args), ctypes.byref(_native.AlignCaps(None, cm[1].data_ptr())), ctypes.byref(kp)) == E_ARG
        with pytest.raises(_native.EngineError, match="sst_align_caps"):
            eng.check(E_ARG, "keep")
    assert _native.K_ALIGN_KEEP == 25 and _native.K_ALIGN_SPLIT_KEEP == 26 < _native.K_COUNT
    assert _native.KERNEL_NAMES[25] == "k_align_windows_keep" and _native.KERNEL_NAMES[26] == "k_align_split_keep"
    eng.synchronize()


def test_run_batch_align_keep(engine, K):
    """run_batch(align_keep=True, align_split=True) on the synthetic spectra,
    the largest spectrum that has fragments forced onto the mirror route: the
    certificate equals align_host(caps=lp_caps(...), keep=lp_row_caps(...)) over
    the whole outcome, spectrum by spectrum; align_keep alone implies the caps."""
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
        g = int(live[np.argmax(peaks[live])])
        kw["limits"] = PD.DeviceLimits(max_peaks=int(peaks[g]) - 1)
        out, al = PD.run_batch(*args, align_keep=True, align_split=True, **kw)
        out_b, al_b = PD.run_batch(*args, align_keep=True, **kw)
        out_c, al_c = PD.run_batch(*args, align_caps=True, align_split=True, **kw)
        assert out.equals(out_b) and out.equals(out_c) and out.equals(plain, ignore=("route", "reason"))
        routed = np.flatnonzero(out.route == PD.ROUTE_MIRROR)
        assert g in routed and len(routed) < len(out)
        caps, row_cap = alignment.lp_caps(dp, out), alignment.lp_row_caps(dp, out)
        want = alignment.align_host(out, dp.tolerance, dp.precision, K, split=True, caps=caps, keep=row_cap)
        KC.same7(al, want, "run_batch")
        for x in (int(routed[0]), int(live[0])):  # ... and spectrum by spectrum: a routed one, a device one
            KC.same7(al.take([x]), want.take([x]), x)
        assert al_b.equals(alignment.align_host(out, dp.tolerance, dp.precision, K, caps=caps, keep=row_cap))
        assert al_c.keep is None and all(np.array_equal(getattr(al, k), getattr(al_c, k)) for k in FIELDS)
        dec = alignment.lp_decisions(al)
        print("DROP / KEEP / SOLVE", [float((dec == v).mean()) for v in (0, 1, 2)], "row-free",
              float(al.spec_free[live].mean()), flush=True)
        assert len(dec) == int(out.frag_off[-1]) > 100 and np.array_equal(dec == 0, al.alignable == 0)
    finally:
        dp.close()
        engine.trim()
        PD.release_length_buffer()
