"""GPU tests of the alignment certificate under the universal modification cap
(sst_align_windows_caps_device, sst_align_split_caps_device: k_align_windows_caps
and k_align_split_caps in csrc/sst_align.hip; alignment.align_device(caps=),
run_batch(align_caps=True)): the device result equals alignment.align_host(...,
caps=...) in all four outputs -- on random small spectra with mixed caps, where
the smallest mass of a position is the modified row's, at the capacity's edge of
the capped lists, in the split's budget test, and through run_batch; and the
uncapped entry points are untouched."""
import ctypes
import math

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_gpu as AG
from _align_gpu import (FIELDS, OBS_W, K, device_args, edge_positions, engine, full_table,  # noqa: F401
                        prefix_counts, window_frags)
from conftest import load_golden

pytestmark = pytest.mark.gpu
START = AC.code_of(True, False)


def run(dp, specs, rm, K, caps, split=True):
    """(outcome, device, host) of a case under `caps`; asserts the device equal
    to the host model at capacity K in all four outputs."""
    return AG.run(dp, specs, rm, K, split=split, caps=caps)


def capped_counts(spec, rm, row_mod, E):
    """The model's |S_E(0, r)| for r = 0 .. L - 1."""
    from spectrseqtools_amd import alignment

    sets = alignment.position_sets(np.array(spec["pos"], dtype=np.uint64).reshape(-1, 2),
                                   np.array(spec["alpha"], dtype=np.uint64), len(rm))
    s, e, out = np.zeros(1, np.int64), np.zeros(1, np.int64), []
    for m, c, _ in alignment._position_costs(sets, rm, row_mod):
        s, e = alignment._extend_capped(s, e, m, c, E)
        out.append(len(s))
    return out


def rows_in(positions, n_rows):
    return {r for p in positions for r in AC.rows_of(p, n_rows)}


def far_pairs(rm, used, gap, n):
    """n pairs of rows outside `used` (and of each other), their mass
    differences above `gap` and more than `gap` apart from each other."""
    rows = [r for r in range(1, len(rm)) if r not in used]
    cands = sorted((abs(rm[a] - rm[b]), a, b) for i, a in enumerate(rows) for b in rows[i + 1:])
    out, taken, last = [], set(), 0
    for D, a, b in cands:
        if D > max(gap, last + gap) and a not in taken and b not in taken:
            out.append((a, b, D))
            taken |= {a, b}
            last = D
            if len(out) == n:
                return out
    raise AssertionError("far_pairs: the alphabet has no such pairs")


def run_lo(run_pos, rm):
    return sum(min(rm[r] for r in AC.rows_of(p, len(rm))) for p in run_pos)


def test_random_small_spectra(full_table, K):
    """420 random spectra (L <= 6, sets of <= 3 rows) over the real masses, a
    random row_mod, mod_cap from ceil(rate * L), 0, L, L + 3 and -1 (F >
    mod_cap whatever the positions): base and split equal the host model, which
    the CPU tests hold to the brute force."""
    from spectrseqtools_amd import alignment

    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    rng = np.random.default_rng(21)
    row_mod = (rng.random(len(rm)) < 0.5).astype(np.uint8)
    row_mod[0] = 0
    specs, caps = [], []
    for i in range(420):
        s = AC.random_spectrum(rng, rm, dp.tolerance, dp.precision)
        specs.append(s)
        caps.append([math.ceil(0.25 * s["L"]), 0, s["L"], s["L"] + 3, -1, math.ceil(0.1 * s["L"]), 1][i % 7])
    mod_cap = np.array(caps, dtype=np.int32)
    o, dev, host = run(dp, specs, rm, K, (row_mod, mod_cap), split=False)
    run(dp, specs, rm, K, (row_mod, mod_cap), split=True)
    plain = alignment.align_host(o, dp.tolerance, dp.precision, K)
    n_spec_of = np.repeat(np.arange(len(specs)), np.diff(o.frag_off))
    by_cap = (plain.status != AC.INFEASIBLE) & (dev.status == AC.INFEASIBLE)
    moved = int(((plain.status == AC.FIT) & (dev.status == AC.NONE)).sum())
    print("INFEASIBLE by the cap", int(by_cap.sum()), "FIT -> NONE", moved, flush=True)
    assert by_cap.sum() >= 100 and moved >= 10 and (dev.alignable <= plain.alignable).all()
    assert by_cap[mod_cap[n_spec_of] == -1].sum() == ((mod_cap[n_spec_of] == -1) & (plain.status != AC.INFEASIBLE)).sum()
    loose = mod_cap[n_spec_of] >= o.seq_len[n_spec_of]
    assert loose.sum() >= 100 and all(np.array_equal(getattr(dev, k)[loose], getattr(plain, k)[loose]) for k in FIELDS)
    assert {AC.NONE, AC.FIT, AC.INFEASIBLE, AC.SKIPPED} <= set(dev.status.tolist())


def test_smallest_mass_is_the_modified_row(full_table, K):
    """Positions {m, c} with w_m < w_c: LO is the all-modified sum, which the
    budget forbids, and the unshifted copy is the one that pays.  E = 0 and E =
    1, forward (START, START_END, internal) and backward (END)."""
    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    m, c = 5, 9
    if rm[m] > rm[c]:
        m, c = c, m
    assert rm[m] < rm[c]
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[m] = 1
    L, prec = 5, dp.precision
    both = AC.mask([m, c])
    frags, n_mod = [], []
    for n_pos in range(1, L + 1):
        for j in range(n_pos + 1):  # j modified rows in a window of n_pos positions
            t = (j * rm[m] + (n_pos - j) * rm[c]) * prec
            for start, end in ((True, False), (False, True), (False, False)) + (((True, True),) if n_pos == L else ()):
                end_at = n_pos - 1 if start else L - n_pos
                frags.append((AC.code_of(start, end), t, 0.0, end_at, end_at))
                n_mod.append(j)
    order = np.argsort([f[1] for f in frags], kind="stable")
    spec = {"L": L, "pos": [both] * L, "alpha": both, "frags": [frags[i] for i in order]}
    n_mod = np.array(n_mod)[order]
    assert (rm[c] - rm[m]) > 0 and len({f[1] for f in frags}) == sum(n + 1 for n in range(1, L + 1))
    for cap in (0, 1, 2):
        for split in (False, True):
            o, dev, host = run(dp, [spec, dict(spec, pos=[both] * (L - 1) + [AC.mask([c])])], rm, K,
                               (row_mod, np.array([cap, cap], dtype=np.int32)), split=split)
            nf = len(frags)
            assert np.array_equal(dev.alignable[:nf], (n_mod <= cap).astype(np.uint8)), cap
            assert np.array_equal(dev.status[:nf], np.where(n_mod <= cap, AC.FIT, AC.NONE))
            assert {(int(x) >> 2) & 3 for x in o.frag_code} == {0, 1, 2, 3}


def edge_case(rm, K, E):
    """(spec, row_mod, mod_cap, n): leading positions {c_i, m_i} (m_i modified,
    the differences far apart) -- one for E = 0, three for E = 1, five for E =
    2 -- then a run of unmodified pairs with K / (number of leading copies
    within E) sums, then the pair that adds one sum per copy.  Capped: exactly K
    sums at [0, n - 1], above K at [0, n]; uncapped: well above K at [0, n - 1]."""
    lead = {0: 1, 1: 3, 2: 5}[E]
    copies = sum(math.comb(lead, j) for j in range(E + 1))  # the choices of at most E modified rows: 1, 4, 16
    assert K % copies == 0
    run_pos, more, d = edge_positions(rm, K // copies)
    span = (K // copies - 1) * d
    pairs = far_pairs(rm, rows_in(run_pos + [more], len(rm)), 2 * span + 64, lead)
    row_mod = np.zeros(len(rm), np.uint8)
    pos = []
    for i, (a, b, D) in enumerate(pairs):
        mod = min(a, b, key=lambda r: rm[r]) if i % 2 == 0 else max(a, b, key=lambda r: rm[r])  # lighter, heavier, ..
        row_mod[mod] = 1
        pos.append(AC.mask([a, b]))
    pos += run_pos + [more]
    spec = {"L": len(pos), "pos": pos, "alpha": AC.mask(range(1, len(rm)))}
    n = lead + len(run_pos)
    return spec, row_mod, E, n, pairs, d, copies


@pytest.mark.parametrize("E", [0, 1, 2])
def test_capacity_edge_under_caps(full_table, K, E):
    """The capped list has exactly K sums at [0, n - 1] (closed: decided by the
    base call) and more at [0, n] (K + 1 for E = 0; K + 4, K + 16 for E = 1, 2,
    where sums reached with one and two modified rows fill the list), counted
    here with the model; uncapped both are open.  Forward, and on the mirrored
    spectrum through the END class's backward sweep."""
    from spectrseqtools_amd import alignment

    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    spec, row_mod, cap, n, pairs, d, copies = edge_case(rm, K, E)
    L, prec = spec["L"], dp.precision
    assert L <= 253 and d >= 3
    counts = capped_counts(spec, rm, row_mod, E)
    plain_counts, _ = prefix_counts(AC.position_masses(spec, rm))
    assert counts[n - 1] == K and counts[n] == K + copies and plain_counts[n - 1] > K, (counts, plain_counts)
    assert E != 0 or counts[n] == K + 1
    lead = len(pairs)
    canon = [next(r for r in (a, b) if not row_mod[r]) for a, b, _ in pairs]
    modif = [next(r for r in (a, b) if row_mod[r]) for a, b, _ in pairs]
    run_min = run_lo(spec["pos"][lead:n], rm)
    base = sum(rm[r] for r in canon) + run_min        # no modified row
    swap = lambda i: rm[modif[i]] - rm[canon[i]]       # noqa: E731  (the change of taking pair i's modified row)
    r1, r2 = n - 1, n
    more_min = run_lo(spec["pos"][n:], rm)
    frags = [(START, (base + 7 * d) * prec, 0.0, r1, r1),                     # a canonical sum: FIT
             (START, (base + 7 * d + 1) * prec, 0.0, r1, r1)]                 # between two sums: NONE
    want = [AC.FIT, AC.NONE]
    for j in range(1, min(lead, 3) + 1):  # the modified rows of the last j leading pairs: FIT iff j <= E
        frags.append((START, (base + sum(swap(lead - 1 - i) for i in range(j)) + (8 + j) * d) * prec, 0.0, r1, r1))
        want.append(AC.FIT if j <= E else AC.NONE)
    assert want.count(AC.FIT) == 1 + E and AC.NONE in want[2:]
    n_closed = len(frags)
    frags += [(START, (base + more_min + 5 * d) * prec, 0.0, r2, r2),          # [0, n] only: open under caps
              (AC.code_of(True, True), (base + more_min + 5 * d + 1) * prec, 0.0, 0, 0)]  # the same interval
    want += [AC.OPEN, AC.OPEN]
    order = np.argsort(np.argsort([f[1] for f in frags], kind="stable"), kind="stable")
    spec["frags"] = sorted(frags, key=lambda f: f[1])
    specs = [spec, CC.mirrored(spec)]
    caps = (row_mod, np.array([cap, cap], dtype=np.int32))
    o, dev, host = run(dp, specs, rm, K, caps, split=False)
    nf = len(frags)
    for side in (0, nf):
        assert dev.status[side + order].tolist() == want, (side, dev.status.tolist())
    assert ((o.frag_code[nf:] >> 2) & 3).tolist().count(2) == nf - 1
    plain = alignment.align_device(dp, o)
    assert (plain.status[order[:n_closed + 1]] == AC.OPEN).all()  # uncapped: both intervals are open
    run(dp, specs, rm, K, caps, split=True)


def test_unmodelled_spectrum_is_skipped_whatever_the_cap(full_table, K):
    """INFEASIBLE by the cap takes precedence among modelled spectra only: a
    spectrum whose positions do not number seq_len, or with L > 253, is
    SKIPPED (alignable 1) also with mod_cap = -1, where F = 0 > mod_cap; a
    modelled one beside them is INFEASIBLE."""
    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    rng = np.random.default_rng(41)
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[2, 3, 5, 8]] = 1
    alpha = AC.mask(range(1, 9))
    good = {"L": 6, "pos": [(0, 0)] * 6, "alpha": alpha}
    good["frags"] = window_frags(rng, AC.position_masses(good, rm), 24, range(1, 7), dp.precision)
    short = dict(good, pos=[(0, 0)] * 4)                       # pos_off[g + 1] - pos_off[g] != seq_len
    long_ = dict(good, L=254, pos=[AC.mask([1])] * 254)        # L > 253
    specs = [short, good, long_, dict(good)]
    nf = len(good["frags"])
    for caps_of in ([-1, -1, -1, 6], [-5, 0, -1, -1]):
        for split in (False, True):
            o, dev, host = run(dp, specs, rm, K, (row_mod, np.array(caps_of, dtype=np.int32)), split=split)
            st = dev.status.reshape(4, nf)
            assert (st[0] == AC.SKIPPED).all() and (st[2] == AC.SKIPPED).all()
            assert (dev.alignable.reshape(4, nf)[[0, 2]] == 1).all()
            assert (st[1] == AC.INFEASIBLE).all() == (caps_of[1] < 0) and (st[3] == AC.INFEASIBLE).all() == (caps_of[3] < 0)
            assert not (st[1 if caps_of[1] >= 0 else 3] == AC.INFEASIBLE).any()


def test_split_budget(full_table, K):
    """E = 1.  First half {c_A, m_A} + a run of K / 2 sums: K capped sums (half
    of them at excess 1); the next position {c_B, m_B} opens it.  Second half
    {c_B, m_B} + the same run: K sums, split-closed; one pair more: K + 2,
    undecided.  A target only the two modified rows together reach is NONE, one
    modified row FIT."""
    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    run_pos, more, d = edge_positions(rm, K // 2)
    span = (K // 2 - 1) * d
    (a1, a2, _), (b1, b2, _) = far_pairs(rm, rows_in(run_pos + [more], len(rm)), 2 * span + 64, 2)
    cA, mA = sorted((a1, a2), key=lambda r: rm[r])      # the modified row is the heavier one
    mB, cB = sorted((b1, b2), key=lambda r: rm[r])      # ... the lighter one: LO of the second half pays
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[mA, mB]] = 1
    pos = [AC.mask([cA, mA])] + run_pos + [AC.mask([cB, mB])] + run_pos + [more]
    spec = {"L": len(pos), "pos": pos, "alpha": AC.mask(range(1, len(rm)))}
    nA = 1 + len(run_pos)
    first = capped_counts(spec, rm, row_mod, 1)
    second = capped_counts(dict(spec, pos=pos[nA:]), rm, row_mod, 1)
    assert first[nA - 1] == K and first[nA] > K and second[nA - 1] == K and second[nA] == K + 2, (first, second)
    lo, prec = 2 * run_lo(run_pos, rm), dp.precision
    r1, r2 = 2 * nA - 1, 2 * nA
    t = lambda a, b, j: (rm[a] + rm[b] + lo + j * d) * prec  # noqa: E731
    frags = [(START, t(cA, cB, 40), 0.0, r1, r1),       # no modified row: FIT
             (START, t(mA, cB, 41), 0.0, r1, r1),       # one: FIT
             (START, t(cA, mB, 42), 0.0, r1, r1),       # the other one: FIT
             (START, t(mA, mB, 43), 0.0, r1, r1),       # both: over budget, NONE
             (START, t(mA, cB, 44) + prec, 0.0, r1, r1),  # between two sums: NONE
             (START, t(cA, cB, 45) + run_lo([more], rm) * prec, 0.0, r2, r2)]  # the second list has K + 2: OPEN
    want = [AC.FIT, AC.FIT, AC.FIT, AC.NONE, AC.NONE, AC.OPEN]
    order = np.argsort(np.argsort([f[1] for f in frags], kind="stable"), kind="stable")
    spec["frags"] = sorted(frags, key=lambda f: f[1])
    caps = (row_mod, np.array([1, 1], dtype=np.int32))
    specs = [spec, CC.mirrored(spec)]
    o, base, _ = run(dp, specs, rm, K, caps, split=False)
    assert (base.status == AC.OPEN).all()
    o, dev, host = run(dp, specs, rm, K, caps, split=True)
    nf = len(frags)
    for side in (0, nf):
        assert dev.status[side + order].tolist() == want, (side, dev.status.tolist())
    # with the budget of two every pair is allowed
    _, loose, _ = run(dp, specs, rm, K, (row_mod, np.array([2, 2], dtype=np.int32)), split=True)
    assert loose.status[order[3]] != AC.NONE


def test_second_list_at_the_capacity_edge_under_caps(full_table, K):
    """E = 0, a {c, m} position inside each half: the first half has exactly K
    capped sums and the next position opens it; the second half exactly K
    (split-closed: decided) and, one pair further, K + 1 (undecided) -- counted
    here with the model.  Uncapped the first list would end much earlier."""
    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    run_pos, more, d = edge_positions(rm, K)
    span = (K - 1) * d
    (a1, a2, _), (b1, b2, _) = far_pairs(rm, rows_in(run_pos + [more], len(rm)), span + 64, 2)
    mA, cA = sorted((a1, a2), key=lambda r: rm[r])      # the lighter row is the modified one
    cB, mB = sorted((b1, b2), key=lambda r: rm[r])
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[mA, mB]] = 1
    pos = [AC.mask([cA, mA])] + run_pos + run_pos[:1] + [AC.mask([cB, mB])] + run_pos[1:] + [more]
    spec = {"L": len(pos), "pos": pos, "alpha": AC.mask(range(1, len(rm)))}
    nA = 1 + len(run_pos)
    first = capped_counts(spec, rm, row_mod, 0)
    second = capped_counts(dict(spec, pos=pos[nA:]), rm, row_mod, 0)
    plain, _ = prefix_counts(AC.position_masses(spec, rm))
    assert first[nA - 1] == K and first[nA] > K and second[nA - 1] == K and second[nA] == K + 1, (first, second)
    assert plain[nA - 2] > K and spec["L"] <= 253
    lo, prec = 2 * run_lo(run_pos, rm), dp.precision
    r1, r2 = 2 * nA - 1, 2 * nA
    t = lambda a, b, j: (rm[a] + rm[b] + lo + j * d) * prec  # noqa: E731
    frags = [(START, t(cA, cB, K), 0.0, r1, r1),                                   # FIT
             (START, t(cA, cB, K) + prec, 0.0, r1, r1),                            # between two sums: NONE
             (START, t(mA, cB, K + 3), 0.0, r1, r1),                               # needs a modified row: NONE
             (START, t(cA, mB, K + 5), 0.0, r1, r1),                               # NONE
             (START, t(cA, cB, K) + run_lo([more], rm) * prec, 0.0, r2, r2)]       # the second list has K + 1: OPEN
    want = [AC.FIT, AC.NONE, AC.NONE, AC.NONE, AC.OPEN]
    order = np.argsort(np.argsort([f[1] for f in frags], kind="stable"), kind="stable")
    spec["frags"] = sorted(frags, key=lambda f: f[1])
    caps = (row_mod, np.array([0, 0], dtype=np.int32))
    specs = [spec, CC.mirrored(spec)]
    _, base, _ = run(dp, specs, rm, K, caps, split=False)
    assert (base.status == AC.OPEN).all()
    _, dev, _ = run(dp, specs, rm, K, caps, split=True)
    nf = len(frags)
    for side in (0, nf):
        assert dev.status[side + order].tolist() == want, (side, dev.status.tolist())
    assert dev.n_fit[order].tolist() == [1, 0, 0, 0, 0]


def test_split_tries_every_b_in_the_window(full_table, K):
    """E = 1, second half one position {m2, c2}, the modified m2 lighter by
    delta <= W: for every a of excess 1 the first b in the window is m2's (over
    budget), the second c2's (within): FIT at W = 30, NONE at W = 0."""
    dp = full_table
    rm = [int(m.mass) for m in dp.masses]
    run_pos, more, d = edge_positions(rm, K // 2)
    span = (K // 2 - 1) * d
    used = rows_in(run_pos, len(rm))
    free = [r for r in range(1, len(rm)) if r not in used]
    # (delta no multiple of the run's step: m1 + x + m2 is then no m1 + x' + c2)
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
    both = (rm[m1] + lo + 20 * d + rm[m2]) * prec
    frags = [(START, both, OBS_W[0], L - 1, L - 1),                                # only m1 + m2 reach it: NONE
             (START, both, OBS_W[30], L - 1, L - 1),                               # m1 + c2 is delta away: FIT
             (START, (rm[m1] + lo + 20 * d + rm[c2]) * prec, OBS_W[0], L - 1, L - 1),  # FIT
             (START, (rm[c1] + lo + 20 * d + rm[m2]) * prec, OBS_W[0], L - 1, L - 1)]  # FIT
    want = [AC.NONE, AC.FIT, AC.FIT, AC.FIT]
    order = np.argsort(np.argsort([f[1] for f in frags], kind="stable"), kind="stable")
    spec["frags"] = sorted(frags, key=lambda f: f[1])
    caps = (row_mod, np.array([1, 1], dtype=np.int32))
    specs = [spec, CC.mirrored(spec)]
    _, base, _ = run(dp, specs, rm, K, caps, split=False)
    assert (base.status == AC.OPEN).all()
    _, dev, _ = run(dp, specs, rm, K, caps, split=True)
    assert dev.status[order].tolist() == want and dev.status[len(frags) + order].tolist() == want, dev.status.tolist()


def mixed_case(dp, rm, seed):
    """The 14 unconstrained positions over rows 1 .. 8 of test_gpu_align_split.py
    (closed up to 6, split-closed up to 12), half of the rows modified."""
    rng = np.random.default_rng(seed)
    spec = {"L": 14, "pos": [(0, 0)] * 14, "alpha": AC.mask(range(1, 9))}
    spec["frags"] = window_frags(rng, AC.position_masses(spec, rm), 120, range(5, 15), dp.precision)
    row_mod = np.zeros(len(rm), np.uint8)
    row_mod[[2, 3, 5, 8]] = 1
    return spec, row_mod


def test_untouched_paths(full_table, K):
    """After the caps calls the uncapped calls still equal align_host(); the
    caps split leaves every fragment that was not base-OPEN bit for bit and is
    idempotent; the caps decide fragments the uncapped split leaves OPEN."""
    from spectrseqtools_amd import alignment

    dp = full_table
    eng = dp.device_table.engine
    lib, handle = eng._lib, dp.device_table.handle
    rm = [int(m.mass) for m in dp.masses]
    spec, row_mod = mixed_case(dp, rm, 31)
    specs = [spec, dict(spec), dict(spec)]
    caps = (row_mod, np.array([2, 5, 14], dtype=np.int32))
    o, base, _ = run(dp, specs, rm, K, caps, split=False)
    _, dev, _ = run(dp, specs, rm, K, caps, split=True)
    keep = base.status != AC.OPEN
    assert (~keep).sum() >= 20 and (dev.status[~keep] != AC.OPEN).any()
    assert all(np.array_equal(getattr(dev, k)[keep], getattr(base, k)[keep]) for k in FIELDS)
    for split in (False, True):
        plain = alignment.align_device(dp, o, split=split)
        assert plain.equals(alignment.align_host(o, dp.tolerance, dp.precision, K, split=split))
    nf = len(spec["frags"])
    assert all(np.array_equal(getattr(dev, k)[2 * nf:], getattr(plain, k)[2 * nf:]) for k in FIELDS)  # mod_cap >= L
    assert (dev.alignable <= plain.alignable).all()
    newly = (plain.status == AC.OPEN) & (dev.status != AC.OPEN)
    print("uncapped split OPEN", int((plain.status == AC.OPEN).sum()), "decided under caps", int(newly.sum()), flush=True)
    assert newly.any()

    import torch

    args, keep_t, outs = device_args(dp, o)
    dev_t = torch.device("cuda", eng.device)
    cm = [torch.as_tensor(caps[0], device=dev_t), torch.as_tensor(caps[1], device=dev_t)]
    from spectrseqtools_amd import _native
    c = _native.AlignCaps(cm[0].data_ptr(), cm[1].data_ptr())
    torch.cuda.synchronize(dev_t)
    eng.check(lib.sst_align_windows_caps_device(handle, ctypes.byref(args), ctypes.byref(c)), "caps")
    eng.check(lib.sst_align_split_caps_device(handle, ctypes.byref(args), ctypes.byref(c)), "caps split")
    eng.synchronize()
    once = [x.cpu().numpy().copy() for x in outs]
    eng.check(lib.sst_align_split_caps_device(handle, ctypes.byref(args), ctypes.byref(c)), "caps split")
    eng.synchronize()
    twice = [x.cpu().numpy() for x in outs]
    assert all(np.array_equal(x, y) for x, y in zip(once, twice))
    assert np.array_equal(once[0], dev.status) and np.array_equal(once[2].view(np.uint32), dev.n_fit)


def test_entry_point_contract(full_table, K):
    """The base calls' argument errors, and SST_E_ARG with a message for a NULL
    caps member; n_spec == 0 is SST_OK; the kernels' profile ids."""
    import torch

    from spectrseqtools_amd import _native

    OK, E_ARG = 0, -1  # SST_OK, SST_E_ARG
    dp = full_table
    eng = dp.device_table.engine
    lib, handle = eng._lib, dp.device_table.handle
    rm = [int(m.mass) for m in dp.masses]
    spec, row_mod = mixed_case(dp, rm, 32)
    o = AC.make_outcome([spec], rm)
    args, keep_t, outs = device_args(dp, o)
    dev_t = torch.device("cuda", eng.device)
    cm = [torch.as_tensor(row_mod, device=dev_t), torch.as_tensor(np.array([3], dtype=np.int32), device=dev_t)]
    torch.cuda.synchronize(dev_t)
    for fn in (lib.sst_align_windows_caps_device, lib.sst_align_split_caps_device):
        a = _native.AlignArgs()
        a.n_spec, a.tol, a.prec = 0, dp.tolerance, dp.precision
        c = _native.AlignCaps(None, None)
        assert fn(handle, ctypes.byref(a), ctypes.byref(c)) == OK       # nothing to do
        assert fn(handle, ctypes.byref(a), None) == E_ARG
        assert fn(None, ctypes.byref(a), ctypes.byref(c)) == E_ARG
        a.n_spec = 1
        assert fn(handle, ctypes.byref(a), ctypes.byref(c)) == E_ARG    # NULL arrays
        a.n_spec, a.prec = 0, 0.0
        assert fn(handle, ctypes.byref(a), ctypes.byref(c)) == E_ARG
        a.n_spec, a.prec = -1, dp.precision
        assert fn(handle, ctypes.byref(a), ctypes.byref(c)) == E_ARG
        for c in (_native.AlignCaps(None, cm[1].data_ptr()), _native.AlignCaps(cm[0].data_ptr(), None)):
            assert fn(handle, ctypes.byref(args), ctypes.byref(c)) == E_ARG
            with pytest.raises(_native.EngineError, match="sst_align_caps"):
                eng.check(E_ARG, "caps")
    assert _native.K_ALIGN_CAPS == 23 and _native.K_ALIGN_SPLIT_CAPS == 24 < _native.K_COUNT
    assert _native.KERNEL_NAMES[23] == "k_align_windows_caps" and _native.KERNEL_NAMES[24] == "k_align_split_caps"
    eng.synchronize()


def test_run_batch_align_caps(engine, K):
    """run_batch(align_caps=True, align_split=True) on the synthetic spectra at
    modification rate 0.05, the largest spectrum that has fragments forced onto
    the mirror route: the certificate equals align_host(caps=lp_caps(...)) over
    the whole outcome; the defaults are unchanged."""
    import _synth_cases as SC
    from spectrseqtools_amd import alignment, pipeline_device as PD
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE, build_breakage_dict

    n = len(load_golden("synth_stages.json.gz")["noise_free_exact"]["spectra"])
    d = SC.variant_inputs("noise_free_exact", n=n)
    assert d["mod_rate"] == 0.05
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
        out_s, al_s = PD.run_batch(*args, align_split=True, **kw)
        out, al = PD.run_batch(*args, align_caps=True, align_split=True, **kw)
        out_b, al_b = PD.run_batch(*args, align_caps=True, **kw)
        assert out.equals(out_s) and out.equals(out_b) and out.equals(plain, ignore=("route", "reason"))
        routed = np.flatnonzero(out.route == PD.ROUTE_MIRROR)
        assert g in routed and len(routed) < len(out)
        caps = alignment.lp_caps(dp, out)
        assert caps[1].tolist() == [int(np.ceil(0.05 * int(L))) for L in out.seq_len] and caps[0].sum() > 4
        assert al.equals(alignment.align_host(out, dp.tolerance, dp.precision, K, split=True, caps=caps))
        assert al_b.equals(alignment.align_host(out, dp.tolerance, dp.precision, K, caps=caps))
        assert al_s.equals(alignment.align_host(out, dp.tolerance, dp.precision, K, split=True))
        assert len(al.status) == int(out.frag_off[-1]) > 100 and (al.alignable <= al_s.alignable).all()
        print("status shares: split", al_s.shares(), "caps + split", al.shares(), flush=True)
    finally:
        dp.close()
        engine.trim()
        PD.release_length_buffer()
