"""The brute-force model of the alignment certificate under the universal
modification cap (alignment.align_host(caps=...), sst_align_windows_caps_device,
sst_align_split_caps_device), shared by tests/test_align_caps_model.py (CPU) and
tests/test_gpu_align_caps.py.

Built on tests/_align_cases.py and tests/_align_split_cases.py.  A spectrum
carries two more keys: "row_mod" (one 0 / 1 per table row) and "mod_cap".  The
definition taken literally: every y over ALL positions of the spectrum
(itertools.product over the position sets' rows) with at most mod_cap modified
rows; an interval's capped sums are the sums those y place on it.  LO / HI of
an open interval stay the uncapped minima / maxima.
TEST INFRASTRUCTURE."""
import itertools
import math

import numpy as np

import _align_cases as AC
import _align_split_cases as ASC  # noqa: F401  (mirrored, for the users of this module)


def position_rows(spec, n_rows):
    out = []
    for p in spec["pos"]:
        rows = set(AC.rows_of(p, n_rows)) & set(AC.rows_of(spec["alpha"], n_rows)) if (p[0] | p[1]) else \
            set(AC.rows_of(spec["alpha"], n_rows))
        out.append(sorted(rows - {0}))
    return out


def capped_sums(spec, row_mass):
    """{(l, r): set of sums} over the cap-feasible y, None if an A_i is empty
    or no y is feasible; and the number of feasible y."""
    L = spec["L"]
    sets = position_rows(spec, len(row_mass))
    if any(not rows for rows in sets):
        return None, 0
    mod, cap = spec["row_mod"], spec["mod_cap"]
    ys = [y for y in itertools.product(*sets) if sum(int(mod[r]) for r in y) <= cap]
    if not ys:
        return None, 0
    sums = {(0xFF, 0xFF): {0}}
    for l in range(L):
        for r in range(l, L):
            sums[l, r] = {sum(int(row_mass[r_]) for r_ in y[l:r + 1]) for y in ys}
    return sums, len(ys)


def brute_caps_spectrum(spec, row_mass, tolerance, precision, capacity, split=False):
    """Per fragment (status, n_fit, first) under the cap; with split, the
    base-OPEN fragments decided again over the open intervals, split-closed by
    the "exists m" definition on the capped sets."""
    L = spec["L"]
    sums, _ = capped_sums(spec, row_mass)
    if sums is None:
        return [(AC.INFEASIBLE, 0, 0xFFFE)] * len(spec["frags"])
    masses = AC.position_masses(spec, row_mass)
    lo = lambda l, r: sum(min(m) for m in masses[l:r + 1])  # noqa: E731  (uncapped)
    hi = lambda l, r: sum(max(m) for m in masses[l:r + 1])  # noqa: E731
    closed = {k: len(v) <= capacity for k, v in sums.items()}
    out = []
    for code, su, obs, mn, mx in spec["frags"]:
        terminal = bool(code & AC.START) != bool(code & AC.END)
        if terminal and not (0 <= mn < L and 0 <= mx < L):
            out.append((AC.SKIPPED, 0, 0xFFFE))
            continue
        target, W = round(su / precision), math.ceil(tolerance * obs / precision)
        meets = lambda l, r: W >= 0 and target - W <= hi(l, r) and target + W >= lo(l, r)  # noqa: E731
        ivs = AC.admissible_intervals(code, mn, mx, L)
        fits = [iv for iv in ivs if closed[iv] and any(abs(v - target) <= W for v in sums[iv])]
        opened = any(not closed[iv] and meets(*iv) for iv in ivs)
        if split and not fits and opened:
            opened = False
            for l, r in ivs:
                if closed[l, r]:
                    continue
                if any(closed[l, m] and closed[m + 1, r] for m in range(l, r)):
                    if any(abs(v - target) <= W for v in sums[l, r]):
                        fits.append((l, r))
                elif meets(l, r):
                    opened = True
        first = min(fits)[0] << 8 | min(fits)[1] if fits else 0xFFFE
        out.append((AC.FIT if fits else AC.OPEN if opened else AC.NONE, len(fits), first))
    return out


def brute_caps(specs, row_mass, tolerance, precision, capacity, split=False):
    """(status, alignable, n_fit, first) arrays over a case's fragments."""
    res = []
    for s in specs:
        if not s.get("default"):
            res += brute_caps_spectrum(s, row_mass, tolerance, precision, capacity, split)
    st = np.array([r[0] for r in res], dtype=np.uint8)
    return (st, ((st != AC.NONE) & (st != AC.INFEASIBLE)).astype(np.uint8),
            np.array([r[1] for r in res], dtype=np.uint32), np.array([r[2] for r in res], dtype=np.uint16))


def caps_of(specs, n_rows):
    """(row_mod, mod_cap) of a case whose spectra share one row_mod (default spectra: cap 0)."""
    live = [s for s in specs if not s.get("default")]
    row_mod = np.asarray(live[0]["row_mod"], dtype=np.uint8) if live else np.zeros(n_rows, np.uint8)
    assert len(row_mod) == n_rows and all(np.array_equal(row_mod, s["row_mod"]) for s in live)
    return row_mod, np.array([0 if s.get("default") else s["mod_cap"] for s in specs], dtype=np.int32)


def random_caps_case(seed, row_mass, tolerance, precision, n, rates=(0.0, 0.1, 0.25, 0.5), p_mod=0.5, **kw):
    """AC.random_spectrum cases with one random row_mod per case and, per
    spectrum, mod_cap = ceil(rate * L) for a rate drawn from `rates`."""
    rng = np.random.default_rng(seed)
    row_mod = np.array([0] + [int(rng.random() < p_mod) for _ in row_mass[1:]], dtype=np.uint8)
    specs = []
    for _ in range(n):
        s = AC.random_spectrum(rng, row_mass, tolerance, precision, **kw)
        rate = float(rng.choice(rates))
        s["row_mod"], s["mod_cap"], s["rate"] = row_mod, int(np.ceil(rate * s["L"])), rate
        specs.append(s)
    return specs


def mirrored(spec):
    return ASC.mirrored(spec)  # (row_mod and mod_cap do not depend on the direction)
