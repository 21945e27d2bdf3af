"""The brute-force model of the alignment certificate's two-list split
(alignment.align_host(split=True), sst_align_split_device), shared by
tests/test_align_split_model.py (CPU) and tests/test_gpu_align_split.py.

Built on tests/_align_cases.py: the base result is its brute force's, and only
the fragments that are OPEN there are decided again.  An open interval is
split-closed by the "exists m" definition (some m in [l, r - 1] with S(l, m)
and S(m + 1, r) both within the capacity), not by a greedy cut; whether it
holds a fitting sum is read off S(l, r) itself, from itertools.product.
TEST INFRASTRUCTURE."""
import itertools
import math

import numpy as np

import _align_cases as AC


def brute_split_spectrum(spec, row_mass, tolerance, precision, capacity):
    """Per fragment (status, n_fit, first) after the split, and the base statuses."""
    base, _ = AC.brute_spectrum(spec, row_mass, tolerance, precision, capacity)
    base_status = [b[0] for b in base]
    if AC.OPEN not in base_status:
        return base, base_status
    L = spec["L"]
    sets = AC.position_masses(spec, row_mass)
    sums = {(l, r): {sum(c) for c in itertools.product(*sets[l:r + 1])} for l in range(L) for r in range(l, L)}
    closed = {k: len(v) <= capacity for k, v in sums.items()}
    out = []
    for (code, su, obs, mn, mx), b in zip(spec["frags"], base):
        if b[0] != AC.OPEN:
            out.append(b)
            continue
        target, W = round(su / precision), math.ceil(tolerance * obs / precision)
        fits, opened = [], False
        for l, r in AC.admissible_intervals(code, mn, mx, L):
            if (l, r) == (0xFF, 0xFF) or closed[l, r]:
                continue  # (a closed interval of a base-OPEN fragment holds no fitting sum)
            s = sums[l, r]
            if any(closed[l, m] and closed[m + 1, r] for m in range(l, r)):
                if any(abs(v - target) <= W for v in s):
                    fits.append((l, r))
            elif W >= 0 and target - W <= max(s) and target + W >= min(s):
                opened = True
        first = min(fits)[0] << 8 | min(fits)[1] if fits else 0xFFFE
        out.append((AC.FIT if fits else AC.OPEN if opened else AC.NONE, len(fits), first))
    return out, base_status


def brute_split(specs, row_mass, tolerance, precision, capacity):
    """(status, alignable, n_fit, first) arrays over a case's fragments after
    the split, and the base status array."""
    res, base = [], []
    for s in specs:
        if s.get("default"):
            continue
        r, b = brute_split_spectrum(s, row_mass, tolerance, precision, capacity)
        res += r
        base += b
    st = np.array([r[0] for r in res], dtype=np.uint8)
    return (st, ((st != AC.NONE) & (st != AC.INFEASIBLE)).astype(np.uint8),
            np.array([r[1] for r in res], dtype=np.uint32), np.array([r[2] for r in res], dtype=np.uint16),
            np.array(base, dtype=np.uint8))


def mirrored(spec):
    """The spectrum read from its other end: positions reversed, START and END
    swapped.  A START-only fragment's intervals [0, r], r in [min(mn, mx), mx],
    become [L - 1 - r, L - 1]: an END-only fragment's with mn' = L - 1 -
    min(mn, mx) and mx' = L - 1 - mx (l in [min(mx', mn'), mn']); an END-only
    fragment's [l, L - 1], l in [min(mx, mn), mn], become [0, L - 1 - l]: a
    START-only fragment's with mx' = L - 1 - min(mn, mx), mn' = L - 1 - mn.
    Ends out of range stay out of range (mn' = mx' = -1)."""
    L = spec["L"]
    frags = []
    for code, su, obs, mn, mx in spec["frags"]:
        start, end = bool(code & AC.START), bool(code & AC.END)
        if start != end:
            if not (0 <= mn < L and 0 <= mx < L):
                mn2 = mx2 = -1
            elif start:
                mn2, mx2 = L - 1 - min(mn, mx), L - 1 - mx
            else:
                mn2, mx2 = L - 1 - mn, L - 1 - min(mn, mx)
        else:
            mn2, mx2 = mn, mx
        frags.append((AC.code_of(end, start, bool(code & 16)), su, obs, mn2, mx2))
    return dict(spec, pos=spec["pos"][::-1], frags=frags)
