"""The base set of tests/test_gpu_grid_reuse.py: B distinct spectra over one
table that share one row_mod and one mixed row_cap table, holding every kind of
spectrum the alignment certificate's kernels and the final program tell apart,
and the gather that tiles them over a launch longer than the persistent grid.

Built on tests/_final_cases.py (random_final_case gives the random part, its
row_mod and its row_cap table) and the builders of the align cases.
TEST INFRASTRUCTURE."""
import numpy as np

import _align_cases as AC
import _align_caps_cases as CC
import _final_cases as FC
from _align_gpu import window_frags

B = 199      # base spectra: a prime, unrelated to any grid
STEP = 61    # launch spectrum i is base spectrum (i * STEP) % B
CHUNK_FRAGS = 520  # above the record chunks of both kernel families (384 and 512)


def launch_index(n):
    """idx[i] = (i * STEP) % B: a workgroup's spectra g, g + grid, ... are different base spectra in a varying order."""
    return (np.arange(n, dtype=np.int64) * STEP) % B


def base_set(rm, tolerance, precision, seed=4242):
    """(specs, row_cap): B spectra in base order.  The hand-built ones sit in
    the middle of random_final_case's; every one carries the case's row_mod."""
    random_specs, row_cap = FC.random_final_case(seed, rm, tolerance, precision, B)
    hand = _hand_built(rm, tolerance, precision, random_specs[0]["row_mod"], row_cap, np.random.default_rng(seed))
    specs = random_specs[:70] + hand + random_specs[70:B - len(hand)]
    assert len(specs) == B and len(hand) < B - 100
    return specs, row_cap


def _hand_built(rm, tolerance, precision, row_mod, row_cap, rng):
    n_rows = len(rm)
    mods = [r for r in range(1, n_rows) if row_mod[r]] or [n_rows - 1]
    unmods = [r for r in range(1, n_rows) if not row_mod[r]]
    u = unmods[:8]

    def spec(sets, frags, **kw):
        return FC.loose_spec(rm, sets, frags, row_mod=row_mod, **kw)

    def noisy(sets, n):
        return FC.random_frags(rng, rm, sets, n, precision)

    def pinned(sets, digits, **kw):
        y = [rows[d] for rows, d in zip(sets, digits)]
        return spec(sets, FC.prefix_pins(rm, sets, y, range(len(sets)), precision), **kw)

    one_fragment = lambda: spec([[u[0]], [u[1]]], [(FC.START_END, (rm[u[0]] + rm[u[1]]) * precision, 100.0, 0, 0)])  # noqa: E731
    small = [[u[0], u[1]], [u[2]], [u[3], u[4]], [u[5]]]  # L = 4: loose row caps (mixed_row_cap), 4 assignments
    out = []
    # default spectra and empty fragment lists
    out += [{"default": True}, spec([[u[0]], [u[1]]], []), {"default": True}, spec(small, []), {"default": True},
            spec([[u[2]]], [])]
    # SKIPPED: positions that do not number L (fewer, more), and a used terminal fragment with an end outside [0, L - 1]
    good = spec(small, noisy(small, 6))
    out += [dict(good, pos=good["pos"][:2]), dict(good, L=2), dict(good, pos=good["pos"] + good["pos"][:1])]
    for code, mn, mx in ((FC.START, 4, 0), (FC.END, 1, -1)):
        out.append(spec(small, noisy(small, 5) + [(code, rm[u[0]] * precision, 100.0, mn, mx)]))
    # INFEASIBLE: an empty A_i, forced positions above mod_cap, mod_cap == -1
    for k in range(2):
        s = spec(small, noisy(small, 4 + k))
        s["pos"] = list(s["pos"])
        s["pos"][1 + k] = AC.mask([u[6]])  # (not in the alphabet)
        out.append(s)
    forced = [[mods[0]], [u[0], u[1]], [mods[-1]]]
    out += [spec(forced, noisy(forced, 5), mod_cap=1), spec(forced, noisy(forced, 3), mod_cap=0),
            spec(small, noisy(small, 5), mod_cap=-1), spec([[u[0], u[1]]], noisy([[u[0]]], 2), mod_cap=-1)]
    # ... beside the same skeletons within their caps
    out += [spec(forced, noisy(forced, 5), mod_cap=2), good]
    # not row-free: three positions over two unmodified rows of which one may appear less often at L = 3
    # (and, beside each, three positions over rows that may fill them)
    cap3 = np.asarray(row_cap).reshape(-1, n_rows)[3]
    tight = [r for r in unmods if cap3[r] < 3]
    free = [r for r in unmods if cap3[r] >= 3]
    assert tight and len(free) >= 2, "the rates give no unmodified row with a cap below 3 at L = 3, or none without"
    for k in range(2):
        sets = [[tight[0], free[0]]] * 3
        out += [spec(sets, noisy(sets, 4 + k)), spec([[free[0], free[1]]] * 2 + [[free[0]]], noisy([[free[0]]] * 3, 3))]
    # L of 0, 1 and 253
    zero_frags = [(FC.START_END, 0.0, 100.0, 0, 0), (FC.INTERNAL, 3.25 * precision, 100.0, 0, 0),
                  (FC.INTERNAL, -2.0 * precision, 100.0, 0, 0), (FC.INTERNAL, 0.0, 0.0, 0, 0)]
    out += [dict(spec([], zero_frags), alpha=AC.mask([0, u[0], mods[0]])), spec([], zero_frags[:2]),
            dict(spec([], zero_frags + [(FC.END, 0.0, 100.0, 0, 0)]), alpha=AC.mask([u[1]]))]
    for sets in ([[u[0], u[1]]], [[mods[0]]], [[u[2], u[3], mods[-1]]]):
        out.append(spec(sets, noisy(sets, 5)))
    lng = FC.long_spec(rm, precision, rng, n_frags=24)
    out.append(dict(lng, row_mod=row_mod))
    # more than one chunk of records, between two spectra of one fragment
    many = [[u[0], u[1]], [u[2]], [u[1], u[3]], [u[0], u[5]], [u[2], u[4]], [u[3]], [u[6]]]  # L = 7, 16 assignments
    out += [one_fragment(), spec(many, noisy(many, CHUNK_FRAGS), use=[int(i % 7 != 3) for i in range(CHUNK_FRAGS)]),
            one_fragment()]
    # as many used fragments as the final program models (16384 of 16390): a count no workgroup may carry over
    out.append(dict(FC.n_used_specs(rm, precision)[0][0], row_mod=row_mod))
    # base-OPEN fragments (14 unconstrained positions over eight rows: closed up to 6 positions, split-closed up to 12)
    # next to spectra with none
    for k, cap in enumerate((4, 7, 14)):
        s = {"L": 14, "pos": [(0, 0)] * 14, "alpha": AC.mask(range(1, 9)), "row_mod": row_mod, "mod_cap": cap}
        s["frags"] = window_frags(rng, AC.position_masses(s, rm), 30, range(1, 15), precision, ws=(0, 1, 4, 30))
        out += [s, spec(small, noisy(small, 3 + k))]
    # 4096 assignments (16 passes of the final program's workgroup) next to 1 and 8; the cap binding in one of them
    pairs = FC.distinct_pairs(rm, 4, skip=mods)
    twelve = [list(pairs[i % 4]) for i in range(12)] + [[pairs[0][0]]]  # L = 13: loose row caps
    digits = [1, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0]
    fixed = [[u[0]], [u[1]], [u[2]], [u[3]]]
    eight = [list(pairs[0]), [u[0]], list(pairs[1]), list(pairs[2])]
    out += [pinned(fixed, [0] * 4), pinned(twelve, digits), pinned(eight, [1, 0, 0, 1]),
            pinned([[r] for r in u[:5]], [0] * 5)]
    capped = [[u[0], mods[0]]] * 3 + [[u[1], mods[-1]]] * 9 + [[u[2]]]
    out += [pinned(capped, [0, 1, 0] + [0] * 10, mod_cap=3), pinned(eight[:2], [0, 0])]
    # more free positions than the final program records (23 of two rows: TOO_LARGE at every max_combos), and one more of 1
    out += [pinned([list(pairs[i % 4]) for i in range(23)], [0] * 23), pinned([[u[5]], [u[6]]], [0, 0])]
    return out


def kinds(specs, n_rows):
    """Per kind that is a property of the input alone, the base indices that hold it."""
    out = {k: [] for k in ("default", "empty", "n_pos", "bad_end", "empty_set", "forced", "no_cap", "L0", "L1", "L253",
                           "chunk", "used_limit")}
    for g, s in enumerate(specs):
        if s.get("default"):
            out["default"].append(g)
            continue
        if not s["frags"]:
            out["empty"].append(g)
            continue
        L = s["L"]
        if len(s["pos"]) != L:
            out["n_pos"].append(g)
            continue
        for name, at in (("L0", 0), ("L1", 1), ("L253", 253)):
            if L == at:
                out[name].append(g)
        use = FC.use_of(s)
        if sum(use) == 16384:
            out["used_limit"].append(g)
        if any(u and bool(f[0] & AC.START) != bool(f[0] & AC.END) and not (0 <= f[3] < L and 0 <= f[4] < L)
               for u, f in zip(use, s["frags"])):
            out["bad_end"].append(g)
        sets = CC.position_rows(s, n_rows)
        if any(not rows for rows in sets):
            out["empty_set"].append(g)
        elif s["mod_cap"] == -1:
            out["no_cap"].append(g)
        elif sum(all(s["row_mod"][r] for r in rows) for rows in sets) > s["mod_cap"]:
            out["forced"].append(g)
        if len(s["frags"]) > 512 and all(0 <= h < len(specs) and not specs[h].get("default") and len(specs[h]["frags"]) == 1
                                         for h in (g - 1, g + 1)):
            out["chunk"].append(g)
    return out
