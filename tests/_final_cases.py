"""The brute-force model, the generator and the edge cases of the final program
(spectrseqtools_amd/final_program.py, sst_final_program_device), shared by
tests/test_final_model.py (CPU) and tests/test_gpu_final.py.

Built on tests/_align_keep_cases.py: a spectrum carries "row_mod" and "mod_cap"
and, optionally, "use" (one 0 / 1 per fragment; absent: all); a case carries one
row_cap table.  The definition taken literally: itertools.product over all
positions' rows (its order is the index order of y), the intervals from the
replay of _set_x (_align_cases.admissible_intervals), Python ints.
TEST INFRASTRUCTURE."""
import itertools
import math

import numpy as np

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC

NONE, SOLVED, TOO_LARGE, INFEASIBLE, SKIPPED, NOT_FREE, UNDECIDED = range(7)
FIX = 65536
NO_GAP = (1 << 64) - 1
FIELDS = ("status", "combos", "n_feas", "best", "n_opt", "gap", "seq", "iv", "sum")
INTERNAL, START, END, START_END = (AC.code_of(False, False), AC.code_of(True, False), AC.code_of(False, True),
                                   AC.code_of(True, True))


def qfix(su, precision):
    """round(su / precision * 65536) to even, None where the model does not hold."""
    with np.errstate(all="ignore"):
        u = float(np.float64(su) / np.float64(precision))
    if not math.isfinite(u) or abs(u) >= 2.0 ** 32:
        return None
    return round(u * 65536.0)


def use_of(spec):
    return [1] * len(spec["frags"]) if spec.get("use") is None else [int(bool(x)) for x in spec["use"]]


def brute_final_spectrum(spec, row_mass, row_cap, precision, max_combos):
    """(status, combos, n_feas, best, n_opt, gap, seq [positions], iv, sum [fragments]) by the definition."""
    n_pos = 0 if spec.get("default") else len(spec["pos"])
    nf = 0 if spec.get("default") else len(spec["frags"])
    blank = lambda st, combos=0: (st, combos, 0, 0, 0, NO_GAP, [0] * n_pos, [0xFFFE] * nf, [0] * nf)  # noqa: E731
    if nf == 0:
        return blank(NONE)
    L, n_rows = spec["L"], len(row_mass)
    if L < 0 or L > KC.MAX_LEN or n_pos != L:
        return blank(SKIPPED)
    use = use_of(spec)
    used = [j for j in range(nf) if use[j]]
    q = {}
    for j in used:
        code, su, _, mn, mx = spec["frags"][j]
        if bool(code & AC.START) != bool(code & AC.END) and not (0 <= mn < L and 0 <= mx < L):
            return blank(SKIPPED)
        q[j] = qfix(su, precision)
        if q[j] is None:
            return blank(SKIPPED)
    if len(used) > 16384:
        return blank(SKIPPED)
    sets = CC.position_rows(spec, n_rows)
    combos = math.prod(len(rows) for rows in sets)
    if combos == 0:
        return blank(INFEASIBLE)
    combos = min(combos, NO_GAP)
    if not KC.row_free(spec, n_rows, row_cap):
        return blank(NOT_FREE, combos)
    if combos > max_combos:
        return blank(TOO_LARGE, combos)
    ivs = {j: AC.admissible_intervals(spec["frags"][j][0], spec["frags"][j][3], spec["frags"][j][4], L) for j in used}

    def fragment_costs(y, j):
        return [abs(q[j] - FIX * sum(int(row_mass[y[i]]) for i in (range(l, r + 1) if l != 0xFF else ())))
                for l, r in ivs[j]]

    objs = []
    for y in itertools.product(*sets):
        if sum(int(spec["row_mod"][r]) for r in y) <= spec["mod_cap"]:
            objs.append((sum(min(fragment_costs(y, j)) for j in used), y))
    if not objs:
        return blank(INFEASIBLE, combos)
    best = min(o for o, _ in objs)
    above = [o for o, _ in objs if o > best]
    y = next(y for o, y in objs if o == best)
    iv, sm = [0xFFFE] * nf, [0] * nf
    for j in used:
        c = fragment_costs(y, j)
        l, r = ivs[j][c.index(min(c))]
        iv[j] = l << 8 | r
        sm[j] = sum(int(row_mass[y[i]]) for i in (range(l, r + 1) if l != 0xFF else ()))
    return (SOLVED, combos, len(objs), best, sum(o == best for o, _ in objs), min(above) - best if above else NO_GAP,
            list(y), iv, sm)


def brute_final(specs, row_mass, row_cap, precision, max_combos):
    """The nine arrays of a case, in FIELDS order."""
    res = [brute_final_spectrum(s, row_mass, row_cap, precision, max_combos) for s in specs]
    dts = (np.uint8, np.uint64, np.uint64, np.uint64, np.uint32, np.uint64)
    per_spec = tuple(np.array([r[k] for r in res], dtype=dt) for k, dt in enumerate(dts))
    flat = lambda k, dt: np.array([x for r in res for x in r[k]], dtype=dt)  # noqa: E731
    return per_spec + (flat(6, np.uint8), flat(7, np.uint16), flat(8, np.uint32))


def use_array(specs):
    return np.array([u for s in specs if not s.get("default") for u in use_of(s)], dtype=np.uint8)


def assert_equal9(got, want, what=""):
    """A FinalOutcome against the nine arrays (or another FinalOutcome)."""
    if not isinstance(want, tuple):
        want = tuple(getattr(want, k) for k in FIELDS)
    for k, w in zip(FIELDS, want):
        g = getattr(got, k)
        assert len(g) == len(w), (what, k, len(g), len(w))
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, k, bad[:8].tolist(), g[bad[:8]].tolist(), np.asarray(w)[bad[:8]].tolist())


def host(specs, row_mass, row_cap, precision, max_combos=1 << 20, **kw):
    from spectrseqtools_amd import final_program as FP

    o = AC.make_outcome(specs, row_mass)
    return FP.final_host(o, precision, CC.caps_of(specs, len(row_mass)), row_cap, use=use_array(specs),
                         max_combos=max_combos, **kw)


# ---------------------------------------------------------------------------
# random spectra
# ---------------------------------------------------------------------------
def mixed_row_cap(rates, n_rows):
    """The row_cap table of `rates`, loose (row_cap = L) at every length that
    is no multiple of three: two thirds of random lengths are row-free whatever
    the rates."""
    t = KC.row_cap_table(rates, n_rows).reshape(KC.MAX_LEN + 1, n_rows)
    for L in range(KC.MAX_LEN + 1):
        if L % 3:
            t[L, :] = L
    return t.reshape(-1)


def random_final_case(seed, row_mass, tolerance, precision, n, **kw):
    """(specs, row_cap): _align_keep_cases.random_keep_case's spectra with the
    terminal fragments' ends repaired into [0, L - 1] (one spectrum in twelve
    keeps them: SKIPPED), no empty A_i in two spectra of three, mod_cap drawn from
    rates up to 1, a use mask on every third spectrum, and loose row caps at two
    thirds of the lengths."""
    specs, _ = KC.random_keep_case(seed, row_mass, tolerance, precision, n, rates=(0.0, 0.25, 0.5, 1.0, 1.0), **kw)
    rng = np.random.default_rng(seed + 200000)
    n_rows = len(row_mass)
    rates = [0.0] + [float(rng.choice(KC.RATES)) for _ in row_mass[1:]]
    for i, s in enumerate(specs):
        L = s["L"]
        if i % 12 != 11:
            clamp = lambda v: min(max(v, 0), L - 1)  # noqa: E731
            s["frags"] = [(c, su, obs, clamp(mn), clamp(mx)) for c, su, obs, mn, mx in s["frags"]]
        if i % 3:
            alpha_rows = [r for r in AC.rows_of(s["alpha"], n_rows) if r]
            s["pos"] = [p if (not (p[0] | p[1])) or (set(AC.rows_of(p, n_rows)) & set(alpha_rows)) else
                        AC.mask(alpha_rows[:1]) for p in s["pos"]]
        if i % 3 == 2:
            s["use"] = [int(rng.random() < 0.7) for _ in s["frags"]]
    return specs, mixed_row_cap(rates, n_rows)


# ---------------------------------------------------------------------------
# edge cases (any table: row masses and precision are the caller's)
# ---------------------------------------------------------------------------
def distinct_pairs(row_mass, n, skip=()):
    """n pairs of rows (a < b) with different masses, rows used once each."""
    rows = [r for r in range(1, len(row_mass)) if r not in skip]
    out = []
    while len(out) < n:
        a = rows.pop(0)
        b = next(r for r in rows if row_mass[r] != row_mass[a])
        rows.remove(b)
        out.append((a, b))
    return out


def prefix_pins(row_mass, sets, y, at, precision, obs=100.0):
    """START fragments that pin the prefix sums of y (one row per position) at
    the positions `at`: mn = mx = r, su exactly the sum of [0, r]."""
    pre = np.cumsum([int(row_mass[r]) for r in y])
    return [(START, float(pre[r]) * precision, obs, r, r) for r in at]


def loose_spec(row_mass, sets, frags, mod_cap=None, row_mod=None, use=None):
    """A spectrum over explicit position sets (row lists), every row of them in the alphabet."""
    alpha = sorted({r for rows in sets for r in rows})
    s = {"L": len(sets), "pos": [AC.mask(rows) for rows in sets], "alpha": AC.mask(alpha + [0]), "frags": list(frags),
         "row_mod": np.zeros(len(row_mass), np.uint8) if row_mod is None else np.asarray(row_mod, dtype=np.uint8),
         "mod_cap": len(sets) if mod_cap is None else mod_cap}
    if use is not None:
        s["use"] = list(use)
    return s


def pinned_binary_spec(row_mass, n_free, digits, precision, skip_pins=(), pairs=None):
    """n_free positions of two rows each (different masses), every prefix sum
    pinned to the y with `digits` (0: the lower row), except the positions in
    skip_pins.  Returns (spec, y)."""
    pairs = pairs or distinct_pairs(row_mass, 1) * n_free
    sets = [list(pairs[i % len(pairs)]) for i in range(n_free)]
    y = [sets[i][d] for i, d in enumerate(digits)]
    frags = prefix_pins(row_mass, sets, y, [r for r in range(n_free) if r not in skip_pins], precision)
    return loose_spec(row_mass, sets, frags), y


def tie_across_passes(row_mass, precision, high=3, low=7, x=5):
    """Two optimal y whose first (index a) sits in an earlier pass of a
    256-lane workgroup but a higher lane than the second (index b = a + 2^low):
    `high` pinned binary positions, then H and Lo over the same pair of rows
    with only the prefix behind Lo pinned -- (lower, upper) and (upper, lower)
    tie -- then `low` pinned binary positions whose digits spell x.
    Returns (spec, a, b)."""
    (p, q), = distinct_pairs(row_mass, 1)
    n = high + 2 + low
    digits = [1] * high + [0, 1] + [(x >> (low - 1 - i)) & 1 for i in range(low)]
    spec, y = pinned_binary_spec(row_mass, n, digits, precision, skip_pins=(high,), pairs=[(p, q)])
    a = int("".join(str(d) for d in digits), 2)
    return spec, a, a + (1 << low)


def long_spec(row_mass, precision, rng, n_frags=24, L=253, free_at=(0, 60, 126, 200, 252)):
    """L positions of one row each except five free ones of three rows; fragments of all classes around sums of a
    random y, terminal ones with ranges of ends, internal ones over long and short windows."""
    rows = list(range(1, len(row_mass)))
    sets = [[rows[i % len(rows)]] for i in range(L)]
    for k, p in enumerate(free_at):
        sets[p] = sorted(rng.choice(rows, size=3, replace=False).tolist())
    return loose_spec(row_mass, sets, random_frags(rng, row_mass, sets, n_frags, precision))


def random_frags(rng, row_mass, sets, n, precision, noise=3):
    """n fragments, the four classes in turn, near the sums a random y places on a random window."""
    L = len(sets)
    frags = []
    for i in range(n):
        cls = i % 4
        y = [int(rng.choice(rows)) for rows in sets]
        l, r = sorted(int(v) for v in rng.integers(0, L, 2))
        if cls in (1, 3):
            l = 0
        if cls in (2, 3):
            r = L - 1
        true = sum(int(row_mass[y[p]]) for p in range(l, r + 1)) + int(rng.integers(-noise, noise + 1))
        if i % 11 == 10:
            true = int(rng.integers(-2, 3))  # the empty interval's
        mn = mx = r if cls == 1 else l
        if i % 5 == 4:
            mn, mx = max(0, mn - int(rng.integers(0, 4))), min(L - 1, mx + int(rng.integers(0, 4)))
        if i % 7 == 6:
            mn, mx = max(mn, mx), min(mn, mx)  # mn > mx
        frags.append((AC.code_of(cls in (1, 3), cls in (2, 3)), (true + float(rng.choice([0.0, 0.25, -0.4]))) * precision,
                      100.0, mn, mx))
    return frags


# ---------------------------------------------------------------------------
# the limits of the model and of the kernel (tests/test_gpu_final_limits.py at full size,
# tests/test_final_model.py and tests/test_align_keep_model.py at a size the brute force enumerates)
# ---------------------------------------------------------------------------
def zero_length_specs(rm, precision):
    """L == 0 (no position, n_pos == 0) with fragments, and what each must be:
    a START_END fragment and internal ones of positive, zero and negative su
    (SOLVED: one assignment, the empty interval everywhere, the objective the
    sum of |qfix|), the same under an alphabet with rows, a used START fragment
    (SKIPPED: no end lies in [0, -1]) and the same fragment unused.
    Returns (specs, statuses, the objective of the SOLVED ones without the START fragment)."""
    frags = [(START_END, 2.5 * precision, 100.0, 0, 0), (INTERNAL, 3.25 * precision, 100.0, 0, 0),
             (INTERNAL, 0.0, 100.0, 0, 0), (INTERNAL, -1.75 * precision, 100.0, 0, 0)]
    start = (START, 1.0 * precision, 100.0, 0, 0)
    bare = loose_spec(rm, [], frags)
    specs = [bare, dict(bare, alpha=AC.mask([0, 1, 2])), loose_spec(rm, [], frags + [start]),
             loose_spec(rm, [], frags + [start], use=[1] * 4 + [0])]
    return specs, [SOLVED, SOLVED, SKIPPED, SOLVED], sum(abs(qfix(f[1], precision)) for f in frags)


SU_OUTSIDE = (math.nan, math.inf, -math.inf, -2.0 ** 32, 2.0 ** 32)  # in units of the precision: the model does not hold
SU_INSIDE = (2.0 ** 32 - 1, -(2.0 ** 32 - 1), -5.3, -0.25)           # ... and holds


def su_value_specs(rm, precision, sets=((1, 2), (3,), (2, 4)), values=SU_OUTSIDE + SU_INSIDE):
    """Per su outside the model and per class a spectrum with that fragment
    used (SKIPPED) and one with it unused (SOLVED); per su at the model's edge
    or negative and per class one with it used (SOLVED).  `values`: su in units
    of the precision.  Returns (specs, statuses)."""
    sets = [list(rows) for rows in sets]
    L = len(sets)
    y = [rows[-1] for rows in sets]
    pins = prefix_pins(rm, sets, y, range(L), precision)
    classes = ((INTERNAL, 0, 0), (START, L - 1, 0), (END, 0, L - 1), (START_END, 0, 0))
    specs, want = [], []
    for u in values:
        for code, mn, mx in classes:
            frags = pins[:1] + [(code, u * precision, 100.0, mn, mx)] + pins[1:]
            specs.append(loose_spec(rm, sets, frags))
            want.append(SOLVED if u in SU_INSIDE else SKIPPED)
            if u not in SU_INSIDE:
                specs.append(loose_spec(rm, sets, frags, use=[1, 0] + [1] * (L - 1)))
                want.append(SOLVED)
    return specs, want


def chunk_mask_spec(rm, sets, n_frags, precision, rng, unused=(512, 1024), noise=400):
    """n_frags noisy fragments of every class over `sets` with the fragments
    [unused[0], unused[1]) out of use: at 512 records a chunk, the middle one of three."""
    use = [int(not unused[0] <= j < unused[1]) for j in range(n_frags)]
    return loose_spec(rm, sets, random_frags(rng, rm, sets, n_frags, precision, noise=noise), use=use)


def n_used_specs(rm, precision, n=16390, limit=16384):
    """n identical START_END fragments over one position of two rows (a, b),
    the mass row b's, with `limit` of them in use (SOLVED) and with limit + 1
    (SKIPPED); the unused ones lie at the start, in the middle and at the end.
    Returns (specs, a, b)."""
    (a, b), = distinct_pairs(rm, 1)
    frags = [(START_END, rm[b] * precision, 100.0, 0, 0)] * n
    specs = []
    for used in (limit, limit + 1):
        off = n - used
        out = set(range(off // 3)) | set(range(n // 2, n // 2 + off // 3))
        out |= set(range(n - (off - len(out)), n))
        assert len(out) == off
        specs.append(loose_spec(rm, [[a, b]], frags, use=[int(j not in out) for j in range(n)]))
    return specs, a, b


def synthetic_masses(n_rows):
    """n_rows distinct row masses (row 0: 0), no two differences alike nearby."""
    return [0] + [100003 + 1009 * r + (r * r) % 13 for r in range(1, n_rows)]


def row_edge_case(n_rows, precision, rng):
    """(rm, specs, row_cap) on a synthetic table of n_rows >= 64 rows: free
    positions over rows {63, 64} and over the last two rows, rows 62 and 64 ..
    modified, every alphabet and every constrained position carrying all bits at
    and above n_rows (rows that do not exist, up to the top of the second word)
    and the alphabet bit 0.  At n_rows == 64 row 64 is such a bit itself.
    One spectrum's position holds stray bits only (an empty A_i), one is not
    row-free through its last row, one is row-free only because that row is
    modified and the cap is 0 (n_rows > 64)."""
    rm = synthetic_masses(n_rows)
    top, sec = n_rows - 1, n_rows - 2
    row_mod = np.zeros(n_rows, np.uint8)
    row_mod[62] = 1
    row_mod[64:] = 1
    stray = ((1 << 128) - 1) & ~((1 << n_rows) - 1)
    s0, s1 = stray & ((1 << 64) - 1), stray >> 64
    assert s1 >> 63 and (n_rows > 64 or s1 & 1)

    def build(pos, alpha_rows, n_frags, mod_cap):
        s = {"L": len(pos), "alpha": AC.mask(alpha_rows), "row_mod": row_mod, "mod_cap": mod_cap, "frags": [],
             "pos": [AC.mask(rows) if rows else (0, 0) for rows in pos]}
        sets = CC.position_rows(s, n_rows)  # (before the stray bits: rows below n_rows only)
        if all(sets):
            y = [rows[0] for rows in sets]  # (observed mass 350: W = 4 and W_in = 2 at tolerance 1e-5, precision 0.001)
            s["frags"] = random_frags(rng, rm, sets, n_frags, precision) + \
                prefix_pins(rm, sets, y, range(len(sets)), precision, obs=350.0)
        else:
            s["frags"] = [(START_END, rm[1] * precision, 100.0, 0, 0)] * n_frags
        s["alpha"] = (s["alpha"][0] | s0 | 1, s["alpha"][1] | s1)
        s["pos"] = [(p0 | s0, p1 | s1) if p0 | p1 else (0, 0) for p0, p1 in s["pos"]]
        assert CC.position_rows(s, n_rows) == sets
        return s

    every = range(n_rows)
    four = [[63, 64], [top, sec], [1], [62, 63]]
    five = four + [[2]]
    specs = [build(four, every, 10, cap) for cap in (4, 1, 0)]
    specs += [build([[]] * 3, [0, 63, 64, top], 6, 3), build([[]] * 2 + [[64, 63]], [62, 63, 64, sec, top], 6, 1)]
    empty = build(four, every, 3, 4)
    empty["pos"][2] = (0, 1 << 63)  # bit 127 alone: constrained, and no row
    empty["frags"] = empty["frags"][:3]
    specs.append(empty)
    specs += [build(five, every, 8, 5), build(five, every, 8, 0)]
    row_cap = KC.loose_row_cap(n_rows).reshape(KC.MAX_LEN + 1, n_rows)
    row_cap[5, top] = 0
    return rm, specs, row_cap.reshape(-1)
