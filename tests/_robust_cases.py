"""The brute-force model and the builders of the robust final program
(spectrseqtools_amd/final_program.py: final_robust_host, robust_decisions;
sst_final_robust_device), shared by tests/test_final_robust_model.py (CPU) and
tests/test_gpu_final_robust.py.

Built on tests/_final_cases.py: a spectrum's "use" holds 0 (unused), 1
(required) or 2 (optional) per fragment; absent: all required.  The definition
taken literally: itertools.product over every y, Python ints, c*_j from the
first optimal y over the required fragments, cap(y) per y.
TEST INFRASTRUCTURE."""
import itertools
import math

import numpy as np

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
import _final_cases as FC

ROBUST_FIELDS = ("n_optional", "cstar", "rbest", "rn_opt", "rgap")
FIELDS14 = FC.FIELDS + ROBUST_FIELDS
NO_GAP = FC.NO_GAP


def use3_of(spec):
    """0 / 1 / 2 per fragment (any other value: 1)."""
    if spec.get("use") is None:
        return [1] * len(spec["frags"])
    return [0 if not x else 2 if x == 2 else 1 for x in spec["use"]]


def use3_array(specs):
    return np.array([u for s in specs if not s.get("default") for u in use3_of(s)], dtype=np.uint8)


def brute_robust_spectrum(spec, row_mass, row_cap, precision, max_combos):
    """The fourteen outputs of one spectrum by the definition: (status, combos,
    n_feas, best, n_opt, gap, seq, iv, sum, n_optional, cstar, rbest, rn_opt, rgap)."""
    n_pos = 0 if spec.get("default") else len(spec["pos"])
    nf = 0 if spec.get("default") else len(spec["frags"])
    blank = lambda st, combos=0: (st, combos, 0, 0, 0, NO_GAP, [0] * n_pos, [0xFFFE] * nf, [0] * nf,  # noqa: E731
                                  0, 0, 0, 0, NO_GAP)
    if nf == 0:
        return blank(FC.NONE)
    L, n_rows = spec["L"], len(row_mass)
    if L < 0 or L > KC.MAX_LEN or n_pos != L:
        return blank(FC.SKIPPED)
    use = use3_of(spec)
    used = [j for j in range(nf) if use[j]]
    required = [j for j in used if use[j] == 1]
    optional = [j for j in used if use[j] == 2]
    q = {}
    for j in used:
        code, su, _, mn, mx = spec["frags"][j]
        if bool(code & AC.START) != bool(code & AC.END) and not (0 <= mn < L and 0 <= mx < L):
            return blank(FC.SKIPPED)
        q[j] = FC.qfix(su, precision)
        if q[j] is None:
            return blank(FC.SKIPPED)
    if len(used) > 16384:
        return blank(FC.SKIPPED)
    sets = CC.position_rows(spec, n_rows)
    combos = math.prod(len(rows) for rows in sets)
    if combos == 0:
        return blank(FC.INFEASIBLE)
    combos = min(combos, NO_GAP)
    if not KC.row_free(spec, n_rows, row_cap):
        return blank(FC.NOT_FREE, combos)
    if combos > max_combos:
        return blank(FC.TOO_LARGE, combos)
    ivs = {j: AC.admissible_intervals(spec["frags"][j][0], spec["frags"][j][3], spec["frags"][j][4], L) for j in used}

    def interval_sum(y, l, r):
        return sum(int(row_mass[y[i]]) for i in (range(l, r + 1) if l != 0xFF else ()))

    def costs(y, j):
        return [abs(q[j] - FC.FIX * interval_sum(y, l, r)) for l, r in ivs[j]]

    feasible = [y for y in itertools.product(*sets) if sum(int(spec["row_mod"][r]) for r in y) <= spec["mod_cap"]]
    if not feasible:
        return blank(FC.INFEASIBLE, combos)

    def summary(objs):
        """(min, how many attain it, the smallest value above it minus it)"""
        lo = min(objs)
        above = [o for o in objs if o > lo]
        return lo, sum(o == lo for o in objs), (min(above) - lo if above else NO_GAP)

    objs = [sum(min(costs(y, j)) for j in required) for y in feasible]
    best, n_opt, gap = summary(objs)
    y_star = feasible[objs.index(best)]
    iv, sm = [0xFFFE] * nf, [0] * nf
    for j in used:
        c = costs(y_star, j)
        l, r = ivs[j][c.index(min(c))]
        iv[j], sm[j] = l << 8 | r, interval_sum(y_star, l, r)
    c_star = {j: min(costs(y_star, j)) for j in optional}
    caps = [sum(min(costs(y, j)) for j in required) + sum(min(min(costs(y, j)), c_star[j]) for j in optional)
            for y in feasible]
    rbest, rn_opt, rgap = summary(caps)
    return (FC.SOLVED, combos, len(feasible), best, n_opt, gap, list(y_star), iv, sm,
            len(optional), sum(c_star.values()), rbest, rn_opt, rgap)


def brute_robust(specs, row_mass, row_cap, precision, max_combos):
    """The fourteen arrays of a case, in FIELDS14 order."""
    res = [brute_robust_spectrum(s, row_mass, row_cap, precision, max_combos) for s in specs]
    per = lambda k, dt: np.array([r[k] for r in res], dtype=dt)  # noqa: E731
    flat = lambda k, dt: np.array([x for r in res for x in r[k]], dtype=dt)  # noqa: E731
    return (per(0, np.uint8), per(1, np.uint64), per(2, np.uint64), per(3, np.uint64), per(4, np.uint32),
            per(5, np.uint64), flat(6, np.uint8), flat(7, np.uint16), flat(8, np.uint32),
            per(9, np.uint32), per(10, np.uint64), per(11, np.uint64), per(12, np.uint32), per(13, np.uint64))


def assert_equal14(got, want, what=""):
    """(FinalOutcome, RobustOutcome) against the fourteen arrays, or against another such pair."""
    fo, ro = got
    if len(want) == 2:
        want = tuple(getattr(want[0], k) for k in FC.FIELDS) + tuple(getattr(want[1], k) for k in ROBUST_FIELDS)
    FC.assert_equal9(fo, tuple(want[:9]), what)
    for k, w in zip(ROBUST_FIELDS, want[9:]):
        g = getattr(ro, k)
        assert len(g) == len(w), (what, k, len(g), len(w))
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, k, bad[:8].tolist(), g[bad[:8]].tolist(), np.asarray(w)[bad[:8]].tolist())


def host(specs, row_mass, row_cap, precision, max_combos=1 << 20):
    """final_robust_host of a case: (FinalOutcome, RobustOutcome)."""
    from spectrseqtools_amd import final_program as FP

    o = AC.make_outcome(specs, row_mass)
    return FP.final_robust_host(o, precision, CC.caps_of(specs, len(row_mass)), row_cap, use=use3_array(specs),
                                max_combos=max_combos)


def random_robust_case(seed, row_mass, tolerance, precision, n, p_unused=0.15, p_optional=0.25):
    """(specs, row_cap): _final_cases.random_final_case's spectra with a random
    0 / 1 / 2 use per fragment (two spectra in seven keep every fragment required)."""
    specs, row_cap = FC.random_final_case(seed, row_mass, tolerance, precision, n)
    rng = np.random.default_rng(seed + 300000)
    for i, s in enumerate(specs):
        draw = rng.random(len(s["frags"]))
        s["use"] = None if i % 7 in (2, 5) else \
            [0 if x < p_unused else 2 if x < p_unused + p_optional else 1 for x in draw]
    return specs, row_cap


def sparse_optional_case(seed, row_mass, tolerance, precision, n, share=0.15, at_most=6):
    """(specs, row_cap): random_final_case's spectra without their use masks,
    `share` of the fragments optional, at most `at_most` per spectrum: few
    enough for every subset to be enumerated."""
    specs, row_cap = FC.random_final_case(seed, row_mass, tolerance, precision, n)
    rng = np.random.default_rng(seed + 400000)
    for s in specs:
        marks = [j for j in range(len(s["frags"])) if rng.random() < share][:at_most]
        s["use"] = [2 if j in marks else 1 for j in range(len(s["frags"]))]
    return specs, row_cap


def subsets(items):
    for k in range(len(items) + 1):
        yield from itertools.combinations(items, k)


def with_use(spec, use):
    return dict(spec, use=list(use))


# ---------------------------------------------------------------------------
# edge cases (any table: row masses and precision are the caller's)
# ---------------------------------------------------------------------------
def mark(spec, optional, unused=()):
    """`spec` with the fragments `optional` optional, `unused` unused and the rest as they were (required if unmasked)."""
    use = use3_of(spec)
    n = len(use)
    for j in optional:
        use[j % n] = 2
    for j in unused:
        use[j % n] = 0
    return with_use(spec, use)


def sets_of_combos(row_mass, combos):
    """Position sets whose sizes multiply to `combos` (1, 256 = 2^8 or 258 = 2 * 3 * 43)."""
    rows = [r for r in range(1, len(row_mass))]
    sizes = {1: [1, 1, 1], 256: [2] * 8, 258: [2, 3, 43]}[combos]
    sets, at = [], 0
    for n in sizes:
        sets.append(rows[at:at + n])
        at = (at + n) % 40
    assert math.prod(map(len, sets)) == combos
    return sets


def chunk_border_specs(row_mass, precision, rng, chunk=512):
    """Spectra of chunk + 1 and 2 chunk + 1 noisy fragments with optional ones
    at 0, chunk - 1, chunk, 2 chunk and last, over 1, 256 and 258 assignments
    (257 is prime and no product of set sizes: 258 is the smallest count above
    one pass of 256 lanes): one and several passes meet one and several chunks."""
    specs = []
    for n in (chunk + 1, 2 * chunk + 1):
        for combos in (1, 256, 258):
            sets = sets_of_combos(row_mass, combos)
            frags = FC.random_frags(rng, row_mass, sets, n, precision, noise=400)
            border = [j for j in (0, chunk - 1, chunk, 2 * chunk, n - 1) if j < n]
            specs.append(mark(FC.loose_spec(row_mass, sets, frags), border))
    return specs


def robust_tie(row_mass, precision, **kw):
    """_final_cases.tie_across_passes with the tie broken among the required
    fragments and restored among the caps: a required START fragment pins the
    open prefix to the first y (index a), an optional one to the second (index
    b): y* = a alone, cap(a) == cap(b).  Returns (spec, a, b)."""
    spec, a, b = FC.tie_across_passes(row_mass, precision, **kw)
    (p, q), = FC.distinct_pairs(row_mass, 1)
    high = kw.get("high", 3)
    before = sum(int(row_mass[q]) for _ in range(high))  # the `high` pinned positions hold the upper row
    pin = lambda m: (FC.START, float(before + int(row_mass[m])) * precision, 100.0, high, high)  # noqa: E731
    frags = list(spec["frags"]) + [pin(p), pin(q)]
    return with_use(dict(spec, frags=frags), [1] * (len(frags) - 1) + [2]), a, b


def pull_specs(row_mass, precision):
    """One position of two rows (p, q), d their mass difference, and what an
    optional START_END fragment does to the required one's choice.  In order:
    required near p by two units of 2 d, optional exactly q (cap(q) < cap(y*):
    rbest < best + cstar); required exactly p, optional nearer q by two units
    (its own best y differs by a small cost: robust); required exactly p,
    optional exactly q (differs by a large cost: cap(q) == cap(p), a tie);
    required exactly p, optional exactly p (c* == 0: it contributes nothing)."""
    (p, q), = FC.distinct_pairs(row_mass, 1)
    mp, mq = int(row_mass[p]), int(row_mass[q])
    mid = (mp + mq) / 2.0
    toward = 1.0 if mq > mp else -1.0
    whole = lambda m: (FC.START_END, m * precision, 100.0, 0, 0)  # noqa: E731
    pairs = [(mid - toward, mq), (mp, mid + toward), (mp, mq), (mp, mp)]
    return [FC.loose_spec(row_mass, [[p, q]], [whole(r), whole(o)], use=[1, 2]) for r, o in pairs], p, q


def class_specs(row_mass, precision, rng):
    """Over sets of 24 assignments with 12 required noisy fragments: one
    spectrum per kind of optional fragment -- an internal one with q <= 0 (the
    empty interval), START and END ones with mn > mx, START and END ones with a
    range of ends, a START_END one, an internal one of positive mass -- and one
    with all of them."""
    sets = [[1, 2], [3], [2, 4, 5], [1, 6], [3, 5]]
    L = len(sets)
    mass = lambda rows: sum(int(row_mass[r]) for r in rows)  # noqa: E731
    kinds = [(FC.INTERNAL, -1.5 * precision, 100.0, 0, 0), (FC.INTERNAL, 0.0, 100.0, 0, 0),
             (FC.START, (mass([2, 3]) + 0.3) * precision, 100.0, 3, 1), (FC.END, (mass([6, 5]) - 0.3) * precision, 100.0, 4, 2),
             (FC.START, (mass([1, 3, 4]) + 2) * precision, 100.0, 0, L - 1), (FC.END, mass([5, 1, 3]) * precision, 100.0, L - 1, 0),
             (FC.START_END, (mass([2, 3, 5, 6, 5]) - 1.25) * precision, 100.0, 0, 0),
             (FC.INTERNAL, (mass([3, 4]) + 0.5) * precision, 100.0, 0, 0)]
    required = FC.random_frags(rng, row_mass, sets, 12, precision)
    specs = [FC.loose_spec(row_mass, sets, required + [k], use=[1] * 12 + [2]) for k in kinds]
    return specs + [FC.loose_spec(row_mass, sets, required + kinds, use=[1] * 12 + [2] * len(kinds))]


def unmodelled_optional_specs(row_mass, precision, rng):
    """An optional fragment outside the fixed-point range, and optional
    terminal ones with an end outside [0, L - 1]: SKIPPED; the same fragments
    unused: SOLVED.  Returns (specs, statuses)."""
    sets = [[1, 2], [3], [2, 4, 5]]
    frags = FC.random_frags(rng, row_mass, sets, 8, precision)
    bad = [(FC.INTERNAL, 2.0 ** 32 * precision, 100.0, 0, 0), (FC.START_END, math.nan, 100.0, 0, 0),
           (FC.END, row_mass[4] * precision, 100.0, 3, 0), (FC.START, row_mass[1] * precision, 100.0, 0, -1)]
    specs, want = [], []
    for b in bad:
        specs += [FC.loose_spec(row_mass, sets, frags + [b], use=[1] * 8 + [2]),
                  FC.loose_spec(row_mass, sets, frags + [b], use=[2] * 8 + [0])]
        want += [FC.SKIPPED, FC.SOLVED]
    return specs, want


def every_third_optional(spec):
    """`spec` with every third of its used fragments optional."""
    use, k = use3_of(spec), 0
    for j, u in enumerate(use):
        if u:
            k += 1
            if k % 3 == 0:
                use[j] = 2
    return with_use(spec, use)
