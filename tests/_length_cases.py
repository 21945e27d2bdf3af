"""The brute-force model, the generator and the edge cases of the length program
(spectrseqtools_amd/length_program.py, sst_length_program_device), shared by
tests/test_length_program_model.py (CPU) and tests/test_gpu_length_program.py.

A spectrum is a dict: "M" (the walk's max_len), "start" / "end" (M row lists
each: the START skeleton and the REVERSED END skeleton), "alpha" (row list),
"lower", "upper", "lb_status", "su_mass", "frags" (tuples (code, su, raw
min_end, raw max_end), code with the side bits START = 4, END = 8).  The
definition taken literally: _set_x replayed on a list, every run of positions
that agrees with the pattern, itertools.product over all positions' rows,
Python ints.  TEST INFRASTRUCTURE."""
import itertools
import math

import numpy as np

INVALID, RAISES, NOT_MODELLED, INFEASIBLE, NOT_FREE, TOO_LARGE, SOLVED = range(7)
FIX = 65536
MAX_LEN = 253
START, END, START_END = 4, 8, 12
FIELDS = ("cand_off", "cand_len", "status", "combos", "n_feas", "best")


def mask(rows):
    m = [0, 0]
    for r in rows:
        m[r >> 6] |= 1 << (r & 63)
    return m


def make_cases(specs, row_mass, row_names=None):
    from spectrseqtools_amd.length_program import LengthCases

    S = len(specs)
    skel = [mask(rows) for s in specs for rows in list(s["start"]) + list(s["end"])]
    frags = [f for s in specs for f in s["frags"]]
    return LengthCases(max_len=[s["M"] for s in specs],
                       skel_off=np.concatenate([[0], np.cumsum([2 * s["M"] for s in specs])]).astype(np.int64),
                       skeleton=np.array(skel, dtype=np.uint64).reshape(-1, 2),
                       alpha=np.array([mask(s["alpha"]) for s in specs], dtype=np.uint64).reshape(S, 2),
                       lower=[s["lower"] for s in specs], upper=[s["upper"] for s in specs],
                       lb_status=[s.get("lb_status", 0) for s in specs], su_mass=[s["su_mass"] for s in specs],
                       frag_off=np.concatenate([[0], np.cumsum([len(s["frags"]) for s in specs])]).astype(np.int64),
                       frag_code=[f[0] for f in frags], frag_su=[f[1] for f in frags],
                       frag_min_end=[f[2] for f in frags], frag_max_end=[f[3] for f in frags],
                       row_names=row_names or [""] + [f"n{r}" for r in range(1, len(row_mass))], row_mass=row_mass)


def row_cap_table(rates, n_rows):
    """row_cap[L * n_rows + r] = ceil(rate_r * L), L in [0, 253], as alignment.lp_row_caps computes it."""
    lengths = np.arange(MAX_LEN + 1, dtype=np.float64)
    return np.stack([np.ceil(np.float64(rates[r]) * lengths).astype(np.int32) for r in range(n_rows)], axis=1).reshape(-1)


def caps_of(specs, n_rows, row_mod, rate, rates=None):
    """(row_mod, mod_cap per candidate, row_cap): mod_cap = int(ceil(rate * c)) in f64."""
    c = np.array([c for s in specs for c in candidates_of(s)], dtype=np.float64)
    return (np.asarray(row_mod, dtype=np.uint8), np.ceil(np.float64(rate) * c).astype(np.int32),
            row_cap_table([1.0] * n_rows if rates is None else rates, n_rows))


def candidates_of(spec):
    return list(range(spec["lower"], spec["upper"] + 1)) if spec.get("lb_status", 0) == 0 else []


def qfix(su, precision):
    with np.errstate(all="ignore"):
        u = float(np.float64(su) / np.float64(precision))
    if not math.isfinite(u) or abs(u) >= 2.0 ** 32:
        return None
    return round(u * 65536.0)


def replay_set_x(code, min_end, max_end, n):
    """linear_program.py:74-102 after skeleton_building.py:267-276, on a list; None where it raises."""
    x = [None] * n
    side = code & 12
    try:
        if side == START_END:
            for i in range(n):
                x[i] = 1
        elif side == START:
            for i in range(min_end - 1 + 1):
                x[i] = 1
            for i in range(max_end - 1 + 1, n):
                x[i] = 0
        elif side == END:
            for i in range(n - max_end):
                x[i] = 0
            for i in range(n - min_end, n):
                x[i] = 1
    except IndexError:
        return None
    return x


def runs_of(x):
    """Every contiguous run (l, r) that holds every fixed 1 and no fixed 0, and None for the empty run."""
    n = len(x)
    out = [(lo, hi) for lo in range(n) for hi in range(lo, n)
           if all(x[i] != 0 for i in range(lo, hi + 1)) and all(x[i] != 1 for i in range(n) if i < lo or i > hi)]
    return out + ([None] if all(v != 1 for v in x) else [])


def modelled(runs, n):
    """WHOLE, EMPTY-only, a PREFIX family or a SUFFIX family."""
    if not runs:
        return False
    if runs == [None]:
        return True
    if None in runs:
        return False
    return all(lo == 0 for lo, _ in runs) or all(hi == n - 1 for _, hi in runs)


def position_rows(spec, c, n_rows):
    """A_i of the combined skeleton at c (1 <= c <= M)."""
    M = spec["M"]
    alpha = sorted(r for r in spec["alpha"] if 0 < r < n_rows)
    out = []
    for i in range(c):
        s, e = set(spec["start"][i]), set(spec["end"][M - c + i])
        comb = (s & e) or (s | e)
        out.append(sorted(comb & set(alpha)) if comb else alpha)
    return out


def brute_candidate(spec, c, valid, row_mass, row_mod, mod_cap, row_cap, precision, max_combos):
    """(status, combos, n_feas, best) by the definition."""
    if not valid:
        return INVALID, 0, 0, 0
    n, n_rows = max(c, 0), len(row_mass)
    pats = [replay_set_x(code, mn, mx, n) for code, _, mn, mx in spec["frags"]]
    if any(p is None for p in pats):
        return RAISES, 0, 0, 0
    q = [qfix(su, precision) for _, su, _, _ in spec["frags"]]
    if c < 1 or c > MAX_LEN or c > spec["M"] or not pats or len(pats) > 16384 or any(v is None for v in q):
        return NOT_MODELLED, 0, 0, 0
    runs = [runs_of(p) for p in pats]
    if not all(modelled(r, n) for r in runs):
        return NOT_MODELLED, 0, 0, 0
    sets = position_rows(spec, c, n_rows)
    combos = math.prod(len(rows) for rows in sets)
    if combos == 0:
        return INFEASIBLE, 0, 0, 0
    combos = min(combos, (1 << 64) - 1)
    cap_c = np.asarray(row_cap).reshape(MAX_LEN + 1, n_rows)[c]
    for r in sorted(x for x in spec["alpha"] if 0 < x < n_rows):
        n_r = sum(r in rows for rows in sets)
        if not (cap_c[r] >= n_r or (row_mod[r] and cap_c[r] >= mod_cap)):
            return NOT_FREE, combos, 0, 0
    if combos > max_combos:
        return TOO_LARGE, combos, 0, 0
    n_feas, best = 0, None
    for y in itertools.product(*sets):
        if sum(int(row_mod[r]) for r in y) > mod_cap:
            continue
        n_feas += 1
        obj = sum(min(abs(q[j] - FIX * (sum(int(row_mass[y[i]]) for i in range(run[0], run[1] + 1)) if run else 0))
                      for run in runs[j]) for j in range(len(pats)))
        best = obj if best is None or obj < best else best
    if n_feas == 0:
        return INFEASIBLE, combos, 0, 0
    return SOLVED, combos, n_feas, best


def brute(specs, valid, row_mass, caps, precision, max_combos):
    """(status, combos, n_feas, best) arrays over all candidates."""
    row_mod, mod_cap, row_cap = caps
    res, k = [], 0
    for s in specs:
        for c in candidates_of(s):
            res.append(brute_candidate(s, c, valid[k], row_mass, row_mod, int(mod_cap[k]), row_cap, precision,
                                       max_combos))
            k += 1
    dts = (np.uint8, np.uint64, np.uint64, np.uint64)
    return tuple(np.array([r[i] for r in res], dtype=dt) for i, dt in enumerate(dts))


def assert_equal4(got, want, what=""):
    """A LengthOutcome against brute's four arrays (or another LengthOutcome)."""
    if not isinstance(want, tuple):
        want = tuple(getattr(want, k) for k in FIELDS[2:])
    for k, w in zip(FIELDS[2:], want):
        g = getattr(got, k)
        assert len(g) == len(w), (what, k, len(g), len(w))
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, k, bad[:8].tolist(), g[bad[:8]].tolist(), np.asarray(w)[bad[:8]].tolist())


# ---------------------------------------------------------------------------
# random spectra
# ---------------------------------------------------------------------------
def random_spec(rng, row_mass, precision, max_M=6, max_rows=3, max_cand=4, max_frags=5):
    """A spectrum whose candidates are mostly SOLVED: a hidden sequence of
    length T, skeletons that hold its rows (and others), a window of candidate
    lengths around T, fragments cut from it with ends near the truth.  One in
    ten is disturbed: wild ends, an empty position, a foreign row."""
    n_rows = len(row_mass)
    rows = list(range(1, n_rows))
    M = int(rng.integers(2, max_M + 1))
    T = int(rng.integers(1, M + 1))
    truth = [int(rng.choice(rows)) for _ in range(T)]
    wild = rng.random() < 0.1

    def side(seq_at):
        out = []
        for i in range(M):
            t = seq_at(i)
            u = rng.random()
            if t is None or u < 0.25:
                out.append([] if t is None or u < 0.15 else sorted({int(x) for x in rng.choice(rows, 2)}))
            else:
                extra = [int(x) for x in rng.choice(rows, int(rng.integers(0, max_rows)))]
                out.append(sorted({t, *extra}))
        return out

    start = side(lambda i: truth[i] if i < T else None)
    end = side(lambda i: truth[i - (M - T)] if i >= M - T else None)  # reversed END: E_{M - T + i} is position i
    alpha = sorted({r for p in start + end for r in p} | set(truth) | ({int(rng.choice(rows))} if rng.random() < 0.5 else set()))
    if wild and rng.random() < 0.5:
        alpha = alpha[1:] or alpha
    lower = max(T - int(rng.choice([0, 0, 0, 0, 0, 1, 2])), int(rng.integers(-1, 2)) if rng.random() < 0.08 else 1)
    upper = lower + int(rng.choice([0, 0, 0, 0, 1, 1, 2, max_cand - 1])) - (1 if rng.random() < 0.05 else 0)
    if rng.random() < 0.03:
        upper = M + 1
        lower = max(lower, upper - max_cand + 1)
    pre = np.concatenate([[0], np.cumsum([row_mass[r] for r in truth])])
    frags = []
    for _ in range(int(rng.integers(0 if rng.random() < 0.04 else 1, max_frags + 1))):
        kind = rng.random()
        noise = float(rng.normal(0, 0.3)) * precision
        if kind < 0.15:
            frags.append((START_END | int(rng.integers(0, 4)), float(pre[T]) * precision + noise, int(rng.integers(0, M + 1)),
                          int(rng.integers(0, M + 1))))
        elif kind < 0.6:  # START: the walk's ends are one past the last position
            e = int(rng.integers(1, T + 1))
            a, b = max(1, e - int(rng.integers(0, 2))), e + int(rng.integers(0, 2))
            if wild:
                a, b = int(rng.integers(-1, M + 3)), int(rng.integers(-1, M + 3))
            frags.append((START | int(rng.integers(0, 4)), float(pre[e]) * precision + noise, a, b))
        else:  # END: the walk counts from the 3' end
            k = int(rng.integers(1, T + 1))
            a, b = max(1, k - int(rng.integers(0, 2))), k + int(rng.integers(0, 2))
            if wild:
                a, b = int(rng.integers(-1, M + 3)), int(rng.integers(-1, M + 3))
            frags.append((END | int(rng.integers(0, 4)), float(pre[T] - pre[T - k]) * precision + noise, a, b))
    # the sequence's mass: mostly inside what validate_sequence_length_by_mass sums at T (an empty union counts 0)
    unions = [(set(start[i]) | set(end[M - T + i])) or {0} for i in range(T)]
    # (a position's smallest and largest mass are its lowest and highest row's: a table's rows ascend by mass)
    lo_m, hi_m = sorted(sum(row_mass[f(u)] for u in unions) for f in (min, max))
    su_mass = (float(rng.uniform(lo_m, hi_m)) if rng.random() < 0.94 else float(pre[T]) + 4.0 / precision) * precision
    return {"M": M, "start": start, "end": end, "alpha": alpha, "lower": lower, "upper": upper,
            "lb_status": int(rng.random() < 0.04) * -3, "su_mass": su_mass, "frags": frags}


def random_case(seed, row_mass, precision, n, **kw):
    """(specs, row_mod, rate, rates): n random spectra, a third of the rows modified, one tight per-row rate in every second case."""
    rng = np.random.default_rng(seed)
    n_rows = len(row_mass)
    row_mod = np.array([0] + [int(rng.random() < 0.35) for _ in range(1, n_rows)], dtype=np.uint8)
    rate = float(rng.choice([0.25, 0.5, 1.0, 1.0]))
    rates = [0.0] + [1.0] * (n_rows - 1)
    if seed % 2:
        rates[int(rng.integers(1, n_rows))] = 0.34  # one row's cap may bind: NOT_FREE
    return [random_spec(rng, row_mass, precision, **kw) for _ in range(n)], row_mod, rate, rates


def host(specs, row_mass, caps, precision, max_combos=1 << 20, valid=None):
    from spectrseqtools_amd import length_program as LP

    cases = make_cases(specs, row_mass)
    valid = LP.length_valid(cases, precision) if valid is None else valid
    return LP.length_program_host(cases, precision, valid, caps, max_combos=max_combos), valid


# ---------------------------------------------------------------------------
# edge cases (any table with at least six rows of distinct masses)
# ---------------------------------------------------------------------------
def fixed_spec(row_mass, sets, frags, cands, precision, M=None, alpha=None, su_mass=None):
    """A spectrum whose START skeleton holds `sets` (row lists, the rest of the
    M positions empty) and whose END skeleton is empty: at c = len(sets) the
    combined skeleton is `sets`.  su_mass defaults to the sum of the sets'
    smallest masses (valid at c = len(sets))."""
    M = len(sets) if M is None else M
    start = [list(r) for r in sets] + [[] for _ in range(M - len(sets))]
    lo = sum(min(row_mass[r] for r in rows) for rows in sets)
    return {"M": M, "start": start[:M], "end": [[] for _ in range(M)],
            "alpha": sorted({r for rows in sets for r in rows}) if alpha is None else list(alpha),
            "lower": cands[0], "upper": cands[1], "su_mass": lo * precision if su_mass is None else su_mass,
            "frags": list(frags)}


def free_positions(row_mass, radices, fixed=0):
    """Position sets with the given radices over rows 1 .., then `fixed` one-row positions."""
    return [list(range(1, 1 + r)) for r in radices] + [[1 + (i % 2)] for i in range(fixed)]


def mass_range(spec, c, row_mass):
    """(min_mass, max_mass) of validate_sequence_length_by_mass at 0 <= c <= M, in integer masses."""
    M = spec["M"]
    unions = [set(spec["start"][i]) | set(spec["end"][M - c + i]) for i in range(c)]
    return (sum(min(row_mass[r] for r in u) for u in unions if u), sum(max(row_mass[r] for r in u) for u in unions if u))


def start_pins(row_mass, y, at, precision):
    """START fragments whose only end is position r (raw ends r + 1), at the prefix sums of y (one row per position)."""
    pre = np.cumsum([int(row_mass[r]) for r in y])
    return [(START, float(pre[r]) * precision, r + 1, r + 1) for r in at]


def solved_spec(row_mass, sets, precision, c=None, M=None, frags=None, cands=None):
    """fixed_spec at candidate c = len(sets) (or the given one), valid there, with START pins at its ends and a
    START_END fragment unless frags are given."""
    c = len(sets) if c is None else c
    y = [rows[-1] for rows in sets]
    if frags is None:
        frags = start_pins(row_mass, y, sorted({0, c // 2, c - 1}), precision) + \
            [(START_END, float(sum(row_mass[r] for r in y[:c])) * precision, 0, 0)]
    spec = fixed_spec(row_mass, sets, frags, cands or (c, c), precision, M=M)
    lo, hi = mass_range(spec, c, row_mass)
    spec["su_mass"] = (lo + hi) / 2 * precision
    return spec


def edge_cases(rm, precision):
    """{name: (specs, row_mod, rate, rates or None (loose), max_combos)} on a table of at least six rows of
    ascending distinct masses: the cases the GPU tests list, at sizes the host model enumerates quickly."""
    n_rows = len(rm)
    zero = np.zeros(n_rows, np.uint8)
    hi_mod = zero.copy()
    hi_mod[2:] = 1
    out = {}
    # c of 1, of M and of 253; lower == upper throughout
    long_sets = free_positions(rm, [2, 3, 2], fixed=250)
    out["lengths_1_M_253"] = ([solved_spec(rm, long_sets, precision),
                               solved_spec(rm, long_sets, precision, c=1, cands=(1, 1)),
                               solved_spec(rm, free_positions(rm, [2, 2], fixed=2), precision)], zero, 1.0, None, 1 << 20)
    # no candidates: lower > upper, and bounds that raised; a window that reaches above M (empty skeletons: every
    # length is valid at su_mass 0.5)
    none = dict(solved_spec(rm, free_positions(rm, [2, 2]), precision), lower=3, upper=2)
    raised = dict(solved_spec(rm, free_positions(rm, [2, 2]), precision), lb_status=-5)
    above = {"M": 3, "start": [[], [], []], "end": [[], [], []], "alpha": [1, 2], "lower": 2, "upper": 5,
             "su_mass": 0.5, "frags": [(START_END, rm[1] * 3 * precision, 0, 0)]}
    out["no_candidates_and_above_M"] = ([none, raised, above, dict(above, lower=0, upper=1)], zero, 1.0, None, 1 << 20)
    # combos == max_combos and max_combos + 1
    sixteen = solved_spec(rm, free_positions(rm, [2, 2, 2, 2]), precision)
    out["combos_at_max"] = ([sixteen], zero, 1.0, None, 16)
    out["combos_above_max"] = ([sixteen], zero, 1.0, None, 15)
    # one lane: every position fixed
    out["one_lane"] = ([solved_spec(rm, free_positions(rm, [], fixed=7), precision)], zero, 1.0, None, 1)
    # the modification cap: binding, and no feasible y (rate 0: mod_cap 0; every row of a position modified)
    mods = solved_spec(rm, [[2, 3], [1, 2], [3, 4], [1]], precision)
    out["mod_cap_binds"] = ([mods], hi_mod, 0.5, None, 1 << 20)
    out["mod_cap_no_feasible"] = ([mods], hi_mod, 0.0, None, 1 << 20)
    # an empty A_i: a position whose rows the alphabet does not hold
    empty = solved_spec(rm, [[1, 2], [3], [1, 4]], precision)
    out["empty_A_i"] = ([dict(empty, alpha=[1, 2, 4])], zero, 1.0, None, 1 << 20)
    # per-row caps that may bind
    out["not_free"] = ([solved_spec(rm, [[1, 2], [1, 3], [1, 4], [1]], precision)], zero, 1.0,
                       [0.0, 0.5] + [1.0] * (n_rows - 2), 1 << 20)
    # each shape and each RAISES condition at its boundary, c = 4
    c = 4
    sets = free_positions(rm, [2, 3, 2, 2])
    total = float(sum(rm[rows[0]] for rows in sets)) * precision
    boundary = {"start_mn_c-1": (START, c, c), "start_mn_c": (START, c + 1, c + 1), "start_mx_over": (START, 2, c + 3),
                "start_mn_gt_mx": (START, 3, 1), "start_empty": (START, 1, 0), "start_empty_wrap": (START, 1, -c),
                "start_raises_wrap": (START, 1, -c - 1), "start_no_ones": (START, 0, 2),
                "end_mx_c": (END, 2, 0), "end_mx_c+1": (END, 2, -1), "end_mn_gt_mx": (END, 1, 3),
                "end_wrapped": (END, c + 1, c), "end_wrapped_last": (END, 2 * c, 1), "end_raises_wrap": (END, 2 * c + 1, 1),
                "end_empty": (END, 0, 0), "end_no_ones": (END, 0, 2), "end_range": (END, 3, 1),
                "internal": (0, 1, 1), "whole": (START_END, 99, -99)}
    out["shape_boundaries"] = ([solved_spec(rm, sets, precision, frags=[(code, total / 2, a, b),
                                                                         (START_END, total, 0, 0)])
                                for code, a, b in boundary.values()], zero, 1.0, None, 1 << 20)
    # 513 fragments: two chunks of records
    y = [rows[-1] for rows in sets]
    many = [start_pins(rm, y, [i % c], precision)[0] for i in range(512)] + [(START_END, total, 0, 0)]
    out["513_fragments"] = ([solved_spec(rm, sets, precision, frags=many)], zero, 1.0, None, 1 << 20)
    # the fixed-point limit: |su / prec| just below 2^32 is modelled, 2^32 is not; NaN and inf are not
    below = float(np.nextafter(np.float64(2.0 ** 32), 0.0)) * precision
    limit = [solved_spec(rm, sets, precision, frags=[(START_END, su, 0, 0), (START, total / 3, 2, 2)])
             for su in (below, -below, 2.0 ** 32 * precision, float("nan"), float("inf"))]
    out["fixed_point_limit"] = (limit, zero, 1.0, None, 1 << 20)
    return out
