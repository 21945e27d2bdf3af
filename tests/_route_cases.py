"""Explain cases that sit on the engine's routing thresholds and inside each
of its routes, with the CPU oracle's answers (no GPU needed: the GPU tests in
test_gpu_routes.py and the CPU companion in test_route_cases.py share them).

The engine classifies a window [lo, hi] (quantised masses) in three places
(sst_kernels.hip: the fused scan, k_bitset_scan for uploaded tables, and the
unclassified items of the deferred scan) by

    pair     hi < 3 w_min              (tables with a pair list), budgets never bind
    shallow  hi < 4 w_min,             budgets never bind
    deep     hi >= 4 w_min,            budgets never bind
    exact / no-memo                    budgets may bind (with_memo / not)

where "budgets never bind" is hi <= fast_limit_B = min over the modification
rows of (cap + 1) w - 1, and hi < (A + 1) w_min_mod.  The answers change at
exactly these values: at 3 w_min the first three-row candidate appears, at
4 w_min the first four-row one, at (A + 1) w_min_mod the first candidate the
budget A excludes and at fast_limit_B + 1 the first one a row's cap excludes.

Masses and thresholds are exact multiples of the precision (as doubles that
quantise to the intended integers: checked here), so the windows are what is
tested, not the quantisation."""
import functools

import numpy as np

import _oracle as oracle
from conftest import load_golden

TOL, PREC = 1e-5, 1e-3
CANONICAL = (305042, 306026, 329053, 345048)
SMALL = (0, 305042, 308042, 319058, 345048)
INF = -1  # the engine's and the oracle's "np.inf" budget
# sst_result_stats indices
SHALLOW, DEEP, EXACT, NOMEMO, PAIR = 0, 1, 2, 3, 6


class Table:
    def __init__(self, name, rows, max_len):
        self.name, self.rows, self.max_len = name, list(rows), max_len
        self.is_mod = [m not in CANONICAL and m != 0 for m in rows]
        self.caps = [round(max_len * (0.5 if md else (1.0 if m else 0.0))) for m, md in zip(rows, self.is_mod)]
        self.A = round(0.5 * max_len)
        self.w_min = min(m for m in rows if m > 0)
        mods = [m for m, md in zip(rows, self.is_mod) if md]
        self.w_min_mod = min(mods) if mods else None
        # min over the modification rows of (cap + 1) w - 1 (sst_table_set_budgets)
        self.fast_limit_B = min((c + 1) * m - 1 for m, md, c in zip(rows, self.is_mod, self.caps) if md) if mods else None
        self.max_mass = max(rows) * 35

    @functools.cached_property
    def host(self):
        return oracle.build_table(self.rows, self.max_mass, 32)

    @functools.cached_property
    def alph(self):
        return oracle.Alphabet(self.rows, self.is_mod, self.caps)


@functools.lru_cache(None)
def tables():
    g = load_golden("alphabet.json")
    full = sorted({r["tolerated_integer_masses"] for r in g["rows"]} | {0})
    t = {f"full_L{L}": Table(f"full_L{L}", full, L) for L in (2, 4, 20)}
    t["canon"] = Table("canon", (0,) + CANONICAL, 20)
    # C, G and the two lightest modifications of distinct mass: small lists at any
    # mass, so the thresholds at 11 w_min_mod (A = 10, caps of 10) can be enumerated
    t["small_L20"] = Table("small_L20", SMALL, 20)
    return t


@functools.lru_cache(None)
def unbudgeted(t):
    """The table's rows with caps no threshold case reaches (max_len 40: 20
    per modification) -- with max_modifications = INF, what the budgets exclude."""
    return Table(t.name + ":free", t.rows, 40)


def exact_inputs(target, thr_q):
    """Doubles (mass, threshold) that quantise to the integers given:
    rint(mass / PREC) == target and ceil(threshold / PREC) == thr_q."""
    target, thr_q = np.asarray(target, dtype=np.int64), np.asarray(thr_q, dtype=np.int64)
    mass, thr = target * PREC, thr_q * PREC
    over = np.ceil(thr / PREC) > thr_q  # q * 1e-3 / 1e-3 can come out an ulp above q
    thr = np.where(over, np.nextafter(thr, 0.0), thr)
    assert np.array_equal(np.rint(mass / PREC).astype(np.int64), target)
    assert np.array_equal(np.ceil(thr / PREC).astype(np.int64), thr_q)
    return mass, thr


class Case:
    """One batch: a table, windows (lo, hi as quantised masses), a budget
    (scalar, or one per query) and what it is meant to reach."""

    def __init__(self, name, table, lo, hi, A, kind, route=None, thresholds=None):
        lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        assert ((hi - lo) % 2 == 0).all() and (hi >= lo).all()
        self.name, self.table, self.kind, self.route = name, table, kind, route
        self.lo, self.hi = lo, hi
        self.A = A if np.isscalar(A) else np.asarray(A, dtype=np.int64)
        self.thresholds = thresholds  # per query: the index of its threshold (threshold cases)
        self.mass, self.thr = exact_inputs((lo + hi) // 2, (hi - lo) // 2)

    @property
    def n(self):
        return len(self.lo)

    @functools.lru_cache(None)
    def answers(self, with_memo=True):
        """(status, count, nbytes, digest) of every query, from the oracle."""
        t = self.table
        return oracle.explain_digest_batch(t.host, 32, t.alph, self.mass, self.thr, self.A, TOL, with_memo=with_memo,
                                           nthreads=16)

    def oracle_list(self, i, with_memo=True, A=None):
        t = self.table
        if A is None:
            A = int(np.broadcast_to(self.A, self.n)[i])
        return oracle.explain_table(t.host, 32, t.alph, self.mass[i], self.thr[i], TOL, A, with_memo=with_memo)[1]

    def n_some(self, with_memo=True):
        st, cnt, _, _ = self.answers(with_memo)
        return int(((st == 1) & (cnt > 0)).sum())


# ---------------------------------------------------------------------------
# threshold cases
# ---------------------------------------------------------------------------
HALF_WIDTHS = (0, 1, 4)  # windows of 1, 3 and 9 masses
# the largest window value at which the full alphabet's lists stay small (a
# few candidates per mass at four rows; the count grows by ~100x per row):
# thresholds past it are not enumerable on that alphabet
FULL_ALPHABET_MAX = 1_300_000


def thresholds(t):
    """[(what, T, budget A of the call)] of a table, sorted by T."""
    out = [("3w_min", 3 * t.w_min, t.A), ("4w_min", 4 * t.w_min, t.A)]
    if t.w_min_mod:
        for A in sorted({0, 1, 2, t.A}):
            out.append((f"A{A}", (A + 1) * t.w_min_mod, A))
        out.append(("fast_limit_B+1", t.fast_limit_B + 1, INF))
    return [x for x in out if len(t.rows) <= 8 or x[1] <= FULL_ALPHABET_MAX]


def threshold_windows(T):
    """Windows whose hi, then whose lo, is T-2 .. T+1, at each half width."""
    lo, hi = [], []
    for d in (-2, -1, 0, 1):
        for hw in HALF_WIDTHS:
            hi.append(T + d), lo.append(T + d - 2 * hw)  # hi on the edge
            lo.append(T + d), hi.append(T + d + 2 * hw)  # lo on the edge
    return np.array(lo), np.array(hi)


@functools.lru_cache(None)
def threshold_cases():
    """Per table: one case per threshold (scalar budget), and one case of all
    its thresholds with the budgets per query (the kernels' per-query-budget
    variants classify on their own)."""
    out = []
    for t in tables().values():
        alo, ahi, aA, aT = [], [], [], []
        for k, (what, T, A) in enumerate(thresholds(t)):
            lo, hi = threshold_windows(T)
            out.append(Case(f"{t.name}:{what}", t, lo, hi, A, "threshold", thresholds=np.full(len(lo), k)))
            alo.append(lo), ahi.append(hi), aA.append(np.full(len(lo), A)), aT.append(np.full(len(lo), k))
        out.append(Case(f"{t.name}:per_query_budgets", t, np.concatenate(alo), np.concatenate(ahi), np.concatenate(aA),
                        "threshold", thresholds=np.concatenate(aT)))
    return out


# ---------------------------------------------------------------------------
# route cases
# ---------------------------------------------------------------------------
def _sums(rng, pool, k, n):
    pool = np.asarray(pool, dtype=np.int64)
    return pool[rng.integers(0, len(pool), (k, n))].sum(axis=0)


def _around(rng, centre, max_hw, jitter=2):
    """Windows of half width 0..max_hw whose centre is at most `jitter` off."""
    n = len(centre)
    c = centre + rng.integers(-jitter, jitter + 1, n)
    hw = rng.integers(0, max_hw + 1, n)
    return c - hw, c + hw


@functools.lru_cache(None)
def route_cases():
    """One group per route, per table, each meant to reach `route` (an index
    of sst_result_stats on a table with the pair list; None: no route).
    On the full alphabet (budgets of max_len 20) and the canonical table."""
    out = []
    for name in ("full_L20", "canon"):
        t = tables()[name]
        full = name != "canon"
        rng = np.random.default_rng(len(t.rows))
        rows = np.array(t.rows[1:], dtype=np.int64)
        canon = np.array(CANONICAL, dtype=np.int64)
        mods = rows[~np.isin(rows, canon)]
        add = lambda grp, lo, hi, A, route: out.append(Case(f"{name}:{grp}", t, lo, hi, A, "route", route))
        # pair: one- and two-row sums (hi < 3 w_min)
        s = np.concatenate([_sums(rng, rows, 1, 48), _sums(rng, rows, 2, 80)])
        lo, hi = _around(rng, s, 20)
        keep = hi < 3 * t.w_min
        add("pair", lo[keep], hi[keep], t.A, PAIR)
        # shallow: three-row sums with 3 w_min <= hi < 4 w_min
        s = _sums(rng, rows[rows < 4 * t.w_min // 3 - 8], 3, 96)
        lo, hi = _around(rng, s, 6)
        keep = (hi >= 3 * t.w_min) & (hi < 4 * t.w_min)
        add("shallow", lo[keep], hi[keep], t.A, SHALLOW)
        # deep: sums of five to eight canonical rows, budgets not binding (the
        # full alphabet's lists grow ~100x per row: five rows there)
        ks = (5,) if full else (5, 6, 7, 8)
        s = np.concatenate([_sums(rng, canon, k, 48 // len(ks)) for k in ks])
        lo, hi = _around(rng, s, 2 if full else 30)
        assert (hi >= 4 * t.w_min).all() and (not full or (hi <= t.fast_limit_B).all())
        add("deep", lo, hi, t.A, DEEP)
        if full:
            # exact / no-memo: windows holding a sum with A + 1 modifications, A = 1
            # and 2, of three or four rows (the oracle excludes that sum; the
            # windows are wide enough for most to hold others)
            for A in (1, 2):
                other = _sums(rng, canon, 1, 64)
                s = _sums(rng, mods[mods < 330000], A + 1, 64) + np.where((rng.random(64) < 0.5) | (A == 1), other, 0)
                lo, hi = _around(rng, s, 40, 0)
                assert (hi >= (A + 1) * t.w_min_mod).all()
                add(f"exact_A{A}", lo, hi, A, EXACT)
        # windows without roots past the pair list: single masses between the reachable ones
        c = rng.integers(3 * t.w_min, 4 * t.w_min, 400)
        case = Case("probe", t, c, c, t.A, "route")
        st = case.answers()[0]
        c = c[st == 0][:64]
        add("no_roots", c, c, t.A, None)
        # windows reaching 0 and below: EMPTY alone, and with candidates
        lo = np.array([0, -4, -10, -300000, -1000, -2, 0, -305042, -320000])
        hi = np.array([0, 4, 0, 310000, 307000, 305042, 305042, 305042, 330000])
        hi += (hi - lo) % 2
        add("zero", lo, hi, t.A, None)
    return out


# the payload a first pass of up to 1024 queries holds before the engine runs
# it again: one scan workgroup's 16 waves x a 2 KB region (alloc_result; the
# fused scan's header compares the pass's dense payload with their sum)
FIRST_PASS_PAYLOAD = 16 * 2048


@functools.lru_cache(None)
def rerun_case():
    """A batch whose first pass outgrows its payload regions, (wide, narrow):
    every wide window spans 200 Da around 650 Da, where the pair list holds
    about one sum per 160 masses (~1300 candidates, ~4 KB), so a handful of
    them pass FIRST_PASS_PAYLOAD; `narrow` has the same centres (two-row sums)
    with windows of 61 masses, which the fused scan answers."""
    t = tables()["full_L20"]
    rng = np.random.default_rng(5)
    c = _sums(rng, [m for m in t.rows if 0 < m < 340000], 2, 400)  # two-row sums: the narrow windows have candidates
    c = c[(c >= 640000) & (c < 660000)][:130]
    wide = Case("rerun:wide", t, c - 100000, c + 100000, t.A, "rerun")
    narrow = Case("rerun:narrow", t, c - 30, c + 30, t.A, "rerun")
    return wide, narrow


def rerun_sizes():
    """(n_fit, n_over): n_over is the smallest n whose first n wide windows'
    lists pass FIRST_PASS_PAYLOAD; n_fit is three short of it, so that those
    lists fit with room to spare for the engine's padding (2 bytes and a
    16-byte round-up per query at most)."""
    nb = np.cumsum(rerun_case()[0].answers()[2])
    n_over = int(np.searchsorted(nb, FIRST_PASS_PAYLOAD, side="right")) + 1
    return n_over - 3, n_over
