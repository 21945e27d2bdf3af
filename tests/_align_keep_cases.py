"""The brute-force model and the edge cases of the alignment certificate's keep
mode (alignment.align_host(keep=...), sst_align_windows_keep_device,
sst_align_split_keep_device), shared by tests/test_align_keep_model.py (CPU) and
tests/test_gpu_align_keep.py.

Built on tests/_align_caps_cases.py: a spectrum carries "row_mod" and "mod_cap";
a case carries one row_cap table (i32 [254 * n_rows], row_cap[L * n_rows + r]).
The definition taken literally: every y over all positions within the universal
cap (itertools.product, _align_caps_cases.capped_sums), then the row-free test,
then the inner window.
TEST INFRASTRUCTURE."""
import math

import numpy as np

import _align_caps_cases as CC
import _align_cases as AC

FIELDS7 = ("status", "alignable", "n_fit", "first", "keep", "keep_first", "spec_free")
MAX_LEN = 253
RATES = (0.1, 0.34, 0.5, 1.0)


def inner_w(obs, tolerance, precision):
    """W_in by the definition: floor(q) - 1 for a finite q >= 1, else -1."""
    q = tolerance * obs / precision
    return math.floor(q) - 1 if math.isfinite(q) and q >= 1 else -1


def row_cap_table(rates, n_rows=None):
    """row_cap[L * n_rows + r] = int(np.ceil(rates[r] * L)), L in [0, 253]."""
    n_rows = len(rates) if n_rows is None else n_rows
    return np.array([int(np.ceil(rates[r] * L)) for L in range(MAX_LEN + 1) for r in range(n_rows)], dtype=np.int32)


def loose_row_cap(n_rows):
    """Every row may fill every position: every spectrum is row-free."""
    return row_cap_table([1.0] * n_rows)


def row_free(spec, n_rows, row_cap):
    """Every row of alpha except row 0 is free: row_cap >= n_r, or the row is
    modified and row_cap >= mod_cap."""
    sets = CC.position_rows(spec, n_rows)
    L = spec["L"]
    for r in AC.rows_of(spec["alpha"], n_rows):
        if r == 0:
            continue
        n_r = sum(r in rows for rows in sets)
        cap = int(row_cap[L * n_rows + r])
        if not (cap >= n_r or (spec["row_mod"][r] and cap >= spec["mod_cap"])):
            return False
    return True


def brute_keep_spectrum(spec, row_mass, row_cap, tolerance, precision, capacity, split=False):
    """([(keep, keep_first)] per fragment, spec_free) from the definition."""
    L, nf = spec["L"], len(spec["frags"])
    sums, _ = CC.capped_sums(spec, row_mass)
    if sums is None:  # an empty A_i, or no y within the universal cap: INFEASIBLE
        return [(0, 0xFFFE)] * nf, 0
    free = row_free(spec, len(row_mass), row_cap)
    closed = {k: len(v) <= capacity for k, v in sums.items()}
    base = CC.brute_caps_spectrum(spec, row_mass, tolerance, precision, capacity, split=False)
    out = []
    for (code, su, obs, mn, mx), (st, _, _) in zip(spec["frags"], base):
        w_in = inner_w(obs, tolerance, precision)
        if st == AC.SKIPPED or not free or w_in < 0:
            out.append((0, 0xFFFE))
            continue
        target = round(su / precision)
        inside = lambda iv: any(abs(v - target) <= w_in for v in sums[iv])  # noqa: E731
        ivs = AC.admissible_intervals(code, mn, mx, L)
        fits = [iv for iv in ivs if closed[iv] and inside(iv)]
        if split and st == AC.OPEN:  # recomputed over the split-closed intervals
            fits += [(l, r) for l, r in ivs if not closed[l, r] and inside((l, r))
                     and any(closed[l, m] and closed[m + 1, r] for m in range(l, r))]
        out.append((1, min(fits)[0] << 8 | min(fits)[1]) if fits else (0, 0xFFFE))
    return out, int(free)


def brute_keep(specs, row_mass, row_cap, tolerance, precision, capacity, split=False):
    """The seven arrays of a case: the four of _align_caps_cases.brute_caps,
    then keep, keep_first (per fragment) and spec_free (per spectrum; 0 for a
    spectrum without fragments)."""
    four = CC.brute_caps(specs, row_mass, tolerance, precision, capacity, split)
    res, free = [], []
    for s in specs:
        if s.get("default") or not s["frags"]:
            free.append(0)
            continue
        r, f = brute_keep_spectrum(s, row_mass, row_cap, tolerance, precision, capacity, split)
        res += r
        free.append(f)
    return four + (np.array([r[0] for r in res], dtype=np.uint8), np.array([r[1] for r in res], dtype=np.uint16),
                   np.array(free, dtype=np.uint8))


def random_keep_case(seed, row_mass, tolerance, precision, n, **kw):
    """(specs, row_cap): _align_caps_cases.random_caps_case and one rate per row
    drawn from RATES, so that some spectra are row-free and some are not."""
    specs = CC.random_caps_case(seed, row_mass, tolerance, precision, n, **kw)
    rng = np.random.default_rng(seed + 100000)
    rates = [0.0] + [1.0 if rng.random() < 0.5 else float(rng.choice(RATES)) for _ in row_mass[1:]]
    for s in specs:
        s["frags"] = [widened(f, rng, tolerance, precision) if rng.random() < 0.5 else f for f in s["frags"]]
    return specs, row_cap_table(rates)


def widened(frag, rng, tolerance, precision):
    """The fragment with an observed mass whose q is 2, 3, 4 or 4.4 (random_spectrum's
    are mostly below 1, where nothing fits inside): W_in = 1, 2, 3, 3."""
    code, su, _, mn, mx = frag
    return (code, su, float(rng.choice([2.0, 3.0, 4.0, 4.4])) * precision / tolerance, mn, mx)


def assert_equal7(got, want, what=""):
    """An AlignOutcome in keep mode against the seven arrays."""
    for k, w in zip(FIELDS7, want):
        g = getattr(got, k)
        assert g is not None and len(g) == len(w), (what, k)
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, k, bad[:8].tolist(), g[bad[:8]].tolist(), np.asarray(w)[bad[:8]].tolist())


def same7(a, b, what=""):
    """Two AlignOutcomes in keep mode, all seven arrays."""
    assert_equal7(a, tuple(getattr(b, k) for k in FIELDS7), what)


# ---------------------------------------------------------------------------
# edge cases (any table: row masses, tolerance and precision are the caller's)
# ---------------------------------------------------------------------------
def observed_masses(tolerance, precision):
    """Observed masses by what q = tolerance * obs / precision is in f64:
    "integer" (q an exact integer >= 3: W - W_in == 1), "above" (q just above an
    integer >= 3: W - W_in == 2), "below_one" (0 < q < 1), "zero", "inf", "nan"
    and "huge" (W and W_in both clamped)."""
    out = {"zero": 0.0, "inf": math.inf, "nan": math.nan, "huge": 1e300}
    for k in range(1, 200000):
        obs = float(k)
        q = tolerance * obs / precision
        if q < 3 or q > 1000:
            if 0 < q < 1:
                out.setdefault("below_one", obs)
            continue
        if q == math.floor(q):
            out.setdefault("integer", obs)
        elif q - math.floor(q) < 1e-9:
            out.setdefault("above", obs)
        if len(out) == 7:
            break
    # ("above" exists only where the two f64 operations round: not for tolerance / precision = 0.02 / 0.5)
    assert len(out) == 7 or (len(out) == 6 and "above" not in out), sorted(out)
    assert math.ceil(tolerance * out["integer"] / precision) - inner_w(out["integer"], tolerance, precision) == 1
    if "above" in out:
        assert math.ceil(tolerance * out["above"] / precision) - inner_w(out["above"], tolerance, precision) == 2
    return out


def window_edge_spec(row_mass, rows, tolerance, precision):
    """One spectrum of L = 2 over two unmodified rows (one row per position),
    START_END and internal fragments whose targets sit at the only sum +- W_in,
    +- (W_in + 1), +- W and +- (W + 1) for every kind of observed mass, and at
    0 +- the same (the empty interval).  Returns (spec, [(kind, delta, W, W_in)])."""
    a, b = rows
    total = int(row_mass[a]) + int(row_mass[b])
    frags, notes = [], []
    for kind, obs in observed_masses(tolerance, precision).items():
        q = tolerance * obs / precision
        w = math.ceil(q) if math.isfinite(q) else -1
        w_in = inner_w(obs, tolerance, precision)
        if kind in ("inf", "huge"):
            deltas = [0, 5, -5]
        else:
            deltas = sorted({s * d for s in (1, -1) for d in (0, max(w_in, 0), w_in + 1, max(w, 0), w + 1)})
        for d in deltas:
            for base, code in ((total, AC.code_of(True, True)), (total, AC.code_of(False, False)),
                               (0, AC.code_of(False, False))):
                frags.append((code, (base + d) * precision, obs, 0, 0))
                notes.append((kind, d, w, w_in))
    order = np.argsort([f[1] for f in frags], kind="stable")
    spec = {"L": 2, "pos": [AC.mask([a]), AC.mask([b])], "alpha": AC.mask([a, b]),
            "frags": [frags[i] for i in order]}
    return spec, [notes[i] for i in order]


def row_edge_specs(row_mass, unmod, mod, tolerance, precision):
    """Four spectra of L = 3 and their per-spectrum expectations, to be run
    with the row_cap table of row_edge_caps: positions {u1, u2} x 3 with row_cap
    of u1 == n_r (free) and, on a second pair, == n_r - 1 (not free); positions
    {u, m} x 3 (m modified, n_m = 3) with mod_cap = 1 and row_cap of m == mod_cap
    (free by the second clause) and, on a second pair, == mod_cap - 1 (not free).
    unmod: four unmodified rows, mod: two modified rows."""
    u1, u2, u3, u4 = unmod
    m1, m2 = mod
    obs = observed_masses(tolerance, precision)["integer"]
    specs = []
    for rows, cap in (((u1, u2), 3), ((u3, u4), 3), ((u1, m1), 1), ((u2, m2), 1)):
        both = AC.mask(rows)
        t = 3 * int(row_mass[rows[0]])
        frags = [(AC.code_of(True, True), t * precision, obs, 0, 0), (AC.code_of(False, False), t * precision, obs, 0, 0),
                 (AC.code_of(True, False), int(row_mass[rows[0]]) * precision, obs, 0, 0)]
        specs.append({"L": 3, "pos": [both] * 3, "alpha": both, "mod_cap": cap,
                      "frags": sorted(frags, key=lambda f: f[1])})
    return specs, [1, 0, 1, 0]


def row_edge_caps(n_rows, unmod, mod):
    """The row_cap table of row_edge_specs: at L = 3, u1 and u2 may appear 3
    times (== n_r), u3 only 2 (== n_r - 1); m1 once (== mod_cap), m2 never
    (== mod_cap - 1); every other entry is L."""
    u1, u2, u3, u4 = unmod
    m1, m2 = mod
    t = loose_row_cap(n_rows).reshape(MAX_LEN + 1, n_rows)
    t[3, u3] = 2
    t[3, m1] = 1
    t[3, m2] = 0
    return t.reshape(-1)
