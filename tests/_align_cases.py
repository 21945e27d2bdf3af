"""Cases and the brute-force model for the alignment certificate
(spectrseqtools_amd/alignment.py, sst_align_windows_device), shared by
tests/test_align_model.py (CPU) and tests/test_gpu_align.py.

A case is a list of spectra, each a dict
    L      seq_len
    pos    [(m0, m1)] position masks over table rows (L of them)
    alpha  (a0, a1)
    frags  [(code, su, obs, min_end, max_end)] in ascending su order
    default (optional) True: a Prediction.default() spectrum (nothing else read)
turned into a BatchOutcome by make_outcome.  brute_spectrum is the
definition taken literally: the intervals from a replay of
LinearProgramInstance._set_x's two loops (linear_program.py:74-102), the
sums from itertools.product over the interval's position sets.
TEST INFRASTRUCTURE."""
import itertools
import math

import numpy as np

START, END = 1 << 2, 1 << 3
NONE, FIT, OPEN, INFEASIBLE, SKIPPED = range(5)
BREAKAGE_NAMES = ["c/y_c/y", "START_c/y", "c/y_END", "START_END"]  # code & 3 (labels only; the side bits decide)


def code_of(start, end, singleton=False):
    return (1 if start and not end else 2 if end and not start else 3 if start else 0) | (START if start else 0) | \
        (END if end else 0) | (16 if singleton else 0)


def mask(rows):
    m = [0, 0]
    for r in rows:
        m[r >> 6] |= 1 << (r & 63)
    return tuple(m)


def rows_of(m, n_rows):
    return [r for r in range(n_rows) if (m[r >> 6] >> (r & 63)) & 1]


def make_outcome(specs, row_mass):
    from spectrseqtools_amd.pipeline_device import BatchOutcome

    S = len(specs)
    live = [s for s in specs if not s.get("default")]
    frags = [f for s in live for f in s["frags"]]
    col = lambda k, dt: np.array([f[k] for f in frags], dtype=dt)  # noqa: E731
    n_pos = [0 if s.get("default") else len(s["pos"]) for s in specs]
    n_frag = [0 if s.get("default") else len(s["frags"]) for s in specs]
    return BatchOutcome(
        default=[bool(s.get("default")) for s in specs], route=np.zeros(S, np.uint8), reason=np.zeros(S, np.uint8),
        alpha=np.array([(0, 0) if s.get("default") else s["alpha"] for s in specs], dtype=np.uint64).reshape(-1, 2),
        seq_len=[0 if s.get("default") else s["L"] for s in specs],
        pos_off=np.concatenate([[0], np.cumsum(n_pos)]),
        skeleton=np.array([p for s in live for p in s["pos"]], dtype=np.uint64).reshape(-1, 2),
        frag_off=np.concatenate([[0], np.cumsum(n_frag)]), frag_index=np.arange(len(frags)), frag_code=col(0, np.uint8),
        frag_su=col(1, np.float64), frag_obs=col(2, np.float64), frag_min_end=col(3, np.int32),
        frag_max_end=col(4, np.int32), breakage_names=BREAKAGE_NAMES,
        row_names=[""] + [f"n{r}" for r in range(1, len(row_mass))], row_mass=row_mass)


# ---------------------------------------------------------------------------
# the definition, literally
# ---------------------------------------------------------------------------
def replay_set_x(code, mn, mx, L):
    """x[i] in {None (free), 0, 1} after _set_x's fixings for one fragment
    (later fixings override earlier ones), its two loops per class replayed."""
    x = [None] * L
    if code & START and code & END:      # breakage == "START_END"
        for i in range(L):
            x[i] = 1
    elif code & START:                   # "START" in breakage
        for i in range(mn + 1):
            x[i] = 1
        for i in range(mx + 1, L):
            x[i] = 0
    elif code & END:                     # "END" in breakage
        for i in range(mx):
            x[i] = 0
        for i in range(mn, L):
            x[i] = 1
    return x


def admissible_intervals(code, mn, mx, L):
    """The contiguous position sets consistent with the fixings, in (l, r)
    order, the empty one (0xFF, 0xFF) last."""
    x = replay_set_x(code, mn, mx, L)
    out = []
    for l, r in [(l, r) for l in range(L) for r in range(l, L)] + [(0xFF, 0xFF)]:
        inside = set(range(l, r + 1)) if l != 0xFF else set()
        if all((x[i] != 1 or i in inside) and (x[i] != 0 or i not in inside) for i in range(L)):
            out.append((l, r))
    return out


def position_masses(spec, row_mass):
    n_rows = len(row_mass)
    out = []
    for p in spec["pos"]:
        rows = set(rows_of(p, n_rows)) & set(rows_of(spec["alpha"], n_rows)) if (p[0] | p[1]) else \
            set(rows_of(spec["alpha"], n_rows))
        out.append([int(row_mass[r]) for r in sorted(rows - {0})])
    return out


def brute_spectrum(spec, row_mass, tolerance, precision, capacity):
    """Per fragment (status, n_fit, first), and the largest |S(l, r)| seen."""
    L = spec["L"]
    sets = position_masses(spec, row_mass)
    if any(not m for m in sets):
        return [(INFEASIBLE, 0, 0xFFFE)] * len(spec["frags"]), 0
    sums = {(0xFF, 0xFF): {0}}
    for l in range(L):
        for r in range(l, L):
            sums[l, r] = {sum(c) for c in itertools.product(*sets[l:r + 1])}
    biggest = max(len(s) for s in sums.values())
    out = []
    for code, su, obs, mn, mx in spec["frags"]:
        terminal = bool(code & START) != bool(code & END)
        if terminal and not (0 <= mn < L and 0 <= mx < L):
            out.append((SKIPPED, 0, 0xFFFE))
            continue
        target, W = round(su / precision), math.ceil(tolerance * obs / precision)
        fits, opened = [], False
        for l, r in admissible_intervals(code, mn, mx, L):
            s = sums[l, r]
            if len(s) <= capacity:
                if any(abs(v - target) <= W for v in s):
                    fits.append((l, r))
            elif W >= 0 and target - W <= max(s) and target + W >= min(s):
                opened = True
        first = min(fits)[0] << 8 | min(fits)[1] if fits else 0xFFFE
        out.append((FIT if fits else OPEN if opened else NONE, len(fits), first))
    return out, biggest


def brute(specs, row_mass, tolerance, precision, capacity):
    """(status, alignable, n_fit, first) arrays over a case's fragments, and the largest |S|."""
    res, biggest = [], 0
    for s in specs:
        if s.get("default"):
            continue
        r, b = brute_spectrum(s, row_mass, tolerance, precision, capacity)
        res += r
        biggest = max(biggest, b)
    st = np.array([r[0] for r in res], dtype=np.uint8)
    return (st, ((st != NONE) & (st != INFEASIBLE)).astype(np.uint8), np.array([r[1] for r in res], dtype=np.uint32),
            np.array([r[2] for r in res], dtype=np.uint16), biggest)


# ---------------------------------------------------------------------------
# random spectra
# ---------------------------------------------------------------------------
def random_spectrum(rng, row_mass, tolerance, precision, max_len=6, max_alpha=6, max_set=3, n_frags=None):
    """L in 1 .. max_len, an alphabet of <= max_alpha rows, position sets of <=
    max_set rows (some masks empty = unconstrained, rarely one disjoint from the
    alphabet = an empty A_i), all four classes, mn > mx, ends out of range,
    near-zero internal fragments (the empty interval)."""
    n_rows = len(row_mass)
    rows = list(range(1, n_rows))
    L = int(rng.integers(1, max_len + 1))
    alpha_rows = sorted(rng.choice(rows, size=min(len(rows), int(rng.integers(1, max_alpha + 1))), replace=False).tolist())
    pos = []
    for _ in range(L):
        u = rng.random()
        if u < 0.12 and len(alpha_rows) <= max_set:
            pos.append((0, 0))  # unconstrained: the alphabet
        elif u < 0.15 and len(alpha_rows) < len(rows):
            pos.append(mask([r for r in rows if r not in alpha_rows][:1]))  # A_i empty
        else:
            k = int(rng.integers(1, min(max_set, len(alpha_rows)) + 1))
            pos.append(mask(rng.choice(alpha_rows, size=k, replace=False).tolist() + ([0] if rng.random() < 0.1 else [])))
    spec = {"L": L, "pos": pos, "alpha": mask(alpha_rows + [0])}
    sets = position_masses(spec, row_mass)
    frags = []
    for _ in range(int(rng.integers(1, 9)) if n_frags is None else n_frags):
        start, end = (bool(x) for x in rng.integers(0, 2, 2))
        l = int(rng.integers(0, L))
        r = int(rng.integers(l, L))
        if start:
            l = 0
        if end:
            r = L - 1
        true = sum(int(rng.choice(m)) if m else 0 for m in sets[l:r + 1])  # a window's sum ...
        u = rng.random()
        if u < 0.1:
            true = 0                                                      # ... the empty interval's
        elif u < 0.2:
            true += int(rng.integers(-40, 41))
        obs = float(rng.choice([0.0, 1.0, 3.0, 40.0]) if rng.random() < 0.5 else rng.uniform(0, 60))
        W = math.ceil(tolerance * obs / precision)
        su = (true + int(rng.integers(-W - 2, W + 3)) + float(rng.choice([0.0, 0.3, -0.3, 0.5, -0.5]))) * precision
        mn, mx = (int(x) for x in rng.integers(0, L, 2))
        if rng.random() < 0.1:
            mn = int(rng.choice([-1, L, L + 3]))
        if rng.random() < 0.1:
            mx = int(rng.choice([-2, L]))
        frags.append((code_of(start, end, rng.random() < 0.2), su, obs, mn, mx))
    spec["frags"] = sorted(frags, key=lambda f: f[1])
    return spec


def random_case(seed, row_mass, tolerance, precision, n, **kw):
    rng = np.random.default_rng(seed)
    return [random_spectrum(rng, row_mass, tolerance, precision, **kw) for _ in range(n)]


def assert_equal(got, want, what=""):
    """An AlignOutcome against (status, alignable, n_fit, first) arrays."""
    for k, w in zip(("status", "alignable", "n_fit", "first"), want):
        g = getattr(got, k)
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, k, bad[:8].tolist(), g[bad[:8]].tolist(), np.asarray(w)[bad[:8]].tolist())
