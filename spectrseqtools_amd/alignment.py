"""The alignment certificate: which fragments of a BatchOutcome no window of
the skeleton can explain (include/sst.h, sst_align_windows_device; DESIGN
"Alignment certificate").

filter_with_lp (prediction.py:229-259) solves one LinearProgramInstance per
surviving fragment to learn whether it can sit on a contiguous run of
skeleton positions within tolerance * observed_mass.  A fragment with
alignable == 0 here is removed by every outcome of that solve, so the solve
can be skipped; alignable == 1 promises nothing.

align_host is the definition in plain numpy / Python (the mirror for spectra
run_batch routed to the host, and the model the tests hold the kernel to),
align_device the kernel (csrc/sst_align.hip) over a whole outcome.

split=True (both) also decides the open intervals that cut into two closed
halves, a fitting sum searched as a + b over the halves' sorted lists
(sst_align_split_device); only fragments that are OPEN without it change.

caps (both) carries the program's universal modification cap (linear_program
.py:180-188) exactly: per distinct sum the fewest modified rows beyond the
forced ones, sums that need more than the spectrum's budget leave the lists
(sst_align_windows_caps_device, sst_align_split_caps_device; lp_caps builds the
two inputs).  The per-row caps (:190-196) stay dropped.

keep (both, with caps) gives the certificate its second side: where a
per-spectrum test shows the per-row caps implied by the universal one
(spec_free; lp_row_caps builds the input), the capped lists are exactly the
program's sums, and a sum inside a slightly narrower window is a feasible
point of the program within the threshold: keep == 1, a solve run to
optimality keeps the fragment (sst_align_windows_keep_device,
sst_align_split_keep_device).  lp_decisions turns an outcome into DROP / KEEP
/ SOLVE.  A solver stopped by its time limit may still lose a KEEP fragment;
DROP holds under every outcome of the solve.
"""
import ctypes
import math
from dataclasses import dataclass

import numpy as np

from . import _native
from ._native import ALIGN_FIT, ALIGN_INFEASIBLE, ALIGN_NONE, ALIGN_OPEN, ALIGN_SKIPPED

ALIGN_CAPACITY = 1024   # sst_align_capacity(): sums a closed interval may have
ALIGN_MAX_LEN = 253     # longer skeletons are not modelled (SKIPPED)
EMPTY_INTERVAL = 0xFFFF  # `first` of the empty interval, (l, r) = (0xFF, 0xFF)
NO_INTERVAL = 0xFFFE     # `first` when n_fit == 0
STATUS_NAMES = {ALIGN_NONE: "NONE", ALIGN_FIT: "FIT", ALIGN_OPEN: "OPEN", ALIGN_INFEASIBLE: "INFEASIBLE",
                ALIGN_SKIPPED: "SKIPPED"}
_CLAMP = 1 << 61


@dataclass
class AlignOutcome:
    """The certificate per fragment, parallel to BatchOutcome's fragment
    arrays (fragment k of spectrum g at frag_off[g] + k), as host arrays."""
    frag_off: np.ndarray   # [S + 1] i64, the BatchOutcome's
    status: np.ndarray     # u8 ALIGN_NONE / FIT / OPEN / INFEASIBLE / SKIPPED
    alignable: np.ndarray  # u8: 0 -> filter_with_lp removes the fragment
    n_fit: np.ndarray      # u32 closed admissible intervals holding a fitting sum
    first: np.ndarray      # u16 l << 8 | r of the first of them, NO_INTERVAL if none
    # keep mode only (None otherwise; all three or none):
    keep: np.ndarray = None        # u8 per fragment: 1 -> a completed solve keeps the fragment
    keep_first: np.ndarray = None  # u16 per fragment: the first interval with an inner fit, NO_INTERVAL if none
    spec_free: np.ndarray = None   # u8 per spectrum: modelled, feasible and row-free

    FRAGMENT_FIELDS = ("status", "alignable", "n_fit", "first")
    _DTYPES = {"frag_off": np.int64, "status": np.uint8, "alignable": np.uint8, "n_fit": np.uint32,
               "first": np.uint16}
    KEEP_FRAGMENT_FIELDS = ("keep", "keep_first")
    _KEEP_DTYPES = {"keep": np.uint8, "keep_first": np.uint16, "spec_free": np.uint8}

    def __post_init__(self):
        for k, dt in self._DTYPES.items():
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))
        if len(self.frag_off) < 1 or any(len(getattr(self, k)) != int(self.frag_off[-1]) for k in self.FRAGMENT_FIELDS):
            raise ValueError("AlignOutcome: arrays do not match frag_off")
        present = [getattr(self, k) is not None for k in self._KEEP_DTYPES]
        if any(present):
            if not all(present):
                raise ValueError("AlignOutcome: keep, keep_first and spec_free come together")
            for k, dt in self._KEEP_DTYPES.items():
                setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))
            if any(len(getattr(self, k)) != int(self.frag_off[-1]) for k in self.KEEP_FRAGMENT_FIELDS) or \
                    len(self.spec_free) != len(self.frag_off) - 1:
                raise ValueError("AlignOutcome: keep arrays do not match frag_off")

    def __len__(self):
        return len(self.frag_off) - 1

    @property
    def has_keep(self):
        return self.keep is not None

    def equals(self, other):
        if self.has_keep != other.has_keep:
            return False
        fields = list(self._DTYPES) + (list(self._KEEP_DTYPES) if self.has_keep else [])
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in fields)

    def shares(self):
        """Share of each status over all fragments, by name."""
        n = max(1, len(self.status))
        return {name: float(np.count_nonzero(self.status == st)) / n for st, name in STATUS_NAMES.items()}

    def take(self, idx):
        """The certificate of spectra idx, in that order (as BatchOutcome.take)."""
        from .pipeline_device import _segments

        idx = np.asarray(idx, dtype=np.int64)
        src, off = _segments(self.frag_off, idx)
        kw = {k: getattr(self, k)[src] for k in self.FRAGMENT_FIELDS}
        if self.has_keep:
            kw.update({k: getattr(self, k)[src] for k in self.KEEP_FRAGMENT_FIELDS}, spec_free=self.spec_free[idx])
        return AlignOutcome(frag_off=off, **kw)

    @classmethod
    def concat(cls, outcomes):
        """Several certificates' spectra one after the other (as BatchOutcome.concat)."""
        outcomes = list(outcomes)
        if not outcomes:
            raise ValueError("AlignOutcome.concat: nothing to concatenate")
        base = np.concatenate([[0], np.cumsum([int(o.frag_off[-1]) for o in outcomes])]).astype(np.int64)
        off = np.concatenate([o.frag_off[:-1] + b for o, b in zip(outcomes, base)] + [base[-1:]])
        fields = cls.FRAGMENT_FIELDS
        if outcomes[0].has_keep:
            if not all(o.has_keep for o in outcomes):
                raise ValueError("AlignOutcome.concat: keep mode in some outcomes only")
            fields = fields + cls.KEEP_FRAGMENT_FIELDS + ("spec_free",)
        elif any(o.has_keep for o in outcomes):
            raise ValueError("AlignOutcome.concat: keep mode in some outcomes only")
        return cls(frag_off=off, **{k: np.concatenate([getattr(o, k) for o in outcomes]) for k in fields})


LP_DROP, LP_KEEP, LP_SOLVE = 0, 1, 2


def lp_decisions(al):
    """filter_with_lp's three-way answer per fragment (u8): LP_DROP (0,
    alignable == 0: every outcome of the solve removes the fragment), LP_KEEP
    (1, keep == 1: a solve run to optimality keeps it) and LP_SOLVE (2: the
    solver decides).  Without keep mode nothing is LP_KEEP."""
    out = np.where(al.alignable == 0, LP_DROP, LP_SOLVE).astype(np.uint8)
    if al.has_keep:
        out[(al.keep != 0) & (al.alignable != 0)] = LP_KEEP
    return out


def _clamp(x):
    return max(-_CLAMP, min(_CLAMP, x))


def quantise(su, obs, tolerance, precision):
    """(target, W) of a fragment: round(su / precision) (ties to even) and
    ceil(tolerance * obs / precision); a negative W is -1 (nothing fits)."""
    t = _clamp(round(su / precision)) if math.isfinite(su / precision) else (_CLAMP if su > 0 else -_CLAMP)
    q = tolerance * obs / precision
    w = _clamp(math.ceil(q)) if math.isfinite(q) else (_CLAMP if q > 0 else -_CLAMP)
    return t, (w if w >= 0 else -1)


def inner_window(obs, tolerance, precision):
    """W_in of a fragment (keep mode): floor(q) - 1 for a finite q = tolerance *
    obs / precision >= 1 (clamped like W), else -1: nothing fits inside."""
    q = tolerance * obs / precision
    return _clamp(math.floor(q) - 1) if math.isfinite(q) and q >= 1 else -1


def lp_row_caps(dp_table, outcome):
    """row_cap i32 [254 * n_rows], row_cap[L * n_rows + r] = int(np.ceil(rate_r
    * L)) for L in [0, 253]: the per-row caps of linear_program.py:190-196 as
    keep mode's input.  rate_r is the modification_rate of the row of
    dp_table.masses whose names contain row r's first name (outcome.row_names,
    the name the program's y variable carries); a first name no row holds has
    no constraint (cap L).  ValueError if a name occurs in two rows: the
    program would then hold two constraints on one variable, which one integer
    per row does not model."""
    owner = {}
    for m in dp_table.masses:
        for name in m.names:
            if name in owner:
                raise ValueError(f"lp_row_caps: name {name!r} occurs in two rows of the table")
            owner[name] = float(m.modification_rate)
    n_rows = len(outcome.row_names)
    lengths = np.arange(ALIGN_MAX_LEN + 1, dtype=np.float64)
    out = np.empty((ALIGN_MAX_LEN + 1, n_rows), np.int32)
    for r, name in enumerate(outcome.row_names):
        # (one f64 product and ceil per entry: the same IEEE operations as the reference's scalar ones)
        out[:, r] = np.ceil(np.float64(owner[name]) * lengths).astype(np.int32) if name in owner else \
            lengths.astype(np.int32)
    return out.reshape(-1)


def _rows_of(m0, m1, n_rows):
    return [r for r in range(1, n_rows) if ((m0 >> r) & 1 if r < 64 else (m1 >> (r - 64)) & 1)]


def position_sets(skeleton, alpha, n_rows):
    """A_i per position as row lists: P_i & alpha where P_i != 0, else alpha; row 0 excluded."""
    a0, a1 = int(alpha[0]), int(alpha[1])
    out = []
    for p in skeleton:
        p0, p1 = int(p[0]), int(p[1])
        out.append(_rows_of(p0 & a0, p1 & a1, n_rows) if (p0 | p1) else _rows_of(a0, a1, n_rows))
    return out


def lp_caps(dp_table, outcome):
    """(row_mod u8 [n_rows], mod_cap i32 [S]): the inputs of the universal cap
    (linear_program.py:180-188).  row_mod[r] = 1 iff the row's first name (the
    one the program's y variables carry, outcome.row_names) is not in
    UNMODIFIED_BASES; row 0 is 0.  mod_cap[g] = int(np.ceil(modification_rate *
    L)) in f64 as the reference computes it."""
    from .masses import UNMODIFIED_BASES

    row_mod = np.array([0] + [int(n not in UNMODIFIED_BASES) for n in outcome.row_names[1:]], dtype=np.uint8)
    rate = float(dp_table.seq.modification_rate)
    # (one f64 product and ceil per spectrum: the same IEEE operations as the reference's scalar ones)
    mod_cap = np.ceil(np.float64(rate) * np.asarray(outcome.seq_len, dtype=np.float64)).astype(np.int32)
    return row_mod, mod_cap


def _position_costs(sets, row_mass, row_mod=None):
    """Per position (distinct masses ascending, the fewest modified rows that
    reach each: 0 / 1, forced: every row of A_i is modified).  Without row_mod
    (no cap) no row counts as modified: every cost is 0 and nothing is forced."""
    out = []
    for rows in sets:
        if row_mod is None:
            masses = np.array(sorted({int(row_mass[r]) for r in rows}), dtype=np.int64)
            out.append((masses, np.zeros(len(masses), np.int64), 0))
            continue
        best = {}
        for r in rows:
            m = int(row_mass[r])
            best[m] = min(best.get(m, 1), int(row_mod[r] != 0))
        masses = np.array(sorted(best), dtype=np.int64)
        forced = int(all(best.values()))
        out.append((masses, np.array([best[int(m)] for m in masses], dtype=np.int64) - forced, forced))
    return out


def _extend_capped(sums, exc, masses, cost, E):
    """S_E extended by one position: (s + w, e + cost) for every mass, equal
    sums keep the smallest excess, entries above E leave."""
    if len(masses) == 1:  # one mass costs nothing (forced, or an unmodified row has it): only the sums move
        return sums + masses[0], exc
    if not cost.any() and not exc.any():  # nothing paid so far, nothing to pay here (always so without the cap)
        s = np.unique(np.add.outer(sums, masses))
        return s, np.zeros(len(s), np.int64)
    s = np.add.outer(sums, masses).reshape(-1)
    e = np.add.outer(exc, cost).reshape(-1)
    keep = e <= E
    s, e = s[keep], e[keep]
    order = np.lexsort((e, s))
    s, e = s[order], e[order]
    head = np.concatenate([[True], s[1:] != s[:-1]]) if len(s) else np.zeros(0, bool)
    return s[head], e[head]


def _align_spectrum(L, pc, E, code, su, obs, mn, mx, tolerance, precision, capacity, split=False, inner=False):
    """The certificate of one modelled spectrum: pc = _position_costs(...), E
    the budget beyond the forced positions (without the cap: costs all 0 and
    E = L, so nothing ever leaves a list).  The lists are S_E(l, r) with the
    smallest excess per sum; LO and HI stay the uncapped sums of minima and
    maxima (a conservative cut only).
    inner=True (keep mode, a row-free spectrum): a fourth result, per fragment
    the smallest interval (closed, or with split and for a base-OPEN fragment
    split-closed) whose list holds a sum within W_in of the target, else
    NO_INTERVAL."""
    n = len(code)
    kept = np.full(n, 1 << 20, np.int64)
    w_in = np.array([inner_window(float(o), tolerance, precision) if inner else -1 for o in obs], dtype=np.int64).reshape(n)
    status = np.zeros(n, np.uint8)
    n_fit = np.zeros(n, np.int64)
    first = np.full(n, 1 << 20, np.int64)
    opened = np.zeros(n, bool)
    cls = (code.astype(np.int64) >> 2) & 3  # 0 internal, 1 START, 2 END, 3 START_END
    skipped = ((cls == 1) | (cls == 2)) & ((mn < 0) | (mn >= L) | (mx < 0) | (mx >= L))
    tw = [quantise(float(s), float(o), tolerance, precision) for s, o in zip(su, obs)]
    t = np.array([x[0] for x in tw], dtype=np.int64).reshape(n)
    w = np.array([x[1] for x in tw], dtype=np.int64).reshape(n)
    live = ~skipped & (w >= 0)
    flo, fhi = t - w, t + w
    lo_end = np.minimum(mn, mx)
    zero = np.zeros(1, np.int64)

    def fwd(l, r):
        return internal | ((cls == 1) & (r >= lo_end) & (r <= mx)) | ((cls == 3) & (r == L - 1))

    def bwd(l, r):
        return (cls == 2) & (l >= lo_end) & (l <= mn)

    def match(ok, l, r, LO, HI, sums):
        """Fragments `ok` against interval (l, r): sums None for an open one."""
        cand = np.flatnonzero(ok & live & (fhi >= LO) & (flo <= HI))
        if not len(cand):
            return
        if sums is None:
            opened[cand] = True
            return
        at = np.searchsorted(sums, flo[cand], side="left")
        fit = cand[(at < len(sums)) & (sums[np.minimum(at, len(sums) - 1)] <= fhi[cand])]
        n_fit[fit] += 1
        first[fit] = np.minimum(first[fit], l << 8 | r)
        cand = cand[w_in[cand] >= 0]
        if len(cand):
            at = np.searchsorted(sums, t[cand] - w_in[cand], side="left")
            fit = cand[(at < len(sums)) & (sums[np.minimum(at, len(sums) - 1)] <= t[cand] + w_in[cand])]
            kept[fit] = np.minimum(kept[fit], l << 8 | r)

    def sweep(start, step, ok_of):
        sums, exc, LO, HI = zero, zero, 0, 0
        last = int(fhi[live].max()) if live.any() else -1
        p = start
        while 0 <= p < L:
            m, c, _ = pc[p]
            LO, HI = LO + int(m[0]), HI + int(m[-1])
            if LO > last:
                break
            if sums is not None:
                sums, exc = _extend_capped(sums, exc, m, c, E)
                if len(sums) > capacity:
                    sums = None
            l, r = (start, p) if step > 0 else (p, start)
            match(ok_of(l, r), l, r, LO, HI, sums)
            p += step

    internal = cls == 0
    if internal.any() or (L == 0 and (cls == 3).any()):
        match(internal | ((cls == 3) & (L == 0)), 0xFF, 0xFF, 0, 0, zero)
    for l in range(L if internal.any() else min(L, 1)):
        sweep(l, 1, fwd if l == 0 else (lambda l, r: internal))
    if (cls == 2).any():
        sweep(L - 1, -1, bwd)

    status[:] = np.where(skipped, ALIGN_SKIPPED, np.where(n_fit > 0, ALIGN_FIT, np.where(opened, ALIGN_OPEN, ALIGN_NONE)))
    todo = status == ALIGN_OPEN
    if not split or not todo.any():
        return status, n_fit, np.where(n_fit > 0, first, NO_INTERVAL), np.where(kept < 1 << 20, kept, NO_INTERVAL)

    # the split: the base-OPEN fragments again, over the open intervals only
    opened[:] = False
    last = int(fhi[todo].max())

    def split_sweep(start, step, ok_of):
        a, ea, lo_a, hi_a = zero, zero, 0, 0  # S_E(start, m*), the last closed interval of the sweep
        p = start
        while 0 <= p < L:
            m, c, _ = pc[p]
            if lo_a + int(m[0]) > last:
                return
            nxt, enxt = _extend_capped(a, ea, m, c, E)
            if len(nxt) > capacity:
                break
            a, ea, lo_a, hi_a = nxt, enxt, lo_a + int(m[0]), hi_a + int(m[-1])
            p += step
        else:
            return  # every interval of the sweep is closed
        halves = p != start  # (else not even one position is closed: nothing splits)
        b, eb, LO, HI = zero, zero, lo_a, hi_a  # S_E(m* + 1, r), its excess against its own forced positions
        while 0 <= p < L:
            m, c, _ = pc[p]
            LO, HI = LO + int(m[0]), HI + int(m[-1])
            if LO > last:
                break
            if halves and b is not None:
                b, eb = _extend_capped(b, eb, m, c, E)
                if len(b) > capacity:
                    b = None  # undecided from here on
            l, r = (start, p) if step > 0 else (p, start)
            cand = np.flatnonzero(ok_of(l, r) & todo & (fhi >= LO) & (flo <= HI))
            if not halves or b is None:
                opened[cand] = True
            elif len(cand):
                # a of excess v takes any b of excess <= E - v
                pairs = [(a[ea == v], b[eb <= E - v]) for v in (np.unique(ea) if ea.any() else (0,))]

                def pair_in(lo_j, hi_j):  # some a + b in [lo_j, hi_j] within the budget
                    for aa, bb in pairs:
                        if not len(bb):
                            continue
                        x = aa[(aa >= lo_j - bb[-1]) & (aa <= hi_j - bb[0])]
                        at = np.searchsorted(bb, lo_j - x, side="left")
                        if ((at < len(bb)) & (bb[np.minimum(at, len(bb) - 1)] <= hi_j - x)).any():
                            return True
                    return False

                for j in cand:
                    if pair_in(flo[j], fhi[j]):
                        n_fit[j] += 1
                        first[j] = min(first[j], l << 8 | r)
                        if w_in[j] >= 0 and pair_in(t[j] - w_in[j], t[j] + w_in[j]):
                            kept[j] = min(kept[j], l << 8 | r)
            p += step

    for l in range(L if (internal & todo).any() else min(L, 1)):
        split_sweep(l, 1, fwd if l == 0 else (lambda l, r: internal))
    if ((cls == 2) & todo).any():
        split_sweep(L - 1, -1, bwd)
    status[todo] = np.where(n_fit[todo] > 0, ALIGN_FIT, np.where(opened[todo], ALIGN_OPEN, ALIGN_NONE))
    return status, n_fit, np.where(n_fit > 0, first, NO_INTERVAL), np.where(kept < 1 << 20, kept, NO_INTERVAL)


def align_host(outcome, tolerance, precision, capacity=ALIGN_CAPACITY, split=False, caps=None, keep=None):
    """The certificate of every fragment of `outcome` (a BatchOutcome), by the
    definition: per left end the achievable sums of the growing interval as a
    sorted array, open once they number more than `capacity`.
    split=True: the fragments that are OPEN by that are decided again over
    the open intervals (include/sst.h, sst_align_split_device): an open
    interval whose greedy first half and the rest are both closed holds a
    fitting sum iff some a + b of the halves' sums fits; where the rest is
    open too the interval is undecided, as every open one is without split.
    The other fragments keep their outputs.
    caps=(row_mod, mod_cap) (lp_caps): the universal modification cap holds
    too (include/sst.h, sst_align_windows_caps_device).  A spectrum with more
    forced positions (every row of A_i modified) than mod_cap[g] is
    INFEASIBLE; else the lists are S_E(l, r), the sums some choice reaches with
    at most E = mod_cap[g] - forced more modified rows than the interval's
    forced positions, closed iff |S_E| <= capacity, and the split matches a + b
    only where the two excesses together stay within E.
    keep=row_cap (lp_row_caps; requires caps): keep mode (include/sst.h,
    sst_align_windows_keep_device).  The four outputs above are unchanged; the
    outcome also carries spec_free (the spectrum is modelled, feasible and
    every row r of its alphabet is free: row_cap[L * n_rows + r] >= n_r, the
    positions whose set holds r, or r is modified and row_cap >= mod_cap[g]),
    and per fragment keep / keep_first: in a row-free spectrum, some closed
    (with split, for a base-OPEN fragment: split-closed) admissible interval's
    list holds a sum within W_in = floor(tolerance * obs / precision) - 1 of
    the target (inner_window).  The program then has a feasible point with an
    error <= tolerance * obs - precision / 2: a solve run to optimality keeps
    the fragment (one stopped by its time limit may not)."""
    row_mod = None
    if caps is not None:
        row_mod = np.ascontiguousarray(caps[0], dtype=np.uint8)
        mod_cap = np.ascontiguousarray(caps[1], dtype=np.int32)
        if len(row_mod) != len(outcome.row_mass) or len(mod_cap) != len(outcome):
            raise ValueError("align_host: caps do not match the outcome's rows / spectra")
    S, nf = len(outcome), int(outcome.frag_off[-1])
    status = np.zeros(nf, np.uint8)
    n_fit = np.zeros(nf, np.uint32)
    first = np.full(nf, NO_INTERVAL, np.uint16)
    n_rows = len(outcome.row_mass)
    row_cap = None
    if keep is not None:
        if caps is None:
            raise ValueError("align_host: keep mode requires caps")
        row_cap = np.ascontiguousarray(keep, dtype=np.int32).reshape(-1)
        if len(row_cap) != (ALIGN_MAX_LEN + 1) * n_rows:
            raise ValueError("align_host: keep is not a row_cap table of 254 lengths by the outcome's rows")
        row_cap = row_cap.reshape(ALIGN_MAX_LEN + 1, n_rows)
    kept = np.zeros(nf, np.uint8)
    keep_first = np.full(nf, NO_INTERVAL, np.uint16)
    spec_free = np.zeros(S, np.uint8)
    if n_rows and (int(outcome.row_mass.min()) < 0 or int(outcome.row_mass.max()) >= (1 << 32) // ALIGN_MAX_LEN):
        raise ValueError("align_host: a row mass outside [0, 2^32 / 253)")
    for g in range(S):
        f = slice(int(outcome.frag_off[g]), int(outcome.frag_off[g + 1]))
        if f.start == f.stop:
            continue
        L = int(outcome.seq_len[g])
        p = slice(int(outcome.pos_off[g]), int(outcome.pos_off[g + 1]))
        if L < 0 or L > ALIGN_MAX_LEN or p.stop - p.start != L:
            status[f] = ALIGN_SKIPPED
            continue
        sets = position_sets(outcome.skeleton[p], outcome.alpha[g], n_rows)
        if any(not rows for rows in sets):
            status[f] = ALIGN_INFEASIBLE
            continue
        pc = _position_costs(sets, outcome.row_mass, row_mod)
        forced = sum(x[2] for x in pc)
        cap = L if caps is None else int(mod_cap[g])  # (no cap: nothing is forced and E = L)
        if forced > cap:
            status[f] = ALIGN_INFEASIBLE
            continue
        if row_cap is not None:
            n_r = {}
            for rows in sets:
                for r in rows:
                    n_r[r] = n_r.get(r, 0) + 1
            spec_free[g] = all(int(row_cap[L, r]) >= n_r.get(r, 0) or
                               (row_mod[r] != 0 and int(row_cap[L, r]) >= int(mod_cap[g]))
                               for r in _rows_of(int(outcome.alpha[g][0]), int(outcome.alpha[g][1]), n_rows))
        st, nn, ff, kf = _align_spectrum(L, pc, min(cap - forced, L), outcome.frag_code[f], outcome.frag_su[f],
                                         outcome.frag_obs[f], outcome.frag_min_end[f].astype(np.int64),
                                         outcome.frag_max_end[f].astype(np.int64), tolerance, precision, int(capacity),
                                         split, inner=bool(spec_free[g]))
        status[f], n_fit[f], first[f], keep_first[f] = st, nn, ff, kf
        kept[f] = kf != NO_INTERVAL
    alignable = ((status != ALIGN_NONE) & (status != ALIGN_INFEASIBLE)).astype(np.uint8)
    extra = {} if row_cap is None else {"keep": kept, "keep_first": keep_first, "spec_free": spec_free}
    return AlignOutcome(frag_off=outcome.frag_off.copy(), status=status, alignable=alignable, n_fit=n_fit, first=first,
                        **extra)


def align_device(dp_table, outcome, split=False, caps=False, keep=False):
    """The certificate of every fragment of `outcome` on dp_table's device
    (sst_align_windows_device, capacity sst_align_capacity()): one upload per
    input array, one launch, one download per output array.  `outcome` must be
    on dp_table's rows.  split=True: sst_align_split_device follows on the
    same stream before the one download (align_host's split=True).
    caps=True: the universal modification cap holds too (lp_caps(dp_table,
    outcome) uploaded, sst_align_windows_caps_device and, with split,
    sst_align_split_caps_device: align_host's caps=lp_caps(...)); a (row_mod,
    mod_cap) pair is taken as it is.
    keep=True (requires caps): keep mode (lp_row_caps(dp_table, outcome)
    uploaded, sst_align_windows_keep_device and, with split,
    sst_align_split_keep_device: align_host's keep=lp_row_caps(...)); a
    row_cap array is taken as it is.  The outcome carries keep, keep_first and
    spec_free."""
    from .pipeline_device import _one_stream

    masses = [int(m.mass) for m in dp_table.masses]
    if masses != [int(x) for x in outcome.row_mass]:
        raise ValueError("align_device: the outcome is not on this table's rows")
    if caps is True:
        caps = lp_caps(dp_table, outcome)
    elif caps is False:
        caps = None
    if caps is not None and (len(caps[0]) != len(masses) or len(caps[1]) != len(outcome)):
        raise ValueError("align_device: caps do not match the table's rows / the outcome's spectra")
    if keep is True:
        keep = lp_row_caps(dp_table, outcome)
    elif keep is False:
        keep = None
    if keep is not None:
        if caps is None:
            raise ValueError("align_device: keep mode requires caps")
        keep = np.ascontiguousarray(keep, dtype=np.int32).reshape(-1)
        if len(keep) != (ALIGN_MAX_LEN + 1) * len(masses):
            raise ValueError("align_device: keep is not a row_cap table of 254 lengths by the table's rows")
    return _one_stream(_align_device)(dp_table, outcome, split, caps, keep)


# (the certificate, then its split) by "under the cap" / "keep"
_ENTRY_POINTS = {False: ("sst_align_windows_device", "sst_align_split_device"),
                 True: ("sst_align_windows_caps_device", "sst_align_split_caps_device"),
                 "keep": ("sst_align_windows_keep_device", "sst_align_split_keep_device")}


def _align_device(dp_table, o, split=False, caps=None, row_cap=None):
    import torch

    dt = dp_table.device_table
    eng = dt.engine
    dev = torch.device("cuda", eng.device)
    S, nf = len(o), int(o.frag_off[-1])
    if nf == 0:
        z = np.zeros(0)
        more = {} if row_cap is None else {"keep": z, "keep_first": z, "spec_free": np.zeros(S)}
        return AlignOutcome(frag_off=o.frag_off.copy(), status=z, alignable=z, n_fit=z, first=z, **more)

    def up(x, dtype, n=1):  # (never an empty allocation: the entry point refuses NULL)
        x = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
        return torch.as_tensor(x if len(x) else np.zeros(n, dtype), device=dev)

    keep = [up(o.seq_len, np.int32), up(o.pos_off, np.int64), up(o.skeleton.view(np.int64), np.int64, 2),
            up(o.alpha.view(np.int64), np.int64, 2), up(o.frag_off, np.int64), up(o.frag_code, np.uint8),
            up(o.frag_su, np.float64), up(o.frag_obs, np.float64), up(o.frag_min_end, np.int32),
            up(o.frag_max_end, np.int32)]
    status = torch.empty(nf, dtype=torch.uint8, device=dev)
    alignable = torch.empty(nf, dtype=torch.uint8, device=dev)
    n_fit = torch.empty(nf, dtype=torch.int32, device=dev)
    first = torch.empty(nf, dtype=torch.int16, device=dev)
    a = _native.AlignArgs()
    a.n_spec = S
    (a.seq_len, a.pos_off, a.skeleton, a.alpha, a.frag_off, a.frag_code, a.frag_su, a.frag_obs, a.frag_min_end,
     a.frag_max_end) = (x.data_ptr() for x in keep)
    a.tol, a.prec = float(dp_table.tolerance), float(dp_table.precision)
    a.status, a.alignable, a.n_fit, a.first = (x.data_ptr() for x in (status, alignable, n_fit, first))
    extra = ()
    if caps is not None:
        keep += [up(caps[0], np.uint8), up(caps[1], np.int32)]
        extra = (ctypes.byref(_native.AlignCaps(keep[-2].data_ptr(), keep[-1].data_ptr())),)
    if row_cap is not None:
        keep.append(up(row_cap, np.int32))
        kept = torch.empty(nf, dtype=torch.uint8, device=dev)
        keep_first = torch.empty(nf, dtype=torch.int16, device=dev)
        spec_free = torch.empty(S, dtype=torch.uint8, device=dev)
        extra += (ctypes.byref(_native.AlignKeep(keep[-1].data_ptr(), kept.data_ptr(), keep_first.data_ptr(),
                                                 spec_free.data_ptr())),)
    torch.cuda.synchronize(dev)
    for name in _ENTRY_POINTS["keep" if row_cap is not None else caps is not None][:2 if split else 1]:
        eng.check(getattr(eng._lib, name)(dt.handle, ctypes.byref(a), *extra), name)
    eng.synchronize()
    more = {} if row_cap is None else {"keep": kept.cpu().numpy(), "keep_first": keep_first.cpu().numpy().view(np.uint16),
                                       "spec_free": spec_free.cpu().numpy()}
    return AlignOutcome(frag_off=o.frag_off.copy(), status=status.cpu().numpy(), alignable=alignable.cpu().numpy(),
                        n_fit=n_fit.cpu().numpy().view(np.uint32), first=first.cpu().numpy().view(np.uint16), **more)
