"""The length program: select_sequence_length_with_lp by exact enumeration
(include/sst.h, sst_length_program_device; DESIGN "The length program").

SkeletonBuilder.build_skeleton chooses the sequence length with a solver first
(skeleton_building.py:198-289): for every candidate length c in [lower, upper]
it combines the two skeletons at c, builds one LinearProgramInstance over the
terminal fragments (determine_lp_score) and reads the optimal objective value;
the smallest value among the lengths validate_sequence_length_by_mass accepts
wins, and only a result below 1 hands the choice to the Jaccard selection
(:44-57).  For a fixed y that program decomposes as the final program does, so
its optimum is a minimum over y of a sum of per-fragment minima, enumerated
here in 2^-16 fixed point.

LengthCases holds the dense inputs as host arrays (length_cases gathers them
from the device stages' arrays), length_program_host is the definition in plain
Python and numpy (_set_x simulated literally on a list per fragment and
candidate, every y enumerated), length_program_device the kernel
(csrc/sst_length_program.hip) over whole cases, and length_decisions the proven
answer per spectrum: a length (LENGTH_TAKE), "returns -1, the Jaccard length
decides" (LENGTH_JACCARD), "predict returns its default" (LENGTH_NONE) or "the
solver decides" (LENGTH_SOLVE).  The claim is for solves run to optimality; no
solver runs in this project.
"""
import ctypes
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from . import _native
from ._native import (LEN_INFEASIBLE, LEN_INVALID, LEN_NOT_FREE, LEN_NOT_MODELLED, LEN_RAISES, LEN_SOLVED,
                      LEN_TOO_LARGE)
from .alignment import ALIGN_MAX_LEN, _rows_of, lp_caps, lp_row_caps, position_sets
from .final_program import FINAL_DEFAULT_COMBOS, FINAL_MAX_USED, FIX, _check_max_combos

LENGTH_NONE, LENGTH_JACCARD, LENGTH_TAKE, LENGTH_SOLVE = 0, 1, 2, 3
DECISION_NAMES = {LENGTH_NONE: "NONE", LENGTH_JACCARD: "JACCARD", LENGTH_TAKE: "TAKE", LENGTH_SOLVE: "SOLVE"}
STATUS_NAMES = {LEN_INVALID: "INVALID", LEN_RAISES: "RAISES", LEN_NOT_MODELLED: "NOT_MODELLED",
                LEN_INFEASIBLE: "INFEASIBLE", LEN_NOT_FREE: "NOT_FREE", LEN_TOO_LARGE: "TOO_LARGE",
                LEN_SOLVED: "SOLVED"}
SHAPE_EMPTY, SHAPE_PREFIX, SHAPE_SUFFIX, SHAPE_WHOLE = 0, 1, 2, 3
RULE_RAISES, RULE_NOT_MODELLED = "RAISES", "NOT_MODELLED"
_HOST_BLOCK = 1 << 14  # assignments of a block (length_program_host)


def _segments(off, idx):
    from .pipeline_device import _segments as seg

    return seg(off, idx)


def _offsets(outcomes, name):
    base = np.concatenate([[0], np.cumsum([int(getattr(o, name)[-1]) for o in outcomes])]).astype(np.int64)
    return np.concatenate([getattr(o, name)[:-1] + b for o, b in zip(outcomes, base)] + [base[-1:]])


@dataclass
class LengthCases:
    """What build_skeleton holds when it calls select_sequence_length_with_lp
    (skeleton_building.py:45), for every spectrum of a batch, as host arrays:
    the walk's max_len M, the START skeleton and the REVERSED END skeleton (M
    position masks each over the table's rows: spectrum g's START position i at
    skel_off[g] + i, its reversed END position i at skel_off[g] + M + i), the
    skeleton alphabet, both length bounds and whether they raised, the
    sequence's SU mass, and the terminal fragments (the START walk's kept rows,
    then the END walk's kept rows whose index no START row has) with their side
    bits and the walk's raw min_end / max_end."""
    max_len: np.ndarray       # [S] i32
    skel_off: np.ndarray      # [S + 1] i64, in positions (2 M per spectrum)
    skeleton: np.ndarray      # [skel_off[S], 2] u64
    alpha: np.ndarray         # [S, 2] u64
    lower: np.ndarray         # [S] i64
    upper: np.ndarray         # [S] i64
    lb_status: np.ndarray     # [S] i32, 0: the bounds are valid
    su_mass: np.ndarray       # [S] f64
    frag_off: np.ndarray      # [S + 1] i64
    frag_code: np.ndarray     # u8: breakage code | START << 2 | END << 3 | singleton << 4
    frag_su: np.ndarray       # f64
    frag_min_end: np.ndarray  # i32 raw
    frag_max_end: np.ndarray  # i32 raw
    row_names: list           # nucleoside name per table row ("" for row 0)
    row_mass: np.ndarray      # [rows] i64

    SPECTRUM_FIELDS = ("max_len", "alpha", "lower", "upper", "lb_status", "su_mass")
    FRAGMENT_FIELDS = ("frag_code", "frag_su", "frag_min_end", "frag_max_end")
    _DTYPES = {"max_len": np.int32, "skel_off": np.int64, "skeleton": np.uint64, "alpha": np.uint64, "lower": np.int64,
               "upper": np.int64, "lb_status": np.int32, "su_mass": np.float64, "frag_off": np.int64,
               "frag_code": np.uint8, "frag_su": np.float64, "frag_min_end": np.int32, "frag_max_end": np.int32,
               "row_mass": np.int64}

    def __post_init__(self):
        for k, dt in self._DTYPES.items():
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))
        self.alpha = self.alpha.reshape(-1, 2)
        self.skeleton = self.skeleton.reshape(-1, 2)
        self.row_names = list(self.row_names)
        S = len(self.max_len)
        if any(len(getattr(self, k)) != S for k in self.SPECTRUM_FIELDS) or \
                len(self.skel_off) != S + 1 or len(self.frag_off) != S + 1:
            raise ValueError("LengthCases: per-spectrum arrays of different lengths")
        if int(self.skel_off[-1]) != len(self.skeleton) or \
                not np.array_equal(np.diff(self.skel_off), 2 * self.max_len.astype(np.int64)) or \
                any(len(getattr(self, k)) != int(self.frag_off[-1]) for k in self.FRAGMENT_FIELDS):
            raise ValueError("LengthCases: dense arrays do not match their offsets")

    def __len__(self):
        return len(self.max_len)

    def candidates(self):
        """(cand_off i64 [S + 1], cand_len i32): spectrum g's candidates are
        lower[g] .. upper[g] in that order, none where its bounds raised."""
        n = np.where(self.lb_status == 0, np.maximum(self.upper - self.lower + 1, 0), 0)
        cand_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        spec = np.repeat(np.arange(len(self)), n)
        c = self.lower[spec] + (np.arange(int(cand_off[-1])) - cand_off[spec])
        if len(c) and (int(c.min()) < -(1 << 31) or int(c.max()) >= 1 << 31):
            raise ValueError("LengthCases: a candidate length outside int32")
        return cand_off, c.astype(np.int32)

    def take(self, idx):
        """The cases of spectra idx, in that order (as BatchOutcome.take)."""
        idx = np.asarray(idx, dtype=np.int64)
        ssrc, soff = _segments(self.skel_off, idx)
        fsrc, foff = _segments(self.frag_off, idx)
        return LengthCases(skel_off=soff, skeleton=self.skeleton[ssrc], frag_off=foff, row_names=self.row_names,
                           row_mass=self.row_mass, **{k: getattr(self, k)[idx] for k in self.SPECTRUM_FIELDS},
                           **{k: getattr(self, k)[fsrc] for k in self.FRAGMENT_FIELDS})

    @classmethod
    def concat(cls, cases):
        """Several cases' spectra one after the other (as BatchOutcome.concat)."""
        cases = list(cases)
        if not cases:
            raise ValueError("LengthCases.concat: nothing to concatenate")
        first = cases[0]
        if any(o.row_names != first.row_names or not np.array_equal(o.row_mass, first.row_mass) for o in cases[1:]):
            raise ValueError("LengthCases.concat: cases of different tables")
        fields = cls.SPECTRUM_FIELDS + cls.FRAGMENT_FIELDS + ("skeleton",)
        return cls(skel_off=_offsets(cases, "skel_off"), frag_off=_offsets(cases, "frag_off"),
                   row_names=first.row_names, row_mass=first.row_mass,
                   **{k: np.concatenate([getattr(o, k) for o in cases]) for k in fields})


@dataclass
class LengthOutcome:
    """The length program's result per candidate (candidate k of spectrum g at
    cand_off[g] + k, its length cand_len), and per spectrum what
    length_decisions reads beside it."""
    cand_off: np.ndarray   # [S + 1] i64
    cand_len: np.ndarray   # i32 per candidate
    status: np.ndarray     # u8 LEN_*
    combos: np.ndarray     # u64 prod |A_i|, saturating
    n_feas: np.ndarray     # u64 feasible y (0 unless SOLVED)
    best: np.ndarray       # u64 min obj (0 unless SOLVED)
    max_len: np.ndarray    # [S] i32
    lower: np.ndarray      # [S] i64
    upper: np.ndarray      # [S] i64
    lb_status: np.ndarray  # [S] i32
    n_frag: np.ndarray     # [S] i64 terminal fragments
    undecided: np.ndarray  # [S] u8: nothing was computed for the spectrum (run_batch: it went to the host mirror)

    SPECTRUM_FIELDS = ("max_len", "lower", "upper", "lb_status", "n_frag", "undecided")
    CANDIDATE_FIELDS = ("cand_len", "status", "combos", "n_feas", "best")
    _DTYPES = {"cand_off": np.int64, "cand_len": np.int32, "status": np.uint8, "combos": np.uint64,
               "n_feas": np.uint64, "best": np.uint64, "max_len": np.int32, "lower": np.int64, "upper": np.int64,
               "lb_status": np.int32, "n_frag": np.int64, "undecided": np.uint8}

    def __post_init__(self):
        for k, dt in self._DTYPES.items():
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))
        S = len(self.cand_off) - 1
        if S < 0 or any(len(getattr(self, k)) != S for k in self.SPECTRUM_FIELDS) or \
                any(len(getattr(self, k)) != int(self.cand_off[-1]) for k in self.CANDIDATE_FIELDS):
            raise ValueError("LengthOutcome: arrays do not match cand_off")

    def __len__(self):
        return len(self.cand_off) - 1

    def equals(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self._DTYPES)

    def shares(self):
        """Share of each status over all candidates, by name."""
        n = max(1, len(self.status))
        return {name: float(np.count_nonzero(self.status == st)) / n for st, name in STATUS_NAMES.items()}

    def take(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        src, off = _segments(self.cand_off, idx)
        return LengthOutcome(cand_off=off, **{k: getattr(self, k)[idx] for k in self.SPECTRUM_FIELDS},
                             **{k: getattr(self, k)[src] for k in self.CANDIDATE_FIELDS})

    @classmethod
    def concat(cls, outcomes):
        outcomes = list(outcomes)
        if not outcomes:
            raise ValueError("LengthOutcome.concat: nothing to concatenate")
        fields = cls.SPECTRUM_FIELDS + cls.CANDIDATE_FIELDS
        return cls(cand_off=_offsets(outcomes, "cand_off"),
                   **{k: np.concatenate([getattr(o, k) for o in outcomes]) for k in fields})

    @classmethod
    def blank(cls, cases, cand_off, cand_len, status=LEN_NOT_MODELLED):
        """Every candidate with `status` and the outputs of one that is not SOLVED."""
        n = len(cand_len)
        return cls(cand_off=cand_off, cand_len=cand_len, status=np.full(n, status, np.uint8),
                   combos=np.zeros(n, np.uint64), n_feas=np.zeros(n, np.uint64), best=np.zeros(n, np.uint64),
                   max_len=cases.max_len, lower=cases.lower, upper=cases.upper, lb_status=cases.lb_status,
                   n_frag=np.diff(cases.frag_off), undecided=np.zeros(len(cases), np.uint8))

    @classmethod
    def not_computed(cls, S):
        """S spectra nothing was computed for: no candidates, undecided (length_decisions: LENGTH_SOLVE)."""
        z = np.zeros
        return cls(cand_off=z(S + 1, np.int64), cand_len=z(0, np.int32), status=z(0, np.uint8), combos=z(0, np.uint64),
                   n_feas=z(0, np.uint64), best=z(0, np.uint64), max_len=z(S, np.int32), lower=z(S, np.int64),
                   upper=z(S, np.int64), lb_status=z(S, np.int32), n_frag=z(S, np.int64),
                   undecided=np.ones(S, np.uint8))


# ---------------------------------------------------------------------------
# The shape of a terminal fragment at a candidate length
# ---------------------------------------------------------------------------
def setx_pattern(cls, min_end, max_end, n):
    """LinearProgramInstance._set_x (linear_program.py:74-102) for one terminal
    fragment of a program of n positions, after determine_lp_score's
    preprocessing of the walk's raw ends (skeleton_building.py:267-276),
    simulated literally on a list: per position 1 / 0 (fixed) or None (free);
    None where an index raises.  cls: the side bits (1 START, 2 END, 3 both)."""
    x = [None] * n
    try:
        if cls == 3:
            for i in range(n):
                x[i] = 1
        elif cls == 1:
            mn, mx = min_end - 1, max_end - 1
            for i in range(mn + 1):
                x[i] = 1
            for i in range(mx + 1, n):
                x[i] = 0
        elif cls == 2:
            mn, mx = n - min_end, n - max_end
            for i in range(mx):
                x[i] = 0
            for i in range(mn, n):
                x[i] = 1
    except IndexError:
        return None
    return x


def pattern_runs(x):
    """The contiguous runs of positions (l, r) that agree with the pattern x --
    every fixed 1 inside, every fixed 0 outside -- and None for the empty run,
    in (l, r) order, the empty one last.  Quadratic: for tests and small n."""
    n = len(x)
    out = [(lo, hi) for lo in range(n) for hi in range(lo, n)
           if all(x[i] != 0 for i in range(lo, hi + 1)) and
           all(x[i] != 1 for i in range(n) if i < lo or i > hi)]
    if all(v != 1 for v in x):
        out.append(None)
    return out


def pattern_shape(x):
    """The shape of a pattern, in time linear in its length: (SHAPE_*, lo, hi)
    -- WHOLE (0, 0), EMPTY (0, 0), PREFIX with its ends e in [lo, hi], SUFFIX
    with its starts s in [lo, hi] -- or RULE_NOT_MODELLED where the runs that
    agree with x are no such set."""
    n = len(x)
    ones = [i for i, v in enumerate(x) if v == 1]
    if not ones:
        return (SHAPE_EMPTY, 0, 0) if all(v == 0 for v in x) and n else RULE_NOT_MODELLED
    first, last = ones[0], ones[-1]
    if any(x[i] == 0 for i in range(first, last + 1)):
        return RULE_NOT_MODELLED
    l_lo = first
    while l_lo > 0 and x[l_lo - 1] != 0:
        l_lo -= 1
    r_hi = last
    while r_hi < n - 1 and x[r_hi + 1] != 0:
        r_hi += 1
    if l_lo == first == 0 and last == r_hi == n - 1:
        return SHAPE_WHOLE, 0, 0
    if l_lo == first == 0:
        return SHAPE_PREFIX, last, r_hi
    if last == r_hi == n - 1:
        return SHAPE_SUFFIX, l_lo, first
    return RULE_NOT_MODELLED


def shape_rule(cls, min_end, max_end, n):
    """The closed form of pattern_shape(setx_pattern(...)) (include/sst.h, the
    kernel's rule): RULE_RAISES, RULE_NOT_MODELLED or (SHAPE_*, lo, hi)."""
    if cls == 3:
        return SHAPE_WHOLE, 0, 0
    if cls == 1:
        mn, mx = min_end - 1, max_end - 1
        if mn >= n or mx + 1 < -n:
            return RULE_RAISES
        if mx + 1 <= 0:
            return SHAPE_EMPTY, 0, 0
        if mn < 0:
            return RULE_NOT_MODELLED
        return _whole_if(SHAPE_PREFIX, min(mn, mx), min(mx, n - 1), n)
    if cls == 2:
        mn, mx = n - min_end, n - max_end
        if mx > n or mn < -n:
            return RULE_RAISES
        if mn < 0:
            return SHAPE_WHOLE, 0, 0
        if mn >= n:
            return (SHAPE_EMPTY, 0, 0) if mx == n else RULE_NOT_MODELLED
        return _whole_if(SHAPE_SUFFIX, max(0, min(mx, mn)), mn, n)
    return RULE_NOT_MODELLED


def _whole_if(shape, lo, hi, n):
    """A PREFIX whose only end is n - 1, or a SUFFIX whose only start is 0, is WHOLE: the same interval."""
    if shape == SHAPE_PREFIX and lo == hi == n - 1 or shape == SHAPE_SUFFIX and lo == hi == 0:
        return SHAPE_WHOLE, 0, 0
    return shape, lo, hi


def shape_runs(shape, lo, hi, n):
    """The runs of a shape, as pattern_runs lists them."""
    if shape == SHAPE_WHOLE:
        return [(0, n - 1)]
    if shape == SHAPE_EMPTY:
        return [None]
    if shape == SHAPE_PREFIX:
        return [(0, e) for e in range(lo, hi + 1)]
    return [(s, n - 1) for s in range(lo, hi + 1)]


# ---------------------------------------------------------------------------
# The inputs the caller computes: validate_sequence_length_by_mass, the caps
# ---------------------------------------------------------------------------
def length_valid(cases, precision):
    """validate_sequence_length_by_mass (skeleton_building.py:291-313) per
    candidate (u8), on the slices select_sequence_length_with_lp passes
    (:244-248): the f64 sums in the reference's order, Python floats; a
    position's smallest and largest mass are its lowest and highest row's (the
    table's rows ascend by mass)."""
    from .fragment_classification import MAX_VARIANCE

    cand_off, cand_len = cases.candidates()
    mass = [int(m) * precision for m in cases.row_mass]
    out = np.zeros(len(cand_len), np.uint8)
    for g in range(len(cases)):
        if cand_off[g] == cand_off[g + 1]:
            continue
        M, so = int(cases.max_len[g]), int(cases.skel_off[g])
        union = [(int(p[0]) | int(p[1]) << 64) for p in cases.skeleton[so:so + 2 * M]]
        start, end = union[:M], union[M:]
        su = float(cases.su_mass[g])
        for k in range(int(cand_off[g]), int(cand_off[g + 1])):
            c = int(cand_len[k])
            min_mass = 0
            max_mass = 0
            for s_nucs, e_nucs in zip(start[:c], end[len(end) - c:]):
                u = s_nucs | e_nucs
                if u:
                    min_mass += mass[(u & -u).bit_length() - 1]
                    max_mass += mass[u.bit_length() - 1]
            out[k] = min_mass - MAX_VARIANCE <= su <= max_mass + MAX_VARIANCE
    return out


def length_caps(dp_table, cases):
    """(row_mod u8 [rows], mod_cap i32 per candidate, row_cap i32 [254 * rows]):
    alignment.lp_caps and lp_row_caps, unchanged, at every candidate's length."""
    shim = SimpleNamespace(row_names=cases.row_names, seq_len=cases.candidates()[1])
    row_mod, mod_cap = lp_caps(dp_table, shim)
    return row_mod, mod_cap, lp_row_caps(dp_table, shim)


def _checked_inputs(cases, valid, caps, who):
    cand_off, cand_len = cases.candidates()
    n_rows = len(cases.row_mass)
    valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)
    row_mod = np.ascontiguousarray(caps[0], dtype=np.uint8)
    mod_cap = np.ascontiguousarray(caps[1], dtype=np.int32)
    row_cap = np.ascontiguousarray(caps[2], dtype=np.int32).reshape(-1)
    if len(valid) != len(cand_len) or len(mod_cap) != len(cand_len):
        raise ValueError(f"{who}: valid / mod_cap do not match the candidates")
    if len(row_mod) != n_rows or len(row_cap) != (ALIGN_MAX_LEN + 1) * n_rows:
        raise ValueError(f"{who}: row_mod / row_cap do not match the table's rows")
    if n_rows and (int(cases.row_mass.min()) < 0 or int(cases.row_mass.max()) >= (1 << 32) // ALIGN_MAX_LEN):
        raise ValueError(f"{who}: a row mass outside [0, 2^32 / 253)")
    return cand_off, cand_len, valid, row_mod, mod_cap, row_cap


def combined_skeleton(cases, g, c):
    """combine_skeleton_sequences (skeleton_building.py:494-516) of spectrum g
    at 1 <= c <= M, as [c, 2] u64 masks."""
    M, so = int(cases.max_len[g]), int(cases.skel_off[g])
    s = cases.skeleton[so:so + c]
    e = cases.skeleton[so + M + M - c:so + 2 * M]
    both = s & e
    return np.where((both != 0).any(axis=1)[:, None], both, s | e)


def length_program_host(cases, precision, valid, caps, max_combos=FINAL_DEFAULT_COMBOS):
    """The length program of every candidate of `cases` by the definition
    (include/sst.h, sst_length_program_device): _set_x simulated on a list per
    fragment and candidate, every y enumerated (numpy over blocks of y, int64).
    valid: length_valid's u8 per candidate; caps = (row_mod, mod_cap per
    candidate, row_cap): length_caps'."""
    max_combos = _check_max_combos(max_combos, "length_program_host")
    cand_off, cand_len, valid, row_mod, mod_cap, row_cap = _checked_inputs(cases, valid, caps, "length_program_host")
    n_rows = len(cases.row_mass)
    row_cap = row_cap.reshape(ALIGN_MAX_LEN + 1, n_rows)
    lo = LengthOutcome.blank(cases, cand_off, cand_len)
    with np.errstate(all="ignore"):
        u = np.asarray(cases.frag_su, dtype=np.float64) / np.float64(precision)
        in_model = np.abs(u) < 2.0 ** 32  # (False for NaN and the infinities)
        qfix = np.where(in_model, np.rint(np.where(in_model, u, 0.0) * float(FIX)), 0.0).astype(np.int64)
    cls_all = (cases.frag_code.astype(np.int64) >> 2) & 3
    for g in range(len(cases)):
        f = slice(int(cases.frag_off[g]), int(cases.frag_off[g + 1]))
        M = int(cases.max_len[g])
        cls, mn, mx = cls_all[f].tolist(), cases.frag_min_end[f].tolist(), cases.frag_max_end[f].tolist()
        for k in range(int(cand_off[g]), int(cand_off[g + 1])):
            c = int(cand_len[k])
            if not valid[k]:
                lo.status[k] = LEN_INVALID
                continue
            n = max(c, 0)
            patterns = [setx_pattern(cls[j], mn[j], mx[j], n) for j in range(len(cls))]
            if any(x is None for x in patterns):
                lo.status[k] = LEN_RAISES
                continue
            if c < 1 or c > ALIGN_MAX_LEN or c > M or not patterns or len(patterns) > FINAL_MAX_USED or \
                    not in_model[f].all():
                continue  # NOT_MODELLED
            shapes = [pattern_shape(x) for x in patterns]
            if any(s == RULE_NOT_MODELLED for s in shapes):
                continue
            sets = position_sets(combined_skeleton(cases, g, c), cases.alpha[g], n_rows)
            combos = 1
            for rows in sets:
                combos *= len(rows)
            lo.combos[k] = min(combos, (1 << 64) - 1)
            if combos == 0:
                lo.status[k] = LEN_INFEASIBLE
                continue
            n_r = {}
            for rows in sets:
                for r in rows:
                    n_r[r] = n_r.get(r, 0) + 1
            cap = int(mod_cap[k])
            if not all(int(row_cap[c, r]) >= n_r.get(r, 0) or (row_mod[r] != 0 and int(row_cap[c, r]) >= cap)
                       for r in _rows_of(int(cases.alpha[g][0]), int(cases.alpha[g][1]), n_rows)):
                lo.status[k] = LEN_NOT_FREE
                continue
            if combos > max_combos:
                lo.status[k] = LEN_TOO_LARGE
                continue
            n_feas, best = _enumerate(c, sets, cases.row_mass, row_mod, cap, shapes, qfix[f])
            if n_feas == 0:
                lo.status[k] = LEN_INFEASIBLE
                continue
            lo.status[k], lo.n_feas[k], lo.best[k] = LEN_SOLVED, n_feas, best
    return lo


def _enumerate(L, sets, row_mass, row_mod, mod_cap, shapes, qfix):
    """(n_feas, min obj) over every y of a modelled candidate."""
    radices = [len(rows) for rows in sets]
    combos = 1
    for r in radices:
        combos *= r
    mass = [np.array([int(row_mass[r]) for r in rows], dtype=np.int64) for rows in sets]
    mod = [np.array([int(row_mod[r] != 0) for r in rows], dtype=np.int64) for rows in sets]
    n_feas, best = 0, None
    for start in range(0, combos, _HOST_BLOCK):
        idx = np.arange(start, min(combos, start + _HOST_BLOCK), dtype=np.int64)
        digits = np.zeros((len(idx), L), np.int64)
        rem = idx.copy()
        for p in range(L - 1, -1, -1):  # position 0 most significant
            if radices[p] > 1:
                rem, digits[:, p] = np.divmod(rem, radices[p])
        n_mod = sum((mod[p][digits[:, p]] for p in range(L)), np.zeros(len(idx), np.int64))
        ok = n_mod <= mod_cap
        if not ok.any():
            continue
        w = np.stack([mass[p][digits[ok, p]] for p in range(L)], axis=1)
        P = np.concatenate([np.zeros((len(w), 1), np.int64), np.cumsum(w, axis=1)], axis=1)
        obj = np.zeros(len(P), np.int64)
        for (shape, lo, hi), q in zip(shapes, qfix.tolist()):
            if shape == SHAPE_WHOLE:
                s = P[:, L:L + 1]
            elif shape == SHAPE_EMPTY:
                s = np.zeros((len(P), 1), np.int64)
            elif shape == SHAPE_PREFIX:
                s = P[:, lo + 1:hi + 2]
            else:
                s = P[:, L:L + 1] - P[:, lo:hi + 1]
            obj += np.abs(q - FIX * s).min(axis=1)
        n_feas += len(P)
        b = int(obj.min())
        best = b if best is None or b < best else best
    return n_feas, (0 if best is None else best)


# ---------------------------------------------------------------------------
# The decision per spectrum
# ---------------------------------------------------------------------------
def length_decisions(lo, min_gap_units=0.5):
    """(decision u8 [S], length i32 [S]): what select_sequence_length_with_lp
    provably does with each spectrum.
    LENGTH_NONE: the bounds raised, or a candidate lies above max_len
    (combine_skeleton_sequences raises): predict returns its default.
    LENGTH_JACCARD: it returns -1 -- no candidate, or every candidate INVALID or
    RAISES (+inf never beats best_val) -- so the Jaccard length decides: what
    the pipeline computes today is the reference's path.
    LENGTH_TAKE with length c*: every candidate is INVALID, RAISES or SOLVED,
    one at least is SOLVED, and best(c) >= best(c*) + max(2 n + 1,
    min_gap_units * 65536) for every other SOLVED c, n the terminal fragments:
    each objective is within n units of 2^-16 precision units of the real one,
    so the real optima are ordered the same way (half a precision unit is the
    margin of the DROP / KEEP / TAKE sides).  A tie or a near tie is the
    solver's.  LENGTH_SOLVE: everything else, and every spectrum nothing was
    computed for.  length is -1 unless the decision is LENGTH_TAKE."""
    S = len(lo)
    decision = np.full(S, LENGTH_SOLVE, np.uint8)
    length = np.full(S, -1, np.int32)
    gap_units = int(np.ceil(min_gap_units * FIX))
    for g in range(S):
        if lo.undecided[g]:
            continue
        k = slice(int(lo.cand_off[g]), int(lo.cand_off[g + 1]))
        if lo.lb_status[g] != 0 or (lo.lower[g] <= lo.upper[g] and lo.upper[g] > lo.max_len[g]):
            decision[g] = LENGTH_NONE
            continue
        st = lo.status[k]
        if np.isin(st, (LEN_INVALID, LEN_RAISES)).all():
            decision[g] = LENGTH_JACCARD
            continue
        if not np.isin(st, (LEN_INVALID, LEN_RAISES, LEN_SOLVED)).all():
            continue
        solved = np.flatnonzero(st == LEN_SOLVED)
        best = [int(x) for x in lo.best[k][solved]]
        at = int(np.argmin(best))
        need = max(2 * int(lo.n_frag[g]) + 1, gap_units)
        if all(b >= best[at] + need for i, b in enumerate(best) if i != at):
            decision[g] = LENGTH_TAKE
            length[g] = int(lo.cand_len[k][solved[at]])
    return decision, length


# ---------------------------------------------------------------------------
# The device
# ---------------------------------------------------------------------------
def length_cases(dp_table, rows, sk, ln, su_seq):
    """The LengthCases of a batch from the device stages' arrays (DeviceRows,
    DeviceSkeleton, DeviceLength; su_seq [S] the sequences' SU masses): one
    download per array and a gather in numpy.  pipeline_device.skeleton_frames
    shows the per-spectrum meaning of the same arrays."""
    from .pipeline_device import _row_names

    S = len(sk.max_len)
    M = sk.max_len.astype(np.int64)
    skel_off = np.asarray(sk.skel_off, dtype=np.int64)
    # the END skeleton reversed: position i of spectrum g is the walked position M - 1 - i
    spec = np.repeat(np.arange(S), 2 * M)
    within = np.arange(int(skel_off[-1])) - skel_off[spec]
    src = np.where(within < M[spec], within, 3 * M[spec] - 1 - within) + skel_off[spec]
    skel = sk.skel.cpu().numpy().view(np.uint64).reshape(-1, 2)[:int(skel_off[-1])][src]
    # the terminal fragments: START rows the walk kept, then END rows it kept that are no kept START row
    peak_off = rows.peak_off.cpu().numpy().astype(np.int64)
    cnt = rows.rows.cpu().numpy().astype(np.int64)[:S]
    n_slots = 4 * int(peak_off[S])
    slot_spec = np.repeat(np.arange(S), 4 * np.diff(peak_off[:S + 1]))
    in_rows = np.arange(n_slots) - 4 * peak_off[slot_spec] < cnt[slot_spec]
    alive = rows.alive.cpu().numpy()[:n_slots] != 0
    meta = rows.meta.cpu().numpy()[:n_slots].astype(np.int64)
    kept = sk.kept.cpu().numpy()[:, :n_slots] != 0
    start = in_rows & alive & ((meta >> 2) & 1 == 1) & kept[0]
    end = in_rows & alive & ((meta >> 3) & 1 == 1) & kept[1] & ~start
    slots = np.concatenate([np.flatnonzero(start), np.flatnonzero(end)])
    side = np.concatenate([np.zeros(int(start.sum()), np.int64), np.ones(int(end.sum()), np.int64)])
    order = np.lexsort((slots, side, slot_spec[slots]))
    slots, side = slots[order], side[order]
    frag_off = np.concatenate([[0], np.cumsum(np.bincount(slot_spec[slots], minlength=S))]).astype(np.int64)
    mn = sk.min_end.cpu().numpy()[:, :n_slots]
    mx = sk.max_end.cpu().numpy()[:, :n_slots]
    return LengthCases(max_len=M, skel_off=skel_off, skeleton=skel, alpha=np.asarray(ln.alpha).reshape(-1, 2)[:S],
                       lower=np.asarray(ln.lower)[:S], upper=np.asarray(ln.upper)[:S],
                       lb_status=np.asarray(ln.lb_status)[:S], su_mass=np.asarray(su_seq, dtype=np.float64)[:S],
                       frag_off=frag_off, frag_code=meta[slots] & 0x1f,
                       frag_su=rows.su.cpu().numpy()[:n_slots][slots], frag_min_end=mn[side, slots],
                       frag_max_end=mx[side, slots], row_names=_row_names(dp_table),
                       row_mass=[m.mass for m in dp_table.masses])


def length_program_device(dp_table, cases, max_combos=FINAL_DEFAULT_COMBOS, valid=None, caps=None, times=None):
    """The length program of every candidate of `cases` on dp_table's device
    (sst_length_program_device): one upload per input array, one launch, one
    download per output array.  valid and caps default to length_valid /
    length_caps of the table.  times: a dict that receives the seconds spent in
    length_valid ("valid_s")."""
    from .pipeline_device import _one_stream

    max_combos = _check_max_combos(max_combos, "length_program_device")
    if [int(m.mass) for m in dp_table.masses] != [int(x) for x in cases.row_mass]:
        raise ValueError("length_program_device: the cases are not on this table's rows")
    if valid is None:
        import time

        t0 = time.perf_counter()
        valid = length_valid(cases, dp_table.precision)
        if times is not None:
            times["valid_s"] = time.perf_counter() - t0
    caps = length_caps(dp_table, cases) if caps is None else caps
    inputs = _checked_inputs(cases, valid, caps, "length_program_device")
    return _one_stream(_length_device)(dp_table, cases, inputs, max_combos)


def _length_device(dp_table, cases, inputs, max_combos):
    import torch

    cand_off, cand_len, valid, row_mod, mod_cap, row_cap = inputs
    dt = dp_table.device_table
    eng = dt.engine
    dev = torch.device("cuda", eng.device)
    S, n_cand = len(cases), len(cand_len)
    lo = LengthOutcome.blank(cases, cand_off, cand_len)
    if S == 0 or n_cand == 0:
        return lo

    def up(x, dtype, n=1):  # (never an empty allocation: the entry point refuses NULL)
        x = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
        return torch.as_tensor(x if len(x) else np.zeros(n, dtype), device=dev)

    ins = [up(cases.max_len, np.int32), up(cases.skel_off, np.int64), up(cases.skeleton.view(np.int64), np.int64, 2),
           up(cases.alpha.view(np.int64), np.int64, 2), up(cases.frag_off, np.int64), up(cases.frag_code, np.uint8),
           up(cases.frag_su, np.float64), up(cases.frag_min_end, np.int32), up(cases.frag_max_end, np.int32),
           up(cand_off, np.int64), up(cand_len, np.int32), up(valid, np.uint8), up(mod_cap, np.int32)]
    more = [up(row_mod, np.uint8), up(row_cap, np.int32)]
    outs = [torch.empty(n_cand, dtype=t, device=dev) for t in (torch.uint8, torch.int64, torch.int64, torch.int64)]
    a = _native.LengthProgramArgs()
    a.n_spec, a.n_cand = S, n_cand
    (a.max_len, a.skel_off, a.skeleton, a.alpha, a.frag_off, a.frag_code, a.frag_su, a.frag_min_end, a.frag_max_end,
     a.cand_off, a.cand_len, a.valid, a.mod_cap) = (x.data_ptr() for x in ins)
    a.prec = float(dp_table.precision)
    a.row_mod, a.row_cap = (x.data_ptr() for x in more)
    a.max_combos = int(max_combos)
    a.status, a.combos, a.n_feas, a.best = (x.data_ptr() for x in outs)
    torch.cuda.synchronize(dev)
    eng.check(eng._lib.sst_length_program_device(dt.handle, ctypes.byref(a)), "sst_length_program_device")
    eng.synchronize()
    status, combos, n_feas, best = (x.cpu().numpy() for x in outs)
    lo.status, lo.combos, lo.n_feas, lo.best = (status, combos.view(np.uint64), n_feas.view(np.uint64),
                                                best.view(np.uint64))
    return lo
