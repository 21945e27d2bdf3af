"""The final program by exact enumeration: the optimal sequence of a spectrum
(include/sst.h, sst_final_program_device; DESIGN "The final program").

After filter_with_lp, Predictor.predict builds one LinearProgramInstance over
the fragments that are left and reads the prediction from its solution
(prediction.py:158-166; linear_program.py:164-225 the program, :238-313
evaluate).  For a fixed y (one row per position) that program decomposes: every
fragment independently takes the admissible interval whose sum is nearest to
its mass, so the optimum is a minimum over y of a sum of per-fragment minima.
Where the spectrum is row-free (keep mode's test) and has at most max_combos
assignments, that minimum is enumerated here, in 2^-16 fixed point.

final_host is the definition in numpy, vectorised over y (the mirror for
spectra run_batch routed to the host, and the model the tests hold the kernel
to), final_device the kernel (csrc/sst_final.hip) over a whole outcome.
final_use turns a keep-mode AlignOutcome into the fragments that enter the
program (the KEEP ones) and the spectra that still hold an LP_SOLVE fragment:
their fragment set is the solver's to decide, so they get FINAL_UNDECIDED and
never reach the kernel.  final_decisions says where the enumeration's optimum
is provably the program's (FINAL_TAKE) and where a solver still has to run
(FINAL_SOLVE).  A solver stopped by its time limit may return anything; TAKE
equals the reference under completed solves only.

The robust final program (sst_final_robust_device; DESIGN "The robust final
program") decides the FINAL_UNDECIDED spectra too: final_use(al, optional=True)
marks the LP_SOLVE fragments optional, final_robust_host / final_robust_device
enumerate once over the required fragments and once more with every optional
cost capped at its cost under the first optimum (a RobustOutcome beside the
FinalOutcome), and robust_decisions says where that optimum is provably the
program's for every subset of the optional fragments the solver may keep.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _native
from ._native import FINAL_INFEASIBLE, FINAL_NONE, FINAL_NOT_FREE, FINAL_SKIPPED, FINAL_SOLVED, FINAL_TOO_LARGE
from .alignment import ALIGN_MAX_LEN, LP_KEEP, LP_SOLVE, _rows_of, lp_caps, lp_decisions, lp_row_caps, position_sets

FINAL_UNDECIDED = 6                 # Python layer only: the spectrum holds an LP_SOLVE fragment
FINAL_MAX_COMBOS = 1 << 22          # sst_final_max_combos()
FINAL_DEFAULT_COMBOS = 1 << 20
FINAL_MAX_USED = 16384              # used fragments of a modelled spectrum
FIX = 65536                         # fixed-point units per precision unit
EMPTY_INTERVAL = 0xFFFF
NO_INTERVAL = 0xFFFE
NO_GAP = np.uint64(0xFFFFFFFFFFFFFFFF)
STATUS_NAMES = {FINAL_NONE: "NONE", FINAL_SOLVED: "SOLVED", FINAL_TOO_LARGE: "TOO_LARGE",
                FINAL_INFEASIBLE: "INFEASIBLE", FINAL_SKIPPED: "SKIPPED", FINAL_NOT_FREE: "NOT_FREE",
                FINAL_UNDECIDED: "UNDECIDED"}
FINAL_SOLVE, FINAL_TAKE = 0, 1
_HOST_BLOCK = 1 << 22               # elements of a block of interval sums (final_host)
SEARCH_MAX_WIDTH = 1 << 16          # sst_final_search_max_width()
SEARCH_DEFAULT_WIDTH = 1 << 12
SEARCH_MAX_HORIZON = 1 << 62
SEARCH_DEFAULT_HORIZON = 1 << 17    # two precision units: above every need of final_decisions / robust_decisions
SEARCH_MAX_FREE = 48                # free positions of a searched spectrum
SEARCH_ENUMERATED, SEARCH_SEARCHED = 1, 2   # SearchOutcome.mode (0: not SOLVED)


@dataclass
class FinalOutcome:
    """The final program's result per spectrum, position and fragment, parallel
    to a BatchOutcome (position p of spectrum g at pos_off[g] + p, fragment k at
    frag_off[g] + k), as host arrays."""
    frag_off: np.ndarray  # [S + 1] i64, the BatchOutcome's
    pos_off: np.ndarray   # [S + 1] i64, the BatchOutcome's
    status: np.ndarray    # u8 FINAL_*
    combos: np.ndarray    # u64 prod |A_i|, saturating
    n_feas: np.ndarray    # u64 feasible y (0 unless SOLVED)
    best: np.ndarray      # u64 min obj
    n_opt: np.ndarray     # u32 feasible y with obj == best
    gap: np.ndarray       # u64 smallest obj above best, minus best; NO_GAP if none
    seq: np.ndarray       # u8 per position: the row of the first optimal y
    iv: np.ndarray        # u16 per fragment: its interval under that y, NO_INTERVAL if unused / not SOLVED
    sum: np.ndarray       # u32 per fragment: that interval's sum

    SPECTRUM_FIELDS = ("status", "combos", "n_feas", "best", "n_opt", "gap")
    FRAGMENT_FIELDS = ("iv", "sum")
    _DTYPES = {"frag_off": np.int64, "pos_off": np.int64, "status": np.uint8, "combos": np.uint64, "n_feas": np.uint64,
               "best": np.uint64, "n_opt": np.uint32, "gap": np.uint64, "seq": np.uint8, "iv": np.uint16,
               "sum": np.uint32}

    def __post_init__(self):
        for k, dt in self._DTYPES.items():
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))
        S = len(self.frag_off) - 1
        if S < 0 or len(self.pos_off) != S + 1 or any(len(getattr(self, k)) != S for k in self.SPECTRUM_FIELDS) or \
                len(self.seq) != int(self.pos_off[-1]) or \
                any(len(getattr(self, k)) != int(self.frag_off[-1]) for k in self.FRAGMENT_FIELDS):
            raise ValueError("FinalOutcome: arrays do not match frag_off / pos_off")

    def __len__(self):
        return len(self.frag_off) - 1

    def equals(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self._DTYPES)

    def shares(self):
        """Share of each status over all spectra, by name."""
        n = max(1, len(self.status))
        return {name: float(np.count_nonzero(self.status == st)) / n for st, name in STATUS_NAMES.items()}

    def n_used(self):
        """Used fragments per spectrum (i64): those with an interval, so 0 where the spectrum is not SOLVED."""
        used = np.concatenate([[0], np.cumsum(self.iv != NO_INTERVAL)])
        return (used[self.frag_off[1:]] - used[self.frag_off[:-1]]).astype(np.int64)

    def take(self, idx):
        """The result of spectra idx, in that order (as BatchOutcome.take)."""
        from .pipeline_device import _segments

        idx = np.asarray(idx, dtype=np.int64)
        fsrc, foff = _segments(self.frag_off, idx)
        psrc, poff = _segments(self.pos_off, idx)
        return FinalOutcome(frag_off=foff, pos_off=poff, seq=self.seq[psrc],
                            **{k: getattr(self, k)[idx] for k in self.SPECTRUM_FIELDS},
                            **{k: getattr(self, k)[fsrc] for k in self.FRAGMENT_FIELDS})

    @classmethod
    def concat(cls, outcomes):
        """Several results' spectra one after the other (as BatchOutcome.concat)."""
        outcomes = list(outcomes)
        if not outcomes:
            raise ValueError("FinalOutcome.concat: nothing to concatenate")

        def offsets(name):
            base = np.concatenate([[0], np.cumsum([int(getattr(o, name)[-1]) for o in outcomes])]).astype(np.int64)
            return np.concatenate([getattr(o, name)[:-1] + b for o, b in zip(outcomes, base)] + [base[-1:]])

        fields = cls.SPECTRUM_FIELDS + cls.FRAGMENT_FIELDS + ("seq",)
        return cls(frag_off=offsets("frag_off"), pos_off=offsets("pos_off"),
                   **{k: np.concatenate([getattr(o, k) for o in outcomes]) for k in fields})

    @classmethod
    def blank(cls, outcome, status=FINAL_NONE):
        """Every spectrum of `outcome` with `status` and the outputs of a spectrum that is not SOLVED."""
        S, nf, n_pos = len(outcome), int(outcome.frag_off[-1]), int(outcome.pos_off[-1])
        return cls(frag_off=np.array(outcome.frag_off, dtype=np.int64), pos_off=np.array(outcome.pos_off, dtype=np.int64),
                   status=np.full(S, status, np.uint8), combos=np.zeros(S, np.uint64), n_feas=np.zeros(S, np.uint64),
                   best=np.zeros(S, np.uint64), n_opt=np.zeros(S, np.uint32), gap=np.full(S, NO_GAP, np.uint64),
                   seq=np.zeros(n_pos, np.uint8), iv=np.full(nf, NO_INTERVAL, np.uint16), sum=np.zeros(nf, np.uint32))


@dataclass
class RobustOutcome:
    """The robust final program's five further results per spectrum, parallel
    to a FinalOutcome (include/sst.h, sst_final_robust_device), as host arrays."""
    n_optional: np.ndarray  # u32 optional fragments (0 unless SOLVED)
    cstar: np.ndarray       # u64 sum over the optional fragments of their cost under seq
    rbest: np.ndarray       # u64 min cap
    rn_opt: np.ndarray      # u32 feasible y with cap == rbest
    rgap: np.ndarray        # u64 smallest cap above rbest, minus rbest; NO_GAP if none

    _DTYPES = {"n_optional": np.uint32, "cstar": np.uint64, "rbest": np.uint64, "rn_opt": np.uint32, "rgap": np.uint64}

    def __post_init__(self):
        for k, dt in self._DTYPES.items():
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))
        if any(len(getattr(self, k)) != len(self.n_optional) for k in self._DTYPES):
            raise ValueError("RobustOutcome: arrays of different lengths")

    def __len__(self):
        return len(self.n_optional)

    def equals(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self._DTYPES)

    def take(self, idx):
        """The result of spectra idx, in that order (as FinalOutcome.take)."""
        idx = np.asarray(idx, dtype=np.int64)
        return RobustOutcome(**{k: getattr(self, k)[idx] for k in self._DTYPES})

    @classmethod
    def concat(cls, outcomes):
        """Several results' spectra one after the other (as FinalOutcome.concat)."""
        outcomes = list(outcomes)
        if not outcomes:
            raise ValueError("RobustOutcome.concat: nothing to concatenate")
        return cls(**{k: np.concatenate([getattr(o, k) for o in outcomes]) for k in cls._DTYPES})

    @classmethod
    def blank(cls, outcome):
        """The outputs of spectra that are not SOLVED, one per spectrum of `outcome`."""
        S = len(outcome)
        return cls(n_optional=np.zeros(S, np.uint32), cstar=np.zeros(S, np.uint64), rbest=np.zeros(S, np.uint64),
                   rn_opt=np.zeros(S, np.uint32), rgap=np.full(S, NO_GAP, np.uint64))


@dataclass
class SearchOutcome:
    """The bounded search's three further results per spectrum, parallel to a
    FinalOutcome (include/sst.h, sst_final_search_device), as host arrays."""
    mode: np.ndarray    # u8 0 not SOLVED, SEARCH_ENUMERATED, SEARCH_SEARCHED
    rounds: np.ndarray  # u32 sweeps run in both passes (0 unless searched)
    nodes: np.ndarray   # u64 nodes kept over all sweeps (0 unless searched)
    horizon: int        # H: gap and rgap of a searched spectrum are min(true gap, H + 1)
    widest: np.ndarray = None  # u32 the widest level of any sweep: the host model's only (None from the device)

    _DTYPES = {"mode": np.uint8, "rounds": np.uint32, "nodes": np.uint64}

    def __post_init__(self):
        for k, dt in self._DTYPES.items():
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))
        self.horizon = int(self.horizon)
        if any(len(getattr(self, k)) != len(self.mode) for k in self._DTYPES):
            raise ValueError("SearchOutcome: arrays of different lengths")

    def __len__(self):
        return len(self.mode)

    def equals(self, other):
        return self.horizon == other.horizon and \
            all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self._DTYPES)

    def take(self, idx):
        """The result of spectra idx, in that order (as FinalOutcome.take)."""
        idx = np.asarray(idx, dtype=np.int64)
        return SearchOutcome(horizon=self.horizon, widest=None if self.widest is None else self.widest[idx],
                             **{k: getattr(self, k)[idx] for k in self._DTYPES})

    @classmethod
    def concat(cls, outcomes):
        """Several results' spectra one after the other (as FinalOutcome.concat); one horizon."""
        outcomes = list(outcomes)
        if not outcomes or len({o.horizon for o in outcomes}) != 1:
            raise ValueError("SearchOutcome.concat: nothing to concatenate, or different horizons")
        widest = None if any(o.widest is None for o in outcomes) else np.concatenate([o.widest for o in outcomes])
        return cls(horizon=outcomes[0].horizon, widest=widest,
                   **{k: np.concatenate([getattr(o, k) for o in outcomes]) for k in cls._DTYPES})

    @classmethod
    def blank(cls, outcome, horizon):
        """The outputs of spectra that are not SOLVED, one per spectrum of `outcome`."""
        S = len(outcome)
        return cls(mode=np.zeros(S, np.uint8), rounds=np.zeros(S, np.uint32), nodes=np.zeros(S, np.uint64),
                   horizon=horizon, widest=np.zeros(S, np.uint32))


def final_use(al, optional=False):
    """(use, undecided) from a keep-mode AlignOutcome: use u8 per fragment, 1
    for the LP_KEEP fragments (filter_with_lp, run to optimality, keeps exactly
    those where nothing is LP_SOLVE); undecided bool per spectrum, True where
    some fragment is LP_SOLVE: the final program's fragment set is then the
    solver's to decide.  optional=True (the robust final program): use is also 2
    at the LP_SOLVE fragments, and no spectrum is undecided."""
    if not al.has_keep:
        raise ValueError("final_use: the AlignOutcome is not in keep mode")
    dec = lp_decisions(al)
    if optional:
        use = np.where(dec == LP_KEEP, 1, np.where(dec == LP_SOLVE, 2, 0)).astype(np.uint8)
        return use, np.zeros(len(al.frag_off) - 1, bool)
    solve = np.concatenate([[0], np.cumsum(dec == LP_SOLVE)])
    return (dec == LP_KEEP).astype(np.uint8), (solve[al.frag_off[1:]] - solve[al.frag_off[:-1]]) > 0


def final_decisions(fo, min_gap_units=0.5):
    """Per spectrum (u8) FINAL_TAKE where the enumeration's optimum is provably
    the program's unique one with a margin: SOLVED, n_opt == 1 and gap >=
    max(2 n_used + 1, min_gap_units * 65536) (the rounding of the fixed-point
    masses moves every objective by less than n_used units; half a precision
    unit is the margin of the DROP and KEEP sides); else FINAL_SOLVE."""
    need = np.maximum(2 * fo.n_used() + 1, int(np.ceil(min_gap_units * FIX))).astype(np.uint64)
    take = (fo.status == FINAL_SOLVED) & (fo.n_opt == 1) & (fo.gap >= need)
    return np.where(take, FINAL_TAKE, FINAL_SOLVE).astype(np.uint8)


def robust_decisions(fo, ro, min_gap_units=0.5):
    """Per spectrum (u8) FINAL_TAKE where seq is provably the unique optimum,
    with a margin, of the program over the required fragments plus ANY subset of
    the optional ones: SOLVED, rbest == best + cstar (y* minimises cap), rn_opt
    == 1 and rgap >= max(2 (n_used + n_optional) + 1, min_gap_units * 65536);
    else FINAL_SOLVE.  fo, ro: final_robust_host's or final_robust_device's
    (fo.n_used() counts the required and the optional fragments there).  Without
    optional fragments this is final_decisions' answer."""
    need = np.maximum(2 * fo.n_used() + 1, int(np.ceil(min_gap_units * FIX))).astype(np.uint64)
    take = (fo.status == FINAL_SOLVED) & (ro.rbest == fo.best + ro.cstar) & (ro.rn_opt == 1) & (ro.rgap >= need)
    return np.where(take, FINAL_TAKE, FINAL_SOLVE).astype(np.uint8)


def sequence_names(fo, outcome, g):
    """The list of names evaluate (linear_program.py:249) would return for
    spectrum g: the first name of the row at every position.  ValueError unless
    the spectrum is SOLVED."""
    if fo.status[g] != FINAL_SOLVED:
        raise ValueError(f"sequence_names: spectrum {g} is {STATUS_NAMES[int(fo.status[g])]}, not SOLVED")
    return [outcome.row_names[int(r)] for r in fo.seq[int(fo.pos_off[g]):int(fo.pos_off[g + 1])]]


def _check_max_combos(max_combos, who, least=1):
    max_combos = int(max_combos)
    if not least <= max_combos <= FINAL_MAX_COMBOS:
        raise ValueError(f"{who}: max_combos outside [{least}, 2^22]")
    return max_combos


def _check_search(horizon, max_width, who):
    horizon, max_width = int(horizon), int(max_width)
    if not 0 <= horizon <= SEARCH_MAX_HORIZON:
        raise ValueError(f"{who}: horizon outside [0, 2^62]")
    if not 1 <= max_width <= SEARCH_MAX_WIDTH:
        raise ValueError(f"{who}: max_width outside [1, 2^16]")
    return horizon, max_width


def _per_fragment(use, nf, who):
    if use is None:
        return np.ones(nf, np.uint8)
    use = (np.asarray(use).reshape(-1) != 0).astype(np.uint8)
    if len(use) != nf:
        raise ValueError(f"{who}: use does not match the outcome's fragments")
    return use


def _per_fragment_robust(use, nf, who):
    """use as 0 unused / 1 required / 2 optional (any other value: 1)."""
    if use is None:
        return np.ones(nf, np.uint8)
    use = np.asarray(use).reshape(-1)
    if len(use) != nf:
        raise ValueError(f"{who}: use does not match the outcome's fragments")
    return np.where(use == 0, 0, np.where(use == 2, 2, 1)).astype(np.uint8)


def _per_spectrum(undecided, S, who):
    if undecided is None:
        return np.zeros(S, bool)
    undecided = np.asarray(undecided).reshape(-1) != 0
    if len(undecided) != S:
        raise ValueError(f"{who}: undecided does not match the outcome's spectra")
    return undecided


def _ends(cls, mn, mx):
    """The range of ends a terminal fragment walks: r in [lo, hi] (START), l in [lo, hi] (END)."""
    return min(mn, mx), (mx if cls == 1 else mn)


def _solve_spectrum(L, sets, row_mass, row_mod, mod_cap, cls, qfix, mn, mx, in_obj=None, cap=None):
    """The enumeration of one modelled, row-free spectrum within max_combos:
    (n_feas, best, n_opt, gap, seq, iv, sum); n_feas == 0: no feasible y.
    in_obj (bool per fragment, None: all): the fragments the objective sums; iv
    and sum are given for every fragment.  cap (i64 per fragment, None: none):
    a fragment's cost enters the objective as min(cost, cap)."""
    radices = [len(rows) for rows in sets]
    combos = int(np.prod(radices, dtype=object)) if L else 1
    mass = [np.array([int(row_mass[r]) for r in rows], dtype=np.int64) for rows in sets]
    mod = [np.array([int(row_mod[r] != 0) for r in rows], dtype=np.int64) for rows in sets]
    ia, ib = np.triu_indices(L + 1, k=1)  # (a, b), a < b, in (a, b) order: the interval [a, b - 1] in (l, r) order
    internal = np.flatnonzero(cls == 0)
    block = max(1, _HOST_BLOCK // max(1, len(ia))) if len(internal) else 1 << 16
    q = qfix.astype(np.int64)

    def digits_of(idx):
        """The mixed-radix digits of the indices idx, position 0 most significant: [n, L]"""
        out = np.zeros((len(idx), L), np.int64)
        rem = np.array(idx, dtype=np.int64)
        for p in range(L - 1, -1, -1):
            if radices[p] > 1:
                rem, out[:, p] = np.divmod(rem, radices[p])
        return out

    def prefix_of(idx):
        digits = digits_of(idx)
        w = np.stack([mass[p][digits[:, p]] for p in range(L)], axis=1) if L else np.zeros((len(idx), 0), np.int64)
        n_mod = sum((mod[p][digits[:, p]] for p in range(L)), np.zeros(len(idx), np.int64))
        return np.concatenate([np.zeros((len(idx), 1), np.int64), np.cumsum(w, axis=1)], axis=1), n_mod

    def costs(P, j, pairs):
        """|qfix_j - 65536 S| over fragment j's admissible intervals, in (l, r) order, the empty one last: [n, n_iv]"""
        if cls[j] == 3:
            s = P[:, L:L + 1]
        elif cls[j] == 1:
            lo, hi = _ends(1, int(mn[j]), int(mx[j]))
            s = P[:, lo + 1:hi + 2]
        elif cls[j] == 2:
            lo, hi = _ends(2, int(mn[j]), int(mx[j]))
            s = P[:, L:L + 1] - P[:, lo:hi + 1]
        else:
            s = np.concatenate([pairs, np.zeros((len(P), 1), np.int64)], axis=1)
        return np.abs(q[j] - FIX * s), s

    n_feas, best, n_opt, nxt, first = 0, None, 0, None, -1
    for start in range(0, combos, block):
        idx = np.arange(start, min(combos, start + block), dtype=np.int64)
        P, n_mod = prefix_of(idx)
        ok = n_mod <= mod_cap
        if not ok.any():
            continue
        P, idx = P[ok], idx[ok]
        pairs = P[:, ib] - P[:, ia] if len(internal) else None
        obj = np.zeros(len(idx), np.int64)
        for j in range(len(cls)):
            if in_obj is not None and not in_obj[j]:
                continue
            c = costs(P, j, pairs)[0].min(axis=1)
            obj += c if cap is None else np.minimum(c, cap[j])
        n_feas += len(idx)
        vals = np.unique(obj)
        for v in vals[:2].tolist():  # the block's smallest two distinct objectives
            if best is None or v < best:
                best, nxt, n_opt, first = v, best, 0, -1
            elif v != best and (nxt is None or v < nxt):
                nxt = v
        at = np.flatnonzero(obj == best)
        if len(at):
            n_opt += len(at)
            if first < 0:
                first = int(idx[at[0]])
    if n_feas == 0:
        return 0, 0, 0, NO_GAP, None, None, None
    seq = np.array([sets[p][int(d)] for p, d in enumerate(digits_of([first])[0])], dtype=np.uint8)
    iv, sm = _intervals_under(L, seq, row_mass, cls, q, mn, mx)
    return n_feas, best, min(n_opt, 0xFFFFFFFF), (NO_GAP if nxt is None else nxt - best), seq, iv, sm


def _interval_sums(P, Q, L, c, mn, mx, pairs):
    """The sums of a fragment's admissible intervals in (l, r) order, the empty
    one last, as differences of prefix sums: P(r + 1) - Q(l) ([n, n_iv]; P is Q
    for the sums of one y).  c, mn, mx: its class and ends; pairs: (ia, ib) of
    np.triu_indices(L + 1, k=1), read by an internal fragment."""
    if c == 3:
        return P[:, L:L + 1] - Q[:, 0:1]
    if c == 1:
        lo, hi = _ends(1, mn, mx)
        return P[:, lo + 1:hi + 2] - Q[:, 0:1]
    if c == 2:
        lo, hi = _ends(2, mn, mx)
        return P[:, L:L + 1] - Q[:, lo:hi + 1]
    return np.concatenate([P[:, pairs[1]] - Q[:, pairs[0]], np.zeros((len(P), 1), np.int64)], axis=1)


def _intervals_under(L, seq, row_mass, cls, q, mn, mx):
    """(iv, sum) per fragment under the assignment seq (one row per position):
    the first minimiser of c_j in (l, r) order, the empty interval last."""
    P = np.concatenate([[0], np.cumsum([int(row_mass[r]) for r in seq], dtype=np.int64)]).astype(np.int64)[None, :]
    ia, ib = np.triu_indices(L + 1, k=1)
    iv = np.empty(len(cls), np.uint16)
    sm = np.empty(len(cls), np.uint32)
    for j in range(len(cls)):
        s = _interval_sums(P, P, L, int(cls[j]), int(mn[j]), int(mx[j]), (ia, ib))
        at = int(np.argmin(np.abs(q[j] - FIX * s[0])))
        sm[j] = int(s[0, at])
        if cls[j] == 3:
            iv[j] = L - 1 if L else EMPTY_INTERVAL
        elif cls[j] == 1:
            iv[j] = _ends(1, int(mn[j]), int(mx[j]))[0] + at
        elif cls[j] == 2:
            iv[j] = (_ends(2, int(mn[j]), int(mx[j]))[0] + at) << 8 | (L - 1)
        else:
            iv[j] = EMPTY_INTERVAL if at == len(ia) else int(ia[at]) << 8 | (int(ib[at]) - 1)
    return iv, sm


class _Search:
    """The bounded search of one modelled, row-free spectrum by the definition
    (include/sst.h, sst_final_search_device): nodes as arrays per level, the
    bound over every admissible interval, Python / numpy integers."""

    def __init__(self, L, sets, row_mass, row_mod, mod_cap, cls, qfix, mn, mx, optional, max_width):
        self.L, self.cls, self.q, self.mn, self.mx = L, cls, qfix.astype(np.int64), mn, mx
        self.optional, self.max_width, self.mod_cap = optional, max_width, mod_cap
        self.free = [p for p in range(L) if len(sets[p]) > 1]
        self.rows = [np.array(sets[p], dtype=np.int64) for p in self.free]
        self.mass = np.array([int(m) for m in row_mass], dtype=np.int64)
        self.is_mod = np.array([int(m != 0) for m in row_mod], dtype=np.int64)
        one = [sets[p][0] for p in range(L)]
        self.fixed_mod = sum(int(self.is_mod[one[p]]) for p in range(L) if len(sets[p]) == 1)
        # per position the smallest and largest mass over A_i (an open position), and the one row's
        self.wmin = np.array([min(int(self.mass[r]) for r in sets[p]) for p in range(L)], dtype=np.int64)
        self.wmax = np.array([max(int(self.mass[r]) for r in sets[p]) for p in range(L)], dtype=np.int64)
        all_mod = [int(all(self.is_mod[r] for r in rows)) for rows in self.rows]
        self.all_mod_from = np.concatenate([np.cumsum(all_mod[::-1])[::-1], [0]]).astype(np.int64)
        self.pairs = np.triu_indices(L + 1, k=1)
        self.rounds = self.nodes = self.widest = 0

    def n_feas(self):
        """The feasible y, counted over the number of modified rows per free position."""
        ways = {0: 1}  # modified rows among the free positions so far -> assignments
        for rows in self.rows:
            m = int(self.is_mod[rows].sum())
            nxt = {}
            for k, v in ways.items():
                for add, mult in ((0, len(rows) - m), (1, m)):
                    if mult and self.fixed_mod + k + add <= self.mod_cap:
                        nxt[k + add] = nxt.get(k + add, 0) + v * mult
            ways = nxt
        return sum(ways.values()) if self.fixed_mod <= self.mod_cap else 0

    def bound(self, fixed, cap=None):
        """lb of the nodes `fixed` ([m, d] rows at the first d free positions):
        the required fragments' lb_j summed, and with cap (c*_j per fragment) the
        optional ones' min(lb_j, c*_j) too."""
        m, d = fixed.shape
        wmin, wmax = np.tile(self.wmin, (m, 1)), np.tile(self.wmax, (m, 1))
        for k in range(d):
            wmin[:, self.free[k]] = wmax[:, self.free[k]] = self.mass[fixed[:, k]]
        zero = np.zeros((m, 1), np.int64)
        Pmin = np.concatenate([zero, np.cumsum(wmin, axis=1)], axis=1)
        Pmax = np.concatenate([zero, np.cumsum(wmax, axis=1)], axis=1)
        lb = np.zeros(m, np.int64)
        for j in range(len(self.cls)):
            if self.optional[j] and cap is None:
                continue
            at = (int(self.cls[j]), int(self.mn[j]), int(self.mx[j]), self.pairs)
            smin = _interval_sums(Pmin, Pmin, self.L, *at)
            smax = _interval_sums(Pmax, Pmax, self.L, *at)
            dist = np.maximum(0, np.maximum(FIX * smin - self.q[j], self.q[j] - FIX * smax)).min(axis=1)
            lb += np.minimum(dist, cap[j]) if self.optional[j] else dist
        return lb

    def sweep(self, T, cap=None):
        """Sweep(T): (leaves [m, n] as rows, their objectives), or None on overflow."""
        T = min(int(T), (1 << 63) - 1)
        self.rounds += 1
        fixed, mods = np.zeros((1, 0), np.int64), np.array([self.fixed_mod], np.int64)
        for d, rows in enumerate(self.rows):
            m = len(fixed)
            fixed = np.concatenate([np.repeat(fixed, len(rows), axis=0), np.tile(rows, m)[:, None]], axis=1)
            mods = np.repeat(mods, len(rows)) + np.tile(self.is_mod[rows], m)
            live = mods + self.all_mod_from[d + 1] <= self.mod_cap
            fixed, mods = fixed[live], mods[live]
            keep = np.zeros(len(fixed), bool)
            for at in range(0, len(fixed), 4096):
                keep[at:at + 4096] = self.bound(fixed[at:at + 4096], cap) <= T
            fixed, mods = fixed[keep], mods[keep]
            if len(fixed) > self.max_width:
                return None
            self.nodes += len(fixed)
            self.widest = max(self.widest, len(fixed))
        return fixed, self.bound(fixed, cap)

    @staticmethod
    def summary(obj, H):
        """(min, how many leaves attain it, the smallest value in (min, min + H] minus it, else H + 1)"""
        lo = int(obj.min())
        above = obj[(obj > lo) & (obj <= min(lo + H, (1 << 63) - 1))]
        return lo, min(int((obj == lo).sum()), 0xFFFFFFFF), (int(above.min()) - lo if len(above) else H + 1)


def _search_spectrum(L, sets, row_mass, row_mod, mod_cap, cls, qfix, mn, mx, optional, H, max_width):
    """The bounded search of one spectrum: None where a sweep overflows, else
    (best, n_opt, gap, seq, iv, sum, cstar, rbest, rn_opt, rgap, rounds, nodes, widest)."""
    s = _Search(L, sets, row_mass, row_mod, mod_cap, cls, qfix, mn, mx, optional, max_width)
    T = max(H, FIX)
    while True:
        got = s.sweep(T)
        if got is None:
            return None
        if len(got[0]):
            break
        T = min(4 * T, (1 << 63) - 1)
    b = int(got[1].min())
    if b + H > T:
        got = s.sweep(b + H)
        if got is None:
            return None
    leaves, obj = got
    best, n_opt, gap = s.summary(obj, H)
    first = min(tuple(int(r) for r in y) for y in leaves[obj == best])
    seq = np.array([sets[p][0] for p in range(L)], dtype=np.uint8)
    seq[s.free] = first
    iv, sm = _intervals_under(L, seq, row_mass, cls, s.q, mn, mx)
    cstar, rbest, rn_opt, rgap = 0, best, n_opt, gap
    if optional.any():
        c_star = np.where(optional, np.abs(s.q - FIX * sm.astype(np.int64)), np.iinfo(np.int64).max)
        cstar = int(c_star[optional].sum())
        got = s.sweep(best + cstar + H, cap=c_star)
        if got is None:
            return None
        rbest, rn_opt, rgap = s.summary(got[1], H)
    return best, n_opt, gap, seq, iv, sm, cstar, rbest, rn_opt, rgap, s.rounds, s.nodes, s.widest


def final_host(outcome, precision, caps, row_cap, use=None, max_combos=FINAL_DEFAULT_COMBOS, undecided=None):
    """The final program of every spectrum of `outcome` (a BatchOutcome) by the
    definition (include/sst.h, sst_final_program_device), vectorised over y.
    caps = (row_mod, mod_cap) (alignment.lp_caps), row_cap the per-row caps
    table (alignment.lp_row_caps); use: u8 per fragment, None = all; undecided:
    bool per spectrum, those get FINAL_UNDECIDED and nothing is computed."""
    use = _per_fragment(use, int(outcome.frag_off[-1]), "final_host")
    return _final_host(outcome, precision, caps, row_cap, use, max_combos, undecided, "final_host")[0]


def final_robust_host(outcome, precision, caps, row_cap, use=None, max_combos=FINAL_DEFAULT_COMBOS):
    """The robust final program of every spectrum of `outcome` by the definition
    (include/sst.h, sst_final_robust_device): (FinalOutcome, RobustOutcome).
    use: u8 per fragment, 0 unused, 1 required, 2 optional (anything else: 1),
    None = all required.  One enumeration over the required fragments (best,
    n_opt, gap, seq: y*), then, where a spectrum holds optional fragments, a
    second one over all of them with every optional cost capped at its cost
    under y*.  The other arguments as final_host's."""
    use = _per_fragment_robust(use, int(outcome.frag_off[-1]), "final_robust_host")
    return _final_host(outcome, precision, caps, row_cap, use, max_combos, None, "final_robust_host")


def final_search_host(outcome, precision, caps, row_cap, use=None, max_combos=FINAL_DEFAULT_COMBOS,
                      horizon=SEARCH_DEFAULT_HORIZON, max_width=SEARCH_DEFAULT_WIDTH):
    """The robust final program with the bounded search, by the definition
    (include/sst.h, sst_final_search_device): (FinalOutcome, RobustOutcome,
    SearchOutcome).  A spectrum within max_combos is enumerated as
    final_robust_host does (mode 1); a larger one (max_combos may be 0: every
    one) is searched level by level over its free positions, keeping the nodes
    whose lower bound is within the threshold (mode 2 where SOLVED): its gap
    and rgap are min(true gap, horizon + 1).  The other arguments as
    final_robust_host's."""
    use = _per_fragment_robust(use, int(outcome.frag_off[-1]), "final_search_host")
    search = _check_search(horizon, max_width, "final_search_host")
    return _final_host(outcome, precision, caps, row_cap, use, max_combos, None, "final_search_host", search)


def _final_host(outcome, precision, caps, row_cap, use, max_combos, undecided, who, search=None):
    """final_host (use in {0, 1}) and final_robust_host (use in {0, 1, 2}): (FinalOutcome, RobustOutcome);
    final_search_host (search = (horizon, max_width)): and a SearchOutcome."""
    max_combos = _check_max_combos(max_combos, who, 0 if search else 1)
    S = len(outcome)
    n_rows = len(outcome.row_mass)
    row_mod = np.ascontiguousarray(caps[0], dtype=np.uint8)
    mod_cap = np.ascontiguousarray(caps[1], dtype=np.int32)
    if len(row_mod) != n_rows or len(mod_cap) != S:
        raise ValueError(f"{who}: caps do not match the outcome's rows / spectra")
    row_cap = np.ascontiguousarray(row_cap, dtype=np.int32).reshape(-1)
    if len(row_cap) != (ALIGN_MAX_LEN + 1) * n_rows:
        raise ValueError(f"{who}: row_cap is not a table of 254 lengths by the outcome's rows")
    row_cap = row_cap.reshape(ALIGN_MAX_LEN + 1, n_rows)
    if n_rows and (int(outcome.row_mass.min()) < 0 or int(outcome.row_mass.max()) >= (1 << 32) // ALIGN_MAX_LEN):
        raise ValueError(f"{who}: a row mass outside [0, 2^32 / 253)")
    undecided = _per_spectrum(undecided, S, who)
    fo = FinalOutcome.blank(outcome)
    ro = RobustOutcome.blank(outcome)
    so = SearchOutcome.blank(outcome, search[0]) if search else None
    with np.errstate(all="ignore"):
        u = np.asarray(outcome.frag_su, dtype=np.float64) / np.float64(precision)
        in_model = np.abs(u) < 2.0 ** 32  # (False for NaN and the infinities)
        qfix = np.where(in_model, np.rint(np.where(in_model, u, 0.0) * float(FIX)), 0.0).astype(np.int64)
    cls_all = (np.asarray(outcome.frag_code).astype(np.int64) >> 2) & 3
    for g in range(S):
        if undecided[g]:
            fo.status[g] = FINAL_UNDECIDED
            continue
        f = slice(int(outcome.frag_off[g]), int(outcome.frag_off[g + 1]))
        if f.start == f.stop:
            continue
        L = int(outcome.seq_len[g])
        p = slice(int(outcome.pos_off[g]), int(outcome.pos_off[g + 1]))
        on = np.flatnonzero(use[f]) + f.start
        cls = cls_all[on]
        mn, mx = outcome.frag_min_end[on].astype(np.int64), outcome.frag_max_end[on].astype(np.int64)
        terminal = (cls == 1) | (cls == 2)
        if L < 0 or L > ALIGN_MAX_LEN or p.stop - p.start != L or len(on) > FINAL_MAX_USED or not in_model[on].all() or \
                (terminal & ((mn < 0) | (mn >= L) | (mx < 0) | (mx >= L))).any():
            fo.status[g] = FINAL_SKIPPED
            continue
        sets = position_sets(outcome.skeleton[p], outcome.alpha[g], n_rows)
        combos = 1
        for rows in sets:
            combos *= len(rows)
        fo.combos[g] = min(combos, (1 << 64) - 1)
        if combos == 0:
            fo.status[g] = FINAL_INFEASIBLE
            continue
        n_r = {}
        for rows in sets:
            for r in rows:
                n_r[r] = n_r.get(r, 0) + 1
        cap = int(mod_cap[g])
        if not all(int(row_cap[L, r]) >= n_r.get(r, 0) or (row_mod[r] != 0 and int(row_cap[L, r]) >= cap)
                   for r in _rows_of(int(outcome.alpha[g][0]), int(outcome.alpha[g][1]), n_rows)):
            fo.status[g] = FINAL_NOT_FREE
            continue
        optional = use[on] == 2
        solve = (L, sets, outcome.row_mass, row_mod, cap, cls, qfix[on], mn, mx)
        if combos > max_combos and search:
            fo.status[g] = _search_into(fo, ro, so, g, p, on, solve, optional, *search)
            continue
        if combos > max_combos:
            fo.status[g] = FINAL_TOO_LARGE
            continue
        n_feas, best, n_opt, gap, seq, iv, sm = _solve_spectrum(*solve, in_obj=~optional if optional.any() else None)
        if n_feas == 0:
            fo.status[g] = FINAL_INFEASIBLE
            continue
        fo.status[g], fo.n_feas[g], fo.best[g], fo.n_opt[g], fo.gap[g] = FINAL_SOLVED, n_feas, best, n_opt, gap
        fo.seq[p], fo.iv[on], fo.sum[on] = seq, iv, sm
        ro.rbest[g], ro.rn_opt[g], ro.rgap[g] = best, n_opt, gap
        if optional.any():  # c*_j: the cost under y* (iv is a minimiser), the cap of the second enumeration
            c_star = np.where(optional, np.abs(qfix[on] - FIX * sm.astype(np.int64)), np.iinfo(np.int64).max)
            ro.n_optional[g], ro.cstar[g] = int(optional.sum()), int(c_star[optional].sum())
            _, ro.rbest[g], ro.rn_opt[g], ro.rgap[g], _, _, _ = _solve_spectrum(*solve, cap=c_star)
        if search:
            so.mode[g] = SEARCH_ENUMERATED
    return (fo, ro, so) if search else (fo, ro)


def _search_into(fo, ro, so, g, p, on, solve, optional, H, max_width):
    """The searched spectrum g: its status, and where that is SOLVED its outputs written."""
    sets = solve[1]
    if sum(len(rows) > 1 for rows in sets) > SEARCH_MAX_FREE:
        return FINAL_TOO_LARGE
    s = _Search(*solve, optional, max_width)
    n_feas = s.n_feas()
    if n_feas == 0:
        return FINAL_INFEASIBLE
    got = _search_spectrum(*solve, optional, H, max_width)
    if got is None:
        return FINAL_TOO_LARGE
    best, n_opt, gap, seq, iv, sm, cstar, rbest, rn_opt, rgap, rounds, nodes, widest = got
    fo.n_feas[g], fo.best[g], fo.n_opt[g], fo.gap[g] = min(n_feas, (1 << 64) - 1), best, n_opt, gap
    fo.seq[p], fo.iv[on], fo.sum[on] = seq, iv, sm
    ro.n_optional[g], ro.cstar[g], ro.rbest[g], ro.rn_opt[g], ro.rgap[g] = int(optional.sum()), cstar, rbest, rn_opt, rgap
    so.mode[g], so.rounds[g], so.nodes[g], so.widest[g] = SEARCH_SEARCHED, rounds, nodes, widest
    return FINAL_SOLVED


def final_device(dp_table, outcome, use=None, max_combos=FINAL_DEFAULT_COMBOS, undecided=None, caps=None, row_cap=None):
    """The final program of every spectrum of `outcome` on dp_table's device
    (sst_final_program_device): one upload per input array, one launch, one
    download per output array.  `outcome` must be on dp_table's rows.  caps and
    row_cap default to alignment.lp_caps / lp_row_caps of the table; a (row_mod,
    mod_cap) pair and a row_cap array are taken as they are.  use, undecided: as
    final_host; undecided spectra are taken out before the upload."""
    from .pipeline_device import _one_stream

    max_combos, row_mod, mod_cap, row_cap = _device_inputs(dp_table, outcome, max_combos, caps, row_cap, "final_device")
    S, nf = len(outcome), int(outcome.frag_off[-1])
    use = _per_fragment(use, nf, "final_device")
    undecided = _per_spectrum(undecided, S, "final_device")
    if not undecided.any():
        return _one_stream(_final_device)(dp_table, outcome, use, row_mod, mod_cap, row_cap, max_combos)
    from .pipeline_device import _segments

    run = np.flatnonzero(~undecided)
    rest = np.flatnonzero(undecided)
    src, _ = _segments(np.asarray(outcome.frag_off, dtype=np.int64), run)
    sub = outcome.take(run)
    part = _one_stream(_final_device)(dp_table, sub, use[src], row_mod, mod_cap[run], row_cap, max_combos)
    where = np.empty(S, np.int64)
    where[run] = np.arange(len(run))
    where[rest] = len(run) + np.arange(len(rest))
    return FinalOutcome.concat([part, FinalOutcome.blank(outcome.take(rest), FINAL_UNDECIDED)]).take(where)


def final_robust_device(dp_table, outcome, use=None, max_combos=FINAL_DEFAULT_COMBOS, caps=None, row_cap=None):
    """The robust final program of every spectrum of `outcome` on dp_table's
    device (sst_final_robust_device): (FinalOutcome, RobustOutcome), with the
    upload / launch / download shape of final_device.  use: as
    final_robust_host's (0 unused, 1 required, 2 optional); caps, row_cap: as
    final_device's."""
    from .pipeline_device import _one_stream

    max_combos, row_mod, mod_cap, row_cap = _device_inputs(dp_table, outcome, max_combos, caps, row_cap,
                                                           "final_robust_device")
    use = _per_fragment_robust(use, int(outcome.frag_off[-1]), "final_robust_device")
    return _one_stream(_final_device)(dp_table, outcome, use, row_mod, mod_cap, row_cap, max_combos, robust=True)


def _device_inputs(dp_table, outcome, max_combos, caps, row_cap, who, least=1):
    """(max_combos, row_mod, mod_cap, row_cap) of a device call, checked against the table and the outcome."""
    max_combos = _check_max_combos(max_combos, who, least)
    masses = [int(m.mass) for m in dp_table.masses]
    if masses != [int(x) for x in outcome.row_mass]:
        raise ValueError(f"{who}: the outcome is not on this table's rows")
    caps = lp_caps(dp_table, outcome) if caps is None else caps
    row_mod = np.ascontiguousarray(caps[0], dtype=np.uint8)
    mod_cap = np.ascontiguousarray(caps[1], dtype=np.int32)
    if len(row_mod) != len(masses) or len(mod_cap) != len(outcome):
        raise ValueError(f"{who}: caps do not match the table's rows / the outcome's spectra")
    row_cap = lp_row_caps(dp_table, outcome) if row_cap is None else row_cap
    row_cap = np.ascontiguousarray(row_cap, dtype=np.int32).reshape(-1)
    if len(row_cap) != (ALIGN_MAX_LEN + 1) * len(masses):
        raise ValueError(f"{who}: row_cap is not a table of 254 lengths by the table's rows")
    return max_combos, row_mod, mod_cap, row_cap


def final_search_device(dp_table, outcome, use=None, max_combos=FINAL_DEFAULT_COMBOS, horizon=SEARCH_DEFAULT_HORIZON,
                        max_width=SEARCH_DEFAULT_WIDTH, caps=None, row_cap=None):
    """The robust final program with the bounded search on dp_table's device
    (sst_final_search_device): (FinalOutcome, RobustOutcome, SearchOutcome), with
    the upload / launch / download shape of final_device.  The arguments as
    final_search_host's; caps, row_cap: as final_device's."""
    from .pipeline_device import _one_stream

    search = _check_search(horizon, max_width, "final_search_device")
    max_combos, row_mod, mod_cap, row_cap = _device_inputs(dp_table, outcome, max_combos, caps, row_cap,
                                                           "final_search_device", least=0)
    use = _per_fragment_robust(use, int(outcome.frag_off[-1]), "final_search_device")
    return _one_stream(_final_device)(dp_table, outcome, use, row_mod, mod_cap, row_cap, max_combos, robust=True,
                                      search=search)


def _final_device(dp_table, o, use, row_mod, mod_cap, row_cap, max_combos, robust=False, search=None):
    """One launch of sst_final_program_device (a FinalOutcome), or with robust of
    sst_final_robust_device (a FinalOutcome and a RobustOutcome), or with search
    = (horizon, max_width) of sst_final_search_device (and a SearchOutcome)."""
    import torch

    dt = dp_table.device_table
    eng = dt.engine
    dev = torch.device("cuda", eng.device)
    S, nf, n_pos = len(o), int(o.frag_off[-1]), int(o.pos_off[-1])
    if S == 0:
        blank = (FinalOutcome.blank(o), RobustOutcome.blank(o)) if robust else FinalOutcome.blank(o)
        return blank + (SearchOutcome(np.zeros(0), np.zeros(0), np.zeros(0), search[0]),) if search else blank

    def up(x, dtype, n=1):  # (never an empty allocation: the entry point refuses NULL)
        x = np.ascontiguousarray(x, dtype=dtype).reshape(-1)
        return torch.as_tensor(x if len(x) else np.zeros(n, dtype), device=dev)

    def out(n, dtype):
        return torch.empty(max(n, 1), dtype=dtype, device=dev)

    ins = [up(o.seq_len, np.int32), up(o.pos_off, np.int64), up(o.skeleton.view(np.int64), np.int64, 2),
           up(o.alpha.view(np.int64), np.int64, 2), up(o.frag_off, np.int64), up(o.frag_code, np.uint8),
           up(o.frag_su, np.float64), up(o.frag_min_end, np.int32), up(o.frag_max_end, np.int32), up(use, np.uint8)]
    more = [up(row_mod, np.uint8), up(mod_cap, np.int32), up(row_cap, np.int32)]
    outs = [out(S, torch.uint8), out(S, torch.int64), out(S, torch.int64), out(S, torch.int64), out(S, torch.int32),
            out(S, torch.int64), out(n_pos, torch.uint8), out(nf, torch.int16), out(nf, torch.int32)]
    r_outs = [out(S, torch.int32), out(S, torch.int64), out(S, torch.int64), out(S, torch.int32),
              out(S, torch.int64)] if robust else []
    s_outs = [out(S, torch.uint8), out(S, torch.int32), out(S, torch.int64)] if search else []
    top = _native.FinalSearchArgs() if search else None
    args = top.robust if search else _native.FinalRobustArgs() if robust else _native.FinalArgs()
    a = args.base if robust else args
    a.n_spec = S
    (a.seq_len, a.pos_off, a.skeleton, a.alpha, a.frag_off, a.frag_code, a.frag_su, a.frag_min_end, a.frag_max_end,
     a.frag_use) = (x.data_ptr() for x in ins)
    a.prec = float(dp_table.precision)
    a.row_mod, a.mod_cap, a.row_cap = (x.data_ptr() for x in more)
    a.max_combos = int(max_combos)
    a.status, a.combos, a.n_feas, a.best, a.n_opt, a.gap, a.seq, a.iv, a.sum = (x.data_ptr() for x in outs)
    if robust:
        args.n_optional, args.cstar, args.rbest, args.rn_opt, args.rgap = (x.data_ptr() for x in r_outs)
    if search:
        top.horizon, top.max_width = search
        top.mode, top.rounds, top.nodes = (x.data_ptr() for x in s_outs)
    name = "sst_final_search_device" if search else "sst_final_robust_device" if robust else "sst_final_program_device"
    torch.cuda.synchronize(dev)
    eng.check(getattr(eng._lib, name)(dt.handle, ctypes.byref(top if search else args)), name)
    eng.synchronize()
    status, combos, n_feas, best, n_opt, gap, seq, iv, sm = (x.cpu().numpy() for x in outs)
    fo = FinalOutcome(frag_off=np.array(o.frag_off, dtype=np.int64), pos_off=np.array(o.pos_off, dtype=np.int64),
                      status=status[:S], combos=combos[:S].view(np.uint64), n_feas=n_feas[:S].view(np.uint64),
                      best=best[:S].view(np.uint64), n_opt=n_opt[:S].view(np.uint32), gap=gap[:S].view(np.uint64),
                      seq=seq[:n_pos], iv=iv[:nf].view(np.uint16), sum=sm[:nf].view(np.uint32))
    if not robust:
        return fo
    n_optional, cstar, rbest, rn_opt, rgap = (x.cpu().numpy()[:S] for x in r_outs)
    ro = RobustOutcome(n_optional=n_optional.view(np.uint32), cstar=cstar.view(np.uint64),
                       rbest=rbest.view(np.uint64), rn_opt=rn_opt.view(np.uint32), rgap=rgap.view(np.uint64))
    if not search:
        return fo, ro
    mode, rounds, nodes = (x.cpu().numpy()[:S] for x in s_outs)
    return fo, ro, SearchOutcome(mode=mode, rounds=rounds.view(np.uint32), nodes=nodes.view(np.uint64),
                                 horizon=search[0])
