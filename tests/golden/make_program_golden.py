#!/usr/bin/env python3
"""Golden vectors that pin the stages which replace a solver call to the
REFERENCE's own programs: what a completed solve of LinearProgramInstance
(linear_program.py) returns in Predictor.filter_with_lp (prediction.py:229-259),
in the last evaluate (prediction.py:160-166) and in SkeletonBuilder
.select_sequence_length_with_lp (skeleton_building.py:198-289).

TEST INFRASTRUCTURE -- runs only in the build container, with the REFERENCE
(read-only at /root/reference) imported unmodified through the pandas-backed
polars stand-in (tests/golden/standin, see make_golden.py).  No solver exists
here.  This generator puts a pulp stand-in of its own into sys.modules before
the reference loads (the one under standin/ refuses every use and stays as it
is): LpVariable, lpSum, products by constants and comparisons build real affine
forms (a coefficient dict and a constant), LpProblem records the objective and
the constraints, and problem.solve() is an EXACT enumeration in
fractions.Fraction over the float coefficients as the program holds them:

  * every integer variable whose name begins "x_" or "y_" is enumerated within
    its bounds (the y ones in the outer loop, the x ones per connected part of
    what is left), assignments that violate a constraint over those variables
    alone are rejected;
  * every other variable is settled by propagating the constraints that have
    one unsettled variable left (an integer variable is settled when ceil(lo)
    == floor(hi), a continuous objective variable takes its lower bound); the
    solver asserts that nothing is left unsettled, that every objective
    coefficient is positive and that every constraint holds at the end.

It knows nothing of positions, fragments or bases beyond those two prefixes.
The programs are tiny at the shapes where a reading of them can go wrong (L <=
4, <= 3 fragments, <= 4 nucleosides), so minimize_error and evaluate run
unmodified and return the program's exact optimum.

Outputs (tests/golden/, read by tests/test_reference_programs.py and
tests/test_gpu_reference_programs.py; inputs in the terms of tests/_align_cases
.make_outcome and tests/_length_cases.make_cases, outputs recorded results only):
  program_filter.json.gz   per fragment: minimize_error exactly, removed or
                           kept by the reference's comparison, the exception
  program_final.json.gz    per spectrum (and per subset of its optional
                           fragments): the optimum, the y -> objective map,
                           the sequence evaluate returns
  program_length.json.gz   per candidate length the value and the validation,
                           per spectrum the length chosen
The filter records come from Predictor.filter_with_lp itself on a stub self
(dp_table only), one fragment at a time; the final ones from the instance of
prediction.py:160-166 and its evaluate; the length ones from determine_lp_score
and validate_sequence_length_by_mass per candidate in [lower, upper] with the
selection loop's rule applied here (the bounds are inputs:
compute_sequence_length_bound and a reference DynamicProgrammingTable are not
part of them).
Every instance carries tags, from its inputs and the reference's results only,
that say why a stage may leave it undecided: "band", "rowcap", "tie", "ends" (a
terminal fragment's end outside [0, L - 1]: the layer's SKIPPED), "raise" (the
reference raised), "subsets" (the optional subsets disagree on the sequence),
"infeasible" (length program: -1 is returned because a program that was
built has no feasible point).  At least two thirds of each family carry none.

Usage:  python tests/golden/make_program_golden.py
"""
import gzip
import itertools
import json
import math
import os
import sys
import types
from fractions import Fraction
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "standin"), "/root/reference"]


# ---------------------------------------------------------------------------
# the pulp stand-in: affine forms, and the exact enumeration behind solve()
# ---------------------------------------------------------------------------
def _q(v):
    if isinstance(v, Fraction):
        return v
    if isinstance(v, float):  # (np.float64 is a float)
        return Fraction(float(v))
    return Fraction(int(v))


class _Ops:
    __array_ufunc__ = None  # numpy scalars on the left defer to the reflected operators
    __hash__ = object.__hash__

    def __add__(self, o):
        a, b = _affine(self), _affine(o)
        t = dict(a.terms)
        for v, c in b.terms.items():
            t[v] = t.get(v, 0) + c
        return Affine(t, a.const + b.const)

    __radd__ = __add__

    def __neg__(self):
        return _affine(self) * -1

    def __sub__(self, o):
        return self + (-_affine(o))

    def __rsub__(self, o):
        return _affine(o) + (-_affine(self))

    def __mul__(self, o):
        a, b = _affine(self), _affine(o)
        if b.terms:
            a, b = b, a
        assert not b.terms, "a product of two variables"
        return Affine({v: c * b.const for v, c in a.terms.items()}, a.const * b.const)

    __rmul__ = __mul__

    def __le__(self, o):
        return Constraint(self - o, -1)

    def __ge__(self, o):
        return Constraint(self - o, 1)

    def __eq__(self, o):
        return Constraint(self - o, 0)


def _affine(x):
    if isinstance(x, Affine):
        return x
    if isinstance(x, LpVariable):
        return Affine({x: Fraction(1)}, Fraction(0))
    return Affine({}, _q(x))


class Affine(_Ops):
    def __init__(self, terms, const):
        self.terms, self.const = terms, const

    def exact(self):
        if any(v.varValue is None for v in self.terms):
            return None
        return self.const + sum(c * v.varValue for v, c in self.terms.items())

    def value(self):
        e = self.exact()
        return None if e is None else float(e)


class LpVariable(_Ops):
    _count = itertools.count()

    def __init__(self, name, lowBound=None, upBound=None, cat="Continuous"):
        self.name, self.cat, self.uid = name, cat, next(self._count)
        self.lo = None if lowBound is None else _q(lowBound)
        self.hi = None if upBound is None else _q(upBound)
        self.varValue = None

    def setInitialValue(self, v):
        self.varValue = _q(v)

    def fixValue(self):  # (as pulp: the bounds collapse to the initial value)
        if self.varValue is not None:
            self.lo = self.hi = self.varValue

    def value(self):
        return None if self.varValue is None else float(self.varValue)


class Constraint:
    def __init__(self, form, sense):
        self.form, self.sense = _affine(form), sense  # form (<=, ==, >=) 0


def lpSum(items):
    t, const = {}, Fraction(0)
    for x in items:
        a = _affine(x)
        const += a.const
        for v, c in a.terms.items():
            t[v] = t.get(v, 0) + c
    return Affine(t, const)


def _ok(s, sense):
    return s <= 0 if sense < 0 else s >= 0 if sense > 0 else s == 0


def _num(c):
    return int(c) if c.denominator == 1 else c


class Solved:
    """What solve() keeps for inspection."""
    optimum = None      # Fraction, None: infeasible
    ymap = None         # {names of the y variables at 1, in creation order: minimal objective}
    minimisers = None   # the keys of ymap that attain the optimum
    n_outer = 0         # assignments of the outer (y) variables that pass their own constraints


LAST = Solved()


class LpProblem:
    def __init__(self, name="", sense=1):
        assert sense == 1, "a minimisation"
        self.objective, self.constraints, self.solved = None, [], None

    def __iadd__(self, other):
        if isinstance(other, Constraint):
            self.constraints.append(other)
        else:
            self.objective = _affine(other)
        return self

    def solve(self, solver=None):
        global LAST
        LAST = self.solved = _solve(self.objective, self.constraints)
        return 1 if LAST.optimum is not None else -1


def getSolver(*a, **k):
    return "exact"


def _solve(objective, constraints):
    out = Solved()
    V = sorted({v for c in constraints for v in c.form.terms} | set(objective.terms), key=lambda v: v.uid)
    at = {v: i for i, v in enumerate(V)}
    n = len(V)
    integer = [v.cat == "Integer" for v in V]
    lo0, hi0 = [v.lo for v in V], [v.hi for v in V]
    obj = [0] * n
    for v, c in objective.terms.items():
        assert c > 0, "an objective coefficient that is not positive"
        obj[at[v]] = _num(c)
    cons = [([(at[v], _num(c)) for v, c in k.form.terms.items() if c != 0], _num(k.form.const), k.sense) for k in constraints]
    enumerated = [integer[i] and V[i].name.startswith(("x_", "y_")) for i in range(n)]
    for i in range(n):
        if enumerated[i]:
            assert lo0[i] is not None and hi0[i] is not None, "an enumerated variable without bounds"
    val = [None] * n
    for i in range(n):
        if lo0[i] is not None and lo0[i] == hi0[i]:
            val[i] = _num(lo0[i])
    free = [i for i in range(n) if val[i] is None]
    outer = [i for i in free if enumerated[i] and V[i].name.startswith("y_")]
    inner = [i for i in free if enumerated[i] and not V[i].name.startswith("y_")]
    rest = [i for i in free if not enumerated[i]]
    outer_set = set(outer)

    # the parts of what is left once the outer variables are settled
    parent = {i: i for i in inner + rest}

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    outer_checks, const_checks = [], []
    for k in cons:
        mine = [i for i, _ in k[0] if i in parent]
        if mine:
            for i in mine[1:]:
                parent[find(i)] = find(mine[0])
        elif any(i in outer_set for i, _ in k[0]):
            outer_checks.append(k)
        else:
            const_checks.append(k)
    parts = {}
    for i in inner + rest:
        parts.setdefault(find(i), {"inner": [], "rest": [], "cons": []})["inner" if enumerated[i] else "rest"].append(i)
    for k in cons:
        mine = [i for i, _ in k[0] if i in parent]
        if mine:
            parts[find(mine[0])]["cons"].append(k)
    parts = list(parts.values())
    rest_set = set(rest)
    for p in parts:
        p["pure"] = [k for k in p["cons"] if not any(i in rest_set for i, _ in k[0])]
        p["mixed"] = [k for k in p["cons"] if any(i in rest_set for i, _ in k[0])]

    def total(k):
        return k[1] + sum(c * val[i] for i, c in k[0])

    def enumerate_over(order, checks):
        """Every assignment of `order` within the bounds that passes `checks`, each checked as soon as its last
        variable is set (its other variables are settled already); val holds it while the caller looks."""
        pos = {i: d for d, i in enumerate(order)}
        due = [[] for _ in order]
        for k in checks:
            due[max(pos[i] for i, _ in k[0] if i in pos)].append(k)

        def go(d):
            if d == len(order):
                yield
                return
            i = order[d]
            for x in range(math.ceil(lo0[i]), math.floor(hi0[i]) + 1):
                val[i] = x
                if all(_ok(total(k), k[2]) for k in due[d]):
                    yield from go(d + 1)
            val[i] = None

        yield from go(0)

    def settle(p):
        """The rest variables of part p by propagation; False where the assignment is infeasible."""
        lo, hi = {i: lo0[i] for i in p["rest"]}, {i: hi0[i] for i in p["rest"]}
        changed = True
        while changed:
            changed = False
            for k in p["mixed"]:
                open_ = [(i, c) for i, c in k[0] if val[i] is None]
                if len(open_) != 1:
                    continue
                (u, c), = open_
                bound = Fraction(-(k[1] + sum(cc * val[i] for i, cc in k[0] if i != u))) / c  # c u (sense) c bound
                upper = k[2] == 0 or (k[2] < 0) == (c > 0)
                lower = k[2] == 0 or (k[2] > 0) == (c > 0)
                if upper and (hi[u] is None or bound < hi[u]):
                    hi[u] = bound
                if lower and (lo[u] is None or bound > lo[u]):
                    lo[u] = bound
                if integer[u] and lo[u] is not None and hi[u] is not None:
                    a, b = math.ceil(lo[u]), math.floor(hi[u])
                    if a > b:
                        return False
                    if a == b:
                        val[u], changed = a, True
        for u in p["rest"]:
            if val[u] is None:
                assert not integer[u] and obj[u] and lo[u] is not None, f"{V[u].name} is left unsettled"
                if hi[u] is not None and lo[u] > hi[u]:
                    return False
                val[u] = _num(lo[u])
        return all(_ok(total(k), k[2]) for k in p["mixed"])

    def best_of(p):
        """(min share of the objective, its first minimiser as {variable: value}) of part p, or None."""
        best = None
        for _ in enumerate_over(p["inner"], p["pure"]):
            if settle(p):
                share = sum(obj[i] * val[i] for i in p["inner"] + p["rest"])
                if best is None or share < best[0]:
                    best = (share, {i: val[i] for i in p["inner"] + p["rest"]})
            for u in p["rest"]:
                val[u] = None
        return best

    out.ymap, witness = {}, {}
    if all(_ok(total(k), k[2]) for k in const_checks):
        fixed_share = sum(obj[i] * val[i] for i in range(n) if val[i] is not None and i not in parent and i not in outer_set)
        for _ in enumerate_over(outer, outer_checks):
            out.n_outer += 1
            got = [best_of(p) for p in parts]
            if any(g is None for g in got):
                continue
            value = objective.const + fixed_share + sum(obj[i] * val[i] for i in outer) + sum(g[0] for g in got)
            key = tuple(V[i].name for i in range(n) if V[i].name.startswith("y_") and val[i] == 1)
            if key not in out.ymap or value < out.ymap[key]:
                out.ymap[key] = Fraction(value)
                witness[key] = ({i: val[i] for i in outer}, [g[1] for g in got])
    if out.ymap:
        out.optimum = min(out.ymap.values())
        out.minimisers = [k for k, v in out.ymap.items() if v == out.optimum]
        first, others = witness[out.minimisers[0]]
        for i in range(n):
            if i in parent or i in outer_set:
                val[i] = None
        for d in [first] + others:
            for i, x in d.items():
                val[i] = x
        assert all(x is not None for x in val)
        assert all(_ok(total(k), k[2]) for k in cons), "the minimiser violates a constraint"
        assert objective.const + sum(obj[i] * val[i] for i in range(n)) == out.optimum
        for i, v in enumerate(V):
            v.varValue = Fraction(val[i])
    else:
        out.minimisers = []
        for v in V:
            v.varValue = None
    return out


pulp = types.ModuleType("pulp")
pulp.__dict__.update(LpProblem=LpProblem, LpVariable=LpVariable, lpSum=lpSum, getSolver=getSolver, LpMinimize=1,
                     LpMaximize=-1, LpInteger="Integer", LpContinuous="Continuous", LpBinary="Binary")
sys.modules["pulp"] = pulp

import typing  # noqa: E402

if not hasattr(typing, "Self"):  # Python 3.10: prediction.py:3 imports it for annotations only
    typing.Self = typing.Any

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402  (behind the polars stand-in)
import polars as pl  # noqa: E402  (the stand-in)

import spectrseqtools.linear_program as RLP  # noqa: E402
import spectrseqtools.prediction as RP  # noqa: E402
import spectrseqtools.skeleton_building as RSB  # noqa: E402

PRECISION, TOLERANCE, FIX = 1e-3, 10e-6, 65536
UNIT = Fraction(PRECISION)            # one precision unit, as the float the programs multiply by
PARAMS = {"fixed": {}, "timeLimit(short)": 1, "timeLimit(long)": 1}
BREAKAGE = {0: "c/y_c/y", 1: "START_c/y", 2: "c/y_END", 3: "START_END"}


def frac(x):
    return None if x is None else f"{x.numerator}/{x.denominator}"


def ref_table(rows, alpha, rates, seq_rate, **seq):
    """The reference's dp_table fields over row 0 and the rows of alpha."""
    masses = [SimpleNamespace(names=list(rows[r][0]), mass=rows[r][1], modification_rate=rates[r],
                              is_modification=rows[r][0][0] not in RLP.UNMODIFIED_BASES) for r in [0] + sorted(alpha)]
    return SimpleNamespace(masses=masses, precision=PRECISION, tolerance=TOLERANCE,
                           seq=SimpleNamespace(modification_rate=seq_rate, **seq))


def skeleton_names(rows, pos):
    return [{rows[r][0][0] for r in p} for p in pos]


def frame(frags):
    """(code, su, obs, min_end, max_end) tuples as the frame predict hands on."""
    cols = {"index": list(range(len(frags))), "orig_index": list(range(len(frags))),
            "breakage": [BREAKAGE[(f[0] >> 2) & 3] for f in frags], "standard_unit_mass": [float(f[1]) for f in frags],
            "observed_mass": [float(f[2]) for f in frags], "min_end": [int(f[3]) for f in frags],
            "max_end": [int(f[4]) for f in frags], "intensity": [1.0] * len(frags)}
    return pl.DataFrame(cols)


def coefficient_effect(rows, alpha, L, n_frags):
    """The most the float coefficients mass * precision can move an objective against mass / 1000 exactly."""
    worst = max(abs(Fraction(float(rows[r][1] * PRECISION)) - Fraction(rows[r][1], 1000)) for r in alpha)
    return worst * L * n_frags


def row_caps_bind(spec):
    """Some row of the program may not fill every position: ceil(rate * L) < L."""
    return any(int(np.ceil(spec["rates"][r] * spec["L"])) < spec["L"] for r in spec["alpha"])


# ---------------------------------------------------------------------------
# filter programs
# ---------------------------------------------------------------------------
def filter_record(rows, spec, frag):
    dp = ref_table(rows, spec["alpha"], spec["rates"], spec["seq_rate"])
    stub = SimpleNamespace(dp_table=dp)
    rec = {"value": None, "float": None, "removed": None, "raised": None, "no_y": None, "tags": []}
    L = spec["L"]
    terminal = ((frag[0] >> 2) & 3) in (1, 2)
    try:
        kept = RP.Predictor.filter_with_lp(stub, fragments=frame([frag]), skeleton_seq=skeleton_names(rows, spec["pos"]),
                                           solver_params=dict(PARAMS, fixed={}))
    except Exception as e:  # noqa: BLE001  (the type is the record)
        rec["raised"] = type(e).__name__
        rec["tags"].append("raise")
    else:
        rec["removed"] = len(kept) == 0
        rec["no_y"] = LAST.n_outer == 0 and LAST.optimum is None
        if LAST.optimum is None:
            rec["float"] = "inf"
        else:
            rec["value"], rec["float"] = frac(LAST.optimum), float(LAST.optimum)
            assert coefficient_effect(rows, spec["alpha"], L, 1) < UNIT / FIX
            # keep mode decides by W_in = floor(q) - 1 and W = ceil(q) around the rounded target: it may leave open
            # what lies within 1.5 units of the threshold
            if abs(LAST.optimum - Fraction(TOLERANCE * frag[2])) <= Fraction(3, 2) * UNIT:
                rec["tags"].append("band")
    if terminal and not (0 <= frag[3] < L and 0 <= frag[4] < L):
        rec["tags"].append("ends")
    if row_caps_bind(spec):
        rec["tags"].append("rowcap")
    return rec


# ---------------------------------------------------------------------------
# final programs
# ---------------------------------------------------------------------------
def final_record(rows, spec, frags):
    """evaluate over `frags` (prediction.py:160-166)."""
    dp = ref_table(rows, spec["alpha"], spec["rates"], spec["seq_rate"])
    rec = {"optimum": None, "float": None, "ymap": None, "n_min": 0, "gap": None, "seq": None, "raised": None,
           "infeasible": None}
    try:
        inst = RLP.LinearProgramInstance(fragments=frame(frags), dp_table=dp, skeleton_seq=skeleton_names(rows, spec["pos"]))
    except Exception as e:  # noqa: BLE001
        rec["raised"] = type(e).__name__
        return rec
    try:
        seq, _ = inst.evaluate(dict(PARAMS, fixed={}))
    except Exception as e:  # noqa: BLE001  (an infeasible program: evaluate compares None)
        rec["raised"], seq = type(e).__name__, None
    got = inst.problem.solved
    rec["infeasible"] = got.optimum is None
    if got.optimum is None:
        return rec
    assert coefficient_effect(rows, spec["alpha"], spec["L"], len(frags)) < UNIT / FIX
    assert len(got.ymap) <= 256

    def names(key):  # "y_<position>,<name>" of the y variables at 1: the names by position
        return [k.split("_", 1)[1].split(",", 1)[1] for k in sorted(key, key=lambda k: int(k[2:].split(",")[0]))]

    rec["optimum"], rec["float"] = frac(got.optimum), float(got.optimum)
    rec["ymap"] = [[names(k), frac(v)] for k, v in got.ymap.items()]
    rec["n_min"] = len(got.minimisers)
    above = [v for v in got.ymap.values() if v > got.optimum]
    rec["gap"] = frac(min(above) - got.optimum) if above else None
    if len(got.minimisers) == 1:
        assert seq == names(got.minimisers[0]), (seq, got.minimisers)
        rec["seq"] = seq
    return rec


def final_instance(rows, spec):
    use = spec.get("use") or [1] * len(spec["frags"])
    required = [f for f, u in zip(spec["frags"], use) if u == 1]
    optional = [j for j, u in enumerate(use) if u == 2]
    assert len(optional) <= 2
    subsets = []
    for k in range(len(optional) + 1):
        for sub in itertools.combinations(optional, k):
            chosen = [f for j, (f, u) in enumerate(zip(spec["frags"], use)) if u == 1 or j in sub]
            subsets.append(dict(final_record(rows, spec, chosen), subset=list(sub), n_used=len(chosen)))
    tags = set()
    for rec in subsets:
        if rec["optimum"] is None:
            continue
        if rec["n_min"] != 1:
            tags.add("tie")
        elif rec["gap"] is not None and Fraction(rec["gap"]) < Fraction(FIX // 2 + 2 * (len(spec["frags"]) + 1), FIX) * UNIT:
            tags.add("band")  # final_decisions asks for half a unit, its own rounding moves a gap by < 2 (n + 1) / 65536
    if len({json.dumps(r["seq"]) for r in subsets}) > 1 or len({r["infeasible"] for r in subsets}) > 1:
        tags.add("subsets")
    if row_caps_bind(spec):
        tags.add("rowcap")
    L = spec["L"]
    if any(u and ((f[0] >> 2) & 3) in (1, 2) and not (0 <= f[3] < L and 0 <= f[4] < L) for f, u in zip(spec["frags"], use)):
        tags.add("ends")
    if any(r["raised"] and r["infeasible"] is None for r in subsets):
        tags.add("raise")
    del required
    return {"subsets": subsets, "tags": sorted(tags)}


# ---------------------------------------------------------------------------
# length programs
# ---------------------------------------------------------------------------
def length_record(rows, spec):
    """The selection loop of select_sequence_length_with_lp (skeleton_building.py:226-252) over the candidates
    [lower, upper], with the reference's own determine_lp_score, combine_skeleton_sequences and
    validate_sequence_length_by_mass; value < best_val and valid is the loop's rule."""
    global LAST
    dp = ref_table(rows, spec["alpha"], spec["rates"], spec["seq_rate"], su_mass=spec["su_mass"], max_len=spec["M"])
    stub = SimpleNamespace(dp_table=dp)
    start_sk = skeleton_names(rows, spec["start"])
    end_sk = skeleton_names(rows, spec["end"])
    nuc = {m.names[0]: m.mass * dp.precision for m in dp.masses[1:]}

    def side(bit):
        fr = [(k, f) for k, f in enumerate(spec["frags"]) if f[0] & bit]
        cols = {"index": [k for k, _ in fr], "breakage": [BREAKAGE[(f[0] >> 2) & 3] for _, f in fr],
                "standard_unit_mass": [float(f[1]) for _, f in fr], "min_end": [int(f[2]) for _, f in fr],
                "max_end": [int(f[3]) for _, f in fr]}
        # (typed columns: an empty walk's frame must not turn the other walk's integer ends into floats in pl.concat)
        return pl.DataFrame(pd.DataFrame(cols).astype({"index": "int64", "breakage": "object", "standard_unit_mass":
                                                       "float64", "min_end": "int64", "max_end": "int64"}))

    start, end = side(4), side(8)
    best_len, best_val, cands = -1, math.inf, []
    for c in range(spec["lower"], spec["upper"] + 1):
        LAST = Solved()
        seq = RSB.combine_skeleton_sequences(seq_len=c, start_skeleton=start_sk, end_skeleton=end_sk)
        value = RSB.SkeletonBuilder.determine_lp_score(stub, start_fragments=start.clone(), end_fragments=end.clone(),
                                                      skeleton_seq=seq, solver_params=dict(PARAMS, fixed={}))
        valid = bool(RSB.SkeletonBuilder.validate_sequence_length_by_mass(
            stub, start_skeleton=start_sk[:c], end_skeleton=end_sk[len(end_sk) - c:], nuc_masses=nuc))
        solved = LAST.ymap is not None  # the constructor did not raise: the solve ran
        rec = {"c": c, "raised": not solved, "valid": valid, "value": None, "float": "inf"}
        if solved and LAST.optimum is not None:
            rec["value"], rec["float"] = frac(LAST.optimum), float(LAST.optimum)
            assert value == float(LAST.optimum)
            assert coefficient_effect(rows, spec["alpha"], c, len(spec["frags"])) < UNIT / FIX
        else:
            assert value == np.inf
        rec["no_y"] = solved and LAST.optimum is None and LAST.n_outer == 0
        cands.append(rec)
        if value < best_val and valid:
            best_val, best_len = value, c
    return {"cands": cands, "chosen": best_len}


def length_tags(spec, rec):
    tags = set()
    finite = sorted((Fraction(c["value"]), c["c"]) for c in rec["cands"] if c["valid"] and c["value"] is not None)
    if len(finite) > 1:
        gap = finite[1][0] - finite[0][0]
        if gap == 0:
            tags.add("tie")
        elif gap < Fraction(FIX // 2 + 2 * (len(spec["frags"]) + 1), FIX) * UNIT:
            tags.add("band")
    if any(int(np.ceil(spec["rates"][r] * c["c"])) < c["c"] for c in rec["cands"] for r in spec["alpha"]):
        tags.add("rowcap")
    if rec["chosen"] == -1 and any(c["valid"] and not c["raised"] for c in rec["cands"]):
        tags.add("infeasible")  # -1 through a program without a feasible point: length_decisions leaves that to the solver
    return sorted(tags)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
# (names, integer mass) per table row: one modified row of two names (the program's variables carry the first
# only), A + m1A == C + C, A + G == C + C + 1, and U, whose rate is 0 in every instance (its cap is 0 at every length)
ROWS = [[["-"], 0], [["A"], 300000], [["C"], 300003], [["m1A", "m6A"], 300006], [["G"], 300007], [["U"], 300010]]
A, C, M1A, G, U = 1, 2, 3, 4, 5
MASS = [r[1] for r in ROWS]
RATES = [0.0, 1.0, 1.0, 1.0, 1.0, 0.0]
INTERNAL, START, END, START_END = 0, 1 | 4, 2 | 8, 3 | 12  # tests/_align_cases.code_of
OBS = 350.0  # tolerance * obs / precision == 3.5: W == 4, W_in == 2


def su(units):
    return float(units) * PRECISION


def spectrum(pos, frags=(), alpha=(A, C, M1A, G), rates=None, seq_rate=1.0, **more):
    rates = list(RATES) if rates is None else [rates.get(r, RATES[r]) for r in range(len(ROWS))]
    return dict({"L": len(pos), "pos": [list(p) for p in pos], "alpha": list(alpha), "rates": rates,
                 "seq_rate": seq_rate, "frags": [list(f) for f in frags]}, **more)


def total(y):
    return sum(MASS[r] for r in y)


def ladder(pos, alpha, deltas, obs):
    """The four classes at the sums the first rows place on a window, moved by `deltas` units."""
    L = len(pos)
    y = [(p or list(alpha))[0] for p in pos]
    r, l = max(0, L - 2), min(1, L - 1)
    out = []
    for d in deltas:
        out += [[INTERNAL, su(total(y[l:]) + d), obs, 0, 0], [START, su(total(y[:r + 1]) + d), obs, r, r],
                [END, su(total(y[l:]) + d), obs, l, l], [START_END, su(total(y) + d), obs, 0, 0]]
    return out


def filter_specs():
    specs = []
    skeletons = [([[A], [C], [A, G]], (A, C, M1A, G)), ([[A, C], [], [M1A]], (A, C, M1A)),
                 ([[C, G], [A, M1A]], (A, C, M1A, G)), ([[A], [C, M1A], [G], [A, C]], (A, C, M1A, G)),
                 ([[G]], (A, C, G))]
    for pos, alpha in skeletons:
        # exact, one unit off, far; then one unit inside and outside W_in / W, and the threshold from both sides
        specs.append(spectrum(pos, ladder(pos, alpha, (0, 1, -1, 12, -12, 40), OBS), alpha))
        specs.append(spectrum(pos, ladder(pos, alpha, (0, -2, 8, 13, -14), 1000.0), alpha))
        specs.append(spectrum(pos, ladder(pos, alpha, (0, 5, -7, 15, 30, -30), 2000.0), alpha))
        specs.append(spectrum(pos, ladder(pos, alpha, (2, 3, 3.5 - 0.25, 3.5 + 0.25, -3.25, 5), OBS), alpha))
    # thresholds whose fraction is not one half: floor, ceil and the rounding of the target all differ
    pos, alpha = skeletons[0]
    specs.append(spectrum(pos, ladder(pos, alpha, (3.7, -3.7, 3.9, 4.4, 2.4), 380.0), alpha))
    specs.append(spectrum(pos, ladder(pos, alpha, (3.4, -3.4, 3.1, 2.6, 1.4), 320.0), alpha))
    # near zero: the empty interval (internal fragments), a negative mass, no window at all (obs 0: W == 0)
    pos, alpha = skeletons[0]
    specs.append(spectrum(pos, [[INTERNAL, su(d), obs, 0, 0] for d in (0, 0.3, -0.3, 1, 6, -6) for obs in (OBS, 0.0)]
                          + [[START_END, su(d), OBS, 0, 0] for d in (0, 0.3)], alpha))
    # every (min_end, max_end) in [-1, L + 1]^2 for the terminal classes at L == 3
    ends = range(-1, 5)
    specs.append(spectrum(pos, [[START, su(total([A, C])), OBS, mn, mx] for mn in ends for mx in ends], alpha, grid="START"))
    specs.append(spectrum(pos, [[END, su(total([C, A])), OBS, mn, mx] for mn in ends for mx in ends], alpha, grid="END"))
    # the universal cap: ceil(rate * L) of 0, 1 and L; a spectrum whose forced positions exceed it
    pos = [[A, M1A], [C, M1A], [A, G]]
    for rate in (0.0, 0.3, 1.0):
        frags = [[START_END, su(total(y)), OBS, 0, 0] for y in ([A, C, A], [M1A, C, A], [M1A, M1A, A], [M1A, M1A, G])]
        frags += [[START, su(total(y)), OBS, 1, 1] for y in ([M1A, M1A], [A, M1A], [A, C])]
        frags += [[INTERNAL, su(total(y)), OBS, 0, 0] for y in ([M1A], [M1A, M1A])]
        frags += [[END, su(total(y)), OBS, 1, 1] for y in ([M1A, A], [C, G])]
        specs.append(spectrum(pos, frags, seq_rate=rate))
    specs.append(spectrum([[M1A], [M1A], [A]], [[START_END, su(total([M1A, M1A, A])), OBS, 0, 0],
                                                [INTERNAL, su(total([M1A])), OBS, 0, 0]], seq_rate=0.3))
    # per-row caps: loose (ceil(0.67 * 3) == 3), binding (ceil(0.34 * 3) == 2 < n_A), a modified row capped below L
    # but not below the universal cap, singletons that break a cap, and U, which no position may take
    pos = [[A], [A, C], [A, C]]
    frags = [[START_END, su(total(y)), 100.0, 0, 0] for y in ([A, A, A], [A, A, C], [A, C, C])] + \
        [[START, su(total([A, A])), 100.0, 1, 1]]
    specs.append(spectrum(pos, frags, (A, C), rates={A: 0.67}))
    specs.append(spectrum(pos, frags, (A, C), rates={A: 0.34}))
    specs.append(spectrum([[A, M1A], [C, M1A], [M1A, G]], [[START_END, su(total(y)), OBS, 0, 0]
                                                           for y in ([M1A, M1A, G], [M1A, M1A, M1A], [A, C, G])],
                          rates={M1A: 0.5}, seq_rate=0.5))
    specs.append(spectrum([[A], [A], [A]], [[START_END, su(total([A, A, A])), OBS, 0, 0]], (A, C), rates={A: 0.34}))
    specs.append(spectrum([[A, U], [C], [A]], [[START_END, su(total(y)), OBS, 0, 0] for y in ([A, C, A], [U, C, A])],
                          (A, C, U)))
    # a pair and a singleton that name no row of the alphabet, a pair that names one
    for middle in ([M1A, U], [M1A], [C, M1A]):
        specs.append(spectrum([[A], middle, [C]], [[START_END, su(total([A, C, C])), OBS, 0, 0],
                                                   [START, su(total([A])), OBS, 0, 0], [INTERNAL, su(0), OBS, 0, 0]],
                              (A, C, G)))
    for s in specs:
        s["frags"].sort(key=lambda f: f[1])
    return specs


def pinned(rng, L, n_sets):
    """A spectrum whose fragments pin every position of a random y: START fragments at the prefix sums, the whole
    sequence, or END fragments at the suffix sums; the su a little off the sums."""
    rows = [A, C, M1A, G]
    pos = [sorted(rng.choice(rows, size=int(rng.integers(1, n_sets + 1)), replace=False).tolist()) for _ in range(L)]
    y = [int(rng.choice(p)) for p in pos]
    off = lambda: float(rng.choice([0.0, 0.1, -0.2]))  # noqa: E731
    frags = []
    for r in range(L):
        kind = int(rng.integers(0, 3))
        if r == L - 1 and kind:
            frags.append([START_END, su(total(y) + off()), OBS, 0, 0])
        elif kind == 0 or r == L - 1:
            frags.append([END, su(total(y[L - 1 - r:]) + off()), OBS, L - 1 - r, L - 1 - r])
        else:
            lo, hi = max(0, r - int(rng.integers(0, 2))), min(L - 1, r + int(rng.integers(0, 2)))
            frags.append([START, su(total(y[:r + 1]) + off()), OBS, lo, hi])
    return pos, y, frags


def final_specs():
    specs = []
    two = [[A, C], [C, G], [A]]  # sums 900003 (ACA), 900006 (CCA), 900007 (AGA), 900010 (CGA)
    whole = lambda u: [START_END, su(u), OBS, 0, 0]  # noqa: E731
    specs += [spectrum(two, [whole(900006)]),                      # unique, the next y one unit away
              spectrum(two, [whole(900006.5 + 3 / FIX)]),          # ... a few fixed-point units away
              spectrum(two, [whole(900006.5)]),                    # an exact tie
              spectrum([[A, C], [C, M1A]], [whole(600006)]),       # A + m1A == C + C: a tie ...
              spectrum([[A, C], [C, M1A]], [whole(600006)], seq_rate=0.0),  # ... that the universal cap decides
              spectrum([[A, M1A], [C, M1A], [A, M1A]], [whole(900012)], seq_rate=0.3),  # one m1A at most: 2 units off
              spectrum([[A, C], [C, M1A], [A, G]], [[START, su(300000), OBS, 0, 1], [END, su(300007), OBS, 2, 2],
                                                    [INTERNAL, su(300003), OBS, 0, 0]]),
              spectrum([[A], [C, G]], [whole(600007), [INTERNAL, su(0.2), OBS, 0, 0]]),  # the empty interval is best
              spectrum([[A], [M1A, U]], [whole(600003)], (A, C, G)),                     # an infeasible position
              spectrum([[A], [M1A]], [whole(600003)], (A, C, G)),                        # ... a singleton: it raises
              spectrum([[M1A], [M1A], [A]], [whole(900012)], seq_rate=0.3),              # the forced rows break the cap
              spectrum([[A, C], [A, C], [M1A, G], [A]], [[START, su(600003), OBS, 0, 2], [END, su(600007), OBS, 3, 2],
                                                         whole(1200010)]),
              spectrum([[A, C], [], [G]], [whole(900013), [START, su(300003), OBS, 0, 0]], (A, C, G)),
              spectrum([[G]], [whole(300007)]), spectrum([[A, G]], [whole(300004)]),
              spectrum([[A, C], [A, C]], [whole(600003)]),          # AC and CA tie
              spectrum([[A, C], [A, C]], [whole(600003), [START, su(300000.25), OBS, 0, 0]]),
              spectrum([[A, C], [A, C], [A, C]], [whole(900003)], (A, C), rates={A: 0.34}),  # a binding row cap
              spectrum([[A, C], [A, C]], [whole(600003), [START, su(300000), OBS, -1, 0]]),   # an end out of range
              # a terminal fragment whose mass fits one position short of its only end: it may not move there
              spectrum([[A, C], [G]], [whole(600007), [START, su(300003), OBS, 1, 1]]),
              spectrum([[G], [A, C]], [whole(600007), [END, su(300003), OBS, 0, 0]]),
              spectrum([[A, C], [G], [A]], [whole(900008), [START, su(600010), OBS, 0, 0]]),
              spectrum([[A], [G], [A, C]], [whole(900008), [END, su(600010), OBS, 2, 2]])]
    # optional fragments: agreeing with the required ones, disagreeing, two of them, one that ties
    specs += [spectrum(two, [whole(900006), [START, su(300003), OBS, 0, 0]], use=[1, 2]),
              spectrum(two, [whole(900006), [START, su(300000), OBS, 0, 0]], use=[1, 2]),
              spectrum(two, [whole(900006), [START, su(300003), OBS, 0, 0], [END, su(300000), OBS, 2, 2]], use=[1, 2, 2]),
              spectrum(two, [whole(900006), [START, su(300002), OBS, 0, 0]], use=[1, 2]),
              spectrum(two, [[START, su(600006), OBS, 1, 1], whole(900006), [INTERNAL, su(300007), OBS, 0, 0]],
                       use=[2, 1, 2]),
              spectrum([[A, C], [C, G]], [[START, su(300003), OBS, 0, 0], whole(600010), [END, su(300007.4), OBS, 1, 1]],
                       use=[1, 1, 2])]
    rng = np.random.default_rng(7)
    for k in range(48):
        L = 1 + k % 4
        pos, _, frags = pinned(rng, L, 3)
        frags = frags[:3] if L < 4 else frags[1:]  # (at most three fragments: position 0 stays open at L == 4)
        use = None
        if k % 4 == 3:
            use = [2 if j == k % len(frags) else 1 for j in range(len(frags))]
        specs.append(spectrum(pos, frags, seq_rate=(1.0, 1.0, 0.5)[k % 3], **({"use": use} if use else {})))
    for s in specs:
        order = sorted(range(len(s["frags"])), key=lambda j: s["frags"][j][1])
        s["frags"] = [s["frags"][j] for j in order]
        if s.get("use"):
            s["use"] = [s["use"][j] for j in order]
    return specs


def length_spectrum(start, end, lower, upper, su_mass, frags, alpha=(A, C, M1A, G), rates=None, seq_rate=1.0, note=""):
    s = spectrum([], [], alpha, rates, seq_rate)
    del s["L"], s["pos"]
    frags = sorted(frags, key=lambda f: 0 if f[0] & 4 else 1)  # the START walk's rows, then the END walk's
    return dict(s, M=len(start), start=[list(p) for p in start], end=[list(p) for p in end], lower=lower, upper=upper,
                su_mass=su_mass, frags=[list(f) for f in frags], note=note)


def length_specs():
    """Fragments as (side bits 4 START / 8 END, su, raw min_end, raw max_end): the walks' ends, one past the last
    position (START) and counted from the 3' end (END)."""
    S, E, SE = 4, 8, 12
    acg = [[A], [C], [G]]
    none = [[], [], []]
    specs = [
        length_spectrum(acg, acg, 3, 3, su(900010), [[S, su(600003), 2, 2], [E, su(300007), 1, 1]], note="one length"),
        length_spectrum(acg, acg, 2, 3, su(900010), [[S, su(600003), 2, 2], [E, su(300007), 1, 1]],
                        note="the shorter length fails validation"),
        length_spectrum([[A], [C], []], [[], [A], []], 2, 3, su(600003), [[S, su(600003), 2, 2], [E, su(300007), 1, 1]],
                        note="both lengths valid (an empty union weighs nothing); the optimum is not the Jaccard length"),
        length_spectrum(acg, acg, 2, 3, su(900010), [[S, su(900010), 3, 3]], note="the constructor raises at c == 2"),
        length_spectrum([[A], [C], []], none, 2, 3, su(600003), [[S, su(300000), 1, 1]],
                        note="two candidates of equal value: the first wins"),
        length_spectrum(acg, none, 2, 3, su(900010), [[S, su(600003), 2, 2], [E, su(300003), 1, 1]],
                        note="the best candidate fails validation"),
        length_spectrum([[A], [C, G], [G]], none, 1, 3, su(900010), [[S, su(300000), 1, 1], [SE, su(900010), 0, 0]],
                        note="three candidates, one valid"),
        length_spectrum(acg, acg, 1, 2, su(900010), [[S, su(300000), 1, 1]], note="every candidate fails validation"),
        length_spectrum(acg, acg, 2, 3, su(900010), [[S, su(900010), 3, 3], [E, su(300007), 7, 7]],
                        note="every candidate raises or is invalid"),
        length_spectrum([[A, M1A], [M1A], []], none, 2, 3, su(600006), [[S, su(600012), 2, 2], [SE, su(900019), 0, 0]],
                        seq_rate=0.5, note="the universal cap differs by length: ceil(0.5 c)"),
        length_spectrum([[M1A], [M1A], []], none, 2, 3, su(600012), [[S, su(300006), 1, 1]], seq_rate=0.3,
                        note="the forced rows break the universal cap: no feasible point at either length"),
        length_spectrum([[A, C], [A, C], []], none, 2, 3, su(600003), [[SE, su(600003), 0, 0]], alpha=(A, C),
                        rates={A: 0.34}, note="a row cap that may bind"),
        length_spectrum([[A, C], [G], [A]], none, 3, 3, su(900007), [[S, su(300003), 2, 2], [SE, su(900007), 0, 0]],
                        note="a START fragment whose mass fits one position short of its only end"),
        length_spectrum([[A], [G], [A, C]], none, 3, 3, su(900007), [[E, su(300003), 2, 2], [SE, su(900007), 0, 0]],
                        note="an END fragment whose mass fits one position past its only start"),
        length_spectrum([[A], [C], []], none, 2, 3, su(600003), [[E, su(300004.5 + 0.25 / FIX), 1, 1]],
                        note="the later candidate is better by half a fixed-point unit"),
    ]
    rng = np.random.default_rng(11)
    rows = [A, C, M1A, G]
    for k in range(36):
        T = 2 + k % 3
        M = T + k % 2
        truth = [int(rng.choice(rows)) for _ in range(T)]
        extra = lambda r: sorted({r, int(rng.choice(rows))}) if rng.random() < 0.5 else [r]  # noqa: E731
        start = [extra(truth[i]) if i < T else [] for i in range(M)]
        end = [extra(truth[i - (M - T)]) if i >= M - T else [] for i in range(M)]
        frags = []
        for _ in range(int(rng.integers(1, 4))):
            kind, e = int(rng.integers(0, 3)), int(rng.integers(1, T + 1))
            off = float(rng.choice([0.0, 0.1, -0.2]))
            if kind == 0:
                frags.append([SE, su(total(truth) + off), 0, 0])
            elif kind == 1:
                frags.append([S, su(total(truth[:e]) + off), max(1, e - int(rng.integers(0, 2))), e])
            else:
                frags.append([E, su(total(truth[T - e:]) + off), e, e + int(rng.integers(0, 2))])
        lower = max(1, T - int(rng.integers(0, 2)))
        upper = min(M, lower + int(rng.integers(0, 3)))
        specs.append(length_spectrum(start, end, lower, upper, su(total(truth)), frags,
                                     seq_rate=(1.0, 1.0, 0.5)[k % 3], note="random"))
    return specs


# ---------------------------------------------------------------------------
def write(name, doc):
    path = os.path.join(HERE, name)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":"), sort_keys=True).encode())
    assert os.path.getsize(path) < 1 << 20
    return path


def shares(name, tagged):
    n, clean = len(tagged), sum(not t for t in tagged)
    kinds = {}
    for t in tagged:
        for k in t:
            kinds[k] = kinds.get(k, 0) + 1
    print(f"{name}: {n} instances, {clean} without a tag, tags {dict(sorted(kinds.items()))}")
    assert 3 * clean >= 2 * n, f"{name}: fewer than two thirds carry no tag"


def main():
    rows = ROWS
    filt = filter_specs()
    for s in filt:
        s["records"] = [filter_record(rows, s, f) for f in s["frags"]]
    shares("filter", [r["tags"] for s in filt for r in s["records"]])
    write("program_filter.json.gz", {"rows": rows, "precision": PRECISION, "tolerance": TOLERANCE, "specs": filt})

    fin = final_specs()
    for s in fin:
        s.update(final_instance(rows, s))
    shares("final", [s["tags"] for s in fin])
    write("program_final.json.gz", {"rows": rows, "precision": PRECISION, "tolerance": TOLERANCE, "specs": fin})

    ln = length_specs()
    for s in ln:
        s.update(length_record(rows, s))
        s["tags"] = length_tags(s, s)
    shares("length", [s["tags"] for s in ln])
    write("program_length.json.gz", {"rows": rows, "precision": PRECISION, "tolerance": TOLERANCE, "specs": ln})


if __name__ == "__main__":
    main()
