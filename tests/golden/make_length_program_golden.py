#!/usr/bin/env python3
"""Golden vectors for the shapes of the length program: what the REFERENCE's
own determine_lp_score preprocessing (skeleton_building.py:262-276) and
LinearProgramInstance._set_x (linear_program.py:74-102) leave of a terminal
fragment's x variables at a candidate length.

TEST INFRASTRUCTURE -- runs only in the build container, with the REFERENCE
(read-only at /root/reference) imported unmodified through the pandas-backed
polars stand-in (tests/golden/standin, see make_golden.py).  No solver exists
here and none is needed: this generator puts a RECORDING pulp stand-in of its
own into sys.modules before the reference loads (the one under standin/ refuses
every use and stays as it is).  Its LpVariable remembers setInitialValue /
fixValue, its LpProblem and lpSum are inert, and its getSolver raises a marker
exception, so that SkeletonBuilder.determine_lp_score runs unmodified up to the
solve: either the constructor raised (it returns np.inf) or the marker arrives
and the x variables' fixings are read.

Cases: every c in 1..6, every raw (min_end, max_end) in [0, 8]^2, the three
classes (a START walk's row, an END walk's row, a START_END row).

Output: tests/golden/length_program_setx.json.gz
  {"lengths": [1..6], "ends": [0..8], "classes": ["START", "END", "START_END"],
   "patterns": {class: [per c [per min_end [per max_end: null where the
                constructor raised, else a string of c characters '1' / '0' /
                '.' (fixed to 1, fixed to 0, free)]]]}}
Usage:  python tests/golden/make_length_program_golden.py
"""
import gzip
import json
import os
import sys
import types
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "standin"), "/root/reference"]

REGISTRY = {}


class _Inert:
    """An expression nobody evaluates."""

    def _same(self, *a, **k):
        return self

    __add__ = __radd__ = __sub__ = __rsub__ = __mul__ = __rmul__ = __neg__ = _same
    __le__ = __ge__ = __eq__ = __iadd__ = _same
    __hash__ = object.__hash__


class LpVariable(_Inert):
    def __init__(self, name, lowBound=None, upBound=None, cat=None):
        self.name, self.initial, self.fixed = name, None, None
        REGISTRY[name] = self

    def setInitialValue(self, v):
        self.initial = v

    def fixValue(self):
        self.fixed = self.initial


class LpProblem(_Inert):
    def __init__(self, *a, **k):
        pass


class Reached(Exception):
    """determine_lp_score got as far as the solve."""


def getSolver(*a, **k):
    raise Reached()


pulp = types.ModuleType("pulp")
pulp.__dict__.update(LpProblem=LpProblem, LpVariable=LpVariable, lpSum=lambda *a, **k: _Inert(), getSolver=getSolver,
                     LpMinimize=1, LpMaximize=-1, LpInteger="Integer", LpContinuous="Continuous", LpBinary="Binary")
sys.modules["pulp"] = pulp

import numpy as np  # noqa: E402
import polars as pl  # noqa: E402  (the stand-in)

import spectrseqtools.skeleton_building as SB  # noqa: E402

LENGTHS = list(range(1, 7))
ENDS = list(range(0, 9))
CLASSES = ("START", "END", "START_END")


def frame(rows):
    cols = ("index", "breakage", "standard_unit_mass", "min_end", "max_end")
    return pl.DataFrame({c: [r[k] for r in rows] for k, c in enumerate(cols)})


def pattern(cls, c, min_end, max_end):
    masses = [SimpleNamespace(names=["-"], mass=0, modification_rate=0.0),
              SimpleNamespace(names=["A"], mass=329053, modification_rate=1.0),
              SimpleNamespace(names=["C"], mass=305042, modification_rate=1.0)]
    dp_table = SimpleNamespace(masses=masses, precision=1e-3, seq=SimpleNamespace(modification_rate=0.5))
    row = (7, cls, 1000.0, min_end, max_end)
    other = (3, "END" if cls != "END" else "START", 500.0, 1, 1)  # the other walk's frame is never empty
    start = frame([row] if cls != "END" else [other])
    end = frame([row] if cls == "END" else [other])
    # the fragment under test is x_.,0 of a START frame and x_.,1 of an END frame
    j = 1 if cls == "END" else 0
    REGISTRY.clear()
    params = {"fixed": {}, "timeLimit(short)": 1}
    try:
        value = SB.SkeletonBuilder.determine_lp_score(SimpleNamespace(dp_table=dp_table), start_fragments=start,
                                                      end_fragments=end, skeleton_seq=[set() for _ in range(c)],
                                                      solver_params=params)
    except Reached:
        return "".join("." if REGISTRY[f"x_{i},{j}"].fixed is None else str(int(REGISTRY[f"x_{i},{j}"].fixed))
                       for i in range(c))
    assert value == np.inf, value
    return None


def main():
    out = {"lengths": LENGTHS, "ends": ENDS, "classes": list(CLASSES), "patterns": {}}
    for cls in CLASSES:
        out["patterns"][cls] = [[[pattern(cls, c, a, b) for b in ENDS] for a in ENDS] for c in LENGTHS]
    path = os.path.join(HERE, "length_program_setx.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    n = sum(p is None for cls in CLASSES for a in out["patterns"][cls] for b in a for p in b)
    print(f"{path}: {len(CLASSES) * len(LENGTHS) * len(ENDS) ** 2} cases, {n} raise")


if __name__ == "__main__":
    main()
