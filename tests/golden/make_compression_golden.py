#!/usr/bin/env python3
"""Golden vectors for the reference's queries at every table compression
(4, 8, 16 and 32 masses per packed word): is_valid_mass,
explain_mass_with_table (max_modifications 0, 2 and inf),
compute_sequence_length_bound (both directions) and, on the ordinary windows,
explain_mass_with_recursion (which reads the rows only) on a table of C, G and two
modifications (8U, 0C) with max_mass = 35 * max, built by the reference's own
set_up_bit_table at that compression.

TEST INFRASTRUCTURE -- runs only in the build container, with the REFERENCE
(read-only at /root/reference) imported unmodified through the pandas-backed
polars stand-in (tests/golden/standin, see make_golden.py); the dp object is
put together by hand as in make_raise_golden.py, with the compression set.

Mid-table answers cannot depend on the compression; these can: the table's
end (n_cols * C), its last packed word (mass_table.py:246 masks it with a
shift that depends on the column count and the word's dtype) and the cells
past max_mass.  So besides ~100 ordinary windows the query set holds, per
compression, windows ending at limit-1, limit and limit+1, windows that start
and end inside the last packed word, windows at limit-C and limit-C-1, windows
that contain max_mass and the cells past it, and windows around the reachable
masses nearest the end.  Thresholds are (q - 0.5) * precision, so that every
window is target +- q whatever the last bit of the division.

Output: tests/golden/compression_cases.json.gz (data only)
Usage:  python tests/golden/make_compression_golden.py
"""
import gzip
import hashlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "standin"), "/root/reference"]

import numpy as np  # noqa: E402

import spectrseqtools.masses as M  # noqa: E402
import spectrseqtools.mass_table as MT  # noqa: E402
import spectrseqtools.mass_explanation as ME  # noqa: E402

KEEP = ("C", "G", "8U", "0C")
MAX_LEN = 40
MOD_RATE = 0.5
BUDGETS = (0, 2, np.inf)
PREC = M.TOLERANCE


def make_dp(C):
    import polars as pl

    frame = M.EXPLANATION_MASSES.filter(pl.col("nucleoside").is_in(list(KEEP)))
    dp = object.__new__(MT.DynamicProgrammingTable)
    dp.compression_per_cell = C
    dp.tolerance = M.MATCHING_THRESHOLD
    dp.precision = PREC
    dp.seq = MT.SequenceInformation(max_len=MAX_LEN, su_mass=0.0, obs_mass=0.0, modification_rate=MOD_RATE)
    dp.masses = MT.initialize_nucleotide_masses(frame)
    dp._adapt_individual_modification_rates_by_universal_one()
    ints = [m.mass for m in dp.masses]
    dp.table = MT.set_up_bit_table(integer_masses=ints, max_mass=max(ints) * MT.MAX_SEQ_LENGTH, compression_rate=C)
    return dp


def rows_of(dp, names_set):
    idx = {}
    for i, x in enumerate(dp.masses):
        for n in ME.MASS_NAMES.get(x.mass, []):
            idx[n] = i
    return sorted(tuple(sorted(idx[n] for n in t)) for t in names_set)


def outcome(dp, fn):
    try:
        r = fn()
    except Exception as e:  # the reference's raises are results too
        return {"status": "raise", "error": type(e).__name__, "message": str(e)}
    if isinstance(r, ME.MassExplanations):
        r = None if r.explanations is None else [list(t) for t in rows_of(dp, r.explanations)]
    elif isinstance(r, (bool, np.bool_)):
        r = bool(r)
    else:
        r = int(r)
    return {"status": "ok", "result": r}


def windows(ints, limit, C, max_mass):
    """[(tag, lo, hi)] as quantised masses, hi - lo even."""
    rng = np.random.default_rng(C)
    w = np.array(ints[1:], dtype=np.int64)
    out = []
    for k in range(100):  # ordinary: sums of 1..12 rows, a little off, 1..81 masses wide
        s = int(w[rng.integers(0, len(w), int(rng.integers(1, 13)))].sum()) + int(rng.integers(-3, 4))
        hw = int(rng.integers(0, 41))
        out.append(("ordinary", s - hw, s + hw))
    for d in (-1, 0, 1):  # ending at limit-1, limit, limit+1
        for hw in (0, 1, 3, 40, 400):
            out.append((f"end{d:+d}", limit + d - 2 * hw, limit + d))
    for lo in range(limit - C, limit):  # inside the last packed word: every cell, and spans of it
        out.append(("last_word_cell", lo, lo))
    out += [("last_word_span", limit - C, limit - 2), ("last_word_span", limit - C + 1, limit - 1),
            ("last_word_span", limit - C + 1, limit - 3 if C > 4 else limit - C + 1)]
    for e in (limit - C - 1, limit - C):  # at the last word's edge
        for hw in (0, 1, 20):
            out.append(("last_word_edge", e - 2 * hw, e))
            out.append(("last_word_edge", e, e + 2 * hw))
    for hw in (0, 1, 2, (limit - 1 - max_mass) // 2, limit - max_mass, 100):  # max_mass and the cells past it
        out.append(("max_mass", max_mass - hw, max_mass + hw))
    for v in range(max_mass + 1, limit):
        out.append(("past_max_mass", v, v))
    # the reachable masses nearest the end (35..39 rows): alone, and in windows that cross it
    near = sorted({sum(c) for k in range(35, 40) for c in itertools.combinations_with_replacement(ints[1:], k)
                   if limit - 4000 <= sum(c) < limit + 200})
    for v in near[-40:]:
        out.append(("near_end", v, v))
        out.append(("near_end", v - 6, v + 6))
    out.append(("near_end_wide", limit - 4001, limit - 1))
    return out


def main():
    out = {"keep": list(KEEP), "max_len": MAX_LEN, "mod_rate": MOD_RATE, "tables": {}, "cases": {}}
    for C in (4, 8, 16, 32):
        dp = make_dp(C)
        ints = [int(m.mass) for m in dp.masses]
        max_mass = max(ints) * MT.MAX_SEQ_LENGTH
        limit = dp.table.shape[1] * C
        out["tolerance"], out["precision"] = dp.tolerance, dp.precision
        out["tables"][str(C)] = {
            "masses": ints, "is_mod": [bool(m.is_modification) for m in dp.masses],
            "rates": [float(m.modification_rate) for m in dp.masses],
            "caps": [round(MAX_LEN * m.modification_rate) for m in dp.masses],
            "max_mass": max_mass, "limit": limit, "shape": list(dp.table.shape), "dtype": str(dp.table.dtype),
            "sha256": hashlib.sha256(np.ascontiguousarray(dp.table).tobytes()).hexdigest(),
            "last_words": [int(x) for x in dp.table[:, -1]],
        }
        cases = []
        for tag, lo, hi in windows(ints, limit, C, max_mass):
            assert (hi - lo) % 2 == 0 and hi >= lo, (tag, lo, hi)
            target, q = (lo + hi) // 2, (hi - lo) // 2
            mass, thr = target * PREC, (q - 0.5) * PREC if q else 0.0
            assert int(round(mass / PREC, 0)) == target and int(np.ceil(thr / PREC)) == q
            rec = {"tag": tag, "lo": lo, "hi": hi, "mass": mass, "threshold": thr}
            rec["is_valid"] = outcome(dp, lambda: ME.is_valid_mass(mass, dp, threshold=thr))
            rec["explain"] = {("inf" if A == np.inf else str(A)): outcome(
                dp, lambda: ME.explain_mass_with_table(mass, dp, max_modifications=A, threshold=thr)) for A in BUDGETS}
            if tag == "ordinary":
                rec["recursion"] = {("inf" if A == np.inf else str(A)): outcome(
                    dp, lambda: ME.explain_mass_with_recursion(mass, dp, max_modifications=A, threshold=thr))
                    for A in BUDGETS}
            # the length bound's window: round(su / prec) +- ceil(tolerance * obs / prec)
            obs = thr / dp.tolerance
            assert int(np.ceil(dp.tolerance * obs / PREC)) == q
            dp.seq.su_mass, dp.seq.obs_mass = mass, obs
            rec["obs_mass"] = obs
            rec["length_bound"] = {d: outcome(dp, lambda: MT.compute_sequence_length_bound(dp, d))
                                   for d in ("lower", "upper")}
            cases.append(rec)
        out["cases"][str(C)] = cases
        n_raise = sum(c["is_valid"]["status"] == "raise" for c in cases)
        n_set = sum(bool(c["explain"]["inf"].get("result")) for c in cases)
        print(f"C = {C}: limit {limit}, {len(cases)} windows, {n_raise} is_valid raises, {n_set} with candidates")
    path = os.path.join(HERE, "compression_cases.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
