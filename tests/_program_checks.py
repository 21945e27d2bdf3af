"""What tests/test_reference_programs.py (CPU) and
tests/test_gpu_reference_programs.py share: the fixtures that
tests/golden/make_program_golden.py records from the reference's own programs
(program_filter / program_final / program_length.json.gz: every instance solved
exactly, no reading of ours in between), their spectra as the project's inputs,
and the implications each stage's result must satisfy against the recorded
results.  The check functions take a stage's result arrays, host model's or
device's alike, and compare them with the RECORDED values only.
TEST INFRASTRUCTURE."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import _align_cases as AC
import _length_cases as LC
from conftest import load_golden

FIX = 65536
DROP, KEEP, SOLVE = 0, 1, 2                      # alignment.LP_*
F_SOLVED, F_INFEASIBLE, F_SKIPPED = 1, 3, 4      # FINAL_*
TAKE = 1                                         # FINAL_TAKE
L_NONE, L_JACCARD, L_TAKE, L_SOLVE = 0, 1, 2, 3  # LENGTH_*


class Family:
    """One fixture: its table and its spectra, grouped into batches that share
    the per-row rates and the universal rate (one dp_table each)."""

    def __init__(self, name):
        doc = load_golden(name)
        self.rows, self.precision, self.tolerance = doc["rows"], doc["precision"], doc["tolerance"]
        self.specs = doc["specs"]
        self.row_mass = [r[1] for r in self.rows]
        self.row_names = [""] + [r[0][0] for r in self.rows[1:]]
        groups = {}
        for s in self.specs:
            groups.setdefault((tuple(s["rates"]), s["seq_rate"]), []).append(s)
        self.batches = list(groups.items())

    def table(self, rates, seq_rate, device_table=None):
        """The DynamicProgrammingTable fields the stages read: every row of the table with all its names."""
        masses = [SimpleNamespace(names=list(r[0]), mass=r[1], modification_rate=rate) for r, rate in zip(self.rows, rates)]
        return SimpleNamespace(masses=masses, precision=self.precision, tolerance=self.tolerance,
                               seq=SimpleNamespace(modification_rate=seq_rate), device_table=device_table,
                               row_mass=self.row_mass)

    def outcome(self, specs):
        o = AC.make_outcome([{"L": s["L"], "pos": [AC.mask(p) for p in s["pos"]], "alpha": AC.mask(s["alpha"] + [0]),
                              "frags": [tuple(f) for f in s["frags"]]} for s in specs], self.row_mass)
        o.row_names = list(self.row_names)
        return o

    def cases(self, specs):
        return LC.make_cases([dict(s, frags=[tuple(f) for f in s["frags"]]) for s in specs], self.row_mass,
                             row_names=list(self.row_names))


def caps_of(dp, o):
    """((row_mod, mod_cap), row_cap) by the project's own reading of the table (alignment.lp_caps / lp_row_caps)."""
    from spectrseqtools_amd import alignment

    return alignment.lp_caps(dp, o), alignment.lp_row_caps(dp, o)


# ---------------------------------------------------------------------------
# filter programs
# ---------------------------------------------------------------------------
ALIGN_VARIANTS = [dict(split=s, caps=c, keep=k) for s in (False, True)
                  for c, k in ((False, False), (True, False), (True, True))]


def check_filter(specs, al, decisions, variant, what):
    """An AlignOutcome and its lp_decisions over the batch `specs` against the
    records.  Returns the number of untagged fragments (all decided in keep mode)."""
    INFEASIBLE, SKIPPED = AC.INFEASIBLE, AC.SKIPPED
    k, clean = 0, 0
    for s in specs:
        for frag, rec in zip(s["frags"], s["records"]):
            at = (what, variant, s["pos"], frag, rec)
            st, dec = int(al.status[k]), int(decisions[k])
            removed = rec["removed"]
            if rec["raised"] is None:
                if not al.alignable[k] or dec == DROP:
                    assert removed, ("dropped, but the reference keeps it", at)
                if dec == KEEP:
                    assert not removed, ("kept, but the reference removes it", at)
                # no y at all: the layer's INFEASIBLE, except through a per-row cap, which the certificate leaves out
                if st == INFEASIBLE:
                    assert rec["no_y"], ("INFEASIBLE, but the program has a y", at)
                elif variant["caps"]:
                    assert not rec["no_y"] or "rowcap" in rec["tags"], ("a program without a y", at)
                else:  # (without the caps only a position that names no row of the alphabet leaves no y)
                    assert not any(p and not set(p) & set(s["alpha"]) for p in s["pos"]), ("an empty A_i", at)
            elif rec["raised"] == "KeyError":
                assert st == INFEASIBLE, ("a singleton that names no row", at)  # (predict fails there; we drop)
            else:
                assert rec["raised"] == "IndexError" and st == SKIPPED, ("the constructor raised", at)
            if st == SKIPPED:
                assert "ends" in rec["tags"], ("SKIPPED with both ends inside", at)
            if "ends" in rec["tags"]:
                assert st in (SKIPPED, INFEASIBLE) and (st == INFEASIBLE or dec == SOLVE), ("an end outside [0, L - 1]", at)
            if not rec["tags"]:
                clean += 1
                if variant["keep"]:
                    assert dec in (DROP, KEEP), ("an untagged fragment is left to the solver", at)
            k += 1
    assert k == len(al.status)
    return clean


# ---------------------------------------------------------------------------
# final programs
# ---------------------------------------------------------------------------
def final_use(specs, optional):
    """use per fragment of a batch: the recorded flags (1 required, 2 optional), or with optional == "all" / "none"
    the optional ones taken as required / left out."""
    out = []
    for s in specs:
        for u in s.get("use") or [1] * len(s["frags"]):
            out.append(u if optional == "robust" or u != 2 else (1 if optional == "all" else 0))
    return np.array(out, dtype=np.uint8)


def record_of(spec, optional):
    """The recorded program the enumeration's `best` belongs to: over the required fragments, or over all of them."""
    opt = [j for j, u in enumerate(spec.get("use") or []) if u == 2]
    want = opt if optional == "all" else []
    return next(r for r in spec["subsets"] if r["subset"] == want)


def check_final(fam, specs, o, fo, decisions, optional, what, ro_decisions=False):
    """A FinalOutcome (and final_decisions or robust_decisions) over the batch `specs` against the records.  Returns
    the number of untagged spectra (all TAKE, or INFEASIBLE where the program is)."""
    from spectrseqtools_amd import final_program as FP

    unit = Fraction(fam.precision) / FIX
    clean = 0
    for g, s in enumerate(specs):
        rec = record_of(s, optional)
        at = (what, optional, g, s["pos"], s["frags"], s.get("use"), rec["float"], s["tags"])
        st = int(fo.status[g])
        if "raise" in s["tags"]:
            assert st == F_INFEASIBLE, ("a singleton that names no row", at)
            continue
        if "ends" in s["tags"]:
            assert st == F_SKIPPED, ("an end outside [0, L - 1]", at)
            continue
        assert (st == F_INFEASIBLE) == bool(rec["infeasible"]) or "rowcap" in s["tags"], ("INFEASIBLE", at)
        if st == F_SOLVED:
            n_used = int(fo.n_used()[g])
            assert n_used >= rec["n_used"]
            got = Fraction(int(fo.best[g])) * unit
            assert abs(got - Fraction(rec["optimum"])) <= (rec["n_used"] + 1) * unit, ("best", at, float(got))
        if decisions[g] == TAKE:
            every = s["subsets"] if ro_decisions else [rec]
            names = FP.sequence_names(fo, o, g)
            for r in every:
                assert r["n_min"] == 1 and names == r["seq"], ("TAKE", at, names, r["subset"], r["seq"], r["n_min"])
        if not s["tags"]:
            clean += 1
            if rec["infeasible"]:
                assert st == F_INFEASIBLE and decisions[g] != TAKE, ("an infeasible program", at)
            else:
                assert decisions[g] == TAKE, ("an untagged spectrum is left to the solver", at, st)
    return clean


# ---------------------------------------------------------------------------
# length programs
# ---------------------------------------------------------------------------
def check_length(fam, specs, lo, decision, length, what):
    """A LengthOutcome and its length_decisions over the batch `specs` against the records."""
    unit = Fraction(fam.precision) / FIX
    clean, k = 0, 0
    for g, s in enumerate(specs):
        at = (what, g, s["note"], s["cands"], s["chosen"], s["tags"])
        assert int(lo.cand_off[g + 1]) - int(lo.cand_off[g]) == len(s["cands"]), at
        for c in s["cands"]:
            st = int(lo.status[k])
            assert int(lo.cand_len[k]) == c["c"]
            if c["valid"]:  # (an invalid candidate is INVALID before anything is looked at)
                assert (st == LC.RAISES) == c["raised"], ("RAISES", at, c, st)
            else:
                assert st == LC.INVALID, ("INVALID", at, c, st)
            if st == LC.SOLVED:
                got = Fraction(int(lo.best[k])) * unit
                assert c["value"] is not None and abs(got - Fraction(c["value"])) <= (len(s["frags"]) + 1) * unit, \
                    ("best", at, c, float(got))
            if st == LC.INFEASIBLE and "rowcap" not in s["tags"]:
                assert c["no_y"], ("INFEASIBLE, but the program has a y", at, c)
            k += 1
        d = int(decision[g])
        if d == L_TAKE:
            assert int(length[g]) == s["chosen"], ("TAKE", at, int(length[g]))
        if d in (L_NONE, L_JACCARD):
            assert s["chosen"] == -1, ("NONE / JACCARD, but the reference chooses a length", at)
        if not s["tags"]:
            clean += 1
            assert d in (L_TAKE, L_NONE, L_JACCARD), ("an untagged spectrum is left to the solver", at, d)
            assert (d in (L_NONE, L_JACCARD)) == (s["chosen"] == -1), at
    assert k == len(lo.status)
    return clean


def float_effect_is_small(fam):
    """The one extra unit of the bounds above: mass * precision in f64 against mass / 1000, over four positions and
    three fragments."""
    worst = max(abs(Fraction(float(m * fam.precision)) - Fraction(m, 1000)) for m in fam.row_mass)
    return worst * 12 < Fraction(fam.precision) / FIX and math.isclose(fam.precision, 1e-3)
