"""BatchOutcome (pipeline_device.run_batch's result) on hand-built outcomes:
concat / take keep the spectra's order and rebase the offsets, pack / unpack
round-trips and refuses other buffers, fragments() / skeleton_seq() /
alphabet_masses() read the dense arrays back per spectrum; the hand-off
entry points are declared and exported.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO
from spectrseqtools_amd import _native
from spectrseqtools_amd import pipeline_device as PD

BRK = ["START_c/y", "c/y_END", "START_END", "c/y_c/y"]
ROWS = ["", "A", "C", "G", "U", "m6A"] + [f"x{r}" for r in range(6, 70)]  # 70 rows: masks use both words
MASS = [0] + [1000 + 7 * r for r in range(1, 70)]


def mask(*rows):
    m = [0, 0]
    for r in rows:
        m[r >> 6] |= 1 << (r & 63)
    return m


def code(name, singleton=False):
    return BRK.index(name) | ("START" in name) << 2 | ("END" in name) << 3 | int(singleton) << 4


def outcome(spectra):
    """spectra: per spectrum None (default) or dict(route, reason, alpha rows,
    skeleton = list of row lists, frags = list of (index, breakage, singleton,
    su, obs, min_end, max_end))."""
    S = len(spectra)
    pos_off, frag_off, skel, fr = [0], [0], [], []
    for s in spectra:
        skel += [mask(*p) for p in s["skeleton"]]
        fr += s["frags"]
        pos_off.append(len(skel))
        frag_off.append(len(fr))
    return PD.BatchOutcome(
        default=[s["default"] for s in spectra], route=[s["route"] for s in spectra],
        reason=[s["reason"] for s in spectra], alpha=np.array([mask(*s["alpha"]) for s in spectra],
                                                              dtype=np.uint64).reshape(S, 2),
        seq_len=[len(s["skeleton"]) for s in spectra], pos_off=pos_off,
        skeleton=np.array(skel, dtype=np.uint64).reshape(-1, 2), frag_off=frag_off,
        frag_index=[f[0] for f in fr], frag_code=[code(f[1], f[2]) for f in fr], frag_su=[f[3] for f in fr],
        frag_obs=[f[4] for f in fr], frag_min_end=[f[5] for f in fr], frag_max_end=[f[6] for f in fr],
        breakage_names=BRK, row_names=ROWS, row_mass=MASS)


DEFAULT = dict(default=True, route=0, reason=0, alpha=[], skeleton=[], frags=[])
SPEC_A = dict(default=False, route=0, reason=0, alpha=[1, 2, 3, 4, 5], skeleton=[[1], [2, 5], [3]],
              frags=[(0, "START_c/y", False, 329.05, 884.18, 0, 0), (3, "c/y_c/y", True, 634.1, 1089.2, 0, 2),
                     (7, "c/y_END", False, 958.15, 1413.3, 1, 2)])
SPEC_B = dict(default=False, route=1, reason=PD.REASON_PEAKS, alpha=[1, 2, 3, 4, 69], skeleton=[[4], [69, 1]],
              frags=[(2, "START_END", False, 650.5, 1205.6, 1, 1)])
SPEC_C = dict(default=False, route=0, reason=0, alpha=[1, 2, 3, 4], skeleton=[[2]], frags=[])
SPEC_D = dict(default=False, route=1, reason=PD.REASON_WALK | PD.REASON_MAX_LEN, alpha=[1, 2, 3, 4, 64],
              skeleton=[[64], [1], [2], [3]],
              frags=[(1, "START_c/y", True, 305.04, 860.17, 0, 0), (5, "c/y_END", False, 1200.0, 1655.1, 2, 3)])


@pytest.fixture()
def two():
    return outcome([SPEC_A, DEFAULT, SPEC_B]), outcome([SPEC_C, SPEC_D])


def check_spectrum(o, g, s):
    assert bool(o.default[g]) == s["default"] and int(o.route[g]) == s["route"] and int(o.reason[g]) == s["reason"]
    assert o.skeleton_seq(g) == [sorted(ROWS[r] for r in p) for p in s["skeleton"]]
    assert int(o.seq_len[g]) == len(s["skeleton"])
    assert o.alphabet_masses(g) == [0] + [MASS[r] for r in sorted(s["alpha"])]
    f = o.fragments(g)
    assert f.columns == ["index", "standard_unit_mass", "observed_mass", "breakage", "is_singleton", "min_end",
                         "max_end"]
    want = [(x[0], x[3], x[4], x[1], x[2], x[5], x[6]) for x in s["frags"]]
    assert f.rows() == want if want else len(f) == 0


def test_accessors(two):
    a, b = two
    for g, s in enumerate([SPEC_A, DEFAULT, SPEC_B]):
        check_spectrum(a, g, s)
    for g, s in enumerate([SPEC_C, SPEC_D]):
        check_spectrum(b, g, s)
    assert len(a) == 3 and len(b) == 2
    assert int(a.frag_off[2]) == int(a.frag_off[1]) and int(a.pos_off[2]) == int(a.pos_off[1])  # the default one


def test_concat_keeps_order_and_rebases(two):
    a, b = two
    c = PD.BatchOutcome.concat([a, b])
    assert len(c) == 5
    assert c.pos_off.tolist() == [0, 3, 3, 5, 6, 10] and c.frag_off.tolist() == [0, 3, 3, 4, 4, 6]
    for g, s in enumerate([SPEC_A, DEFAULT, SPEC_B, SPEC_C, SPEC_D]):
        check_spectrum(c, g, s)
    assert c.equals(outcome([SPEC_A, DEFAULT, SPEC_B, SPEC_C, SPEC_D]))
    assert PD.BatchOutcome.concat([a]).equals(a)
    # the splice run_batch does: pieces concatenated, then put in the batch's order
    t = c.take([4, 1, 0, 3, 2])
    assert t.equals(outcome([SPEC_D, DEFAULT, SPEC_A, SPEC_C, SPEC_B]))
    assert not t.equals(c) and t.equals(c.take([4, 1, 0, 3, 2]))
    other = outcome([SPEC_C])
    other.breakage_names = BRK[::-1]
    with pytest.raises(ValueError):
        PD.BatchOutcome.concat([a, other])


def test_pack_unpack_round_trip(two):
    for x in two + (PD.BatchOutcome.concat(two), outcome([]), outcome([DEFAULT])):
        buf = x.pack()
        assert buf.dtype == np.uint8 and buf.ndim == 1
        y = PD.BatchOutcome.unpack(buf)
        for k in PD.BatchOutcome.array_fields():
            got, want = getattr(y, k), getattr(x, k)
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), k
        assert y.breakage_names == x.breakage_names and y.row_names == x.row_names
        assert y.equals(x)


def test_unpack_refuses_other_buffers(two):
    buf = two[0].pack()
    for bad in (buf[:-1], buf[:200], buf[:64], buf[:10], np.concatenate([buf, np.zeros(8, np.uint8)])):
        with pytest.raises(ValueError):
            PD.BatchOutcome.unpack(bad)
    wrong = buf.copy()
    wrong[0] ^= 0xFF  # the magic word
    with pytest.raises(ValueError):
        PD.BatchOutcome.unpack(wrong)
    with pytest.raises(ValueError):  # pack_outcomes' buffers are another format
        PD.BatchOutcome.unpack(np.array([PD.OUTCOME_MAGIC] + [0] * 7, dtype=np.int64).view(np.uint8))


def test_inconsistent_outcome_refused():
    s = dict(SPEC_A)
    o = outcome([s])
    with pytest.raises(ValueError):
        PD.BatchOutcome(**{**{k: getattr(o, k) for k in PD.BatchOutcome.array_fields()}, "frag_su": [1.0],
                           "breakage_names": BRK, "row_names": ROWS})


def test_device_limits_defaults():
    lim = PD.DeviceLimits()
    assert (lim.max_peaks, lim.max_len, lim.walk_caps, lim.walk_big_caps, lim.walk_max_rounds,
            lim.frontier_workspace) == (16383, 253, (64, 32), (8192, 8192), 4096, 0)
    assert lim.max_peaks == PD.MAX_PEAKS


def test_handoff_symbols_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sst.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (sst_\w+)", out))
    for name in ("sst_handoff_count_device", "sst_handoff_emit_device"):
        assert re.search(rf"\b{name}\s*\(", src), name
        assert name in _native.EXPORTS and name in exported, name
    assert "sst_handoff_args" in src and re.search(r"#define\s+SST_K_HANDOFF\s+19\b", src)
    assert _native.K_HANDOFF == 19 < _native.K_COUNT and _native.KERNEL_NAMES[_native.K_HANDOFF] == "k_handoff"
    # the ctypes struct has the header's fields, in its order
    body = re.search(r"typedef struct sst_handoff_args \{(.*?)\} sst_handoff_args;", src, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [n for n, _ in _native.HandoffArgs._fields_]


def test_mirror_outcome_vs_reference():
    """The host mirror's result as run_batch splices it in for a routed
    spectrum (mirror_outcome, on the oracle engine) against the REFERENCE's
    own results for the first spectra of a synthetic variant
    (synth_stages.json.gz); child process under the reference run's hash
    seed, as the mirrors' own checks run."""
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONHASHSEED="0")
    p = subprocess.run([sys.executable, os.path.join(here, "_handoff_check.py"), "short_fragments_missing", "mirror",
                        "3"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "handoff ok short_fragments_missing mirror post=" in p.stdout
