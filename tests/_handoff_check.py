"""Child-process check (run with PYTHONHASHSEED=0, the seed of the reference
run in tests/golden/make_synth_golden.py): pipeline_device.run_batch on the
synthetic spectra of tests/_synth_cases.py against the REFERENCE's own results
(synth_stages.json.gz) -- per spectrum whether Predictor.predict returns its
default, else the combined skeleton, the fragments after the skeleton-based
reduction (index, min_end, max_end) and the reduced alphabet, all read from
the BatchOutcome's dense arrays; every spectrum on the device route.

usage: python tests/_handoff_check.py VARIANT            (run_batch on the device, all spectra)
       python tests/_handoff_check.py VARIANT mirror N   (mirror_outcome on the oracle engine, first N: the
                                                          conversion run_batch splices in for routed spectra)
TEST INFRASTRUCTURE."""
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import numpy as np  # noqa: E402


def check_spectrum(out, g, k, w):
    """Spectrum k of outcome `out` against the reference's record w of spectrum g."""
    p = w["post"]
    assert bool(out.default[k]) == p["default"], (g, "default")
    if p["default"]:
        assert out.frag_off[k] == out.frag_off[k + 1] and out.pos_off[k] == out.pos_off[k + 1], g
        assert not out.alpha[k].any() and int(out.seq_len[k]) == 0, g
        return 0
    j = w["skeleton"]["jaccard"]
    assert int(out.seq_len[k]) == j["seq_len"] == int(out.pos_off[k + 1] - out.pos_off[k]), g
    assert out.skeleton_seq(k) == j["combined"], (g, "combined skeleton")
    fr, wf = out.fragments(k), p["reduction"]["fragments"]
    for key in ("index", "min_end", "max_end"):
        assert fr.get_column(key).to_list() == wf[key], (g, key, fr.get_column(key).to_list(), wf[key])
    assert out.alphabet_masses(k) == p["reduction"]["masses"], (g, "post alphabet")
    return 1


def check_mirror(want, d, first):
    import pytest

    import _fake_engine
    import _synth_cases as SC
    from spectrseqtools_amd import pipeline_device as PD
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE, build_breakage_dict

    mp = pytest.MonkeyPatch()
    _fake_engine.install(mp)
    seq = SequenceInformation(max_len=20, su_mass=float(d["su_seq"][0]), obs_mass=float(d["seq_mass"][0]),
                              modification_rate=d["mod_rate"])
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq)
    bd = build_breakage_dict(*SC.TAGS)
    outs = []
    for g in range(first):
        obs = d["obs"][d["offsets"][g]:d["offsets"][g + 1]]
        o = PD.mirror_outcome(dp, obs, d["su_seq"][g], d["seq_mass"][g], d["max_len"][g], bd, reason=PD.REASON_WALK)
        assert len(o) == 1 and int(o.route[0]) == PD.ROUTE_MIRROR and int(o.reason[0]) == PD.REASON_WALK
        outs.append(o)
    both = PD.BatchOutcome.concat(outs)
    n_post = sum(check_spectrum(both, g, g, want[g]) for g in range(first))
    mp.undo()
    return n_post


def main():
    variant = sys.argv[1]
    assert os.environ.get("PYTHONHASHSEED") == "0", "run with PYTHONHASHSEED=0"
    from conftest import load_golden
    import _synth_cases as SC
    from spectrseqtools_amd import _native, pipeline_device as PD
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE, build_breakage_dict

    want = load_golden("synth_stages.json.gz")[variant]
    d = SC.variant_inputs(variant, n=len(want["spectra"]))
    assert d["mod_rate"] == want["mod_rate"]
    for g, w in enumerate(want["spectra"]):  # the same inputs the reference ran
        obs = d["obs"][d["offsets"][g]:d["offsets"][g + 1]]
        assert hashlib.sha256(np.ascontiguousarray(obs, dtype=np.float64).tobytes()).hexdigest() == w["obs_sha256"]
        assert (w["su_mass"], w["seq_mass"], w["max_len"]) == (float(d["su_seq"][g]), float(d["seq_mass"][g]),
                                                              int(d["max_len"][g])), g
    n = len(want["spectra"])
    assert n == 48
    if sys.argv[2:3] == ["mirror"]:
        n_post = check_mirror(want["spectra"], d, int(sys.argv[3]))
        print(f"handoff ok {variant} mirror post={n_post}")
        return
    seq = SequenceInformation(max_len=20, su_mass=float(d["su_seq"][0]), obs_mass=float(d["seq_mass"][0]),
                              modification_rate=d["mod_rate"])
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq, engine=_native.get_engine(0))
    bd = build_breakage_dict(*SC.TAGS)
    out = PD.run_batch(dp, d["obs"], d["offsets"], d["su_seq"], d["seq_mass"], bd, max_len=d["max_len"])
    assert len(out) == n and not out.route.any() and not out.reason.any()
    n_post = sum(check_spectrum(out, g, g, w) for g, w in enumerate(want["spectra"]))
    assert PD.BatchOutcome.unpack(out.pack()).equals(out)
    print(f"handoff ok {variant} post={n_post}")


if __name__ == "__main__":
    main()
