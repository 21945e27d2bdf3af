"""GPU tests of the whole-batch call and its dense hand-off
(pipeline_device.run_batch, BatchOutcome; sst_handoff_count_device /
sst_handoff_emit_device, csrc/sst_handoff.hip):
  * the two kernels on synthetic tensors, fed straight to the C ABI, against
    a numpy compaction -- every output array exactly, guard elements after
    the outputs untouched;
  * run_batch against the REFERENCE's own results (synth_stages.json.gz) in a
    child process under the reference run's hash seed (tests/_handoff_check.py);
  * routing: with one engine limit shrunk at a time, the spectra outside it run
    the host mirror and the outcome equals the all-device baseline."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def engine():
    from spectrseqtools_amd import _native

    return _native.get_engine(0)


@pytest.fixture(scope="module")
def table(engine):
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE

    seq = SequenceInformation(max_len=20, su_mass=3000.0, obs_mass=3500.0, modification_rate=0.5)
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq, engine=engine)
    yield dp
    dp.close()


# ---------------------------------------------------------------------------
# 1. the kernels against numpy
# ---------------------------------------------------------------------------
def flag_pattern(kind, n):
    f = np.zeros(n, np.uint8)
    if kind == "all":
        f[:] = 1
    elif kind == "alternating":
        f[::2] = 1
    elif kind == "last" and n:
        f[-1] = 1
    elif kind == "lane63":
        f[63::64] = 1
    elif kind == "random":
        f[:] = np.random.default_rng(n).random(n) < 0.4
    return f * np.uint8(1 + n % 3)  # any non-zero byte is a set flag


def build_case(specs, seed):
    """specs: per spectrum (rows, flag pattern, active, seq_len, max_len,
    spare slots).  Row slots of spectrum g start at 4 * peak_off[g]; it has
    ceil((rows + spare) / 4) peaks, so cnt[g] <= 4 * peaks with gaps; the
    slots past cnt[g] carry set flags that must be ignored."""
    rng = np.random.default_rng(seed)
    S = len(specs)
    peaks = np.array([-(-(r + sp) // 4) for r, _, _, _, _, sp in specs], dtype=np.int64)
    peak_off = np.concatenate([[0], np.cumsum(peaks)]).astype(np.int64)
    slots = max(1, int(4 * peak_off[-1]))
    c = {"peak_off": peak_off, "cnt": np.array([s[0] for s in specs], dtype=np.int32),
         "su": rng.uniform(300, 5000, slots), "obs": rng.uniform(300, 5000, slots),
         "meta": rng.integers(0, 1 << 22, slots).astype(np.int32), "flags": np.ones(slots, np.uint8),
         "min_end": rng.integers(-1, 250, slots).astype(np.int32), "max_end": rng.integers(-1, 250, slots).astype(np.int32),
         "active": np.array([s[2] for s in specs], dtype=np.uint8),
         "seq_len": np.array([s[3] for s in specs], dtype=np.int32)}
    ml = np.array([s[4] for s in specs], dtype=np.int64)
    c["comb_off"] = np.concatenate([[0], np.cumsum(ml)]).astype(np.int64)
    c["comb"] = rng.integers(0, 1 << 62, (max(1, int(ml.sum())), 2)).astype(np.int64)
    for g, (r, kind, _, _, _, _) in enumerate(specs):
        o = 4 * int(peak_off[g])
        c["flags"][o:o + r] = flag_pattern(kind, r)
    c["S"] = S
    return c


def numpy_handoff(c):
    S = c["S"]
    n_frag, n_pos = np.zeros(S, np.int64), np.zeros(S, np.int64)
    keep, pos = [], []
    for g in range(S):
        if not c["active"][g]:
            continue
        o, r = 4 * int(c["peak_off"][g]), int(c["cnt"][g])
        idx = np.flatnonzero(c["flags"][o:o + r])
        n_frag[g] = len(idx)
        keep.append((o + idx, idx))
        L = int(c["seq_len"][g])
        n_pos[g] = L
        pos.append(np.arange(int(c["comb_off"][g]), int(c["comb_off"][g]) + L))
    slot = np.concatenate([k[0] for k in keep]).astype(np.int64) if keep else np.zeros(0, np.int64)
    index = np.concatenate([k[1] for k in keep]).astype(np.int32) if keep else np.zeros(0, np.int32)
    p = np.concatenate(pos).astype(np.int64) if pos else np.zeros(0, np.int64)
    return {"n_frag": n_frag, "n_pos": n_pos, "frag_off": np.concatenate([[0], np.cumsum(n_frag)]),
            "pos_off": np.concatenate([[0], np.cumsum(n_pos)]), "index": index,
            "code": (c["meta"][slot] & 0x1f).astype(np.uint8), "su": c["su"][slot], "obs": c["obs"][slot],
            "min_end": c["min_end"][slot], "max_end": c["max_end"][slot], "skeleton": c["comb"][p]}


def device_handoff(dp, c, want):
    """The two C calls on the case's tensors; outputs sized from the numpy
    totals plus GUARD sentinel elements each."""
    import torch

    from spectrseqtools_amd import _native

    dt = dp.device_table
    eng = dt.engine
    dev = torch.device("cuda", eng.device)
    S = c["S"]
    up = {k: torch.as_tensor(v, device=dev) for k, v in c.items() if k != "S"}
    if S == 0:  # (no per-spectrum input is read)
        up["cnt"] = up["active"] = up["seq_len"] = torch.zeros(1, dtype=torch.int32, device=dev)
    n_frag = torch.full((max(1, S) + GUARD,), -7, dtype=torch.int32, device=dev)
    n_pos = torch.full((max(1, S) + GUARD,), -7, dtype=torch.int32, device=dev)
    frag_off = torch.full((S + 1 + GUARD,), -7, dtype=torch.int64, device=dev)
    pos_off = torch.full((S + 1 + GUARD,), -7, dtype=torch.int64, device=dev)
    a = _native.HandoffArgs()
    a.n_spec = S
    a.peak_off, a.cnt = up["peak_off"].data_ptr(), up["cnt"].data_ptr()
    a.r_su, a.r_ob, a.r_meta = up["su"].data_ptr(), up["obs"].data_ptr(), up["meta"].data_ptr()
    a.flags, a.min_end, a.max_end = up["flags"].data_ptr(), up["min_end"].data_ptr(), up["max_end"].data_ptr()
    a.active, a.seq_len = up["active"].data_ptr(), up["seq_len"].data_ptr()
    a.comb_off, a.comb = up["comb_off"].data_ptr(), up["comb"].data_ptr()
    a.n_frag, a.n_pos, a.frag_off, a.pos_off = (n_frag.data_ptr(), n_pos.data_ptr(), frag_off.data_ptr(),
                                                pos_off.data_ptr())
    torch.cuda.synchronize(dev)
    eng.check(eng._lib.sst_handoff_count_device(dt.handle, ctypes.byref(a)), "sst_handoff_count_device")
    eng.synchronize()
    got = {"n_frag": n_frag.cpu().numpy(), "n_pos": n_pos.cpu().numpy(), "frag_off": frag_off.cpu().numpy(),
           "pos_off": pos_off.cpu().numpy()}
    # the emit's outputs are sized from the expected totals: the counts must be right before it runs
    assert got["frag_off"][:S + 1].tolist() == want["frag_off"].tolist()
    assert got["pos_off"][:S + 1].tolist() == want["pos_off"].tolist()
    nf, npos = int(want["frag_off"][-1]), int(want["pos_off"][-1])
    dts = {"index": torch.int32, "code": torch.uint8, "su": torch.float64, "obs": torch.float64,
           "min_end": torch.int32, "max_end": torch.int32}
    outs = {k: torch.full((nf + GUARD,), 77, dtype=t, device=dev) for k, t in dts.items()}
    outs["skeleton"] = torch.full((npos + GUARD, 2), 77, dtype=torch.int64, device=dev)
    a.index, a.code, a.su, a.obs = (outs[k].data_ptr() for k in ("index", "code", "su", "obs"))
    a.out_min_end, a.out_max_end, a.skeleton = (outs[k].data_ptr() for k in ("min_end", "max_end", "skeleton"))
    torch.cuda.synchronize(dev)
    eng.check(eng._lib.sst_handoff_emit_device(dt.handle, ctypes.byref(a)), "sst_handoff_emit_device")
    eng.synchronize()
    got.update({k: v.cpu().numpy() for k, v in outs.items()})
    return got


def check_case(dp, specs, seed):
    c = build_case(specs, seed)
    want = numpy_handoff(c)
    got = device_handoff(dp, c, want)
    S = c["S"]
    nf, npos = int(want["frag_off"][-1]), int(want["pos_off"][-1])
    for k, n in (("n_frag", S), ("n_pos", S), ("frag_off", S + 1), ("pos_off", S + 1)):
        assert np.array_equal(got[k][:n], want[k]), k
        assert (got[k][max(n, 1) if k.startswith("n_") else n:] == -7).all(), (k, "guard")
    assert (np.diff(got["frag_off"][:S + 1]) >= 0).all() and (np.diff(got["pos_off"][:S + 1]) >= 0).all()
    for k in ("index", "code", "su", "obs", "min_end", "max_end"):
        assert got[k][:nf].dtype == want[k].dtype and np.array_equal(got[k][:nf], want[k]), k
        assert (got[k][nf:] == 77).all(), (k, "guard")
    assert np.array_equal(got["skeleton"][:npos], want["skeleton"])
    assert (got["skeleton"][npos:] == 77).all(), "skeleton guard"
    return nf, npos


def test_kernels_no_spectra(table):
    assert check_case(table, [], 1) == (0, 0)


def test_kernels_one_spectrum_without_rows(table):
    assert check_case(table, [(0, "all", 1, 0, 5, 0)], 2) == (0, 0)
    assert check_case(table, [(0, "all", 1, 3, 5, 0)], 3) == (0, 3)
    assert check_case(table, [(0, "all", 0, 3, 5, 4)], 4) == (0, 0)


def test_kernels_tile_edges(table):
    """Spectra of 1 .. 200 rows (the 64-row tile's edges) under every flag
    pattern, with gaps between the spectra's slots, an inactive spectrum
    between two active ones, and seq_len 0, 1 and below max_len."""
    specs = []
    for rows in (1, 63, 64, 65, 128, 129, 200):
        for kind in ("all", "none", "alternating", "last", "lane63", "random"):
            g = len(specs)
            specs.append((rows, kind, 1, (0, 1, 7, 12)[g % 4], 12, (0, 1, 5, 9)[g % 4]))
    specs[10] = specs[10][:2] + (0,) + specs[10][3:]   # inactive between two active ones: "all" flags, seq_len 7
    specs[23] = specs[23][:2] + (0,) + specs[23][3:]
    nf, npos = check_case(table, specs, 5)
    assert nf > 1000 and npos > 100
    # every pattern alone as well (the running base starts at 0 for each)
    for kind in ("all", "none", "alternating", "last", "lane63"):
        check_case(table, [(200, kind, 1, 1, 3, 2)], 6)


def test_kernels_many_small_spectra(table):
    """3000 spectra of 0-3 rows: more spectra than one pass of the grid's
    waves takes when the grid is capped, and a last workgroup with idle waves
    (3000 = 4 x 750; 2999 leaves one)."""
    rng = np.random.default_rng(9)
    for S in (3000, 2999):
        specs = [(int(rng.integers(0, 4)), ("all", "random", "last")[g % 3], int(g % 11 != 0), int(rng.integers(0, 4)),
                  3, int(rng.integers(0, 6))) for g in range(S)]
        nf, npos = check_case(table, specs, 10)
        assert nf > 1000 and npos > 1000


# ---------------------------------------------------------------------------
# 2. run_batch against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["short_fragments_missing", "noise_free_exact"])
def test_run_batch_vs_reference(variant):
    """run_batch over the 48 synthetic spectra of a variant against the
    REFERENCE's Predictor.predict up to its MILP stages (synth_stages.json.gz:
    default or not, the combined skeleton, the fragments after the
    skeleton-based reduction with min_end / max_end, the reduced alphabet).
    Child process under the reference run's hash seed."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONHASHSEED="0")
    p = subprocess.run([sys.executable, os.path.join(here, "_handoff_check.py"), variant], env=env,
                       capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert f"handoff ok {variant}" in p.stdout


# ---------------------------------------------------------------------------
# 3. routing
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch(engine):
    """16 synthetic spectra, their table and the all-device baseline."""
    import _synth_cases as SC
    from spectrseqtools_amd import pipeline, pipeline_device as PD
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE, build_breakage_dict
    from spectrseqtools_amd.synthetic import make_spectra

    b = make_spectra(16, seed=5, len_range=(6, 14))
    bd = build_breakage_dict(*SC.TAGS)
    w_full = [k for k, v in bd.items() if "START_END" in v][0]
    su_seq = b.seq_mass - w_full * TOLERANCE
    min_int = min(EXPLANATION_MASSES.get_column("tolerated_integer_masses").to_list())
    max_len = pipeline.max_len_of(su_seq, TOLERANCE, min_int)
    seq = SequenceInformation(max_len=20, su_mass=float(su_seq[0]), obs_mass=float(b.seq_mass[0]), modification_rate=0.5)
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq, engine=engine)
    args = (dp, b.observed, b.offsets, su_seq, b.seq_mass, bd)
    rec = {}
    base = PD.run_batch(*args, record=rec)
    assert len(base) == 16 and not base.route.any() and not base.reason.any()
    assert int((~base.default).sum()) >= 8  # most spectra reach the MILP stages
    assert np.array_equal(rec["device_index"], np.arange(16))
    yield {"args": args, "max_len": max_len, "base": base, "record": rec}
    dp.close()


def routed(batch, limits, bit, expect=None):
    from spectrseqtools_amd import pipeline_device as PD

    rec = {}
    out = PD.run_batch(*batch["args"], limits=limits, record=rec)
    mirrored = np.flatnonzero(out.route == PD.ROUTE_MIRROR)
    print(f"reason {bit}: mirrored {mirrored.tolist()}", flush=True)
    assert 1 <= len(mirrored) < 16, mirrored
    assert (out.reason[mirrored] == bit).all() and not out.reason[out.route == PD.ROUTE_DEVICE].any()
    if expect is not None:
        assert mirrored.tolist() == np.flatnonzero(expect).tolist()
    base = batch["base"]
    for k in PD.BatchOutcome.array_fields():
        if k not in ("route", "reason"):
            assert np.array_equal(getattr(out, k), getattr(base, k)), (k, getattr(out, k), getattr(base, k))
    assert out.equals(base, ignore=("route", "reason"))
    return out, rec


def test_routing_max_peaks(batch):
    from spectrseqtools_amd import _native, pipeline_device as PD

    peaks = np.diff(batch["args"][2])
    cap = int(np.median(peaks))
    over = peaks > cap
    assert 1 <= over.sum() < 16
    routed(batch, PD.DeviceLimits(max_peaks=cap), PD.REASON_PEAKS, expect=over)
    with pytest.raises(_native.EngineError) as e:
        PD.run_batch(*batch["args"], limits=PD.DeviceLimits(max_peaks=cap), fallback="raise")
    for g in np.flatnonzero(over):
        assert f"spectrum {int(g)}:" in str(e.value), (g, str(e.value))
    for g in np.flatnonzero(~over):
        assert f"spectrum {int(g)}:" not in str(e.value), (g, str(e.value))


def test_routing_max_len(batch):
    from spectrseqtools_amd import pipeline_device as PD

    cap = int(np.median(batch["max_len"]))
    over = batch["max_len"] > cap
    assert 1 <= over.sum() < 16
    routed(batch, PD.DeviceLimits(max_len=cap), PD.REASON_MAX_LEN, expect=over)


def test_routing_walk_capacities(batch):
    from spectrseqtools_amd import _native, pipeline_device as PD

    _, rec = routed(batch, PD.DeviceLimits(walk_caps=(4, 2), walk_big_caps=(8, 4)), PD.REASON_WALK)
    st = rec["walk_status"].reshape(-1, 2)
    print("walk status per spectrum:", st.tolist(), flush=True)
    assert (st == _native.WALK_LIMIT).any()


def test_routing_frontier_workspace(batch):
    """A frontier workspace sized as test_frontier_split_and_abort sizes its
    aborting one (376 bytes per slot, a power-of-two slot count whose node
    capacity, 8 per slot, is below the heavier spectra's memo entries; the
    engine keeps at least 1 024 slots, i.e. 8 192 entries: measured on this
    batch, two spectra (29 504 and 10 102 entries) are beyond that)."""
    from spectrseqtools_amd import _native, pipeline_device as PD

    nodes = np.asarray(batch["record"]["replay_nodes"])
    live = nodes[~batch["base"].default]
    print("memo entries per spectrum:", nodes.tolist(), flush=True)
    small = int(np.sort(live)[len(live) // 2])  # node capacity below the heavier half's
    S2 = 1 << int(np.floor(np.log2(small // 8)))
    _, rec = routed(batch, PD.DeviceLimits(frontier_workspace=376 * S2), PD.REASON_FRONTIER)
    assert (rec["lb_status"] == _native.SST_ABORTED).any()
