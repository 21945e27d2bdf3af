"""Run in a child process by test_gpu_scan_lds_hits.py, once per forced
capacity of the scan waves' LDS hit-record slots (SST_SCAN_LDS_HITS is read
once per process; unset: the default).  Runs every case of CASES through
sst_step_device or sst_explain_batch_device and writes, per case, SHA-256
digests of the result's parts and what the wave's hit counts say about the
capacity in force, as JSON to the path given.  With --reference (the K = 0
run) each step case is also compared per query with the two separate calls
and a sample with the CPU oracle's lists, and every case's every query with
the oracle's status, count and list digest."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _oracle as oracle  # noqa: E402
import test_gpu_step_shapes as S  # noqa: E402
from conftest import load_golden  # noqa: E402
from spectrseqtools_amd import _native  # noqa: E402
from spectrseqtools_amd.parallel import canonical_digest, device_bytes, scan_order_key  # noqa: E402

W_STEP, W_PLAIN = 4096, 8192  # scan waves: one / two 1024-lane workgroups per CU on 256 CUs
N_PEAKS = 513
# (name, entry point, query kind, full tile rounds per wave).  n = 64 W rounds
# + 17: one more, partial tile for the first wave.  Below one full round no
# wave owns two tiles, so nothing smaller can cross a capacity.
CASES = [(f"{api}_{kind}_{rounds}", api, kind, rounds)
         for api in ("step", "plain")
         for kind, rounds in (("all", 3), ("mixed", 3), ("mixed", 2), ("mixed", 1), ("routed", 3), ("wide", 3))]
# crafted tiles (hits per tile of virtual wave vw, by round): a wave that
# holds exactly 1 record after its first tile, one that holds exactly 64
# after its first and 100 after its second
CRAFT = {3: (1, 64, 5), 4: (64, 36, 64)}
WIDE_VW, WIDE_ROUND, N_WIDE = 6, 1, 8
N_ROUTED = 100


def build_queries(rng, rows, kind, n, waves, rounds):
    """The kind's queries: the masses of test_gpu_step_shapes._queries;
    "mixed" with thresholds of 3 to 20 mDa and its two-row sums past 900 Da
    (3 w_min = 915 Da: routed windows with long candidate lists) replaced by
    one-row masses, so that the payload stays within what the first pass
    allows -- otherwise the engine re-runs the pass unfused at these sizes,
    and a re-run answers nothing from the fused scan.  "routed": "mixed" plus
    N_ROUTED three-row sums.  "wide": "mixed" plus N_WIDE windows 20 000 masses wide
    around 746 Da, where the pair list holds more than 254 sums (it has about
    one sum per 100 masses: narrower windows cannot pass a count of 254).
    The crafted tiles come on top, except on "all"."""
    masses, thr = S._queries(rng, rows, n, "all" if kind == "all" else "mixed")
    masses, thr = np.array(masses, dtype=np.float64), np.array(thr, dtype=np.float64)
    ints = np.array(rows[1:], dtype=np.int64)
    if kind != "all":
        thr = 1e-5 * rng.uniform(300, 2000, n)
        heavy = np.flatnonzero(masses > 900.0)
        masses[heavy] = ints[rng.integers(0, len(ints), len(heavy))] * 1e-3 + rng.normal(0, 0.004, len(heavy))
    wide = np.zeros(0, np.int64)
    if kind == "routed":  # N_ROUTED three-row sums (the deferred DFS is slow), off the crafted waves
        q = rng.integers(0, n, 2 * N_ROUTED)
        q = q[~np.isin((q >> 6) % waves, list(CRAFT))][:N_ROUTED]
        m3 = ints[rng.integers(0, len(ints), (3, len(q)))].sum(axis=0)
        masses[q], thr[q] = m3 * 1e-3 + rng.normal(0, 0.004, len(q)), 1e-5 * rng.uniform(300, 14000, len(q))
    if kind != "all" and rounds >= 3:
        for vw, hits in CRAFT.items():
            for r, k in enumerate(hits):
                q = (vw + r * waves) * 64 + np.arange(64)
                masses[q], thr[q] = 0.5, 0.005  # below the first reachable mass: no hit
                lanes = rng.permutation(64)[:k]
                masses[q[lanes]], thr[q[lanes]] = ints[rng.integers(0, len(ints), k)] * 1e-3, 0.02
    if kind == "wide":
        wide = (WIDE_VW + WIDE_ROUND * waves) * 64 + np.arange(N_WIDE)
        masses[wide], thr[wide] = 746.0 + rng.uniform(-3, 3, N_WIDE), 10.0
    return masses, thr, wide


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def wave_cumulative(q, n, n_wg):
    """[scan wave][round]: its hit records after that tile."""
    waves = 16 * n_wg
    tile = q >> 6
    rounds = -(-((n + 63) // 64) // waves)
    c = np.zeros((waves, rounds), np.int64)
    np.add.at(c, (tile % waves, tile // waves), 1)
    return np.cumsum(c, axis=1)


def run_case(eng, dev, rows, host, alph, case, K, reference):
    name, api, kind, rounds = case
    waves = W_STEP if api == "step" else W_PLAIN
    n = 64 * waves * rounds + 17
    rng = np.random.default_rng(1000 + 7 * rounds + len(kind))
    masses, thr, wide = build_queries(rng, rows, kind, n, waves, rounds)
    dev_t = torch.device("cuda", eng.device)
    obs = np.sort(rng.uniform(150.0, 9000.0, N_PEAKS))
    dm, dt, do = (torch.from_numpy(x).to(dev_t) for x in (masses, thr, obs))
    valid = torch.full((4 * N_PEAKS,), 9, dtype=torch.int8, device=dev_t)
    torch.cuda.synchronize()  # the engine queues on its own stream
    if api == "step":
        res = dev.step_device(do.data_ptr(), N_PEAKS, S.SHIFTS, valid.data_ptr(), dm.data_ptr(), dt.data_ptr(), n,
                              S.TOL, S.PREC, 10)
    else:
        res = dev.explain_device(dm.data_ptr(), dt.data_ptr(), n, S.TOL, S.PREC, 10)
    hits_p, n_hits = res.hit_list_device()
    refs_p, n_pair, pair_bytes, n_wg = res.pair_hits_device()
    assert 16 * n_wg == waves, (n_wg, waves)  # the grid the engine selects
    h = device_bytes(hits_p, 16 * n_hits, dev_t).cpu().numpy().view(np.uint32).reshape(-1, 4)
    refs = device_bytes(refs_p, 2 * n_pair, dev_t).cpu().numpy().view(np.uint16)
    res.fetch_device()
    eng.synchronize()
    # the fused scan answered its queries (not a re-run pass: that one reports no pair hits)
    assert 0 < n_pair <= n_hits and n_pair >= n_hits - 20000, (name, n_pair, n_hits, len(res.payload))
    q = h[:n_pair, 0].astype(np.int64)
    assert (np.diff(scan_order_key(q, n, n_wg)) > 0).all(), name  # the scan's order
    cum = wave_cumulative(q, n, n_wg)
    out = {
        "n": n, "n_hits": n_hits, "n_pair": n_pair, "pair_bytes": pair_bytes, "payload_bytes": len(res.payload),
        "status": sha(res.status), "pair_hits": sha(h[:n_pair]), "refs": sha(refs),
        "pair_payload": sha(res.payload[:pair_bytes]),
        "answers": str(canonical_digest(res.status, res.count, res.offset, res.payload)),
        "valid": sha(valid.cpu().numpy()) if api == "step" else "",
        "max_wave_hits": int(cum[:, -1].max()), "exceeds": bool((cum[:, -1] > K).any()),
        "boundary": bool((cum == K).any()), "max_count": int(h[:n_pair, 1].max()) if n_pair else 0,
    }
    if kind == "all":
        assert (res.status == _native.SST_SOME).all() and (cum[:, 0] == 64).sum() >= waves - 1, name
    if kind == "routed":  # windows past the pair list were answered (three and more rows)
        assert n_hits > n_pair, name
    if kind == "wide":  # the wide windows are pair hits, and their counts do not fit the record's u8
        pos = np.flatnonzero(np.isin(q, wide))
        assert len(pos) == N_WIDE and (h[pos, 1] > 254).any(), (
            name, h[pos, 1], res.status[wide], res.count[wide], n_pair, n_hits,
            np.flatnonzero(np.isin(h[:, 0] & 0x7FFFFFFF, wide)))
        n_big = 0
        for i in wide:
            st, sols, _, _ = oracle.explain_table(host, 32, alph, masses[i], thr[i], S.TOL, 10)
            assert st >= 0 and res.candidates(int(i)) == sols, (name, i)
            n_big += len(sols) > 254
        assert n_big >= 1, name  # from the oracle: a count past the field
    if reference:
        if api == "step":  # against the two separate calls, per query
            out_b = torch.full_like(valid, 7)
            dev.is_valid_peaks_device(do.data_ptr(), N_PEAKS, S.SHIFTS, S.TOL, S.PREC, out_b.data_ptr())
            ref = dev.explain_device(dm.data_ptr(), dt.data_ptr(), n, S.TOL, S.PREC, 10)
            ref.fetch_device()
            eng.synchronize()
            assert np.array_equal(valid.cpu().numpy(), out_b.cpu().numpy()), name
            assert np.array_equal(res.status, ref.status), name
            counted = np.isin(res.status, (_native.SST_SOME, _native.SST_OVERFLOW))
            assert np.array_equal(res.count[counted], ref.count[counted]), name
            (ln_a, by_a), (ln_b, by_b) = S._candidate_bytes(res), S._candidate_bytes(ref)
            assert np.array_equal(ln_a, ln_b) and np.array_equal(by_a, by_b), name
            ref.close()
        crafted = [(vw + r * waves) * 64 + lane for vw in CRAFT for r in range(3) for lane in (0, 63)] if rounds >= 3 else []
        for i in np.concatenate([rng.integers(0, n, 40), [0, 63, 64, n - 18, n - 17, n - 1], crafted]).astype(np.int64):
            st, sols, n_empty, _ = oracle.explain_table(host, 32, alph, masses[i], thr[i], S.TOL, 10)
            want = _native.SST_OUT_OF_TABLE if st < 0 else (
                _native.SST_SOME if sols else (_native.SST_EMPTY if n_empty else _native.SST_NONE))
            assert int(res.status[i]) == want, (name, i)
            if sols:
                assert res.candidates(int(i)) == sols, (name, i)
        S.check_vs_oracle(res, (host, alph), masses, thr, None, name)
    res.close()
    return out


def main():
    out_path = sys.argv[1]
    reference = "--reference" in sys.argv[2:]
    g = load_golden("alphabet.json")
    rows = sorted({r["tolerated_integer_masses"] for r in g["rows"]} | {0})
    eng = _native.get_engine(0)
    dev = _native.DeviceTable.build(rows, max(rows) * 35, 32, engine=eng)
    dev.set_budgets(*S._budgets(rows))
    K = dev.scan_lds_hits()
    host = oracle.build_table(rows, max(rows) * 35, 32)
    alph = oracle.Alphabet(rows, *S._budgets(rows))
    out = {"K": K, "cases": {}}
    only = [a[7:] for a in sys.argv[2:] if a.startswith("--only=")]  # (by hand: some cases)
    for case in CASES:
        if not only or any(o in case[0] for o in only):
            out["cases"][case[0]] = run_case(eng, dev, rows, host, alph, case, K, reference)
    with open(out_path, "w") as f:
        json.dump(out, f)
    print(f"scan lds hits ok: K = {K}, {len(out['cases'])} cases")


if __name__ == "__main__":
    main()
