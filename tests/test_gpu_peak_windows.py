"""GPU tests of is_valid over peaks x breakage weights on peaks whose windows
take each path of the window arithmetic (peak_window, sst_kernels.hip), through
both callers of it: the fused step (sst_step_device, the is_valid workgroups
of k_step) and sst_is_valid_peaks_device.  Every is_valid byte of all four
breakage rows equals the CPU oracle's (is_valid_batch on the expanded rows)
and the other caller's; the step's explain answers equal
sst_explain_batch_device's by canonical digest and the oracle's per query,
with the pair hits strictly increasing under scan_order_key(q, n, n_wg).

Peak counts sit around the is_valid workgroups' 1 024 peaks (one lane per
peak): below one wave, one workgroup and one peak more, several workgroups
with a partial last one; beside one scan workgroup and beside several.  The
crafted peaks (crafted_peaks) are checked to be what they claim from the
oracle and the window arithmetic, not from the engine.  One result object
serves steps with different peak counts."""
import numpy as np
import pytest

import _oracle as oracle
import test_gpu_step_shapes as S
from conftest import load_golden
from spectrseqtools_amd import _native
from spectrseqtools_amd.parallel import canonical_digest, device_bytes, scan_order_key

pytestmark = pytest.mark.gpu

# name: (explain queries, peaks)
CASES = {
    "p1": (300, 1), "p63": (300, 63), "p65": (300, 65), "p1024": (300, 1024), "p1025": (300, 1025),
    "one_scan_wg": (300, 5000), "two_scan_wg": (2000, 4999), "lookback": (20000, 3001),
}


def crafted_peaks(rng, limit_da):
    """Peaks whose windows (su = obs - shift, +- 1e-5 obs) take each path of
    the is_valid arithmetic, per breakage shift where it matters: su just
    above 0 (below the first reachable mass); su <= 0; su at multiples of 64
    mDa between 300 and 4 000 Da (a window of 2 x 1e-5 obs / 1e-3 + 1 masses
    around a word boundary: two bitset words); su around the table's end
    (hi >= limit: -1); heavy peaks (the all-reachable run); obs = (j + 0.5)
    mDa and obs = 100 j Da (the rint / ceil quotients land on a rounding
    point: the exact division of quantise_lean runs)."""
    sh = S.SHIFTS
    parts = [s + rng.uniform(1e-4, 0.4, 12) for s in sh]
    parts += [rng.uniform(1.0, 370.0, 24), sh[1:] - 1e-3, sh[1:].copy()]
    parts += [s + 64e-3 * rng.integers(300000 // 64, 4000000 // 64, 40) + rng.normal(0, 2e-3, 40) for s in sh]
    parts += [s + rng.uniform(limit_da - 2.0, limit_da + 5.0, 12) for s in sh]
    parts += [rng.uniform(6000.0, 9000.0, 24)]
    parts += [rng.integers(300000, 3000000, 24) * 1e-3 + 5e-4, 100.0 * rng.integers(3, 60, 24)]
    return np.concatenate(parts)


def build_peaks(rng, n_peaks, limit_da):
    """Uniform peaks with the crafted ones spread over random positions (so
    they fall into different waves and workgroups); short batches take crafted peaks only."""
    obs = rng.uniform(150.0, 9000.0, n_peaks)
    c = rng.permutation(crafted_peaks(rng, limit_da))[:n_peaks]
    obs[rng.permutation(n_peaks)[:len(c)]] = c
    return obs


def build_queries(rng, rows, n):
    """test_gpu_step_shapes' "mixed" masses with thresholds of 3 to 20 mDa
    and the sums past 900 Da replaced by one-row masses, so that the payload
    stays within what the fused pass allows at every size here (a re-run pass
    would not be the fused step)."""
    masses, _ = S._queries(rng, rows, n)
    masses = np.array(masses, dtype=np.float64)
    ints = np.array(rows[1:], dtype=np.int64)
    heavy = np.flatnonzero(masses > 900.0)
    masses[heavy] = ints[rng.integers(0, len(ints), len(heavy))] * 1e-3 + rng.normal(0, 0.004, len(heavy))
    return masses, 1e-5 * rng.uniform(300, 2000, n)


class Bench:
    """The table, its oracle and the cases' inputs (built once per process)."""

    def __init__(self):
        import torch
        self.torch = torch
        g = load_golden("alphabet.json")
        self.rows = sorted({r["tolerated_integer_masses"] for r in g["rows"]} | {0})
        self.eng = _native.get_engine(0)
        self.dev = _native.DeviceTable.build(self.rows, max(self.rows) * 35, 32, engine=self.eng)
        self.dev.set_budgets(*S._budgets(self.rows))
        self.dev_t = torch.device("cuda", self.eng.device)
        self.limit_da = self.dev.n_cols * self.dev.compression * S.PREC
        self.orc = (oracle.build_table(self.rows, max(self.rows) * 35, 32),
                    oracle.Alphabet(self.rows, *S._budgets(self.rows)))

    def inputs(self, name):
        n, n_peaks = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))  # (a seed per case)
        masses, thr = build_queries(rng, self.rows, n)
        return masses, thr, build_peaks(rng, n_peaks, self.limit_da)

    def step(self, masses, thr, obs, reuse=None):
        """One fused step; returns (result, is_valid bytes, pair-hit queries, n_wg)."""
        torch = self.torch
        n, P = len(masses), len(obs)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.dev_t)
        self.keep = dm, dt, do = up(masses), up(thr), up(obs)
        out = torch.full((4 * P + 64,), 9, dtype=torch.int8, device=self.dev_t)  # 64 guard bytes behind the rows
        torch.cuda.synchronize()  # the engine queues on its own stream
        res = self.dev.step_device(do.data_ptr(), P, S.SHIFTS, out.data_ptr(), dm.data_ptr(), dt.data_ptr(), n, S.TOL,
                                   S.PREC, 10, reuse=reuse)
        hits_p, n_hits = res.hit_list_device()
        _, n_pair, _, n_wg = res.pair_hits_device()
        h = device_bytes(hits_p, 16 * n_hits, self.dev_t).cpu().numpy().view(np.uint32).reshape(-1, 4)
        res.fetch_device()
        self.eng.synchronize()
        valid = out.cpu().numpy()
        assert (valid[4 * P:] == 9).all(), "is_valid wrote past its rows"
        assert 0 < n_pair <= n_hits, (n_pair, n_hits)  # the fused scan answered (not a re-run pass)
        return res, valid[:4 * P], h[:n_pair, 0].astype(np.int64), n_wg

    def check(self, masses, thr, obs, res, valid, q, n_wg, what):
        """A step's outputs against the unfused pair and the CPU oracle."""
        torch = self.torch
        n, P = len(masses), len(obs)
        dm, dt, do = self.keep
        assert (np.diff(scan_order_key(q, n, n_wg)) > 0).all(), what  # the scan's order, strictly
        out_b = torch.full((4 * P,), 7, dtype=torch.int8, device=self.dev_t)
        self.dev.is_valid_peaks_device(do.data_ptr(), P, S.SHIFTS, S.TOL, S.PREC, out_b.data_ptr())
        ref = self.dev.explain_device(dm.data_ptr(), dt.data_ptr(), n, S.TOL, S.PREC, 10)
        ref.fetch_device()
        self.eng.synchronize()
        want = out_b.cpu().numpy()
        bad = np.flatnonzero(valid != want)
        assert not len(bad), (what, "is_valid bytes differ from the separate call at", bad[:8], n_wg)
        su = np.concatenate([obs - s for s in S.SHIFTS])
        host_want = oracle.is_valid_batch(self.orc[0], 32, su, S.TOL * np.tile(obs, 4), S.TOL, nthreads=16)
        bad = np.flatnonzero(valid != host_want)
        assert not len(bad), (what, "is_valid bytes differ from the oracle at", bad[:8], n_wg)
        assert np.array_equal(res.status, ref.status), what
        assert canonical_digest(res.status, res.count, res.offset, res.payload) == canonical_digest(
            ref.status, ref.count, ref.offset, ref.payload), what
        ref.close()
        S.check_vs_oracle(res, self.orc, masses, thr, None, what)
        return host_want


@pytest.fixture(scope="module")
def bench():
    pytest.importorskip("torch")
    return Bench()


@pytest.mark.parametrize("name", list(CASES))
def test_step_peaks_vs_unfused_and_oracle(bench, name):
    masses, thr, obs = bench.inputs(name)
    res, valid, q, n_wg = bench.step(masses, thr, obs)
    P = len(obs)
    want = bench.check(masses, thr, obs, res, valid, q, n_wg, name)
    res.close()
    if name == "lookback":
        assert n_wg > 2
    if P >= 3000:  # the crafted peaks brought every outcome
        assert (want == -1).any() and (want == 0).any() and (want == 1).any()


def test_crafted_peaks_take_each_path(bench):
    """The crafted peaks are what they claim (from the oracle and the window
    arithmetic, not from the engine)."""
    rng = np.random.default_rng(5)
    obs = crafted_peaks(rng, bench.limit_da)
    su = np.concatenate([obs - s for s in S.SHIFTS])
    thr = S.TOL * np.tile(obs, 4)
    want = oracle.is_valid_batch(bench.orc[0], 32, su, thr, S.TOL, nthreads=16)
    assert (want[su <= 0.0] == 0).all() and (su <= 0.0).sum() >= 24
    tiny = (su > 0.0) & (su < 0.5)
    assert tiny.sum() >= 48 and (want[tiny] == 0).all()  # below the first reachable mass
    assert (want == -1).sum() >= 12  # past the table's end
    heavy = (su > 5500.0) & (su < bench.limit_da - 10.0)
    assert heavy.sum() >= 24 and (want[heavy] == 1).all()  # the all-reachable run
    target = np.rint(su / S.PREC)
    half = np.ceil(thr / S.PREC)
    two_words = ((target - half) // 64 != (target + half) // 64) & (su > 300.0) & (su < 4000.0)
    assert two_words.sum() >= 40
    qm, qt = su * (1.0 / S.PREC), thr * (1.0 / S.PREC)
    assert (0.5 - np.abs(qm - np.rint(qm)) <= np.abs(qm) * 2.0 ** -50).sum() >= 8  # rint on a tie: exact division
    assert (np.abs(qt - np.rint(qt)) <= np.abs(qt) * 2.0 ** -50).sum() >= 8  # ceil on an integer: exact division


def test_result_reused_with_another_peak_count(bench):
    """One result object, steps with different peak counts (and back)."""
    rng = np.random.default_rng(77)
    masses, thr = build_queries(rng, bench.rows, 300)
    res = None
    for P in (5000, 777, 5000 + 64):
        obs = build_peaks(rng, P, bench.limit_da)
        res, valid, q, n_wg = bench.step(masses, thr, obs, reuse=res)
        bench.check(masses, thr, obs, res, valid, q, n_wg, f"reused result, P = {P}")
    res.close()
