"""What the GPU tests of the alignment certificate share (test_gpu_align.py,
test_gpu_align_split.py, test_gpu_align_caps.py): the engine, capacity and
full-table fixtures (a test module imports the ones it uses), the device /
host comparison of a case, the entry points' argument struct over device
copies, and the builders of fragments and positions at the capacity's edge."""
import math

import numpy as np
import pytest

import _align_cases as AC

CHUNK = 384  # fragment records the kernels hold at a time
FIELDS = ("status", "alignable", "n_fit", "first")
OBS_W = {0: 0.0, 1: 50.0, 4: 350.0, 30: 2950.0}  # observed masses whose W = ceil(0.01 obs) is the key (full table)


@pytest.fixture(scope="module")
def engine():
    from spectrseqtools_amd import _native

    return _native.get_engine(0)


@pytest.fixture(scope="module")
def K(engine):
    from spectrseqtools_amd import alignment

    k = int(engine._lib.sst_align_capacity())
    assert k == alignment.ALIGN_CAPACITY and k >= 1024 and k % 4 == 0
    return k


@pytest.fixture(scope="module")
def full_table(engine):
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE

    seq = SequenceInformation(max_len=20, su_mass=3000.0, obs_mass=3500.0, modification_rate=0.5)
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq, engine=engine)
    for w, obs in OBS_W.items():
        assert math.ceil(dp.tolerance * obs / dp.precision) == w
    yield dp
    dp.close()


def run(dp, specs, rm, K, split=False, caps=None):
    """(outcome, device, host model at capacity K) of a case, with the split
    and under `caps` as asked; asserts the device equal to the host in all four
    outputs."""
    from spectrseqtools_amd import alignment

    o = AC.make_outcome(specs, rm)
    host = alignment.align_host(o, dp.tolerance, dp.precision, K, split=split, caps=caps)
    dev = alignment.align_device(dp, o, split=split, caps=caps)
    assert np.array_equal(dev.frag_off, o.frag_off)
    AC.assert_equal(dev, tuple(getattr(host, k) for k in FIELDS), ("split", split, rm[:8]))
    return o, dev, host


def device_args(dp, o):
    """sst_align_args over device copies of an outcome's arrays, and the tensors (inputs, outputs)."""
    import torch

    from spectrseqtools_amd import _native

    dev = torch.device("cuda", dp.device_table.engine.device)
    up = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x, dtype=dt).reshape(-1), device=dev)  # noqa: E731
    keep = [up(o.seq_len, np.int32), up(o.pos_off, np.int64), up(o.skeleton.view(np.int64), np.int64),
            up(o.alpha.view(np.int64), np.int64), up(o.frag_off, np.int64), up(o.frag_code, np.uint8),
            up(o.frag_su, np.float64), up(o.frag_obs, np.float64), up(o.frag_min_end, np.int32),
            up(o.frag_max_end, np.int32)]
    nf = int(o.frag_off[-1])
    outs = [torch.zeros(nf, dtype=dt, device=dev) for dt in (torch.uint8, torch.uint8, torch.int32, torch.int16)]
    a = _native.AlignArgs()
    a.n_spec = len(o)
    (a.seq_len, a.pos_off, a.skeleton, a.alpha, a.frag_off, a.frag_code, a.frag_su, a.frag_obs, a.frag_min_end,
     a.frag_max_end) = (x.data_ptr() for x in keep)
    a.tol, a.prec = float(dp.tolerance), float(dp.precision)
    a.status, a.alignable, a.n_fit, a.first = (x.data_ptr() for x in outs)
    torch.cuda.synchronize(dev)
    return a, keep, outs


def window_frags(rng, sets_mass, n, lengths, prec, ws=(0, 1, 30)):
    """n fragments, the four classes in turn, at sums of one random mass per
    position of a window of `lengths` positions (START_END: all of them); W
    cycles through `ws`; every third is a shifted copy (likely a miss); every
    fifth terminal one has its end range widened by one position each way."""
    L = len(sets_mass)
    frags = []
    for i in range(n):
        cls = i % 4
        start, end = bool(cls & 1), bool(cls & 2)
        n_pos = L if cls == 3 else int(rng.choice([x for x in lengths if x <= L]))
        l = 0 if start else L - n_pos if end else int(rng.integers(0, L - n_pos + 1))
        r = l + n_pos - 1
        true = sum(int(rng.choice(sets_mass[p])) for p in range(l, r + 1))
        if i % 3 == 2:
            true += int(rng.integers(1, 400)) * (1 if i % 2 else -1)
        mn, mx = (r, r) if start and not end else (l, l) if end and not start else (0, 0)
        if i % 5 == 4:
            mn, mx = max(0, mn - 1), min(L - 1, mx + 1)
        frags.append((AC.code_of(start, end), true * prec, OBS_W[ws[(i // 4) % len(ws)]], mn, mx))
    return sorted(frags, key=lambda f: f[1])


def edge_positions(rm, K):
    """Pairs of rows on the full alphabet whose run has exactly K sums, an
    arithmetic progression of step d (the smallest difference of two row
    masses), and one more pair, d apart, that makes it K + 1: the construction
    of test_gpu_align.py's test_capacity_edge_and_open.  Returns (positions of
    the K sums, the further pair, d)."""
    rows = range(1, len(rm))
    d = min(abs(rm[a] - rm[b]) for a in rows for b in rows if rm[a] != rm[b])
    pair = {}
    for a in rows:
        for b in rows:
            if rm[b] > rm[a] and (rm[b] - rm[a]) % d == 0:
                pair.setdefault((rm[b] - rm[a]) // d, (a, b))
    pos, steps = [], 0
    while steps < K - 1:  # K - 1 steps: K sums
        k = max(k for k in pair if k <= min(steps + 1, K - 1 - steps))
        pos.append(AC.mask(pair[k]))
        steps += k
    assert steps == K - 1 and 1 in pair
    return pos, AC.mask(pair[1]), d


def prefix_counts(sets):
    out, sums = [], np.zeros(1, np.int64)
    for m in sets:
        sums = np.unique(np.add.outer(sums, np.array(m, dtype=np.int64)))
        out.append(len(sums))
    return out, sums
