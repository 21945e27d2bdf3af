"""GPU tests of the queries at every table compression (4, 8, 16 and 32
masses per packed word).  Mid-table answers cannot depend on the compression;
the table's end (n_cols * C), its last packed word and a reduced alphabet's
extent ceil((35 max + 1) / C) * C can.  Per compression, on a table built on
the device: is_valid, explain, length_bound (first-visit frontier and
SST_LB_REPLAY) and explain_recursion reproduce the reference's answers
(compression_cases.json.gz: ordinary windows, windows at the table's end,
inside its last packed word, at max_mass and past it) and agree with the CPU
oracle (pinned to the same fixture in test_oracle.py) on 2 000 random windows
plus the fixture's end-of-table windows; explain_alpha and length_bound_alpha
with a mask that drops the heaviest row answer OUT_OF_TABLE / ABORTED at the
reduced extent as include/sst.h states and as the oracle on the rebuilt
reduced table below it.  A 70-row table at C = 8 covers the two-word row
masks."""
import numpy as np
import pytest

import _digest
import _oracle as oracle
from conftest import load_golden
from spectrseqtools_amd import _native
from spectrseqtools_amd.pipeline import row_masks

pytestmark = pytest.mark.gpu
COMPRESSIONS = (4, 8, 16, 32)
PREC = 1e-3


@pytest.fixture(scope="module")
def golden():
    return load_golden("compression_cases.json.gz")


class Ctx:
    def __init__(self, golden, C):
        t = golden["tables"][str(C)]
        self.C, self.t, self.cases = C, t, golden["cases"][str(C)]
        self.tol, self.max_len = golden["tolerance"], golden["max_len"]
        self.A = round(golden["mod_rate"] * golden["max_len"])
        self.dev = _native.DeviceTable.build(t["masses"], t["max_mass"], C, engine=_native.get_engine(0))
        self.dev.set_budgets(t["is_mod"], t["caps"])
        self.host = oracle.build_table(t["masses"], t["max_mass"], C)
        self.alph = oracle.Alphabet(t["masses"], t["is_mod"], t["caps"])
        self.limit = t["limit"]


@pytest.fixture(scope="module")
def ctxs(golden):
    made = {}

    def get(C):
        if C not in made:
            made[C] = Ctx(golden, C)
        return made[C]

    yield get
    for c in made.values():
        c.dev.close()


def _inputs(lo, hi):
    """Doubles that quantise to the windows [lo, hi] (as the fixture's)."""
    lo, hi = np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
    q = (hi - lo) // 2
    mass, thr = ((lo + hi) // 2) * PREC, np.where(q > 0, (q - 0.5) * PREC, 0.0)
    assert np.array_equal(np.rint(mass / PREC), (lo + hi) // 2) and np.array_equal(np.ceil(thr / PREC), q)
    return mass, thr


def _budget(A):
    return np.inf if A in ("inf", -1) else int(A)


def _want_status(o):
    if o["status"] == "raise":
        return _native.SST_OUT_OF_TABLE
    if o["result"] is None:
        return _native.SST_NONE
    return _native.SST_SOME if o["result"] else _native.SST_EMPTY


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_table_is_the_references(ctxs, C):
    c = ctxs(C)
    words = c.dev.download()
    assert list(words.shape) == c.t["shape"] and str(words.dtype) == c.t["dtype"]
    assert [int(x) for x in words[:, -1]] == c.t["last_words"]
    assert np.array_equal(words, c.host)


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_fixture_is_valid_and_explain(ctxs, C):
    c = ctxs(C)
    mass = np.array([x["mass"] for x in c.cases])
    thr = np.array([x["threshold"] for x in c.cases])
    got = c.dev.is_valid(mass, thr, c.tol, PREC)
    want = [-1 if x["is_valid"]["status"] == "raise" else int(x["is_valid"]["result"]) for x in c.cases]
    assert got.tolist() == want
    n_some = n_last = 0
    for A in ("0", "2", "inf"):
        res = c.dev.explain(mass, thr, c.tol, PREC, _budget(A))
        for i, x in enumerate(c.cases):
            o = x["explain"][A]
            assert int(res.status[i]) == _want_status(o), (C, A, x["tag"], x["lo"], x["hi"], int(res.status[i]))
            if o["status"] == "ok" and o["result"]:
                assert sorted(res.candidates(i)) == [tuple(r) for r in o["result"]], (C, A, x["tag"], x["lo"])
                n_some += 1
                n_last += x["hi"] >= c.limit - C
        res.close()
    assert n_some > 200 and n_last >= 20


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_fixture_recursion(ctxs, C):
    c = ctxs(C)
    cases = [x for x in c.cases if "recursion" in x]
    assert len(cases) == 100
    mass = np.array([x["mass"] for x in cases])
    thr = np.array([x["threshold"] for x in cases])
    for A in ("0", "2", "inf"):
        res = c.dev.explain_recursion(mass, thr, c.tol, PREC, _budget(A))
        for i, x in enumerate(cases):
            o = x["recursion"][A]
            assert int(res.status[i]) == _want_status(o), (C, A, x["lo"], x["hi"])
            if o["result"]:
                assert sorted(res.candidates(i)) == [tuple(r) for r in o["result"]], (C, A, x["lo"])
        res.close()


@pytest.mark.parametrize("replay", (False, True), ids=("frontier", "replay"))
@pytest.mark.parametrize("C", COMPRESSIONS)
def test_fixture_length_bound(ctxs, C, replay):
    c = ctxs(C)
    su = np.array([x["mass"] for x in c.cases])
    obs = np.array([x["obs_mass"] for x in c.cases])
    for d in ("lower", "upper"):
        out, st = c.dev.length_bound(su, obs, c.tol, PREC, c.max_len, c.A, d, replay=replay)
        for i, x in enumerate(c.cases):
            o = x["length_bound"][d]
            if o["status"] == "raise":
                assert int(st[i]) == _native.SST_OUT_OF_TABLE, (C, d, x["tag"], x["lo"], x["hi"], int(st[i]))
            else:
                assert (int(st[i]), int(out[i])) == (0, o["result"]), (C, d, x["tag"], x["lo"], x["hi"])


def _random_windows(c, n=2000):
    """n random windows (sums of 1..14 rows a little off, and a tenth of them
    anywhere in the table's last 5 000 masses and just past it) plus the
    fixture's windows at the end of the table."""
    rng = np.random.default_rng(100 + c.C)
    w = np.array(c.t["masses"][1:], dtype=np.int64)
    k = rng.integers(1, 15, n)
    s = np.array([w[rng.integers(0, len(w), kk)].sum() for kk in k]) + rng.integers(-3, 4, n)
    far = rng.random(n) < 0.1
    s[far] = rng.integers(c.limit - 5000, c.limit + 100, int(far.sum()))
    hw = rng.integers(0, 41, n)
    end = [(x["lo"], x["hi"]) for x in c.cases if x["tag"] != "ordinary"]
    lo = np.concatenate([s - hw, [e[0] for e in end]])
    hi = np.concatenate([s + hw, [e[1] for e in end]])
    return lo, hi


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_random_windows_vs_oracle(ctxs, C):
    c = ctxs(C)
    lo, hi = _random_windows(c)
    mass, thr = _inputs(lo, hi)
    assert np.array_equal(c.dev.is_valid(mass, thr, c.tol, PREC),
                          oracle.is_valid_batch(c.host, C, mass, thr, c.tol, nthreads=16))
    for A, memo in ((0, True), (2, True), (-1, True), (2, False)):
        want = oracle.explain_digest_batch(c.host, C, c.alph, mass, thr, A, c.tol, with_memo=memo, nthreads=16)
        res = c.dev.explain(mass, thr, c.tol, PREC, _budget(A), with_memo=memo)
        one = lambda i: oracle.explain_table(c.host, C, c.alph, mass[i], thr[i], c.tol, A, with_memo=memo)[1]
        n_some = _digest.assert_equals_oracle(res, want, one, _native, f"C = {C}, A = {A}, memo = {memo}")
        assert n_some > 100 and (want[0] < 0).sum() > 40
        res.close()


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_random_length_bounds_vs_oracle(ctxs, C):
    c = ctxs(C)
    lo, hi = _random_windows(c)
    su, thr = _inputs(lo, hi)
    obs = thr / c.tol
    assert np.array_equal(np.ceil(c.tol * obs / PREC), (hi - lo) // 2)
    for d in ("lower", "upper"):
        want = [oracle.length_bound(c.host, C, c.alph, su[i], obs[i], c.tol, c.max_len, c.A, d) for i in range(len(su))]
        for replay in (False, True):
            out, st = c.dev.length_bound(su, obs, c.tol, PREC, c.max_len, c.A, d, replay=replay)
            for i, wv in enumerate(want):
                if wv is None:
                    assert int(st[i]) == _native.SST_OUT_OF_TABLE, (C, d, replay, lo[i], hi[i], int(st[i]))
                else:
                    assert (int(st[i]), int(out[i])) == (0, wv), (C, d, replay, lo[i], hi[i])
        assert sum(wv is None for wv in want) > 30


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_random_recursion_vs_oracle(ctxs, C):
    c = ctxs(C)
    lo, hi = _random_windows(c, 600)
    keep = hi < 9 * 345048  # sums of up to eight rows: explain_mass_with_recursion enumerates without a table
    mass, thr = _inputs(lo[keep][:300], hi[keep][:300])
    for A in (1, -1):
        res = c.dev.explain_recursion(mass, thr, c.tol, PREC, _budget(A))
        n_some = 0
        for i in range(len(mass)):
            st, sols, _ = oracle.explain_recursion(c.alph, mass[i], thr[i], c.tol, A)
            assert sorted(res.candidates(i)) == sorted(sols), (C, A, i)
            assert (int(res.status[i]) == _native.SST_SOME) == bool(sols), (C, A, i)
            n_some += bool(sols)
        assert n_some > 60
        res.close()


@pytest.mark.parametrize("C", COMPRESSIONS)
def test_reduced_alphabet_extent(ctxs, C):
    """explain_alpha and length_bound_alpha with the heaviest row dropped: the
    reduced table's extent is lim = ceil((35 max(kept) + 1) / C) * C.  A
    window reaching lim is OUT_OF_TABLE, one ending in [lim - C, lim) (the
    reduced table's last packed word) ABORTED, and below that the answer is
    the oracle's on the rebuilt reduced table."""
    c = ctxs(C)
    ms = c.t["masses"]
    kept = list(range(len(ms) - 1))  # rows 0 .. n-2
    red = [ms[r] for r in kept]
    lim = -(-(35 * max(red) + 1) // C) * C
    assert lim < c.limit - 1000
    red_tab = oracle.build_table(red, 35 * max(red), C)
    assert red_tab.shape[1] * C == lim
    alph = oracle.Alphabet(red, [c.t["is_mod"][r] for r in kept], [c.t["caps"][r] for r in kept])
    masks = row_masks(np.array([[r in kept and r > 0 for r in range(len(ms))]]))
    rng = np.random.default_rng(C)
    w = np.array(red[1:], dtype=np.int64)
    lo, hi = [], []
    for e in (lim - C - 1, lim - C, lim - 1, lim):
        for hw in (0, 1, 3, 300):
            hi.append(e), lo.append(e - 2 * hw)
    s = np.array([w[rng.integers(0, len(w), kk)].sum() for kk in rng.integers(1, 13, 120)])
    s = np.concatenate([s, rng.integers(lim - 3000, lim - C, 80)])  # and near the reduced extent, below its last word
    hw = rng.integers(0, 41, len(s))
    s = np.minimum(s, lim - C - 1 - hw)
    lo, hi = np.concatenate([lo, s - hw]), np.concatenate([hi, s + hw])
    mass, thr = _inputs(lo, hi)
    spec = np.zeros(len(mass), np.int32)
    n = {"oot": 0, "aborted": 0, "some": 0}
    for A in (2, -1):
        res = c.dev.explain_alpha(mass, thr, spec, masks, c.tol, PREC, np.full(len(mass), A))
        for i in range(len(mass)):
            if hi[i] >= lim:
                want, key = _native.SST_OUT_OF_TABLE, "oot"
            elif hi[i] >= lim - C:
                want, key = _native.SST_ABORTED, "aborted"
            else:
                st, sols, n_e, _ = oracle.explain_table(red_tab, C, alph, mass[i], thr[i], c.tol, A)
                assert st >= 0
                want = _native.SST_SOME if sols else (_native.SST_EMPTY if n_e else _native.SST_NONE)
                key = "some" if sols else None
                if sols:
                    assert res.candidates(i) == [tuple(kept[x] for x in t) for t in sols], (C, A, lo[i], hi[i])
            assert int(res.status[i]) == want, (C, A, lo[i], hi[i], int(res.status[i]), want)
            if key:
                n[key] += 1
        res.close()
    assert n["oot"] == 8 and n["aborted"] == 16 and n["some"] > 100, n
    obs = thr / c.tol
    out, st = c.dev.length_bound_alpha(mass, obs, spec, masks, c.tol, PREC, c.max_len, c.A, "lower")
    for i in range(len(mass)):
        if hi[i] >= lim:
            assert int(st[i]) == _native.SST_OUT_OF_TABLE, (C, lo[i], hi[i], int(st[i]))
        elif hi[i] >= lim - C:
            assert int(st[i]) == _native.SST_ABORTED, (C, lo[i], hi[i], int(st[i]))
        else:
            want = oracle.length_bound(red_tab, C, alph, mass[i], obs[i], c.tol, c.max_len, c.A, "lower")
            assert want is not None and (int(st[i]), int(out[i])) == (0, want), (C, lo[i], hi[i], int(st[i]))


def test_two_word_row_masks_at_compression_8():
    """A table of more than 64 rows at C = 8 (the lightest 70 rows of the
    alphabet): ordinary windows with the usual budgets, and the windows at the
    table's end with no modification allowed (the full lists there cannot be
    enumerated on 70 rows; with max_modifications = 0 the candidates are the
    canonical rows' sums, while the walk still crosses every row)."""
    C, max_len, tol = 8, 20, 1e-5
    g = load_golden("alphabet.json")
    rows = sorted({r["tolerated_integer_masses"] for r in g["rows"]} | {0})[:71]
    canonical = (305042, 306026, 329053, 345048)
    is_mod = [m not in canonical and m != 0 for m in rows]
    caps = [round(max_len * (0.5 if md else (1.0 if m else 0.0))) for m, md in zip(rows, is_mod)]
    max_mass = 35 * max(rows)
    dev = _native.DeviceTable.build(rows, max_mass, C, engine=_native.get_engine(0))
    dev.set_budgets(is_mod, caps)
    host = oracle.build_table(rows, max_mass, C)
    assert np.array_equal(dev.download(), host)
    alph = oracle.Alphabet(rows, is_mod, caps)
    limit = host.shape[1] * C
    rng = np.random.default_rng(70)
    w = np.array(rows[1:], dtype=np.int64)
    # ordinary: sums of one to three rows (row 70 among them)
    s = np.array([w[rng.integers(0, len(w), kk)].sum() for kk in rng.integers(1, 4, 300)])
    s[:20] = w[-1] + w[rng.integers(0, len(w), 20)]
    hw = rng.integers(0, 21, len(s))
    mass, thr = _inputs(s - hw, s + hw)
    one = lambda A: (lambda i: oracle.explain_table(host, C, alph, mass[i], thr[i], tol, A)[1])
    for A in (10, 1):
        want = oracle.explain_digest_batch(host, C, alph, mass, thr, A, tol, nthreads=16)
        res = dev.explain(mass, thr, tol, PREC, A)
        assert _digest.assert_equals_oracle(res, want, one(A), _native, f"70 rows, A = {A}") > 120
        assert max(max(t) for i in range(20) for t in res.candidates(i)) == 70
        res.close()
    assert np.array_equal(dev.is_valid(mass, thr, tol, PREC), oracle.is_valid_batch(host, C, mass, thr, tol))
    # the table's end: at limit-1, limit, limit+1, inside the last packed word, at its edge, and
    # around the canonical rows' sums nearest the end
    lo, hi = [], []
    for e in (limit - C - 1, limit - C, limit - 1, limit, limit + 1):
        for q in (0, 1, 3, 40):
            hi.append(e), lo.append(e - 2 * q)
    for v in range(limit - C, limit):
        lo.append(v), hi.append(v)
    near = sorted({a * 305042 + b * 306026 + cc * 329053 + d * 345048
                   for a in range(21) for b in range(21) for cc in range(21) for d in range(21)
                   if limit - 3000 <= a * 305042 + b * 306026 + cc * 329053 + d * 345048 < limit})
    assert len(near) >= 10
    for v in near[-30:]:
        lo += [v, v - 4]
        hi += [v, v + 4]
    mass, thr = _inputs(lo, hi)
    want = oracle.explain_digest_batch(host, C, alph, mass, thr, 0, tol, nthreads=16)
    res = dev.explain(mass, thr, tol, PREC, 0)
    n_some = _digest.assert_equals_oracle(res, want, lambda i: oracle.explain_table(
        host, C, alph, mass[i], thr[i], tol, 0)[1], _native, "70 rows, table end")
    assert n_some >= 10 and (want[0] < 0).sum() >= 8
    res.close()
    assert np.array_equal(dev.is_valid(mass, thr, tol, PREC), oracle.is_valid_batch(host, C, mass, thr, tol))
    dev.close()
