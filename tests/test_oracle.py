"""Pin the CPU oracle (oracle/sst_oracle.c) to the reference's own outputs
(tests/golden/, produced by running spectrseq/spectrseqtools unmodified; see
tests/golden/make_golden.py).  CPU only."""
import hashlib

import numpy as np
import pytest

import _digest
import _oracle as oracle
from _golden_ctx import budget, ctx_alphabet, ctx_table, sha
from conftest import load_golden


def test_tiny_tables_verbatim(golden_tables):
    for tiny in golden_tables["tiny"]:
        t = oracle.build_table(tiny["masses"], tiny["max_mass"], tiny["compression"])
        assert list(t.shape) == tiny["shape"]
        assert t.tolist() == tiny["words"], (tiny["masses"], tiny["max_mass"], tiny["compression"])


def test_packed_tables_sha(golden_tables):
    for p in golden_tables["packed"]:
        t = oracle.build_table(p["masses"], p["max_mass"], 32)
        assert list(t.shape) == p["shape"]
        assert sha(t) == p["sha256"], p["what"]
        assert [int(np.bitwise_xor.reduce(t[r])) for r in range(t.shape[0])] == p["checksums_per_row"]


def _table_cases(golden_cases, fn):
    return [c for c in golden_cases["cases"] if c["fn"] == fn]


def test_explain_with_table_cases(golden_cases):
    ctxs = golden_cases["contexts"]
    n = 0
    for c in _table_cases(golden_cases, "table"):
        ctx = ctxs[c["ctx"]]
        st, sols, n_empty, _ = oracle.explain_table(ctx_table(ctx), 32, ctx_alphabet(ctx), c["mass"], c["threshold"],
                                                    ctx["tolerance"], budget(c["max_modifications"]),
                                                    with_memo=c["with_memo"])
        if c["status"] == "raise":
            assert st == -1, c
            continue
        if c["status"] == "none":
            assert st == 0 and not sols, c
            continue
        assert st == 1
        assert sorted(sols) == sorted(tuple(r) for r in c["rows"]), (c["tag"], c["mass"], c["max_modifications"])
        assert len(set(sols)) == len(sols)  # the reference's list has no duplicates either
        n += 1
    assert n > 1500


def test_memo_quirk_is_exercised(golden_cases):
    """Some golden queries differ between with_memo=True and False: the oracle
    must reproduce the memo-on semantics, not the budget-exact one."""
    ctxs = golden_cases["contexts"]
    differ = 0
    for c in _table_cases(golden_cases, "table"):
        if c["status"] != "set" or c["ctx"] not in ("full_L2", "full_L3"):
            continue
        ctx = ctxs[c["ctx"]]
        st, sols, _, _ = oracle.explain_table(ctx_table(ctx), 32, ctx_alphabet(ctx), c["mass"], c["threshold"],
                                              ctx["tolerance"], budget(c["max_modifications"]), with_memo=False)
        if sorted(sols) != sorted(tuple(r) for r in c["rows"]):
            differ += 1
    assert differ > 0


@pytest.fixture(scope="module")
def digest_groups(golden_cases):
    """The golden explain cases grouped by (context, with_memo): one
    explain_digest_batch call each."""
    groups = {}
    for c in _table_cases(golden_cases, "table"):
        groups.setdefault((c["ctx"], bool(c["with_memo"])), []).append(c)
    return groups


def _digest_batch(golden_cases, key, cases, nthreads):
    ctx = golden_cases["contexts"][key[0]]
    return oracle.explain_digest_batch(ctx_table(ctx), 32, ctx_alphabet(ctx), [c["mass"] for c in cases],
                                       [oracle._thr(c["threshold"]) for c in cases],
                                       [oracle._A(budget(c["max_modifications"])) for c in cases], ctx["tolerance"],
                                       with_memo=key[1], nthreads=nthreads)


def test_digest_batch_equals_explain_table_lists(golden_cases, digest_groups):
    """explain_digest_batch on the golden explain cases: status and count are
    explain_table's, byte length and digest are those of explain_table's list
    ([k][rows] per candidate, its order) computed here; the numpy helper gives
    the same from a payload laid out as the engine's (lists apart, not in
    query order)."""
    n_some = 0
    for key, cases in digest_groups.items():
        ctx = golden_cases["contexts"][key[0]]
        st, cnt, nb, dg = _digest_batch(golden_cases, key, cases, 1)
        pay, off, est = [], np.zeros(len(cases), np.int64), np.zeros(len(cases), np.int8)
        for i in reversed(range(len(cases))):  # payload pieces in another order than the queries
            c = cases[i]
            s1, sols, n_empty, _ = oracle.explain_table(ctx_table(ctx), 32, ctx_alphabet(ctx), c["mass"],
                                                        c["threshold"], ctx["tolerance"],
                                                        budget(c["max_modifications"]), with_memo=key[1])
            assert (int(st[i]), int(cnt[i])) == (s1, len(sols)), c
            assert (int(nb[i]), int(dg[i])) == _digest.list_digest(sols), c
            if sols:
                est[i] = _digest.SOME
                pay += [7, 7, 7]  # bytes between the lists
                off[i] = len(pay)
                pay += [b for s in sols for b in (len(s), *s)]
                n_some += 1
        hnb, hdg = _digest.result_digests(est, cnt, off, np.array(pay + [0], dtype=np.uint8))
        assert np.array_equal(hnb, nb) and np.array_equal(hdg, dg), key
    assert n_some > 1500


def test_digest_is_order_sensitive(golden_cases, digest_groups):
    """Swapping two candidates of a list, or two rows inside one candidate,
    changes the digest (every golden list that allows the swap)."""
    n_cand = n_rows = 0
    for key, cases in digest_groups.items():
        ctx = golden_cases["contexts"][key[0]]
        for c in cases[::7]:
            _, sols, _, _ = oracle.explain_table(ctx_table(ctx), 32, ctx_alphabet(ctx), c["mass"], c["threshold"],
                                                 ctx["tolerance"], budget(c["max_modifications"]), with_memo=key[1])
            base = _digest.list_digest(sols)
            if len(sols) >= 2:
                assert _digest.list_digest([sols[-1]] + sols[1:-1] + [sols[0]]) != base, c
                assert _digest.list_digest([sols[1], sols[0]] + sols[2:]) != base, c
                n_cand += 1
            for j, s in enumerate(sols):
                if len(set(s)) >= 2:
                    assert _digest.list_digest(sols[:j] + [s[::-1]] + sols[j + 1:]) != base, c
                    n_rows += 1
                    break
    assert n_cand > 50 and n_rows > 100


def test_digest_batch_thread_count(golden_cases, digest_groups):
    for key, cases in digest_groups.items():
        one, many = (_digest_batch(golden_cases, key, cases, t) for t in (1, 16))
        assert all(np.array_equal(a, b) for a, b in zip(one, many)), key
        st, cnt, _ = oracle.explain_batch(  # the entry point bench.py times: same statuses and counts
            ctx_table(golden_cases["contexts"][key[0]]), 32, ctx_alphabet(golden_cases["contexts"][key[0]]),
            [c["mass"] for c in cases], [oracle._thr(c["threshold"]) for c in cases],
            [oracle._A(budget(c["max_modifications"])) for c in cases], golden_cases["contexts"][key[0]]["tolerance"],
            with_memo=key[1], nthreads=16)
        assert np.array_equal(st, one[0]) and np.array_equal(cnt, one[1]), key


def test_recursion_cases(golden_cases):
    ctxs = golden_cases["contexts"]
    for c in _table_cases(golden_cases, "recursion"):
        ctx = ctxs[c["ctx"]]
        st, sols, _ = oracle.explain_recursion(ctx_alphabet(ctx), c["mass"], c["threshold"], ctx["tolerance"],
                                               budget(c["max_modifications"]))
        assert st == 1
        assert sorted(sols) == sorted(tuple(r) for r in c["rows"]), (c["ctx"], c["mass"])


def test_is_valid_cases(golden_cases):
    ctxs = golden_cases["contexts"]
    for c in _table_cases(golden_cases, "is_valid"):
        ctx = ctxs[c["ctx"]]
        r = oracle.is_valid(ctx_table(ctx), 32, c["mass"], c["threshold"], ctx["tolerance"])
        want = -1 if c["result"] == "raise" else int(c["result"])
        assert r == want, c


def test_length_bound_cases(golden_cases):
    ctxs = golden_cases["contexts"]
    cases = _table_cases(golden_cases, "length_bound")
    assert cases
    for c in cases:
        ctx = ctxs[c["ctx"]]
        su = c.get("su_mass", ctx["su_mass"])
        obs = c.get("obs_mass", ctx["obs_mass"])
        A = round(ctx["mod_rate"] * ctx["max_len"])
        got = oracle.length_bound(ctx_table(ctx), 32, ctx_alphabet(ctx), su, obs, ctx["tolerance"], ctx["max_len"], A,
                                  c["dir"])
        assert got == c["result"], c


def test_population_a7(golden_population):
    ctxs = golden_population["contexts"]
    by_ctx = {}
    for cid, m, t, v in golden_population["a7"]:
        by_ctx.setdefault(cid, []).append((m, t, v))
    for cid, rows in by_ctx.items():
        ctx = ctxs[cid]
        m = np.array([r[0] for r in rows])
        t = np.array([r[1] for r in rows])
        got = oracle.is_valid_batch(ctx_table(ctx), 32, m, t, ctx["tolerance"])
        assert got.tolist() == [int(r[2]) for r in rows], cid


def test_population_a8(golden_population):
    ctxs = golden_population["contexts"]
    for cid, m, t, A, rows in golden_population["a8"][::3]:
        ctx = ctxs[cid]
        st, sols, n_empty, _ = oracle.explain_table(ctx_table(ctx), 32, ctx_alphabet(ctx), m, t, ctx["tolerance"], A)
        if rows is None:
            assert st == 0, (cid, m)
        else:
            assert st == 1 and sorted(sols) == sorted(tuple(r) for r in rows), (cid, m)


def test_is_singleton_restatement_vs_reference():
    g = load_golden("singleton.json.gz")
    ctx = g["context"]
    q = np.array([[x[0], x[1]] for x in g["queries"]])
    want = np.array([x[2] for x in g["queries"]])
    got = oracle.is_singleton_batch(q[:, 0], q[:, 1], ctx["masses"], ctx["tolerance"], ctx["precision"])
    assert want.sum() > 1000 and np.array_equal(got, want)


def test_length_bound_reference_depth():
    """compute_sequence_length_bound at config 5's depth (length_cases.json.gz,
    tests/golden/make_length_golden.py: the reference's own call on 40 reduced
    alphabets it rebuilt itself, windows of 6..20 nucleotides, per-row rate
    profiles and max_modifications of 0..3 or round(0.5 L)): the oracle's
    rebuilt tables have the reference's SHA-256, and both directions equal the
    reference on every window (None: the reference raised).  Budgets bind:
    enough windows' bounds differ from the budget-free ones."""
    import concurrent.futures as cf

    g = load_golden("length_cases.json.gz")
    tabs = {}
    for ai, a in enumerate(g["alphabets"]):
        t = oracle.build_table(a["masses"], max(a["masses"]) * 35, 32)
        assert list(t.shape) == a["table_shape"] and sha(t) == a["table_sha256"], ai
        tabs[ai] = t
    cases = g["cases"]
    assert len(cases) >= 280 and sum(c["lower"] is None for c in cases) == len(g["alphabets"])
    assert sum(c["nucleotides"] >= 15 for c in cases) >= 20  # windows of 15..20 nucleotides

    def one(c, free=False):
        a = g["alphabets"][c["alpha"]]
        caps = [255] * len(c["caps"]) if free else c["caps"]
        alph = oracle.Alphabet(a["masses"], c["is_mod"], caps)
        return tuple(oracle.length_bound(tabs[c["alpha"]], 32, alph, c["su_mass"], c["obs_mass"], c["tolerance"],
                                         c["max_len"], 255 if free else c["max_modifications"], d)
                     for d in ("lower", "upper"))

    with cf.ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL
        got = list(ex.map(one, cases))
    for c, (lo, up) in zip(cases, got):
        assert (lo, up) == (c["lower"], c["upper"]), (c["alpha"], c["su_mass"], lo, up, c["lower"], c["upper"])
    # budgets bind on these windows (the first 60 answered ones are enough to show it)
    live = [c for c in cases if c["lower"] is not None][:60]
    with cf.ThreadPoolExecutor(8) as ex:
        free = list(ex.map(lambda c: one(c, True), live))
    assert sum(f != (c["lower"], c["upper"]) for c, f in zip(live, free)) >= 20


@pytest.mark.parametrize("C", (4, 8, 16, 32))
def test_compression_cases(C):
    """The reference's queries on a table of every compression
    (compression_cases.json.gz, tests/golden/make_compression_golden.py: C, G
    and two modifications; windows in the middle, at the table's end, inside
    its last packed word and past max_mass): the oracle builds the
    reference's table (SHA-256) and gives the reference's is_valid, explain
    (max_modifications 0, 2, inf) and length bounds (both directions) on
    every window, raises included, and explain_mass_with_recursion on the
    ordinary ones."""
    g = load_golden("compression_cases.json.gz")
    t, cases = g["tables"][str(C)], g["cases"][str(C)]
    table = oracle.build_table(t["masses"], t["max_mass"], C)
    assert list(table.shape) == t["shape"] and str(table.dtype) == t["dtype"] and sha(table) == t["sha256"]
    assert table.shape[1] * C == t["limit"]
    alph = oracle.Alphabet(t["masses"], t["is_mod"], t["caps"])
    tol = g["tolerance"]
    n_raise = n_set = n_last = 0
    for c in cases:
        want = c["is_valid"]
        got = oracle.is_valid(table, C, c["mass"], c["threshold"], tol)
        assert got == (-1 if want["status"] == "raise" else int(want["result"])), (C, c["tag"], c["lo"], c["hi"])
        for A, want in c["explain"].items():
            st, sols, n_empty, _ = oracle.explain_table(table, C, alph, c["mass"], c["threshold"], tol,
                                                        budget(A) if A == "inf" else int(A))
            if want["status"] == "raise":
                assert st == -1, (C, c["tag"], c["lo"], c["hi"], A)
                n_raise += 1
            elif want["result"] is None:
                assert st == 0 and not sols, (C, c["tag"], c["lo"], c["hi"], A)
            else:
                assert st == 1 and sorted(sols) == [tuple(r) for r in want["result"]], (C, c["tag"], c["lo"], A)
                n_set += bool(sols)
                n_last += bool(sols) and c["hi"] >= t["limit"] - C
        for A, want in c.get("recursion", {}).items():  # (reads the rows only: the same at every C)
            st, sols, _ = oracle.explain_recursion(alph, c["mass"], c["threshold"], tol,
                                                   budget(A) if A == "inf" else int(A))
            assert want["status"] == "ok" and st == (want["result"] is not None), (C, c["lo"], A)
            assert sorted(sols) == [tuple(r) for r in want["result"] or []], (C, c["lo"], c["hi"], A)
        for d, want in c["length_bound"].items():
            got = oracle.length_bound(table, C, alph, c["mass"], c["obs_mass"], tol, g["max_len"],
                                      round(g["mod_rate"] * g["max_len"]), d)
            assert got == (None if want["status"] == "raise" else want["result"]), (C, c["tag"], c["lo"], c["hi"], d)
    assert n_raise > 100 and n_set > 200 and n_last >= 20, (n_raise, n_set, n_last)
