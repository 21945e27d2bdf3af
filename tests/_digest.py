"""Per-query digests of an explain result's candidate lists, in numpy: the
same byte length and 64-bit digest as oracle.explain_digest_batch (oracle/
sst_oracle.c: digest_term), so that every query of a result can be compared
with the oracle's exact list, not a sample.  No GPU needed.

A list is the bytes [k][k row indices ascending] of its candidates in the
reference's order; its digest is the sum over its bytes of
splitmix64((position << 8 | byte) + golden) mod 2^64."""
import numpy as np

_G, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
SOME = 1  # _native.SST_SOME (asserted by the GPU tests' use: include/sst.h)


def digest_terms(pos, byte):
    with np.errstate(over="ignore"):
        z = ((pos.astype(np.uint64) << np.uint64(8)) | byte.astype(np.uint64)) + _G
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def list_digest(sols):
    """(byte length, digest) of one list of row tuples (oracle.explain_table's)."""
    by = np.array([b for s in sols for b in (len(s), *s)], dtype=np.uint8)
    return len(by), int(digest_terms(np.arange(len(by)), by).sum(dtype=np.uint64)) if len(by) else 0


def list_lengths(status, count, offset, payload, some=SOME):
    """(the SOME queries, where their lists start, their byte lengths):
    candidate by candidate over all queries at once (as many rounds as the
    longest list has candidates)."""
    qs = np.flatnonzero(np.asarray(status) == some)
    beg = np.asarray(offset)[qs].astype(np.int64)
    c = np.asarray(count)[qs].astype(np.int64)
    pos = beg.copy()
    act = np.flatnonzero(c > 0)
    k = 0
    while len(act):
        pos[act] += 1 + payload[pos[act]].astype(np.int64)
        k += 1
        act = act[c[act] > k]
    return qs, beg, pos - beg


def result_digests(status, count, offset, payload, some=SOME):
    """-> (nbytes, digest), one entry per query: the list's byte length and
    digest where status == some, 0 elsewhere."""
    n = len(status)
    qs, beg, ln = list_lengths(status, count, offset, payload, some)
    nbytes = np.zeros(n, np.int64)
    digest = np.zeros(n, np.uint64)
    nbytes[qs] = ln
    total = int(ln.sum())
    if total:
        start = np.cumsum(ln) - ln  # of each list in the concatenation (ln > 0: a SOME query has a candidate)
        rel = np.arange(total) - np.repeat(start, ln)
        terms = digest_terms(rel, np.asarray(payload)[np.repeat(beg, ln) + rel])
        digest[qs] = np.add.reduceat(terms, start)
    return nbytes, digest


def decode(payload, offset, count):
    """One query's list as row tuples (for a mismatch report)."""
    out, p = [], int(offset)
    for _ in range(int(count)):
        k = int(payload[p])
        out.append(tuple(int(x) for x in payload[p + 1:p + 1 + k]))
        p += 1 + k
    return out


def engine_status(ost, ocnt, native):
    """The oracle's (status, count) as the engine's status codes."""
    return np.where(ost < 0, native.SST_OUT_OF_TABLE,
                    np.where(ost == 0, native.SST_NONE, np.where(ocnt > 0, native.SST_SOME, native.SST_EMPTY)))


def assert_equals_oracle(res, want, oracle_list, native, what="", check_overflow=False):
    """Every query of the fetched result `res` against want = (status, count,
    nbytes, digest) from oracle.explain_digest_batch: status, and for SOME
    queries count, byte length and digest.  On a mismatch: the first query
    and both decoded lists (oracle_list(i) -> the oracle's list of query i)."""
    ost, ocnt, onb, odg = want
    st = np.asarray(res.status).astype(np.int64)
    wst = engine_status(ost, ocnt, native)
    if check_overflow is not False:  # cap_per_query: more candidates than the cap -> OVERFLOW
        wst = np.where((wst == native.SST_SOME) & (ocnt > check_overflow), native.SST_OVERFLOW, wst)
    some = wst == native.SST_SOME
    nb, dg = result_digests(res.status, res.count, res.offset, res.payload, native.SST_SOME)
    cnt = np.asarray(res.count).astype(np.int64)
    bad = (st != wst) | (some & ((cnt != ocnt) | (nb != onb) | (dg != odg)))
    if check_overflow is not False:
        bad |= (wst == native.SST_OVERFLOW) & (cnt != ocnt)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        got = decode(res.payload, res.offset[i], res.count[i]) if st[i] == native.SST_SOME else None
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(st)} queries differ from the oracle; first: query {i}, "
                             f"status {st[i]} (oracle {wst[i]}), count {cnt[i]} ({ocnt[i]}), bytes {nb[i]} ({onb[i]});"
                             f" engine list {got}; oracle list {oracle_list(i)}")
    return int(some.sum())
