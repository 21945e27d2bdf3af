"""Config 5 with every stage's arrays in HBM: classify_fragments,
the filter_by_explanation fixpoint and the skeleton's speculative bin
queries over many spectra, driven from the host one launch per stage / round
(sst_classify_rows_device, sst_fix_round_device, sst_valid_rows_alpha_device,
sst_bins_count_device / sst_bins_emit_device; kernels in csrc/sst_pipe.hip
and csrc/sst_alpha.hip).  The host only loops the rounds (one 4-byte read per
round: how many spectra are still reducing) and sizes the bin answers (one
8-byte read).

Rows of spectrum g sit in slots 4 * peak_off[g] + i (i < rows[g]), in the
SU order of its classify_fragments frame, so a row's slot offset is the
`index` Predictor.predict gives it (prediction.py:68-72).  PyTorch provides
the device memory, plus the index gathers that set up a masked-explain pass's
per-query budget rows (_lens_pass); every stage's computation -- the rounds'
re-query merge included (sst_requery_merge_device) -- is the library's.

run_batch is the one call over a batch: the six stages, then the dense
per-spectrum hand-off to the MILP stages (sst_handoff_count_device /
sst_handoff_emit_device, csrc/sst_handoff.hip) as a BatchOutcome of host
arrays; a spectrum outside a per-spectrum engine limit (DeviceLimits) runs
the host mirror instead and is spliced in at its position.
"""
import ctypes
import dataclasses
import os
import sys
import time
from dataclasses import dataclass

import numpy as np

from . import _native
from .masses import PHOSPHATE_LINK_MASS
from .pipeline import mask_rows, row_masks

_PROGRESS = os.environ.get("SST_PIPE_PROGRESS") == "1"  # per-launch lines of the long stages on stderr

# Stage 5's one device buffer per GPU for a pass's reach bitsets and
# lowest-rank bytes (tens of GB at 100 k spectra): kept between length passes
# unless the pass trims (allocating and releasing it per call put up to a few
# seconds of hipMalloc / hipFree into the stage, from run to run).
_LEN_BUF = {}


def _length_buffer(dev, nbytes):
    import torch

    key = dev.index if dev.index is not None else 0
    b = _LEN_BUF.get(key)
    if b is None or b.numel() < nbytes:
        _LEN_BUF.pop(key, None)
        b = None
        torch.cuda.empty_cache()
        b = torch.empty(max(256, int(nbytes)), dtype=torch.uint8, device=dev)
        _LEN_BUF[key] = b
    return b


def reserve_length_buffer(dev, nbytes=64 << 30):
    """Allocate stage 5's reach buffer ahead (a serving process's warm-up):
    passes whose batches fit it (length_device's reach_budget_bytes is the
    default size) then allocate nothing.  At most half of the device's free
    memory (ranks sharing a GPU; the frontier's own workspace is allocated in
    the warm-up's pass before this); a pass that needs more allocates it
    then, as without a reservation."""
    import torch

    free, _ = torch.cuda.mem_get_info(dev)
    try:
        _length_buffer(dev, min(int(nbytes), int(free) // 2))
    except torch.OutOfMemoryError:
        release_length_buffer(dev)


def release_length_buffer(dev=None):
    """Free stage 5's reach buffer (every GPU's when dev is None)."""
    import torch

    if dev is None:
        _LEN_BUF.clear()
    else:
        _LEN_BUF.pop(dev.index if dev.index is not None else 0, None)
    torch.cuda.empty_cache()
LB_NOT_RUN = -6  # length_device(spectra=...): the bounds of a spectrum outside the sample
MAX_PEAKS = 16383  # peaks per spectrum (sst_internal.h kPipeMaxPeaksBig: above 4096 in HBM slices)
ERR_BITS = {1: f"a spectrum has more than {MAX_PEAKS} peaks", 2: "a spectrum has more rows than the reserved slices hold",
            4: "a window outside the pair class", 8: "is_valid_mass raised (a window past a table's end)",
            16: "an explanation dict too large for the LDS hash", 32: "rows out of mass order",
            64: "an exact-mode query list overflowed", 128: "an exact-mode answer raised or was capped"}


def _one_stream(fn):
    """Run a stage with the engine and PyTorch on one stream.  The stages mix
    engine launches (the ctx's stream) with PyTorch uploads, fills and reads
    (the caller's current stream); on two streams a kernel could read an
    input before its upload lands, or a read see a buffer before the kernel
    that fills it has run.  The stage runs on a private stream that first
    waits for the caller's, with the engine queued on it
    (sst_ctx_set_stream); the caller's stream waits for it at the end."""
    import functools

    @functools.wraps(fn)
    def run(dp_table, *args, **kw):
        import torch

        eng = dp_table.device_table.engine
        dev = torch.device("cuda", eng.device)
        st = _STREAMS.get(eng.device)
        if st is None:
            st = _STREAMS[eng.device] = torch.cuda.Stream(device=dev)
        caller = torch.cuda.current_stream(dev)
        prev = getattr(eng, "_stage_stream", None)  # an enclosing stage's (stages nest)
        st.wait_stream(caller)
        try:
            with torch.cuda.stream(st):
                eng.set_stream(st.cuda_stream)
                eng._stage_stream = st.cuda_stream
                return fn(dp_table, *args, **kw)
        finally:
            eng.set_stream(prev)
            eng._stage_stream = prev
            caller.wait_stream(st)
    return run


_STREAMS = {}


class _Heartbeat:
    """Prints `what` every `period` seconds on stderr until stop() (a long
    device call holds no Python lock, so a watcher sees the run is alive)."""

    def __init__(self, what, period):
        import threading
        import time

        self._stop = threading.Event()
        t0 = time.perf_counter()

        def run():
            while not self._stop.wait(period):
                print(f"{what}: {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)

        self._t = threading.Thread(target=run, daemon=True)
        self._t.start()

    def stop(self):
        self._stop.set()
        self._t.join()


def _check_err(err):
    e = int(err.item())
    if e:
        known = [v for k, v in ERR_BITS.items() if e & k]
        rest = e & ~sum(ERR_BITS)
        if rest:
            known.append(f"unknown error bits {rest:#x}")
        raise _native.EngineError("device pipeline: " + "; ".join(known))


@dataclass
class DeviceRows:
    """classify_fragments' frames of a batch, on the device."""
    peak_off: object   # torch int64 [S + 1]
    su: object         # torch f64 [4 P] row slots
    obs: object
    meta: object       # torch int32: breakage | sides << 2 | singleton << 4 | peak << 8
    alive: object      # torch uint8
    rows: object       # torch int32 [S]
    valid: object      # torch int8 [4 P] A7 codes (breakage-major) or None
    names: list        # breakage label per code

    def slots(self):
        """The rows as the stages take them (sst_row_slots), from the live tensors."""
        return _native.RowSlots(len(self.peak_off) - 1, self.peak_off.data_ptr(), self.su.data_ptr(),
                                self.obs.data_ptr(), self.meta.data_ptr(), self.alive.data_ptr(), self.rows.data_ptr())


@_one_stream
def classify_device(dp_table, obs, offsets, su_seq, breakage_dict, intensity=None, intensity_cutoff=0.5e6,
                    mass_cutoff=50000, keep_valid=False, device=None):
    """Stage 1 on the device.  obs: every spectrum's peaks (spectrum g:
    obs[offsets[g]:offsets[g+1]]), su_seq[g] its SequenceInformation.su_mass.
    Peaks may come in any order: the kernel ranks each spectrum's peaks by
    mass in LDS (equal masses keep their order, so the rows' SU order and its
    ties are the reference's); the rows' peak positions are the caller's."""
    import torch

    dev = device or torch.device("cuda", dp_table.device_table.engine.device)
    obs_t = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float64), device=dev)
    off_t = torch.as_tensor(np.ascontiguousarray(offsets, dtype=np.int64), device=dev)
    su_t = torch.as_tensor(np.ascontiguousarray(su_seq, dtype=np.float64), device=dev)
    int_t = None if intensity is None else torch.as_tensor(np.ascontiguousarray(intensity, dtype=np.float64),
                                                           device=dev)
    P, S = len(obs), len(offsets) - 1
    weights = list(breakage_dict.keys())
    names = [breakage_dict[w][0] for w in weights]
    shifts = np.array([w * dp_table.precision for w in weights], dtype=np.float64)
    sides = np.array([("START" in n) | (("END" in n) << 1) for n in names], dtype=np.uint8)
    max_w = _max_weight()
    eng = dp_table.device_table.engine
    # spectra of more than 2048 rows run in the context's HBM slices (sst_pipe_reserve_rows)
    peaks = np.diff(np.asarray(offsets, dtype=np.int64))
    if len(peaks):
        eng.check(eng._lib.sst_pipe_reserve_rows(dp_table.device_table.handle,
                                                 min(int(peaks.max()), MAX_PEAKS) * len(shifts)),
                  "sst_pipe_reserve_rows")
    su = torch.empty(max(1, 4 * P), dtype=torch.float64, device=dev)
    ob = torch.empty_like(su)
    meta = torch.empty(max(1, 4 * P), dtype=torch.int32, device=dev)
    alive = torch.zeros(max(1, 4 * P), dtype=torch.uint8, device=dev)
    rows = torch.zeros(max(1, S), dtype=torch.int32, device=dev)
    valid = torch.empty(max(1, len(weights) * P), dtype=torch.int8, device=dev) if keep_valid else None
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    out = DeviceRows(off_t, su, ob, meta, alive, rows, valid, names)
    a = _native.ClassifyArgs(obs_t.data_ptr(), P, None if int_t is None else int_t.data_ptr(), float(intensity_cutoff),
                             float(mass_cutoff), su_t.data_ptr(), shifts.ctypes.data, sides.ctypes.data, len(shifts),
                             float(max_w), float(dp_table.tolerance), float(dp_table.precision),
                             None if valid is None else valid.data_ptr())
    eng.check(eng._lib.sst_classify_rows_device(dp_table.device_table.handle, ctypes.byref(out.slots()),
                                                ctypes.byref(a), err.data_ptr()), "sst_classify_rows_device")
    eng.synchronize()
    _check_err(err)
    return out


def _max_weight(explanation_masses=None):
    from .masses import EXPLANATION_MASSES

    em = explanation_masses if explanation_masses is not None else EXPLANATION_MASSES
    return max(em.get_column("monoisotopic_mass").to_list()) + PHOSPHATE_LINK_MASS


class _ExactLists:
    """Exact-mode (budget-binding) spectra's query lists and their answers
    (sst_exact_io): capacity for a round's queries, the masked explain per
    max_len group, the answers' references."""

    def __init__(self, dp_table, rows, pair_ok, max_len, cap=None):
        import torch

        self.dp = dp_table
        self.rows = rows
        self.max_len = np.asarray(max_len, dtype=np.int64)
        self.dev = rows.su.device
        S = len(rows.rows)
        self.ok = torch.as_tensor(np.asarray(pair_ok, dtype=np.uint8), device=self.dev)
        self.exact = torch.as_tensor(~np.asarray(pair_ok, bool), device=self.dev)
        self.block = torch.zeros(max(1, S), dtype=torch.int64, device=self.dev)
        self.count = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.cap = 0
        self.results = []
        self.io = _native.ExactIO()
        self.io.pair_ok = self.ok.data_ptr()
        self.io.xq_count = self.count.data_ptr()
        self.io.xq_block = self.block.data_ptr()
        self._alloc(max(1024, int(cap or 0)))

    def _alloc(self, cap):
        import torch

        self.cap = cap
        self.mass = torch.empty(cap, dtype=torch.float64, device=self.dev)
        self.thr = torch.empty(cap, dtype=torch.float64, device=self.dev)
        self.spec = torch.empty(cap, dtype=torch.int32, device=self.dev)
        self.single = torch.empty(cap, dtype=torch.uint8, device=self.dev)
        self.st = torch.empty(cap, dtype=torch.int8, device=self.dev)
        self.n = torch.empty(cap, dtype=torch.int32, device=self.dev)
        self.ptr = torch.empty(cap, dtype=torch.int64, device=self.dev)
        io = self.io
        io.xq_mass, io.xq_thr, io.xq_spec = self.mass.data_ptr(), self.thr.data_ptr(), self.spec.data_ptr()
        io.xq_single, io.xq_cap = self.single.data_ptr(), cap
        io.xa_st, io.xa_n, io.xa_ptr = self.st.data_ptr(), self.n.data_ptr(), self.ptr.data_ptr()

    def reset(self):
        self.count.zero_()
        self.results = []

    def prepare(self, active):
        """Before a fixpoint round: room for the exact-mode active spectra's
        queries (their count from sst_dict_count_device on the current rows)."""
        import torch

        dp, r = self.dp, self.rows
        eng = dp.device_table.engine
        S = len(r.rows)
        n_q = torch.zeros(max(1, S), dtype=torch.int32, device=self.dev)
        off = torch.zeros(S + 1, dtype=torch.int64, device=self.dev)
        err = torch.zeros(1, dtype=torch.int32, device=self.dev)
        a = _native.DictArgs(max_weight=float(_max_weight()), tol=float(dp.tolerance), n_q=n_q.data_ptr(),
                             off=off.data_ptr())
        eng.check(eng._lib.sst_dict_count_device(dp.device_table.handle, ctypes.byref(r.slots()), ctypes.byref(a),
                                                 err.data_ptr()), "sst_dict_count_device")
        need = int((n_q[:S].to(torch.int64) * (active[:S].to(torch.bool) & self.exact[:S])).sum().item())
        if need > self.cap:
            self._alloc(need)
        self.reset()

    def answer(self, alpha_dev):
        """The listed queries through the exact masked explain (one pass per
        max_len group), their references into xa_*."""
        import torch

        n = int(self.count.item())
        if n > self.cap:
            raise _native.EngineError("exact-mode query list overflow")
        if n == 0:
            return
        self.st[:n].fill_(-10)
        dst = torch.arange(n, dtype=torch.int64, device=self.dev)
        self.results = _masked_explain_refs(self.dp, alpha_dev, self.mass, self.thr, self.spec, n, self.max_len, dst,
                                            self.ptr, self.n, self.st)


@dataclass
class DeviceFixpoint:
    alpha: np.ndarray     # [S, 2] u64 final alphabets (row masks of the full table)
    rounds: np.ndarray    # [S]
    queries: np.ndarray   # [S] explain queries over all rounds
    history: list         # per round (recorded): (active [S] bool, alpha [S, 2], alive slots)
    n_rounds: int


@_one_stream
def fixpoint_device(dp_table, rows: DeviceRows, max_len, tolerance=None, record=False):
    """Stage 2 on the device: Predictor.filter_by_explanation (prediction.py:
    170-202) for every spectrum, one sst_fix_round_device + one
    sst_valid_rows_alpha_device launch per round, until no alphabet shrinks.
    max_len[s] bounds the budgets (checked as in pipeline.filter_fixpoint)."""
    tolerance = dp_table.tolerance if tolerance is None else tolerance  # prediction.py:219, :280, :315
    import torch

    masses = dp_table.masses
    N = len(masses)
    S = len(rows.rows)
    dev = rows.su.device
    is_mod = np.array([m.is_modification for m in masses])
    rate = np.array([m.modification_rate for m in masses], dtype=np.float64)
    max_len = np.ascontiguousarray(np.broadcast_to(np.asarray(max_len, dtype=np.int64), (S,)))
    # spectra whose budgets can bind on pair windows run in exact mode: their
    # queries go to the exact masked explain (sst_exact_io)
    ok = budgets_pair_ok(dp_table, max_len)
    xio = None if ok.all() else _ExactLists(dp_table, rows, ok, max_len)
    full = np.zeros((1, N), bool)
    full[0, 1:] = True
    alpha = torch.as_tensor(np.repeat(row_masks(full), S, axis=0).view(np.int64), device=dev).contiguous()
    alpha_next = torch.empty_like(alpha)
    active = torch.ones(S, dtype=torch.uint8, device=dev)
    active_next = torch.empty_like(active)
    rounds = torch.zeros(S, dtype=torch.int32, device=dev)
    queries = torch.zeros(S, dtype=torch.int32, device=dev)
    ctl = torch.zeros(2, dtype=torch.int32, device=dev)  # [0] spectra whose alphabet shrank, [1] error bits
    n_active, err = ctl[0:1], ctl[1:2]
    eng = dp_table.device_table.engine
    L = eng._lib
    h = dp_table.device_table.handle
    history = []
    n_rounds = 0
    slots = ctypes.byref(rows.slots())
    fa = _native.FixArgs(rounds=rounds.data_ptr(), queries=queries.data_ptr(), n_active=n_active.data_ptr(),
                         max_weight=float(_max_weight()), tol=float(tolerance), prec=float(dp_table.precision))
    torch.cuda.synchronize(dev)
    while True:  # per round: two launches, one synchronize, one 8-byte read
        xp = None
        if xio is not None:  # list capacity: the round's queries of the exact-mode spectra
            xio.prepare(active)
            xp = ctypes.byref(xio.io)
        fa.alpha, fa.alpha_next = alpha.data_ptr(), alpha_next.data_ptr()
        fa.active, fa.active_next = active.data_ptr(), active_next.data_ptr()
        eng.check(L.sst_fix_round_device(h, slots, ctypes.byref(fa), err.data_ptr(), xp), "sst_fix_round_device")
        if xio is not None:  # the listed queries answered exactly, then the exact-mode half of the round
            xio.answer(alpha)
            eng.check(L.sst_fix_finish_device(h, slots, ctypes.byref(fa), err.data_ptr(), xp),
                      "sst_fix_finish_device")
        # re-filter only the spectra whose alphabet shrank: an unchanged alphabet is
        # the table the rows already passed (round 1: classify's full table)
        eng.check(L.sst_valid_rows_alpha_device(h, slots, alpha_next.data_ptr(), active_next.data_ptr(),
                                                float(tolerance), float(dp_table.precision), err.data_ptr()),
                  "sst_valid_rows_alpha_device")
        eng.synchronize()
        n_rounds += 1
        if record:
            history.append((active.cpu().numpy().astype(bool), alpha_next.cpu().numpy().view(np.uint64).copy(),
                            rows.alive.cpu().numpy().astype(bool)))
        n_act, e = (int(x) for x in ctl.cpu().tolist())
        if e:
            _check_err(err)
        alpha, alpha_next = alpha_next, alpha
        active, active_next = active_next, active
        if n_act == 0:
            break
    return DeviceFixpoint(alpha.cpu().numpy().view(np.uint64).copy(), rounds.cpu().numpy(),
                          queries.cpu().numpy(), history, n_rounds)


def to_classified(rows: DeviceRows, alive_only=True):
    """The device rows back on the host as pipeline.Classified (spectrum-major,
    each spectrum's rows in SU order; with alive_only the rows the fixpoint
    kept) -- the input of the host stages after the fixpoint (bin queries)."""
    from .pipeline import Classified

    off = rows.peak_off.cpu().numpy()
    cnt = rows.rows.cpu().numpy().astype(np.int64)[:len(off) - 1]
    S = len(cnt)
    spec = np.repeat(np.arange(S), cnt)
    local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    slot = 4 * off[:-1][spec] + local
    su, ob = rows.su.cpu().numpy()[slot], rows.obs.cpu().numpy()[slot]
    meta = rows.meta.cpu().numpy()[slot]
    keep = rows.alive.cpu().numpy()[slot].astype(bool) if alive_only else np.ones(len(slot), bool)
    spec, su, ob, meta = spec[keep], su[keep], ob[keep], meta[keep]
    offsets = np.searchsorted(spec, np.arange(S + 1))
    return Classified(spec, su, ob, (meta >> 8).astype(np.int64), (meta & 3).astype(np.int64),
                      ((meta >> 4) & 1).astype(bool), rows.names, offsets, 0, 0)


@dataclass
class DeviceBins:
    """The skeleton's speculative bin queries of every spectrum, answered on
    its alphabet (spectrum-major: START side, then END; bins in order)."""
    q_off: np.ndarray     # [S + 1] query offsets per spectrum
    status: object        # torch int8 [Q]: SST_NONE / EMPTY / SOME (-10 off the pair class when not answered)
    count: object         # torch int32 [Q] candidates
    deferred: dict = None  # the off-pair-class queries' masked explain: n, per max_len group results, tallies
    q_off_dev: object = None  # torch int64 [S + 1] (the walk's view of the speculative queries)
    q0_dev: object = None     # torch int32 [S] the START side's count
    alpha_dev: object = None  # torch int64 [S, 2] the alphabets they were answered on


@_one_stream
def bins_device(dp_table, rows: DeviceRows, alpha, tolerance=None, max_len=None):
    """Stage 3 on the device (SkeletonBuilder._predict_skeleton's bins,
    skeleton_building.py:114-160) over the rows the fixpoint kept
    (rows.alive) and the final alphabets `alpha` ([S, 2] u64 row masks).
    Pair-class windows are answered by k_bins_emit; with max_len (per
    spectrum) the others -- the sides' first bins' whole masses and wide bin
    differences -- are listed by it and answered by the masked explain
    (sst_explain_alpha_batch_device, the DFS roles on each spectrum's
    alphabet), one pass per max_len group (its budgets: round(0.5 max_len),
    caps round(max_len * rate), common.py:55, mass_explanation.py:158-172)."""
    tolerance = dp_table.tolerance if tolerance is None else tolerance  # prediction.py:219, :280, :315
    import torch

    S = len(rows.rows)
    dev = rows.su.device
    a = torch.as_tensor(np.ascontiguousarray(alpha, dtype=np.uint64).view(np.int64), device=dev)
    n_q = torch.zeros(max(1, S), dtype=torch.int32, device=dev)
    n_q0 = torch.zeros(max(1, S), dtype=torch.int32, device=dev)
    q_off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    eng = dp_table.device_table.engine
    L = eng._lib
    h = dp_table.device_table.handle
    slots = ctypes.byref(rows.slots())
    ba = _native.BinsArgs(alpha=a.data_ptr(), tol=float(tolerance), prec=float(dp_table.precision),
                          n_q=n_q.data_ptr(), n_q0=n_q0.data_ptr(), q_off=q_off.data_ptr())
    torch.cuda.synchronize(dev)
    eng.check(L.sst_bins_count_device(h, slots, ctypes.byref(ba), err.data_ptr()), "sst_bins_count_device")
    eng.synchronize()
    _check_err(err)
    total = int(q_off[S].item())
    status = torch.empty(max(1, total), dtype=torch.int8, device=dev)
    count = torch.empty(max(1, total), dtype=torch.int32, device=dev)
    defer = max_len is not None
    pok = None
    if defer:
        ok = budgets_pair_ok(dp_table, np.broadcast_to(np.asarray(max_len, dtype=np.int64), (S,)))
        if not ok.all():  # exact-mode spectra: every window to the masked explain
            pok = torch.as_tensor(ok.astype(np.uint8), device=dev)
        d_mass = torch.empty(max(1, total), dtype=torch.float64, device=dev)
        d_thr = torch.empty_like(d_mass)
        d_spec = torch.empty(max(1, total), dtype=torch.int32, device=dev)
        d_q = torch.empty(max(1, total), dtype=torch.int64, device=dev)
        n_def = torch.zeros(1, dtype=torch.int32, device=dev)
        ba.def_mass, ba.def_thr, ba.def_spec = d_mass.data_ptr(), d_thr.data_ptr(), d_spec.data_ptr()
        ba.def_q, ba.n_def, ba.pair_ok = d_q.data_ptr(), n_def.data_ptr(), None if pok is None else pok.data_ptr()
    ba.status, ba.count = status.data_ptr(), count.data_ptr()
    eng.check(L.sst_bins_emit_device(h, slots, ctypes.byref(ba), err.data_ptr()), "sst_bins_emit_device")
    eng.synchronize()
    _check_err(err)
    out = DeviceBins(q_off.cpu().numpy(), status[:total], count[:total], q_off_dev=q_off, q0_dev=n_q0,
                     alpha_dev=a)
    if defer:
        out.deferred = answer_deferred(dp_table, a, d_mass, d_thr, d_spec, d_q, int(n_def.item()), max_len,
                                       status, count)
    return out


def answer_deferred(dp_table, alpha, d_mass, d_thr, d_spec, d_q, n, max_len, status, count):
    """The listed off-pair-class windows through the masked explain with
    their spectra's budgets (one pass, per-query budgets: the rows' caps
    follow max_len); statuses and counts scattered into the bin-query
    arrays.  Returns the pass's result and the list (in its order)."""
    import torch

    info = {"queries": n, "groups": [], "results": []}
    if n == 0:
        return info
    spec = d_spec[:n].cpu().numpy()
    ml = np.asarray(max_len, dtype=np.int64)[spec]
    info["spec"], info["mass"], info["thr"] = spec, d_mass[:n].cpu().numpy(), d_thr[:n].cpu().numpy()
    res = _lens_pass(dp_table, alpha, d_mass, d_thr, d_spec, n, max_len)
    res.fetch_device()
    idx = d_q[:n]
    status[idx] = torch.as_tensor(res.status, device=status.device)
    count[idx] = torch.as_tensor(res.count.astype(np.int32), device=count.device)
    Ls, ks = np.unique(ml, return_counts=True)
    info["groups"] = [(int(L), int(k)) for L, k in zip(Ls, ks)]
    info["results"].append((0, res))
    info["order"] = np.arange(n)
    info["dst"] = idx.contiguous()  # list position -> bin-query index
    return info


# ---------------------------------------------------------------------------
# Stage 4: SkeletonBuilder._predict_skeleton's walk on the device
# (skeleton_building.py:114-196, 372-482; kernels in csrc/sst_skel.hip)
# ---------------------------------------------------------------------------
def budgets_pair_ok(dp_table, max_len):
    """Per spectrum: budgets cannot bind on a pair-class window (<= 2 items):
    max_modifications = round(0.5 max_len) (common.py:55) and every
    modification row's cap round(max_len * rate) (mass_explanation.py:158-172)
    are >= 2 -- the fast-path theorem for the lane's pair-list answers."""
    masses = dp_table.masses
    is_mod = np.array([m.is_modification for m in masses])
    rate = np.array([m.modification_rate for m in masses], dtype=np.float64)
    ml = np.asarray(max_len, dtype=np.int64).astype(np.float64)
    A = np.round(dp_table.seq.modification_rate * ml).astype(np.int64)
    cap_min = (np.round(np.outer(ml, rate[is_mod])).min(axis=1).astype(np.int64) if is_mod.any()
               else np.full(len(ml), 2, dtype=np.int64))
    return (A >= 2) & (cap_min >= 2)


def name_hashes(dp_table):
    """hash() of each table row's nucleoside name in this interpreter (the
    set order the reference's explanation lists follow, common.py:60-65)."""
    from .mass_explanation import MASS_NAMES

    out = np.zeros(len(dp_table.masses), np.int64)
    for r, m in enumerate(dp_table.masses):
        if r == 0:
            continue
        names = MASS_NAMES[m.mass]
        if len(names) != 1:  # mass_explanation.py:302-318 would expand the product of equal-mass names
            raise NotImplementedError("skeleton walk: an integer mass with several nucleoside names")
        out[r] = hash(names[0])
    return out


@dataclass
class DeviceDict:
    off: object    # torch int64 [S + 1]
    n: object      # torch int32 [S]
    key: object    # torch int64 (double bits, ascending per spectrum)
    thr: object    # torch f64


@_one_stream
def final_dict_device(dp_table, rows: DeviceRows, alpha_dev, tolerance=None, max_len=None):
    """filter_by_explanation's final explanation dict of every spectrum
    (prediction.py:261-329 over the fixpoint's rows and alphabets), as
    sorted (key, last writer's threshold) lists on the device."""
    import torch

    tolerance = dp_table.tolerance if tolerance is None else tolerance
    S = len(rows.rows)
    dev = rows.su.device
    eng = dp_table.device_table.engine
    L = eng._lib
    h = dp_table.device_table.handle
    n_q = torch.zeros(max(1, S), dtype=torch.int32, device=dev)
    off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    slots = ctypes.byref(rows.slots())
    da = _native.DictArgs(alpha_dev.data_ptr(), float(_max_weight()), float(tolerance), float(dp_table.precision),
                          n_q.data_ptr(), off.data_ptr())
    args = (h, slots, ctypes.byref(da), err.data_ptr())
    torch.cuda.synchronize(dev)
    eng.check(L.sst_dict_count_device(*args), "sst_dict_count_device")
    eng.synchronize()
    total = int(off[S].item())
    key = torch.empty(max(1, total), dtype=torch.int64, device=dev)
    thr = torch.empty(max(1, total), dtype=torch.float64, device=dev)
    n_ent = torch.zeros(max(1, S), dtype=torch.int32, device=dev)
    da.key, da.thr, da.n_ent = key.data_ptr(), thr.data_ptr(), n_ent.data_ptr()
    xp = None
    if max_len is not None:
        ok = budgets_pair_ok(dp_table, np.broadcast_to(np.asarray(max_len, dtype=np.int64), (S,)))
        if not ok.all():  # exact-mode spectra: their final-round queries answered by the exact masked explain
            xio = _ExactLists(dp_table, rows, ok, max_len, cap=total)
            xio.reset()
            xp = ctypes.byref(xio.io)
            eng.check(L.sst_dict_list_device(*args, xp), "sst_dict_list_device")
            xio.answer(alpha_dev)
    eng.check(L.sst_dict_build_device(*args, xp), "sst_dict_build_device")
    eng.synchronize()
    _check_err(err)
    return DeviceDict(off, n_ent, key, thr)


def _lens_pass(dp_table, alpha_dev, mass, thr, spec, n, max_len):
    """The masked explain of windows [0, n) on their spectra's alphabets with
    their spectra's budgets (round(max_len * rate) per row,
    round(seq.modification_rate * max_len) modifications: the budgets the
    rebuilt table of skeleton_building.py:212 / prediction.py:207 carries),
    in one pass (sst_explain_alpha_lens_batch_device)."""
    import torch

    dt = dp_table.device_table
    dev = mass.device
    masses = dp_table.masses
    lens = np.unique(np.asarray(max_len, dtype=np.int64))
    caps = np.array([[round(int(L) * m.modification_rate) for m in masses] for L in lens], dtype=np.int64)
    mods_l = torch.as_tensor(np.array([round(dp_table.seq.modification_rate * int(L)) for L in lens], np.int64),
                             device=dev)
    ml_q = torch.as_tensor(np.asarray(max_len, dtype=np.int64), device=dev)[spec[:n].long()]
    qlen = torch.searchsorted(torch.as_tensor(lens, device=dev), ml_q).to(torch.int32).contiguous()
    mods = mods_l[qlen.long()].contiguous()
    res = dt.explain_alpha_lens_device(mass.data_ptr(), thr.data_ptr(), spec.data_ptr(), alpha_dev.data_ptr(),
                                       qlen.data_ptr(), caps, n, dp_table.tolerance, dp_table.precision,
                                       mods.data_ptr())
    res.keep_alive = (qlen, mods)  # read by the pass until it settles
    return res


def _masked_explain_refs(dp_table, alpha_dev, mass, thr, spec, n, max_len, dst, ptr, cnt, st):
    """Windows answered by the masked explain (_lens_pass); each window's
    candidate reference lands at dst[i] of (ptr, cnt, st).  Returns the
    results (their payload backs the references)."""
    if n == 0:
        return []
    res = _lens_pass(dp_table, alpha_dev, mass, thr, spec, n, max_len)
    eng = dp_table.device_table.engine
    eng.check(eng._lib.sst_result_refs_device(res.handle, dst.data_ptr(), ptr.data_ptr(), cnt.data_ptr(),
                                              st.data_ptr()), "sst_result_refs_device")
    return [res]


def merge_requery_round(dp_table, merged, n_merged, block, p_, n_, s_, n_sides):
    """Append one re-query round's answers to the merged per-side lists the
    walk reads as a single round (sst_requery_merge_device: per side the
    earlier rounds' entries, then this round's; sides in order).  merged:
    the previous view (block, ptr, n, st) or None; n_merged its entries;
    block[sid] = start << 32 | count: side sid's entries of this round in p_
    / n_ / s_.  Returns the new view (start << 32 | count per side, ptr, n,
    st) and its entry count -- known on the host, so no device read-back."""
    import torch

    dev = block.device
    n_new = n_merged + len(p_)
    m_block = torch.empty(max(1, n_sides), dtype=torch.int64, device=dev)
    m_ptr = torch.empty(max(1, n_new), dtype=torch.int64, device=dev)
    m_n = torch.empty(max(1, n_new), dtype=torch.int32, device=dev)
    m_st = torch.empty(max(1, n_new), dtype=torch.int8, device=dev)
    tot = torch.empty(max(1, n_sides), dtype=torch.int32, device=dev)
    off = torch.empty(n_sides + 1, dtype=torch.int64, device=dev)
    a = _native.RequeryMergeArgs()
    if merged is not None:
        a.o_block, a.o_ptr, a.o_n, a.o_st = (t.data_ptr() for t in merged)
    a.block, a.ptr, a.n, a.st = block.data_ptr(), p_.data_ptr(), n_.data_ptr(), s_.data_ptr()
    a.n_sides = n_sides
    a.m_block, a.m_ptr, a.m_n, a.m_st = m_block.data_ptr(), m_ptr.data_ptr(), m_n.data_ptr(), m_st.data_ptr()
    dt = dp_table.device_table
    dt.engine.check(dt.engine._lib.sst_requery_merge_device(dt.handle, ctypes.byref(a), tot.data_ptr(),
                                                            off.data_ptr()), "sst_requery_merge_device")
    return (m_block, m_ptr, m_n, m_st), n_new


@dataclass
class DeviceSkeleton:
    """_predict_skeleton of both sides of every spectrum (device arrays)."""
    max_len: np.ndarray   # [S]
    skel_off: np.ndarray  # [S + 1] exclusive prefix of 2 max_len (positions)
    skel: object          # torch int64 [2 total, 2]: spectrum g, side sd, position i at skel_off[g] + sd max_len + i
    min_end: object       # torch int32 [2, slots] (row slots; side 0 START, 1 END)
    max_end: object
    kept: object          # torch uint8 [2, slots]: rows the walk did not reject (alive rows of the side)
    status: np.ndarray    # [2 S] SST_WALK_* per side
    launches: int         # walk launches (re-query rounds + 1, and big-capacity reruns)
    requeries: int        # re-query windows the masked explain answered
    dict_entries: int
    results: list         # the masked explain results the references point into


@_one_stream
def skeleton_device(dp_table, rows: DeviceRows, alpha, max_len, bins=None, tolerance=None, caps=(64, 32),
                    big_caps=(8192, 8192), max_rounds=4096, name_hash=None):
    """Stage 4 on the device: SkeletonBuilder._predict_skeleton for the START
    and END rows of every spectrum (the rows the fixpoint kept, its final
    alphabets `alpha` [S, 2] u64), with filter_by_explanation's final dict.
    `bins`: stage 3's bins_device(..., max_len=max_len) result (computed here
    when None).  caps = (explanations per bin, candidates per query) of the
    lanes' scratch; sides that outgrow them are walked again with big_caps.
    max_rounds bounds the re-query rounds (each answers every suspended side's
    next re-query bin).  name_hash: hash() of each row's nucleoside name (the
    reference's set order, common.py:60-65); None = this interpreter's
    (name_hashes).  A sharded run passes rank 0's to every rank, so that
    every spectrum's walk follows one interpreter's order."""
    import torch

    tolerance = dp_table.tolerance if tolerance is None else tolerance
    S = len(rows.rows)
    dev = rows.su.device
    eng = dp_table.device_table.engine
    L = eng._lib
    h = dp_table.device_table.handle
    max_len = np.ascontiguousarray(np.broadcast_to(np.asarray(max_len, dtype=np.int64), (S,)))
    if bins is None:
        bins = bins_device(dp_table, rows, alpha, tolerance=tolerance, max_len=max_len)
    alpha_dev = bins.alpha_dev
    dct = final_dict_device(dp_table, rows, alpha_dev, tolerance, max_len=max_len)
    Q = int(bins.q_off[-1])
    s_ptr = torch.zeros(max(1, Q), dtype=torch.int64, device=dev)
    s_n = torch.zeros(max(1, Q), dtype=torch.int32, device=dev)
    s_st = torch.full((max(1, Q),), -10, dtype=torch.int8, device=dev)
    results = []
    if bins.deferred is not None and bins.deferred["queries"]:
        d = bins.deferred
        dst = d["dst"]
        for s0, res in d["results"]:
            eng.check(L.sst_result_refs_device(res.handle, dst.data_ptr() + 8 * s0, s_ptr.data_ptr(), s_n.data_ptr(),
                                               s_st.data_ptr()), "sst_result_refs_device")
            results.append(res)
    elif bins.deferred is None:
        raise ValueError("skeleton_device: stage 3 must answer its off-pair-class queries (bins_device(max_len=...))")
    ml_t = torch.as_tensor(max_len.astype(np.int32), device=dev)
    pair_ok = torch.as_tensor(budgets_pair_ok(dp_table, max_len).astype(np.uint8), device=dev)
    skel_off = np.concatenate([[0], np.cumsum(2 * max_len)]).astype(np.int64)
    skel = torch.zeros((max(1, int(skel_off[-1])), 2), dtype=torch.int64, device=dev)
    skel_off_t = torch.as_tensor(skel_off, device=dev)
    slots = int(rows.su.numel())
    min_end = torch.zeros((2, slots), dtype=torch.int32, device=dev)
    max_end = torch.full((2, slots), -1, dtype=torch.int32, device=dev)
    kept = torch.zeros((2, slots), dtype=torch.uint8, device=dev)
    side_rows = torch.zeros(2 * slots, dtype=torch.int16, device=dev)
    status = torch.zeros(max(1, 2 * S), dtype=torch.uint8, device=dev)
    ctl = torch.zeros(3, dtype=torch.int32, device=dev)  # suspended, big, request count
    # the names' str hashes fix the explanation sets' iteration order: this
    # interpreter's, or the caller's (a sharded run uses rank 0's on every rank)
    nh = torch.as_tensor(name_hashes(dp_table) if name_hash is None else np.asarray(name_hash, np.int64), device=dev)
    ml_max = int(max_len.max()) if S else 1
    len_cap = ml_max + 2
    if len_cap > 255:
        raise NotImplementedError("skeleton walk: max_len above 253")
    pos_cap = _native.pyset_table_size(ml_max + 1)
    req_cap = max(1 << 16, Q)
    req_mass = torch.empty(req_cap, dtype=torch.float64, device=dev)
    req_thr = torch.empty_like(req_mass)
    req_spec = torch.empty(req_cap, dtype=torch.int32, device=dev)
    a = _native.WalkArgs()
    a.peak_off, a.cnt, a.r_su, a.r_ob = (rows.peak_off.data_ptr(), rows.rows.data_ptr(), rows.su.data_ptr(),
                                         rows.obs.data_ptr())
    a.r_meta, a.alive, a.alpha, a.max_len = rows.meta.data_ptr(), rows.alive.data_ptr(), alpha_dev.data_ptr(), \
        ml_t.data_ptr()
    a.pair_ok, a.n_spec, a.slots = pair_ok.data_ptr(), S, slots
    a.tol, a.prec, a.rprec = float(tolerance), float(dp_table.precision), 1.0 / float(dp_table.precision)
    a.d_off, a.d_n, a.d_key, a.d_thr = dct.off.data_ptr(), dct.n.data_ptr(), dct.key.data_ptr(), dct.thr.data_ptr()
    a.q_off, a.q0 = bins.q_off_dev.data_ptr(), bins.q0_dev.data_ptr()
    a.s_ptr, a.s_n, a.s_st = s_ptr.data_ptr(), s_n.data_ptr(), s_st.data_ptr()
    a.req_mass, a.req_thr, a.req_spec = req_mass.data_ptr(), req_thr.data_ptr(), req_spec.data_ptr()
    a.req_count, a.req_cap = ctl.data_ptr() + 8, req_cap
    a.name_hash = nh.data_ptr()
    a.side_rows, a.skel_off, a.skel = side_rows.data_ptr(), skel_off_t.data_ptr(), skel.data_ptr()
    a.min_end, a.max_end, a.kept = min_end.data_ptr(), max_end.data_ptr(), kept.data_ptr()
    a.side_status, a.n_suspended, a.n_big = status.data_ptr(), ctl.data_ptr(), ctl.data_ptr() + 4
    a.pos_cap, a.len_cap = pos_cap, len_cap
    # every re-query answer so far, merged per side in round order (block =
    # start << 32 | count per side, then ptr / n / st): the lanes see one
    # round, so the number of re-query rounds is not bounded by the ABI's
    # SST_WALK_MAX_ROUNDS (exact-mode spectra re-query every bin whose
    # predecessor had no explanations through the host)
    merged, n_merged = None, 0
    keep_alive = []
    n_rounds = 0
    run = np.arange(2 * S, dtype=np.int32)
    big = np.zeros(0, np.int32)
    launches = 0
    n_req_total = 0
    # scratch slots: every side's at the small caps (slot = side id), the
    # sides that outgrew them at the big caps (slots in the order they did);
    # a suspended side's state stays in its slot and the relaunch resumes it
    t_small, t_big = _native.pyset_table_size(caps[1]), _native.pyset_table_size(big_caps[1])
    stride_small = _native.walk_scratch_bytes(pos_cap, len_cap, caps[0], caps[1], t_small)
    stride_big = _native.walk_scratch_bytes(pos_cap, len_cap, big_caps[0], big_caps[1], t_big)
    scratch_small = torch.empty(max(1, 2 * S) * stride_small, dtype=torch.uint8, device=dev)
    scratch_big = torch.zeros(0, dtype=torch.uint8, device=dev)  # zeroed: a new slot holds no state
    big_slot = {}
    torch.cuda.synchronize(dev)
    while len(run) or len(big):
        req_block = torch.zeros(max(1, 2 * S), dtype=torch.int64, device=dev)
        a.req_block = req_block.data_ptr()
        a.n_rounds = 0 if merged is None else 1
        if merged is not None:
            a.rq_block[0], a.rq_ptr[0], a.rq_n[0], a.rq_st[0] = (t.data_ptr() for t in merged)
        ctl.zero_()
        for b in big.tolist():
            big_slot.setdefault(b, len(big_slot))
        need = len(big_slot) * stride_big
        if need > scratch_big.numel():
            grown = torch.zeros(max(need, 2 * scratch_big.numel()), dtype=torch.uint8, device=dev)
            grown[:scratch_big.numel()].copy_(scratch_big)
            scratch_big = grown
        for sides, (e_cap, c_cap), t_cap, stride, scr in ((run, caps, t_small, stride_small, scratch_small),
                                                          (big, big_caps, t_big, stride_big, scratch_big)):
            if not len(sides):
                continue
            sides_t = torch.as_tensor(sides, device=dev)
            slots_t = sides_t if scr is scratch_small else torch.as_tensor(
                np.array([big_slot[b] for b in sides.tolist()], np.int32), device=dev)
            a.sides, a.n_sides = sides_t.data_ptr(), len(sides)
            a.slot, a.resume = slots_t.data_ptr(), int(launches > 0)
            a.scratch, a.scratch_stride = scr.data_ptr(), stride
            a.expl_cap, a.cand_cap, a.tset_cap = e_cap, c_cap, t_cap
            eng.check(L.sst_skel_walk_device(h, ctypes.byref(a)), "sst_skel_walk_device")
            keep_alive.append((sides_t, slots_t))
            launches += 1
        eng.synchronize()
        keep_alive.clear()
        n_susp, n_big, n_req = (int(x) for x in ctl.cpu().tolist())
        if _PROGRESS:
            print(f"[skeleton walk] launch {launches}: {n_susp} suspended, {n_big} big, {n_req} re-queries",
                  file=sys.stderr, flush=True)
        st_h = status.cpu().numpy()
        was_big = np.zeros(2 * S, bool)
        was_big[big] = True
        new_big = np.flatnonzero((st_h == _native.WALK_BIG) & ~was_big).astype(np.int32)
        st_h[big[st_h[big] == _native.WALK_BIG]] = _native.WALK_LIMIT  # outgrew the big capacities too
        if len(big):
            status[torch.as_tensor(big.astype(np.int64), device=dev)] = torch.as_tensor(st_h[big], device=dev)
        susp = np.flatnonzero(st_h == _native.WALK_SUSPENDED).astype(np.int32)
        run = susp[~was_big[susp]]
        big = np.concatenate([susp[was_big[susp]], new_big]).astype(np.int32)
        if n_req:
            if n_rounds >= max_rounds:
                break  # the sides still suspended keep SST_WALK_SUSPENDED
            if n_req > req_cap:
                raise _native.EngineError("skeleton walk: re-query list overflow")
            p_ = torch.zeros(n_req, dtype=torch.int64, device=dev)
            n_ = torch.zeros(n_req, dtype=torch.int32, device=dev)
            s_ = torch.full((n_req,), -10, dtype=torch.int8, device=dev)
            dst = torch.arange(n_req, dtype=torch.int64, device=dev)
            res = _masked_explain_refs(dp_table, alpha_dev, req_mass, req_thr, req_spec, n_req, max_len, dst, p_, n_,
                                       s_)
            results.extend(res)
            merged, n_merged = merge_requery_round(dp_table, merged, n_merged, req_block[:2 * S], p_, n_, s_, 2 * S)
            n_rounds += 1
            n_req_total += n_req
    return DeviceSkeleton(max_len, skel_off, skel, min_end, max_end, kept, status.cpu().numpy()[:2 * S], launches,
                          n_req_total, int(dct.n.sum().item()), results)


def skeleton_frames(dp_table, rows: DeviceRows, sk: DeviceSkeleton, g):
    """Spectrum g's walk as the reference's values: per side (START, END) the
    skeleton (sorted names per position), the kept rows' `index` (their place
    among the spectrum's rows: Predictor.predict's SU-order index), min_end
    and max_end -- the fields tests/golden/callers.json.gz records."""
    from .mass_explanation import MASS_NAMES

    ml = int(sk.max_len[g])
    off = int(rows.peak_off[g].item()) * 4
    n = int(rows.rows[g].item())
    alive = rows.alive[off:off + n].cpu().numpy().astype(bool)
    meta = rows.meta[off:off + n].cpu().numpy().astype(np.int64)
    out = {}
    skel = sk.skel[int(sk.skel_off[g]):int(sk.skel_off[g]) + 2 * ml].cpu().numpy().view(np.uint64)
    names = [None] + [MASS_NAMES[m.mass][0] for m in dp_table.masses[1:]]
    for sd, side in enumerate(("START", "END")):
        pos = []
        for i in range(ml):
            m0, m1 = int(skel[sd * ml + i, 0]), int(skel[sd * ml + i, 1])
            rows_i = [r for r in range(len(names)) if (m0 >> r) & 1 or (r >= 64 and (m1 >> (r - 64)) & 1)]
            pos.append(sorted(names[r] for r in rows_i))
        on = alive & (((meta >> (2 + sd)) & 1) == 1)
        kp = sk.kept[sd, off:off + n].cpu().numpy().astype(bool) & on
        idx = np.flatnonzero(kp)
        out[side] = {"skeleton": pos, "kept_index": idx.tolist(),
                     "min_end": sk.min_end[sd, off + idx].cpu().numpy().tolist() if len(idx) else [],
                     "max_end": sk.max_end[sd, off + idx].cpu().numpy().tolist() if len(idx) else []}
    return out


# ---------------------------------------------------------------------------
# Stage 5: select_sequence_length_with_jaccard on the device (its two length
# bounds on each spectrum's skeleton alphabet) and combine_skeleton_sequences
# (skeleton_building.py:315-370, 494-516; mass_table.py:343-487)
# ---------------------------------------------------------------------------
@dataclass
class DeviceLength:
    alpha: np.ndarray     # [S, 2] u64 the skeleton's alphabets
    lower: np.ndarray     # [S] compute_sequence_length_bound(dir="lower")
    upper: np.ndarray     # [S] (dir="upper")
    lb_status: np.ndarray  # [S] 0 ok, else the bound raised (SST_OUT_OF_TABLE / ABORTED / -5)
    seq_len: np.ndarray   # [S] the chosen length
    status: np.ndarray    # [S] SST_JAC_*
    comb_off: np.ndarray  # [S + 1]
    comb: object          # torch int64 [total, 2] the combined skeleton (masks)
    reach_batches: int
    distinct_alphabets: int = 0  # skeleton alphabets (each one's row bitsets built once)
    replay_nodes: object = None  # [S] frontier: memo entries of the bounds' DFS; replay: phase-1 nodes over attempts
    engine: str = "frontier"
    frontier: dict = None  # sst_lbf_stats summed over the batches (frontier engine)


@_one_stream
def length_bounds_alpha_device(dp_table, alpha_sk, su, ob, max_len, caps_len, a0_len, sel=None, engine="frontier",
                               reach_budget_bytes=64 << 30, share_alphabets=True, length_chunk=1 << 30,
                               soft_nodes=1 << 20, heavy_memo=1 << 22, frontier_workspace=0, keep_buffers=False):
    """compute_sequence_length_bound(dir="lower") and (dir="upper")
    (mass_table.py:343-487) for spectra on reduced alphabets (alpha_sk [S, 2]
    u64 row masks; su / ob the SequenceInformation masses; max_len [S]), with
    the budgets per max_len: caps_len[L, r] = round(L * rate_r) (row stride
    MAX_ROWS) and a0_len[L] = round(modification_rate * L).  Only spectra
    `sel` are computed (the others keep lb_status LB_NOT_RUN).  engine:
    "frontier" (the first-visit frontier) or "replay" (the round-4
    per-spectrum DFS replay).  Returns (lower, upper, lb_status, nodes, stats)."""
    import torch

    dt = dp_table.device_table
    eng = dt.engine
    L = eng._lib
    h = dt.handle
    S = len(alpha_sk)
    dev = torch.device("cuda", eng.device) if hasattr(eng, "device") else torch.device("cuda")
    su = np.asarray(su, dtype=np.float64)
    ob = np.asarray(ob, dtype=np.float64)
    ml = np.asarray(max_len, dtype=np.int64)
    prec, tol = dp_table.precision, dp_table.tolerance
    hi = np.rint(su / prec) + np.ceil(tol * ob / prec)  # the window's top (mass_table.py:354-359)
    words = (np.maximum(hi, 0).astype(np.int64) >> 5) + 2
    from .pipeline import mask_rows

    n_rows = len(dp_table.masses)
    # spectra with one skeleton alphabet share its rows' bitsets (built up to
    # the heaviest of their windows): few distinct alphabets among many spectra
    sel = np.arange(S) if sel is None else np.asarray(sel, dtype=np.int64)
    lower = np.zeros(S, np.int64)
    upper = np.zeros(S, np.int64)
    lb_st = np.full(S, LB_NOT_RUN, np.int8)
    lb_st[sel] = 0
    nodes = np.zeros(S, np.int64)
    masses = dp_table.masses
    is_mod = [m.is_modification for m in masses]
    caps_len = np.ascontiguousarray(caps_len, dtype=np.int32)
    a0_len = [int(x) for x in a0_len]
    ml_hi = int(ml[sel].max()) if len(sel) else 1
    if caps_len.shape[0] <= ml_hi or len(a0_len) <= ml_hi or caps_len.shape[1] != _native.MAX_ROWS:
        raise ValueError("length bounds: caps_len / a0_len must cover every max_len")
    # value ranges: the replay's int8 value slots hold max_len + 1 for max_len <= 120 (sst_api.cpp), the
    # frontier's u8 lower values max_len + 1 <= 254
    if ml_hi > (120 if engine == "replay" else 253):
        raise NotImplementedError(f"length bounds ({engine}): max_len {ml_hi} above the engine's limit")
    caps_t = torch.as_tensor(caps_len, device=dev)
    a0_t = torch.as_tensor(np.asarray(a0_len, np.int32), device=dev)
    dt.set_budgets(is_mod, [int(c) for c in caps_len[ml_hi, :len(masses)]])  # the rows' modification flags
    stats = {"batches": 0, "distinct": 0, "frontier": {}}

    def bounds_pass(sel, soft_nodes, memo_first):
        """Both bounds of spectra `sel`, in batches whose row bitsets fit
        the budget; returns the spectra left SST_LB_HEAVY (over soft_nodes)."""
        # spectra with one skeleton alphabet share its rows' bitsets (built up
        # to the heaviest of their windows)
        if share_alphabets:
            uniq, inv = np.unique(alpha_sk[sel], axis=0, return_inverse=True)
            inv = inv.reshape(-1)
        else:
            uniq, inv = alpha_sk[sel], np.arange(len(sel))
        U = len(uniq)
        stats["distinct"] = max(stats["distinct"], U)
        words_u = np.zeros(U, np.int64)
        np.maximum.at(words_u, inv, words[sel])
        K_u = mask_rows(uniq, n_rows)[:, 1:].sum(axis=1).astype(np.int64)
        need_u = 4 * K_u * words_u
        by_u = np.argsort(inv, kind="stable")  # spectra grouped by alphabet
        u_first = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=U))])
        u0 = 0
        while u0 < U:
            u1, tot = u0, 0
            while u1 < U and (u1 == u0 or tot + need_u[u1] <= reach_budget_bytes):
                tot += int(need_u[u1])
                u1 += 1
            nu = u1 - u0
            off_u = np.concatenate([[0], np.cumsum(need_u[u0:u1] // 4)[:-1]]).astype(np.int64)
            bits = torch.empty(max(1, int(tot // 4)), dtype=torch.int32, device=dev)
            # (every device array stays referenced until the batch is done: a
            # temporary's block can be handed to the next allocation at once)
            alu_t = torch.as_tensor(uniq[u0:u1].view(np.int64), device=dev).contiguous()
            wu_t = torch.as_tensor(words_u[u0:u1], device=dev)
            ou_t = torch.as_tensor(off_u, device=dev)
            eng.check(L.sst_reach_rows_device(h, alu_t.data_ptr(), wu_t.data_ptr(), ou_t.data_ptr(), nu,
                                              bits.data_ptr()), "sst_reach_rows_device")
            lu_src = by_u[u_first[u0]:u_first[u1]]
            members = sel[lu_src]  # this batch's spectra
            n = len(members)
            if _PROGRESS:
                eng.synchronize()
                print(f"[length] batch {stats['batches']}: {n} spectra, {nu} alphabets, {tot / 2**20:.1f} MiB of row "
                      f"bitsets, soft node budget {soft_nodes}", file=sys.stderr, flush=True)
            lu = inv[lu_src] - u0  # their alphabets within the batch
            al_t = torch.as_tensor(uniq[u0:u1][lu].view(np.int64), device=dev).contiguous()
            w_t = torch.as_tensor(words_u[u0:u1][lu], device=dev)
            o_t = torch.as_tensor(off_u[lu], device=dev)
            order = np.argsort(ml[members], kind="stable")
            su_t = torch.as_tensor(su[members][order], device=dev)
            ob_t = torch.as_tensor(ob[members][order], device=dev)
            sp_t = torch.as_tensor(order.astype(np.int32), device=dev)
            ql_t = torch.as_tensor(ml[members][order].astype(np.int32), device=dev)
            lo_t = torch.zeros(n, dtype=torch.int64, device=dev)
            up_t = torch.zeros(n, dtype=torch.int64, device=dev)
            st_t = torch.zeros(n, dtype=torch.int8, device=dev)
            nd_t = torch.zeros(n, dtype=torch.int64, device=dev)
            # every max_len in one launch (per-query budgets); a heartbeat line
            # every 30 s while a long replay runs (the call releases the GIL)
            beat = _Heartbeat("[length] replay running", 30.0) if _PROGRESS else None
            for s0 in range(0, n, length_chunk):
                s1 = min(n, s0 + length_chunk)
                q = _native.LengthQueries(
                    su_t.data_ptr() + 8 * s0, ob_t.data_ptr() + 8 * s0, sp_t.data_ptr() + 4 * s0, al_t.data_ptr(),
                    s1 - s0, float(tol), float(prec), ml_hi, a0_len[ml_hi], lo_t.data_ptr() + 8 * s0,
                    up_t.data_ptr() + 8 * s0, st_t.data_ptr() + s0, ql_t.data_ptr() + 4 * s0, caps_t.data_ptr(),
                    a0_t.data_ptr(), nd_t.data_ptr() + 8 * s0)
                eng.check(L.sst_length_bounds_reach_device(
                    h, ctypes.byref(q), bits.data_ptr(), o_t.data_ptr(), w_t.data_ptr(), int(soft_nodes),
                    int(memo_first), int(K_u.max() <= 64)), "sst_length_bounds_reach_device")
            if beat is not None:
                beat.stop()
            idx = members[order]
            lower[idx] = lo_t.cpu().numpy()
            upper[idx] = up_t.cpu().numpy()
            lb_st[idx] = st_t.cpu().numpy()
            nodes[idx] += nd_t.cpu().numpy()
            del bits
            stats["batches"] += 1
            u0 = u1
        return sel[lb_st[sel] == _native.LB_HEAVY]

    def frontier_pass(sel):
        """Both bounds of spectra `sel` by the first-visit frontier
        (sst_length_bounds_frontier_device): per batch of alphabets, the row
        bitsets, then one byte per mass (the lowest kept rank reaching it),
        then every spectrum of the batch in one call."""
        if share_alphabets:
            uniq, inv = np.unique(alpha_sk[sel], axis=0, return_inverse=True)
            inv = inv.reshape(-1)
        else:
            uniq, inv = alpha_sk[sel], np.arange(len(sel))
        U = len(uniq)
        stats["distinct"] = max(stats["distinct"], U)
        words_u = np.zeros(U, np.int64)
        np.maximum.at(words_u, inv, words[sel])
        K_u = mask_rows(uniq, n_rows)[:, 1:].sum(axis=1).astype(np.int64)
        need_u = 4 * K_u * words_u + 32 * words_u
        by_u = np.argsort(inv, kind="stable")
        u_first = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=U))])
        batches, u0 = [], 0
        while u0 < U:
            u1, tot = u0, 0
            while u1 < U and (u1 == u0 or tot + need_u[u1] <= reach_budget_bytes):
                tot += int(need_u[u1])
                u1 += 1
            batches.append((u0, u1))
            u0 = u1
        # one buffer for every batch's row bitsets and lowest-rank bytes, sized
        # to the largest (a fresh allocation of tens of GB per batch, and its
        # release, idled the GPU for 0.1 s each), kept across passes unless
        # keep_buffers is False (_length_buffer)
        kw_b = [int((K_u[b0:b1] * words_u[b0:b1]).sum()) for b0, b1 in batches]
        lw_b = [int(32 * words_u[b0:b1].sum()) for b0, b1 in batches]
        lr_at = [(4 * max(1, kw) + 255) // 256 * 256 for kw in kw_b]  # the lowest-rank bytes after the bitsets
        buf = _length_buffer(dev, max([256] + [a_ + max(1, lw) for a_, lw in zip(lr_at, lw_b)]))
        bits = lr = None
        for bi, (u0, u1) in enumerate(batches):
            nu = u1 - u0
            wb = words_u[u0:u1]
            off_u = np.concatenate([[0], np.cumsum(K_u[u0:u1] * wb)[:-1]]).astype(np.int64)
            lr_off = np.concatenate([[0], np.cumsum(32 * wb)[:-1]]).astype(np.int64)
            bits = buf[:4 * max(1, kw_b[bi])].view(torch.int32)
            lr = buf[lr_at[bi]:lr_at[bi] + max(1, lw_b[bi])]
            alu_t = torch.as_tensor(uniq[u0:u1].view(np.int64), device=dev).contiguous()
            wu_t = torch.as_tensor(wb, device=dev)
            ou_t = torch.as_tensor(off_u, device=dev)
            lo_u_t = torch.as_tensor(lr_off, device=dev)
            t_batch = time.perf_counter()
            eng.check(L.sst_reach_rows_device(h, alu_t.data_ptr(), wu_t.data_ptr(), ou_t.data_ptr(), nu,
                                              bits.data_ptr()), "sst_reach_rows_device")
            eng.check(L.sst_reach_lowest_device(h, alu_t.data_ptr(), wu_t.data_ptr(), ou_t.data_ptr(), nu,
                                                bits.data_ptr(), lo_u_t.data_ptr(), lr.data_ptr()),
                      "sst_reach_lowest_device")
            if _PROGRESS:
                eng.synchronize()
            t_reach = time.perf_counter() - t_batch
            lu_src = by_u[u_first[u0]:u_first[u1]]
            members = sel[lu_src]
            n = len(members)
            lu = (inv[lu_src] - u0).astype(np.int32)
            su_t = torch.as_tensor(su[members], device=dev)
            ob_t = torch.as_tensor(ob[members], device=dev)
            sp_t = torch.as_tensor(lu, device=dev)
            ql_t = torch.as_tensor(ml[members].astype(np.int32), device=dev)
            lo_t = torch.zeros(n, dtype=torch.int64, device=dev)
            up_t = torch.zeros(n, dtype=torch.int64, device=dev)
            st_t = torch.zeros(n, dtype=torch.int8, device=dev)
            nd_t = torch.zeros(n, dtype=torch.int64, device=dev)
            fs = _native.LbfStats()
            beat = _Heartbeat("[length] frontier running", 30.0) if _PROGRESS else None
            q = _native.LengthQueries(
                su_t.data_ptr(), ob_t.data_ptr(), sp_t.data_ptr(), alu_t.data_ptr(), n, float(tol), float(prec), ml_hi,
                a0_len[ml_hi], lo_t.data_ptr(), up_t.data_ptr(), st_t.data_ptr(), ql_t.data_ptr(), caps_t.data_ptr(),
                a0_t.data_ptr(), nd_t.data_ptr())
            eng.check(L.sst_length_bounds_frontier_device(h, ctypes.byref(q), lr.data_ptr(), lo_u_t.data_ptr(),
                                                          int(frontier_workspace), ctypes.byref(fs)),
                      "sst_length_bounds_frontier_device")
            if beat is not None:
                beat.stop()
            lower[members] = lo_t.cpu().numpy()
            upper[members] = up_t.cpu().numpy()
            lb_st[members] = st_t.cpu().numpy()
            nodes[members] += nd_t.cpu().numpy()
            fd = fs.as_dict()
            for k_, v_ in fd.items():
                if k_ in ("bands", "key_words", "max_band_groups", "max_band_nodes", "table_slots", "node_cap"):
                    stats["frontier"][k_] = max(stats["frontier"].get(k_, 0), v_)
                elif k_ == "overflow_bits":
                    stats["frontier"][k_] = stats["frontier"].get(k_, 0) | v_
                else:
                    stats["frontier"][k_] = stats["frontier"].get(k_, 0) + v_
            if _PROGRESS:
                print(f"[length] frontier batch {stats['batches']}: {n} spectra, {nu} alphabets, reach "
                      f"{t_reach:.3f}s, batch {time.perf_counter() - t_batch:.3f}s: {fd}", file=sys.stderr, flush=True)
            stats["batches"] += 1
        buf = bits = lr = None  # (views of the cached buffer)
        if not keep_buffers:
            release_length_buffer(dev)

    if engine == "frontier":
        frontier_pass(sel)
        heavy = []
    elif engine == "replay":
        # light spectra first, under a soft node budget, so that no batch waits
        # for its few heavy spectra; then the heavy ones together, with a larger
        # first memo
        heavy = bounds_pass(sel, soft_nodes, 0) if soft_nodes else sel
    else:
        raise ValueError(f"length_device: engine {engine!r}")
    if len(heavy):
        if _PROGRESS:
            print(f"[length] {len(heavy)} spectra over {soft_nodes} nodes: replayed together", file=sys.stderr,
                  flush=True)
        bounds_pass(heavy, 0, heavy_memo if soft_nodes else 0)
    return lower, upper, lb_st, nodes, stats


@_one_stream
def length_device(dp_table, sk: DeviceSkeleton, alpha_dev, su_seq, obs_seq, reach_budget_bytes=64 << 30,
                  share_alphabets=True, length_chunk=1 << 30, spectra=None, soft_nodes=1 << 20,
                  heavy_memo=1 << 22, engine="frontier", frontier_workspace=0, trim=True):
    """Stage 5: each spectrum's skeleton alphabet (the canonical rows and the
    modifications its START / END skeletons name), both length bounds on it,
    then the Jaccard selection and the combined skeleton (k_jaccard).
    engine="frontier" (default): sst_reach_rows_device + sst_reach_lowest_device
    + sst_length_bounds_frontier_device -- the reduced table's pairs from its
    rows' reachability, every node's first visit computed band by band over
    descending masses, no DFS replay; batches of alphabets whose
    bitsets fit `reach_budget_bytes`, every max_len in one call
    (frontier_workspace: the call's device workspace, 0 = its default).
    engine="replay": sst_length_bounds_reach_device, one replay of the
    reference's DFS per spectrum (the round-4 engine, kept for comparison).
    spectra: the bounds for these spectra only (indices; the others get
    lb_status LB_NOT_RUN and Jaccard status SST_JAC_BOUNDS) -- a bounded
    sample where the reference's DFS is too large to replay for all.
    trim: release the frontier's cached workspace (sst_ctx_trim) and the
    reach buffer once the bounds are done, so later stages and other
    allocators get that HBM (trim=False keeps both for the next call, as a
    serving process would; reserve_length_buffer sizes the reach buffer
    ahead)."""
    import torch

    dt = dp_table.device_table
    eng = dt.engine
    L = eng._lib
    h = dt.handle
    S = len(sk.max_len)
    dev = sk.skel.device
    ml = sk.max_len.astype(np.int64)
    ml_t = torch.as_tensor(ml.astype(np.int32), device=dev)
    skel_off_t = torch.as_tensor(sk.skel_off, device=dev)
    a_sk = torch.empty((max(1, S), 2), dtype=torch.int64, device=dev)
    eng.check(L.sst_skeleton_alpha_device(h, S, ml_t.data_ptr(), skel_off_t.data_ptr(), sk.skel.data_ptr(),
                                          alpha_dev.data_ptr(), a_sk.data_ptr()), "sst_skeleton_alpha_device")
    alpha_sk = a_sk.cpu().numpy().view(np.uint64)[:S].copy()
    su = np.asarray(su_seq, dtype=np.float64)
    ob = np.asarray(obs_seq, dtype=np.float64)
    prec = dp_table.precision
    sel = np.arange(S) if spectra is None else np.unique(np.asarray(spectra, dtype=np.int64))
    masses = dp_table.masses
    # budgets by max_len (mass_explanation.py:158-172 as set_budgets): caps
    # round(L * rate) per row, max_modifications round(modification_rate * L)
    ml_hi = int(ml[sel].max()) if len(sel) else 1
    caps_len = np.zeros((ml_hi + 1, _native.MAX_ROWS), np.int32)
    for Lm in range(ml_hi + 1):
        caps_len[Lm, :len(masses)] = [min(round(Lm * m.modification_rate), 1 << 30) for m in masses]
    a0_len = [min(round(dp_table.seq.modification_rate * Lm), 1 << 30) for Lm in range(ml_hi + 1)]
    lower, upper, lb_st, nodes, stats = length_bounds_alpha_device(
        dp_table, alpha_sk, su, ob, ml, caps_len, a0_len, sel=sel, engine=engine,
        reach_budget_bytes=reach_budget_bytes, share_alphabets=share_alphabets, length_chunk=length_chunk,
        soft_nodes=soft_nodes, heavy_memo=heavy_memo, frontier_workspace=frontier_workspace, keep_buffers=not trim)
    if trim:
        eng.trim()
    n_batches, U = stats["batches"], stats["distinct"]
    # Jaccard + combine
    comb_off = np.concatenate([[0], np.cumsum(ml)]).astype(np.int64)
    comb = torch.zeros((max(1, int(comb_off[-1])), 2), dtype=torch.int64, device=dev)
    lo_d = torch.as_tensor(lower, device=dev)
    up_d = torch.as_tensor(upper, device=dev)
    st_d = torch.as_tensor(lb_st, device=dev)
    su_d = torch.as_tensor(su, device=dev)
    rm = torch.as_tensor(np.array([m.mass * prec for m in masses], dtype=np.float64), device=dev)
    co_d = torch.as_tensor(comb_off, device=dev)
    seq_len = torch.zeros(max(1, S), dtype=torch.int32, device=dev)
    jst = torch.zeros(max(1, S), dtype=torch.int8, device=dev)
    from .fragment_classification import MAX_VARIANCE

    ja = _native.JaccardArgs(S, ml_t.data_ptr(), skel_off_t.data_ptr(), sk.skel.data_ptr(), lo_d.data_ptr(),
                             up_d.data_ptr(), st_d.data_ptr(), su_d.data_ptr(), rm.data_ptr(), co_d.data_ptr(),
                             comb.data_ptr(), seq_len.data_ptr(), jst.data_ptr(), float(MAX_VARIANCE))
    eng.check(L.sst_jaccard_device(h, ctypes.byref(ja)), "sst_jaccard_device")
    eng.synchronize()
    return DeviceLength(alpha_sk, lower, upper, lb_st, seq_len.cpu().numpy()[:S], jst.cpu().numpy()[:S], comb_off,
                        comb, n_batches, U, nodes, engine, stats["frontier"])


# ---------------------------------------------------------------------------
# After the skeleton: build_skeleton's fragments and the skeleton-based
# alphabet reduction (prediction.py:88-103, skeleton_building.py:67-109)
# ---------------------------------------------------------------------------
@dataclass
class DevicePost:
    alpha: np.ndarray   # [S, 2] u64 the alphabet after _reduce_alphabet(skeleton nucleotides)
    active: np.ndarray  # [S] 1: the spectrum reached the reduction (its Jaccard length stands)
    alive: object       # torch uint8 row slots: the fragments after the reduction's is_valid filter
    alive_skeleton: object  # torch uint8 row slots: build_skeleton's fragments (before the filter)
    min_end: object     # torch int32 row slots (build_skeleton's, clamped to [0, len))
    max_end: object
    rows_before: int    # fragments build_skeleton returned (all spectra)
    rows_after: int     # after the is_valid filter


@_one_stream
def post_skeleton_device(dp_table, rows: DeviceRows, sk: DeviceSkeleton, ln: DeviceLength, tolerance=None):
    """Predictor.predict after build_skeleton (prediction.py:88-103), every
    spectrum at once: build_skeleton's fragments -- the START walk's kept
    rows, the END walk's kept rows START did not keep, the internal rows no
    kept terminal row shares a peak with, min_end / max_end as
    skeleton_building.py:67-109 sets them (sst_post_skeleton_device) -- then
    _reduce_alphabet on the combined skeleton's nucleotides: the alphabet
    without the modifications the skeleton does not name, and is_valid_mass of
    every remaining fragment on it (sst_valid_rows_alpha_device, :204-227)."""
    import torch

    dt = dp_table.device_table
    eng = dt.engine
    L = eng._lib
    h = dt.handle
    S = len(sk.max_len)
    dev = sk.skel.device
    tol = dp_table.tolerance if tolerance is None else tolerance
    slots = int(rows.alive.numel())
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)  # noqa: E731
    seq_len = i32(ln.seq_len)
    # build_skeleton first runs select_sequence_length_with_lp (skeleton_building.py:
    # 45-57, 198-251): without a solver it only combines the skeletons at every
    # candidate length in [lower, upper], which raises IndexError past max_len
    # (:494-512) -- build_skeleton raises and predict returns its default
    jac_post = np.array(ln.status, dtype=np.int8, copy=True)
    lp_raises = (ln.lb_status == 0) & (ln.lower <= ln.upper) & (ln.upper > np.asarray(sk.max_len, np.int64))
    jac_post[lp_raises & (jac_post == _native.JAC_OK)] = _native.JAC_INDEX
    jst = torch.as_tensor(jac_post, device=dev)
    comb_off = torch.as_tensor(np.ascontiguousarray(ln.comb_off[:-1] if len(ln.comb_off) > S else ln.comb_off,
                                                    dtype=np.int64), device=dev)
    alpha = torch.as_tensor(np.ascontiguousarray(ln.alpha).view(np.int64), device=dev)
    alpha_out = torch.empty_like(alpha)
    active = torch.zeros(max(1, S), dtype=torch.uint8, device=dev)
    alive_out = torch.zeros_like(rows.alive)
    min_out = torch.zeros(slots, dtype=torch.int32, device=dev)
    max_out = torch.zeros(slots, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _native.PostArgs(S, rows.peak_off.data_ptr(), rows.rows.data_ptr(), rows.meta.data_ptr(),
                         rows.alive.data_ptr(), sk.kept.data_ptr(), sk.min_end.data_ptr(), sk.max_end.data_ptr(), slots,
                         seq_len.data_ptr(), jst.data_ptr(), comb_off.data_ptr(), ln.comb.data_ptr(), alpha.data_ptr(),
                         alpha_out.data_ptr(), active.data_ptr(), alive_out.data_ptr(), min_out.data_ptr(),
                         max_out.data_ptr(), err.data_ptr())
    eng.check(L.sst_post_skeleton_device(h, ctypes.byref(a)), "sst_post_skeleton_device")
    alive_skel = alive_out.clone()
    before = int(alive_out.sum().item())
    err2 = torch.zeros(1, dtype=torch.int32, device=dev)
    eng.check(L.sst_valid_rows_alpha_device(h, ctypes.byref(dataclasses.replace(rows, alive=alive_out).slots()),
                                            alpha_out.data_ptr(), active.data_ptr(), float(tol),
                                            float(dp_table.precision), err2.data_ptr()), "sst_valid_rows_alpha_device")
    eng.synchronize()
    if int(err.item()):
        raise _native.EngineError(f"post-skeleton stage: a spectrum of more than {MAX_PEAKS} peaks")
    _check_err(err2)
    return DevicePost(alpha_out.cpu().numpy().view(np.uint64)[:S].copy(), active.cpu().numpy()[:S].copy(),
                      alive_out, alive_skel, min_out, max_out, before, int(alive_out.sum().item()))


# ---------------------------------------------------------------------------
# Per-spectrum outcomes, packed for the gather to rank 0 (config 5 on N GPUs)
# ---------------------------------------------------------------------------
OUTCOME_MAGIC = 0x35435453  # "STC5"


def pack_outcomes(rows: DeviceRows, fx, sk: DeviceSkeleton, ln: DeviceLength, post=None):
    """One rank's config-5 outcome per spectrum as one uint8 device tensor:
    the fixpoint's and the skeleton's alphabets, both length bounds and their
    status, the Jaccard length and status, the walk's per-side status, the
    rows each side's walk kept (a bit per row slot), the combined skeleton
    (max_len positions reserved per spectrum, seq_len used), and with `post`
    (post_skeleton_device) the alphabet after the skeleton-based reduction
    and the fragments that survive it (a bit per row slot)."""
    import torch

    dev = sk.skel.device
    S = len(sk.max_len)
    u8 = lambda t: t.contiguous().view(torch.uint8).reshape(-1)  # noqa: E731
    host = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    kept = (sk.kept & rows.alive.view(1, -1)).reshape(-1)
    pad = (-kept.numel()) % 8
    if pad:
        kept = torch.cat([kept, torch.zeros(pad, dtype=torch.uint8, device=dev)])
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=dev)
    kept_bits = (kept.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8)
    def bits(flags):
        f = flags.reshape(-1)
        pad = (-f.numel()) % 8
        if pad:
            f = torch.cat([f, torch.zeros(pad, dtype=torch.uint8, device=dev)])
        return (f.view(-1, 8).to(torch.int32) * weights).sum(dim=1).to(torch.uint8)

    post_bits = bits(post.alive & rows.alive) if post is not None else None
    head = np.array([OUTCOME_MAGIC, S, int(rows.su.numel()), int(sk.skel_off[-1]), int(ln.comb_off[-1]),
                     int(kept_bits.numel()), 0 if post is None else int(post_bits.numel()), 0], dtype=np.int64)
    parts = [host(head), host(np.asarray(fx.alpha, dtype=np.uint64).view(np.int64)),
             host(ln.alpha.view(np.int64)), host(ln.lower), host(ln.upper), host(ln.lb_status),
             host(ln.seq_len.astype(np.int32)), host(ln.status), host(sk.status), host(sk.max_len.astype(np.int32)),
             ln.comb[:int(ln.comb_off[-1])], kept_bits]
    if post is not None:
        parts += [host(post.alpha.view(np.int64)), host(post.active.astype(np.uint8)), post_bits]
    return torch.cat([u8(p) for p in parts])


def unpack_outcomes(buf):
    """pack_outcomes' bytes (host numpy uint8) -> dict of numpy arrays."""
    b = np.asarray(buf, dtype=np.uint8)
    head = b[:64].view(np.int64)
    if int(head[0]) != OUTCOME_MAGIC:
        raise ValueError("not a config-5 outcome buffer")
    S, slots, _, n_comb, n_kept, n_post = (int(x) for x in head[1:7])
    o = 64
    out = {}

    def take(name, dtype, count):
        nonlocal o
        nb = np.dtype(dtype).itemsize * count
        out[name] = b[o:o + nb].view(dtype).copy()
        o += nb

    take("alpha", np.uint64, 2 * S)
    take("alpha_skeleton", np.uint64, 2 * S)
    take("lower", np.int64, S)
    take("upper", np.int64, S)
    take("lb_status", np.int8, S)
    take("seq_len", np.int32, S)
    take("status", np.int8, S)
    take("walk_status", np.uint8, 2 * S)
    take("max_len", np.int32, S)
    take("combined", np.uint64, 2 * n_comb)
    take("kept_bits", np.uint8, n_kept)
    out["kept"] = np.unpackbits(out.pop("kept_bits"), bitorder="little")[:2 * slots].reshape(2, slots)
    if n_post:
        take("alpha_post", np.uint64, 2 * S)
        take("post_active", np.uint8, S)
        take("post_bits", np.uint8, n_post)
        out["alpha_post"] = out["alpha_post"].reshape(S, 2)
        out["post_alive"] = np.unpackbits(out.pop("post_bits"), bitorder="little")[:slots]
    out["alpha"] = out["alpha"].reshape(S, 2)
    out["alpha_skeleton"] = out["alpha_skeleton"].reshape(S, 2)
    out["combined"] = out["combined"].reshape(-1, 2)
    if o != len(b):
        raise ValueError("outcome buffer size mismatch")
    return out


# ---------------------------------------------------------------------------
# The whole batch in one call, with the dense per-spectrum hand-off to the
# MILP stages (prediction.py:112-168): sst_handoff_count_device /
# sst_handoff_emit_device (csrc/sst_handoff.hip), BatchOutcome, run_batch
# ---------------------------------------------------------------------------
HANDOFF_MAGIC = 0x4F485453  # "STHO"
ROUTE_DEVICE, ROUTE_MIRROR = 0, 1
REASON_PEAKS, REASON_MAX_LEN, REASON_WALK, REASON_FRONTIER = 1, 2, 4, 8
REASON_NAMES = {REASON_PEAKS: "more peaks than limits.max_peaks", REASON_MAX_LEN: "max_len above limits.max_len",
                REASON_WALK: "a side's skeleton walk outgrew the walk capacities",
                REASON_FRONTIER: "the length bounds' frontier outgrew its workspace"}


@dataclass(frozen=True)
class DeviceLimits:
    """The device engines' per-spectrum limits; a spectrum outside
    one is routed to the host mirror by run_batch.  The defaults are the
    engines' own values."""
    max_peaks: int = MAX_PEAKS         # peaks per spectrum (classify_device)
    max_len: int = 253                 # skeleton walk / frontier value range
    walk_caps: tuple = (64, 32)        # skeleton_device caps
    walk_big_caps: tuple = (8192, 8192)  # skeleton_device big_caps
    walk_max_rounds: int = 4096        # skeleton_device max_rounds
    frontier_workspace: int = 0        # length_device frontier_workspace (0: the engine's default)


@_one_stream
def handoff_device(dp_table, rows: DeviceRows, ln: DeviceLength, post: DevicePost, active=None):
    """The hand-off kernels over a batch the six stages have run: the
    fragments that survive the skeleton-based reduction (post.alive) of every
    active spectrum, compacted per spectrum in row order with min_end /
    max_end, and the combined skeleton's seq_len positions
    (sst_handoff_count_device, one 16-byte read of the totals,
    sst_handoff_emit_device), then one download per output array.  active:
    [S] spectra to hand off (default post.active).  Returns a dict of host
    numpy arrays (frag_off, pos_off, index, code, su, obs, min_end, max_end,
    skeleton [total, 2] u64) and "bytes", the bytes the downloads moved."""
    import torch

    dt = dp_table.device_table
    eng = dt.engine
    L = eng._lib
    S = len(ln.seq_len)
    dev = rows.su.device
    act = np.ascontiguousarray(post.active if active is None else active, dtype=np.uint8)[:S]
    act_t = torch.as_tensor(act if S else np.zeros(1, np.uint8), device=dev)
    sl_t = torch.as_tensor(np.ascontiguousarray(ln.seq_len, dtype=np.int32) if S else np.zeros(1, np.int32),
                           device=dev)
    co_t = torch.as_tensor(np.ascontiguousarray(ln.comb_off, dtype=np.int64), device=dev)
    n_frag = torch.zeros(max(1, S), dtype=torch.int32, device=dev)
    n_pos = torch.zeros(max(1, S), dtype=torch.int32, device=dev)
    off = torch.zeros((2, S + 1), dtype=torch.int64, device=dev)  # frag_off, pos_off
    a = _native.HandoffArgs()
    a.n_spec = S
    a.peak_off, a.cnt = rows.peak_off.data_ptr(), rows.rows.data_ptr()
    a.r_su, a.r_ob, a.r_meta = rows.su.data_ptr(), rows.obs.data_ptr(), rows.meta.data_ptr()
    a.flags, a.min_end, a.max_end = post.alive.data_ptr(), post.min_end.data_ptr(), post.max_end.data_ptr()
    a.active, a.seq_len, a.comb_off, a.comb = act_t.data_ptr(), sl_t.data_ptr(), co_t.data_ptr(), ln.comb.data_ptr()
    a.n_frag, a.n_pos = n_frag.data_ptr(), n_pos.data_ptr()
    a.frag_off, a.pos_off = off[0].data_ptr(), off[1].data_ptr()
    torch.cuda.synchronize(dev)
    eng.check(L.sst_handoff_count_device(dt.handle, ctypes.byref(a)), "sst_handoff_count_device")
    eng.synchronize()
    off_h = off.cpu().numpy()
    nf, npos = int(off_h[0, S]), int(off_h[1, S])
    index = torch.empty(max(1, nf), dtype=torch.int32, device=dev)
    code = torch.empty(max(1, nf), dtype=torch.uint8, device=dev)
    su = torch.empty(max(1, nf), dtype=torch.float64, device=dev)
    ob = torch.empty(max(1, nf), dtype=torch.float64, device=dev)
    lo = torch.empty(max(1, nf), dtype=torch.int32, device=dev)
    hi = torch.empty(max(1, nf), dtype=torch.int32, device=dev)
    skel = torch.empty((max(1, npos), 2), dtype=torch.int64, device=dev)
    a.index, a.code, a.su, a.obs = index.data_ptr(), code.data_ptr(), su.data_ptr(), ob.data_ptr()
    a.out_min_end, a.out_max_end, a.skeleton = lo.data_ptr(), hi.data_ptr(), skel.data_ptr()
    eng.check(L.sst_handoff_emit_device(dt.handle, ctypes.byref(a)), "sst_handoff_emit_device")
    eng.synchronize()
    out = {"frag_off": off_h[0].copy(), "pos_off": off_h[1].copy(), "index": index[:nf].cpu().numpy(),
           "code": code[:nf].cpu().numpy(), "su": su[:nf].cpu().numpy(), "obs": ob[:nf].cpu().numpy(),
           "min_end": lo[:nf].cpu().numpy(), "max_end": hi[:nf].cpu().numpy(),
           "skeleton": skel[:npos].cpu().numpy().view(np.uint64)}
    out["bytes"] = int(sum(v.nbytes for v in out.values()))
    return out


def _row_names(dp_table):
    from .mass_explanation import MASS_NAMES

    return [""] + [MASS_NAMES[m.mass][0] for m in dp_table.masses[1:]]


def _segments(off, idx):
    """Source positions of segments idx of a ragged array with offsets off,
    concatenated in that order, and the new offsets."""
    off = np.asarray(off, dtype=np.int64)
    n = (off[1:] - off[:-1])[idx]
    new = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    src = np.repeat(off[:-1][idx] - new[:-1], n) + np.arange(int(new[-1]), dtype=np.int64)
    return src, new


@dataclass
class BatchOutcome:
    """What Predictor.predict holds for every spectrum of a batch when it
    reaches its MILP stages (prediction.py:112-168), as host numpy arrays
    (no device reference is kept): per spectrum whether predict returns
    Prediction.default() (build_skeleton raised; such a spectrum has no
    positions, no fragments and a zero alphabet), where it was computed
    (route / reason), the alphabet after the skeleton-based reduction, the
    skeleton sequence (position masks over the table's rows) and the
    surviving fragments with min_end / max_end, both dense."""
    default: np.ndarray       # [S] bool
    route: np.ndarray         # [S] u8 ROUTE_DEVICE / ROUTE_MIRROR
    reason: np.ndarray        # [S] u8 REASON_* bits (0 on the device route)
    alpha: np.ndarray         # [S, 2] u64 row masks of the table
    seq_len: np.ndarray       # [S] i32
    pos_off: np.ndarray       # [S + 1] i64
    skeleton: np.ndarray      # [pos_off[S], 2] u64 row masks per position
    frag_off: np.ndarray      # [S + 1] i64
    frag_index: np.ndarray    # i32: the fragment's `index` (prediction.py:68-72)
    frag_code: np.ndarray     # u8: breakage code | START << 2 | END << 3 | singleton << 4
    frag_su: np.ndarray       # f64 standard_unit_mass
    frag_obs: np.ndarray      # f64 observed_mass
    frag_min_end: np.ndarray  # i32
    frag_max_end: np.ndarray  # i32
    breakage_names: list      # breakage label per code
    row_names: list           # nucleoside name per table row ("" for row 0)
    row_mass: np.ndarray      # [rows] i64 integer mass per table row

    SPECTRUM_FIELDS = ("default", "route", "reason", "alpha", "seq_len")
    POSITION_FIELDS = ("skeleton",)
    FRAGMENT_FIELDS = ("frag_index", "frag_code", "frag_su", "frag_obs", "frag_min_end", "frag_max_end")
    _DTYPES = {"default": np.bool_, "route": np.uint8, "reason": np.uint8, "alpha": np.uint64, "seq_len": np.int32,
               "pos_off": np.int64, "skeleton": np.uint64, "frag_off": np.int64, "frag_index": np.int32,
               "frag_code": np.uint8, "frag_su": np.float64, "frag_obs": np.float64, "frag_min_end": np.int32,
               "frag_max_end": np.int32, "row_mass": np.int64}

    def __post_init__(self):
        for k, dt in self._DTYPES.items():
            setattr(self, k, np.ascontiguousarray(getattr(self, k), dtype=dt))
        self.alpha = self.alpha.reshape(-1, 2)
        self.skeleton = self.skeleton.reshape(-1, 2)
        self.breakage_names = list(self.breakage_names)
        self.row_names = list(self.row_names)
        S = len(self.default)
        if not (len(self.route) == len(self.reason) == len(self.alpha) == len(self.seq_len) == S and
                len(self.pos_off) == len(self.frag_off) == S + 1):
            raise ValueError("BatchOutcome: per-spectrum arrays of different lengths")
        if int(self.pos_off[-1]) != len(self.skeleton) or \
                any(len(getattr(self, k)) != int(self.frag_off[-1]) for k in self.FRAGMENT_FIELDS):
            raise ValueError("BatchOutcome: dense arrays do not match their offsets")

    def __len__(self):
        return len(self.default)

    @classmethod
    def array_fields(cls):
        return tuple(cls._DTYPES)

    def equals(self, other, ignore=()):
        """Field by field (arrays exactly), apart from the fields in `ignore`."""
        for k in self.array_fields():
            if k not in ignore and not np.array_equal(getattr(self, k), getattr(other, k)):
                return False
        return all(k in ignore or getattr(self, k) == getattr(other, k) for k in ("breakage_names", "row_names"))

    def _names_of(self, mask):
        m0, m1 = int(mask[0]), int(mask[1])
        return [self.row_names[r] for r in range(1, len(self.row_names))
                if ((m0 >> r) & 1 if r < 64 else (m1 >> (r - 64)) & 1)]

    def skeleton_seq(self, g):
        """Spectrum g's skeleton sequence: per position the sorted names."""
        return [sorted(self._names_of(p)) for p in self.skeleton[int(self.pos_off[g]):int(self.pos_off[g + 1])]]

    def fragments(self, g):
        """Spectrum g's fragments as predict's frame at its MILP stages."""
        from .frame import Frame

        s = slice(int(self.frag_off[g]), int(self.frag_off[g + 1]))
        code = self.frag_code[s]
        return Frame({"index": self.frag_index[s].tolist(), "standard_unit_mass": self.frag_su[s].tolist(),
                      "observed_mass": self.frag_obs[s].tolist(),
                      "breakage": [self.breakage_names[c & 3] for c in code.tolist()],
                      "is_singleton": ((code >> 4) & 1).astype(bool).tolist(),
                      "min_end": self.frag_min_end[s].tolist(), "max_end": self.frag_max_end[s].tolist()})

    def alphabet_masses(self, g):
        """The integer masses of spectrum g's alphabet after the skeleton-based
        reduction, as [m.mass for m in dp_table.masses] (0 first)."""
        m0, m1 = int(self.alpha[g, 0]), int(self.alpha[g, 1])
        return [0] + [int(self.row_mass[r]) for r in range(1, len(self.row_mass))
                      if ((m0 >> r) & 1 if r < 64 else (m1 >> (r - 64)) & 1)]

    def take(self, idx):
        """The outcome of spectra idx, in that order."""
        idx = np.asarray(idx, dtype=np.int64)
        p_src, p_off = _segments(self.pos_off, idx)
        f_src, f_off = _segments(self.frag_off, idx)
        kw = {k: getattr(self, k)[idx] for k in self.SPECTRUM_FIELDS}
        kw.update({k: getattr(self, k)[p_src] for k in self.POSITION_FIELDS})
        kw.update({k: getattr(self, k)[f_src] for k in self.FRAGMENT_FIELDS})
        return BatchOutcome(pos_off=p_off, frag_off=f_off, breakage_names=self.breakage_names,
                            row_names=self.row_names, row_mass=self.row_mass, **kw)

    @classmethod
    def concat(cls, outcomes):
        """Several outcomes' spectra one after the other (ranks' shards in
        rank order; the pieces of a splice), offsets rebased."""
        outcomes = list(outcomes)
        if not outcomes:
            raise ValueError("BatchOutcome.concat: nothing to concatenate")
        first = outcomes[0]
        for o in outcomes[1:]:
            if o.breakage_names != first.breakage_names or o.row_names != first.row_names or \
                    not np.array_equal(o.row_mass, first.row_mass):
                raise ValueError("BatchOutcome.concat: outcomes of different tables or breakage dicts")
        kw = {k: np.concatenate([getattr(o, k) for o in outcomes])
              for k in cls.SPECTRUM_FIELDS + cls.POSITION_FIELDS + cls.FRAGMENT_FIELDS}
        for k in ("pos_off", "frag_off"):
            base = np.concatenate([[0], np.cumsum([int(getattr(o, k)[-1]) for o in outcomes])]).astype(np.int64)
            kw[k] = np.concatenate([getattr(o, k)[:-1] + b for o, b in zip(outcomes, base)] + [base[-1:]])
        return cls(breakage_names=first.breakage_names, row_names=first.row_names, row_mass=first.row_mass, **kw)

    def pack(self):
        """One flat uint8 array (magic word, sizes, then every array's bytes):
        what parallel.Gatherer ships from a rank."""
        names = "\n".join(self.breakage_names).encode() + b"\0" + "\n".join(self.row_names).encode()
        parts = [np.ascontiguousarray(getattr(self, k)).reshape(-1).view(np.uint8) for k in self.array_fields()]
        parts.append(np.frombuffer(names, dtype=np.uint8))
        head = np.array([HANDOFF_MAGIC, len(self), int(self.pos_off[-1]), int(self.frag_off[-1]), len(self.row_mass),
                         len(names), 0, 0], dtype=np.int64)
        head[6] = 64 + sum(p.nbytes for p in parts)
        return np.concatenate([head.view(np.uint8)] + parts)

    @classmethod
    def unpack(cls, buf):
        """pack()'s bytes -> BatchOutcome; ValueError for another buffer, a
        truncated or an over-long one."""
        b = np.ascontiguousarray(np.asarray(buf), dtype=np.uint8).reshape(-1)
        if len(b) < 64:
            raise ValueError("not a batch outcome buffer (shorter than its header)")
        head = b[:64].copy().view(np.int64)
        if int(head[0]) != HANDOFF_MAGIC:
            raise ValueError("not a batch outcome buffer (magic word)")
        S, n_pos, n_frag, n_rows, n_names, total = (int(x) for x in head[1:7])
        if min(S, n_pos, n_frag, n_rows, n_names) < 0 or total != len(b):
            raise ValueError("batch outcome buffer size mismatch")
        counts = {"alpha": 2 * S, "pos_off": S + 1, "frag_off": S + 1, "skeleton": 2 * n_pos, "row_mass": n_rows}
        counts.update({k: S for k in ("default", "route", "reason", "seq_len")})
        counts.update({k: n_frag for k in cls.FRAGMENT_FIELDS})
        o = 64
        kw = {}
        for k in cls.array_fields():
            nb = np.dtype(cls._DTYPES[k]).itemsize * counts[k]
            if o + nb > len(b):
                raise ValueError("batch outcome buffer size mismatch")
            kw[k] = b[o:o + nb].copy().view(cls._DTYPES[k])
            o += nb
        if o + n_names != len(b):
            raise ValueError("batch outcome buffer size mismatch")
        brk, _, rown = b[o:].tobytes().partition(b"\0")
        return cls(breakage_names=brk.decode().split("\n") if brk else [],
                   row_names=rown.decode().split("\n") if n_rows else [], **kw)


def _empty_outcome(dp_table, names, S, route=ROUTE_DEVICE):
    z = np.zeros
    return BatchOutcome(default=np.ones(S, bool), route=np.full(S, route, np.uint8), reason=z(S, np.uint8),
                        alpha=z((S, 2), np.uint64), seq_len=z(S, np.int32), pos_off=z(S + 1, np.int64),
                        skeleton=z((0, 2), np.uint64), frag_off=z(S + 1, np.int64), frag_index=z(0, np.int32),
                        frag_code=z(0, np.uint8), frag_su=z(0), frag_obs=z(0), frag_min_end=z(0, np.int32),
                        frag_max_end=z(0, np.int32), breakage_names=names, row_names=_row_names(dp_table),
                        row_mass=[m.mass for m in dp_table.masses])


def mirror_outcome(dp_table, obs, su_mass, seq_mass, max_len, breakage_dict, intensity=None, intensity_cutoff=0.5e6,
                   mass_cutoff=50000, explanation_masses=None, reason=0):
    """One spectrum through the host mirror -- classify_fragments and
    Predictor.predict_skeleton_stage on a DynamicProgrammingTable of its own
    (its SequenceInformation from max_len, su_mass, seq_mass and dp_table's
    modification rate; closed afterwards) -- as a one-spectrum BatchOutcome on
    dp_table's rows.  The mirror has none of the device engines' limits."""
    from .fragment_classification import classify_fragments
    from .frame import Frame
    from .mass_explanation import MASS_NAMES
    from .mass_table import DynamicProgrammingTable, SequenceInformation
    from .masses import EXPLANATION_MASSES
    from .prediction import Predictor

    em = EXPLANATION_MASSES if explanation_masses is None else explanation_masses
    names = [breakage_dict[w][0] for w in breakage_dict]
    out = _empty_outcome(dp_table, names, 1, ROUTE_MIRROR)
    out.reason[0] = reason
    seq = SequenceInformation(max_len=int(max_len), su_mass=float(su_mass), obs_mass=float(seq_mass),
                              modification_rate=dp_table.seq.modification_rate)
    dp = DynamicProgrammingTable(em, compression_rate=dp_table.compression_per_cell, tolerance=dp_table.tolerance,
                                 precision=dp_table.precision, seq=seq, engine=dp_table._engine)
    try:
        cols = {"observed_mass": [float(x) for x in obs]}
        if intensity is not None:
            cols["intensity"] = [float(x) for x in intensity]
        fr = classify_fragments(Frame(cols), dp, breakage_dict, intensity_cutoff=intensity_cutoff,
                                mass_cutoff=mass_cutoff)
        res = Predictor(dp, em).predict_skeleton_stage(fr)
        kept = [m.mass for m in dp.masses[1:]]
    finally:
        dp.close()
    if res is None:
        return out
    skeleton_seq, frags = res
    row_of_mass = {m.mass: r for r, m in enumerate(dp_table.masses) if r}
    row_of_name = {n: r for r, m in enumerate(dp_table.masses) if r for n in MASS_NAMES[m.mass]}

    def mask(rows):
        m = [0, 0]
        for r in rows:
            m[r >> 6] |= 1 << (r & 63)
        return m

    cols = frags.to_dict() if hasattr(frags, "to_dict") else {c: frags.get_column(c).to_list() for c in frags.columns}
    brk = cols["breakage"]
    code = [names.index(b) | ("START" in b) << 2 | ("END" in b) << 3 | bool(s) << 4
            for b, s in zip(brk, cols["is_singleton"])]
    n = len(brk)
    return BatchOutcome(default=[False], route=[ROUTE_MIRROR], reason=[reason],
                        alpha=np.array([mask(row_of_mass[m] for m in kept)], dtype=np.uint64),
                        seq_len=[len(skeleton_seq)], pos_off=[0, len(skeleton_seq)],
                        skeleton=np.array([mask(row_of_name[x] for x in p) for p in skeleton_seq],
                                          dtype=np.uint64).reshape(-1, 2),
                        frag_off=[0, n], frag_index=cols["index"], frag_code=code,
                        frag_su=cols["standard_unit_mass"], frag_obs=cols["observed_mass"],
                        frag_min_end=cols["min_end"], frag_max_end=cols["max_end"], breakage_names=names,
                        row_names=out.row_names, row_mass=out.row_mass)


def run_batch(dp_table, obs, offsets, su_seq, seq_mass, breakage_dict, max_len=None, intensity=None,
              intensity_cutoff=0.5e6, mass_cutoff=50000, limits=DeviceLimits(), fallback="mirror", name_hash=None,
              trim=True, explanation_masses=None, record=None, align=False, align_split=False, align_caps=False,
              align_keep=False, align_final=False, final_max_combos=None, align_robust=False, align_search=False,
              search_horizon=None, search_width=None, length_program=False, length_max_combos=None):
    """These spectra -> what Predictor.predict holds when it reaches its MILP
    stages (prediction.py:63-103), as a BatchOutcome: the six device stages
    (classify_device, fixpoint_device, bins_device, skeleton_device,
    length_device, post_skeleton_device) with `limits`' capacities, the two
    hand-off calls (handoff_device), one download per output array.
    obs / offsets: every spectrum's peaks (spectrum g: obs[offsets[g]:
    offsets[g + 1]]; intensity likewise); su_seq / seq_mass [S] the
    SequenceInformation masses; max_len [S] (None: pipeline.max_len_of over
    explanation_masses' integer masses, cli.py:158-170); name_hash as
    skeleton_device's; trim as length_device's.

    A spectrum outside an engine limit does not fail or starve the batch: one
    over limits.max_peaks or limits.max_len is taken out before stage 1, one
    with a side whose walk ends WALK_LIMIT / WALK_SUSPENDED / WALK_ROUNDS /
    WALK_MISSING after stage 4, one whose length bound is SST_ABORTED after
    stage 5.  fallback="mirror": each of them runs the host mirror
    (mirror_outcome) and its result is spliced in at its position (route 1,
    reason the limit's REASON_* bit); fallback="raise": EngineError naming the
    spectra and the reasons.  The mirror's explanation lists follow this
    interpreter's set order (its str hashes), the device walk name_hash's: a
    sharded run that passes rank 0's hashes runs its ranks under one
    PYTHONHASHSEED so that routed spectra follow the same order.

    The stages' batch-level error bits other than the peak count (ERR_BITS: a
    window outside the pair class, an explanation dict too large for the LDS
    hash, ...) still raise EngineError for the whole batch: the kernels report
    them as one word per batch, and per-spectrum bits would change them.

    record: a dict that receives diagnostics (walk_status [2 S], lb_status,
    replay_nodes, jaccard_status of the spectra the device ran, device_index
    their positions in the batch).

    align=True: also the alignment certificate of every fragment (alignment.py:
    which fragments no window of the skeleton can explain, so filter_with_lp
    need not solve for them); returns (BatchOutcome, AlignOutcome).  Spectra
    the device ran take align_device, mirror-routed ones align_host at the
    device's capacity; the BatchOutcome is the default call's.
    align_split=True implies align and returns the split certificate (both
    with split=True: the open intervals that cut into two closed halves are
    decided too).
    align_caps=True implies align and returns the certificate under the
    program's universal modification cap (align_device(caps=True) on the
    device's spectra, align_host(caps=lp_caps(...)) on the routed ones); it
    combines with align_split.
    align_keep=True implies align_caps and returns the certificate in keep
    mode (align_device(caps=True, keep=True) on the device's spectra,
    align_host(caps=lp_caps(...), keep=lp_row_caps(...)) on the routed ones):
    the AlignOutcome also carries keep, keep_first and spec_free
    (alignment.lp_decisions: DROP / KEEP / SOLVE); it combines with
    align_split.
    align_final=True implies align_keep and align_split and also runs the final
    program by exact enumeration (final_program.py) over the KEEP fragments of
    every spectrum that holds no LP_SOLVE fragment (final_program.final_use);
    returns (BatchOutcome, AlignOutcome, FinalOutcome).  Spectra the device ran
    take final_device, mirror-routed ones final_host; final_max_combos (None:
    final_program.FINAL_DEFAULT_COMBOS) bounds the assignments enumerated per
    spectrum.  The first two are what align_keep with align_split returns.
    align_robust=True implies align_final and runs the robust final program
    instead (final_program.final_use(optional=True): the LP_SOLVE fragments are
    optional, no spectrum is FINAL_UNDECIDED); returns (BatchOutcome,
    AlignOutcome, FinalOutcome, RobustOutcome).  Spectra the device ran take
    final_robust_device, mirror-routed ones final_robust_host
    (final_program.robust_decisions reads the pair).
    align_search=True implies what align_robust implies and runs the robust
    final program with the bounded search in its place: a spectrum above
    final_max_combos (0 is allowed here: every one) is searched, not given up
    (final_program.final_search_host; search_horizon, search_width: its horizon
    and max_width, None: the defaults); returns (BatchOutcome, AlignOutcome,
    FinalOutcome, RobustOutcome, SearchOutcome).  Spectra the device ran take
    final_search_device, mirror-routed ones final_search_host.
    length_program=True: also the length program (length_program.py: the optimum
    of the program select_sequence_length_with_lp builds per candidate length, by
    exact enumeration); a LengthOutcome is returned after the other results
    (alone with the BatchOutcome: a pair).  Spectra the device ran take
    length_program_device on length_cases of the stages' arrays (record
    receives them as length_cases); length_max_combos (None:
    final_program.FINAL_DEFAULT_COMBOS) bounds the assignments enumerated per
    candidate.  The mirror does not expose its two skeletons and bounds, so a
    mirror-routed spectrum has no candidates and is marked undecided:
    length_decisions answers LENGTH_SOLVE for it.  No other result changes, and
    seq_len stays the Jaccard length."""
    from .masses import EXPLANATION_MASSES, TOLERANCE
    from .pipeline import max_len_of

    if fallback not in ("mirror", "raise"):
        raise ValueError(f"run_batch: fallback {fallback!r}")
    em = EXPLANATION_MASSES if explanation_masses is None else explanation_masses
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    S = len(offsets) - 1
    su_seq = np.ascontiguousarray(np.broadcast_to(np.asarray(su_seq, dtype=np.float64), (S,)))
    seq_mass = np.ascontiguousarray(np.broadcast_to(np.asarray(seq_mass, dtype=np.float64), (S,)))
    inten = None if intensity is None else np.ascontiguousarray(intensity, dtype=np.float64)
    if max_len is None:
        max_len = max_len_of(su_seq, TOLERANCE, min(em.get_column("tolerated_integer_masses").to_list()))
    max_len = np.ascontiguousarray(np.broadcast_to(np.asarray(max_len, dtype=np.int64), (S,)))
    names = [breakage_dict[w][0] for w in breakage_dict]
    reason = np.zeros(S, np.uint8)
    peaks = np.diff(offsets)
    reason[peaks > limits.max_peaks] |= REASON_PEAKS
    reason[max_len > limits.max_len] |= REASON_MAX_LEN

    def refuse():
        bad = np.flatnonzero(reason)
        if fallback == "raise" and len(bad):
            what = "; ".join(f"spectrum {int(g)}: " + ", ".join(v for k, v in REASON_NAMES.items() if reason[g] & k)
                             for g in bad[:32])
            raise _native.EngineError(f"device pipeline: {len(bad)} spectra outside the engine limits ({what}"
                                      + (", ..." if len(bad) > 32 else "") + ")")

    refuse()
    d_idx = np.flatnonzero(reason == 0)  # the spectra the device runs
    dev_out = _empty_outcome(dp_table, names, len(d_idx))
    dev_lo = None
    if length_program:
        from . import length_program as length_mod

        dev_lo = length_mod.LengthOutcome.not_computed(len(d_idx))

    def with_length(res, n_mirrored=0, where=None):
        """The results, and the LengthOutcome after them where it was asked for."""
        if dev_lo is None:
            return res
        lo = dev_lo
        if n_mirrored:
            lo = length_mod.LengthOutcome.concat([dev_lo, length_mod.LengthOutcome.not_computed(n_mirrored)]).take(where)
        return (res if isinstance(res, tuple) else (res,)) + (lo,)

    if len(d_idx):
        cut = np.concatenate([[0], np.cumsum(peaks[d_idx])]).astype(np.int64)
        if len(d_idx) == S:
            d_obs, d_int = obs, inten
        else:
            src, _ = _segments(offsets, d_idx)
            d_obs, d_int = obs[src], None if inten is None else inten[src]
        ml = max_len[d_idx]
        rows = classify_device(dp_table, d_obs, cut, su_seq[d_idx], breakage_dict, intensity=d_int,
                               intensity_cutoff=intensity_cutoff, mass_cutoff=mass_cutoff)
        fx = fixpoint_device(dp_table, rows, ml)
        bins = bins_device(dp_table, rows, fx.alpha, max_len=ml)
        sk = skeleton_device(dp_table, rows, fx.alpha, ml, bins=bins, caps=tuple(limits.walk_caps),
                             big_caps=tuple(limits.walk_big_caps), max_rounds=limits.walk_max_rounds,
                             name_hash=name_hash)
        side = np.isin(sk.status, (_native.WALK_LIMIT, _native.WALK_SUSPENDED, _native.WALK_ROUNDS,
                                   _native.WALK_MISSING)).reshape(-1, 2)
        r_dev = np.where(side.any(axis=1), REASON_WALK, 0).astype(np.uint8)
        reason[d_idx] |= r_dev
        refuse()
    if len(d_idx) and (r_dev == 0).any():  # (else: every spectrum goes to the mirror)
        ln = length_device(dp_table, sk, bins.alpha_dev, su_seq[d_idx], seq_mass[d_idx],
                           spectra=np.flatnonzero(r_dev == 0) if r_dev.any() else None,
                           frontier_workspace=int(limits.frontier_workspace), trim=trim)
        r_dev[(ln.lb_status == _native.SST_ABORTED) & (r_dev == 0)] |= REASON_FRONTIER
        reason[d_idx] |= r_dev
        refuse()
        post = post_skeleton_device(dp_table, rows, sk, ln)
        if length_program:
            l_cases = length_mod.length_cases(dp_table, rows, sk, ln, su_seq[d_idx])
            dev_lo = length_mod.length_program_device(
                dp_table, l_cases,
                max_combos=length_mod.FINAL_DEFAULT_COMBOS if length_max_combos is None else length_max_combos)
            dev_lo.undecided[r_dev != 0] = 1  # (the mirror's result takes their place below)
            if record is not None:
                record.update(length_cases=l_cases)
        act = (np.asarray(post.active[:len(d_idx)]) != 0) & (r_dev == 0)
        h = handoff_device(dp_table, rows, ln, post, active=act)
        if record is not None:
            record.update(device_index=d_idx, walk_status=sk.status.copy(), lb_status=ln.lb_status.copy(),
                          replay_nodes=None if ln.replay_nodes is None else np.asarray(ln.replay_nodes).copy(),
                          jaccard_status=ln.status.copy(), handoff_bytes=h["bytes"])
        dev_out = BatchOutcome(default=~act, route=np.zeros(len(d_idx), np.uint8), reason=np.zeros(len(d_idx), np.uint8),
                               alpha=np.where(act[:, None], post.alpha[:len(d_idx)], np.uint64(0)),
                               seq_len=np.where(act, ln.seq_len[:len(d_idx)], 0), pos_off=h["pos_off"],
                               skeleton=h["skeleton"], frag_off=h["frag_off"], frag_index=h["index"],
                               frag_code=h["code"], frag_su=h["su"], frag_obs=h["obs"], frag_min_end=h["min_end"],
                               frag_max_end=h["max_end"], breakage_names=names, row_names=dev_out.row_names,
                               row_mass=dev_out.row_mass)
    m_idx = np.flatnonzero(reason)
    align_robust = align_robust or align_search
    align_final = align_final or align_robust
    align_keep = align_keep or align_final
    align_split = align_split or align_final
    align_caps = align_caps or align_keep
    align = align or align_split or align_caps
    if align:
        from . import alignment

        dev_al = alignment.align_device(dp_table, dev_out, split=align_split, caps=bool(align_caps),
                                        keep=bool(align_keep))
    if align_final:
        from . import final_program

        combos = final_program.FINAL_DEFAULT_COMBOS if final_max_combos is None else final_max_combos
        use, undecided = final_program.final_use(dev_al, optional=align_robust)
        search = dict(horizon=final_program.SEARCH_DEFAULT_HORIZON if search_horizon is None else search_horizon,
                      max_width=final_program.SEARCH_DEFAULT_WIDTH if search_width is None else search_width)
        if align_search:
            dev_fo, dev_ro, dev_so = final_program.final_search_device(dp_table, dev_out, use=use, max_combos=combos,
                                                                       **search)
        elif align_robust:
            dev_fo, dev_ro = final_program.final_robust_device(dp_table, dev_out, use=use, max_combos=combos)
        else:
            dev_fo = final_program.final_device(dp_table, dev_out, use=use, max_combos=combos, undecided=undecided)
    if not len(m_idx):
        if align_search:
            return with_length((dev_out, dev_al, dev_fo, dev_ro, dev_so))
        if align_robust:
            return with_length((dev_out, dev_al, dev_fo, dev_ro))
        return with_length((dev_out, dev_al, dev_fo) if align_final else (dev_out, dev_al) if align else dev_out)
    mirrored = [mirror_outcome(dp_table, obs[offsets[g]:offsets[g + 1]], su_seq[g], seq_mass[g], max_len[g],
                               breakage_dict, None if inten is None else inten[offsets[g]:offsets[g + 1]],
                               intensity_cutoff, mass_cutoff, em, int(reason[g])) for g in m_idx.tolist()]
    both = BatchOutcome.concat([dev_out] + mirrored)
    where = np.empty(S, np.int64)  # spectrum g's place in `both`: its device slot, or its mirror run
    where[d_idx] = np.arange(len(d_idx))
    where[m_idx] = len(d_idx) + np.arange(len(m_idx))
    if align:
        cap = int(dp_table.device_table.engine._lib.sst_align_capacity())
        m_al = [alignment.align_host(o, dp_table.tolerance, dp_table.precision, cap, split=align_split,
                                     caps=alignment.lp_caps(dp_table, o) if align_caps else None,
                                     keep=alignment.lp_row_caps(dp_table, o) if align_keep else None)
                for o in mirrored]
        al = alignment.AlignOutcome.concat([dev_al] + m_al)
        if align_final:
            m_fo, m_ro, m_so = [], [], []
            for o, a in zip(mirrored, m_al):
                use, undecided = final_program.final_use(a, optional=align_robust)
                host_args = (o, dp_table.precision, alignment.lp_caps(dp_table, o), alignment.lp_row_caps(dp_table, o))
                if align_search:
                    f, r, so = final_program.final_search_host(*host_args, use=use, max_combos=combos, **search)
                    m_ro.append(r)
                    m_so.append(so)
                elif align_robust:
                    f, r = final_program.final_robust_host(*host_args, use=use, max_combos=combos)
                    m_ro.append(r)
                else:
                    f = final_program.final_host(*host_args, use=use, max_combos=combos, undecided=undecided)
                m_fo.append(f)
            fo = final_program.FinalOutcome.concat([dev_fo] + m_fo).take(where)
            if align_search:
                return with_length((both.take(where), al.take(where), fo,
                                    final_program.RobustOutcome.concat([dev_ro] + m_ro).take(where),
                                    final_program.SearchOutcome.concat([dev_so] + m_so).take(where)), len(m_idx), where)
            if align_robust:
                return with_length((both.take(where), al.take(where), fo,
                                    final_program.RobustOutcome.concat([dev_ro] + m_ro).take(where)), len(m_idx), where)
            return with_length((both.take(where), al.take(where), fo), len(m_idx), where)
        return with_length((both.take(where), al.take(where)), len(m_idx), where)
    return with_length(both.take(where), len(m_idx), where)
