#!/usr/bin/env python3
"""Config-5 harness: the prediction pipeline's explanation
stages over many synthetic spectra, batched on the GPU engine
(spectrseqtools_amd/pipeline.py):

  stage 1  classify_fragments      is_valid (peaks x 4 breakages) + is_singleton
  stage 2  filter_by_explanation, every round of every spectrum batched
           (pipeline.filter_fixpoint): sliding-window SU differences of both
           sides + singleton masses explained against each spectrum's own
           reduced alphabet (k_pairs_alpha), the dict's observed rows
           (sst_dict_union), alphabet reduction as row masks, is_valid of the
           remaining fragments on the reduced tables (k_valid_alpha); until
           every spectrum's alphabet is stable
  stage 3  skeleton bins on the surviving fragments and reduced alphabets:
           each side's bins, first bin's whole masses and every later bin
           against its predecessor -> explain (pair-class windows:
           k_bins_emit's masked pair list; the rest -- whole masses, wide
           differences -- through the masked explain's DFS roles on each
           spectrum's alphabet, one pass per max_len group; the host-driven
           path counts them)
  stage 4  SkeletonBuilder._predict_skeleton per side (device-resident path):
           filter_by_explanation's final dict (k_dict), the walk (k_skel_walk:
           bins, re-queries against older bins through the masked explain,
           update_skeleton_for_given_explanations in CPython's set order,
           min_end / max_end, rejected rows)
  stage 5  select_sequence_length_with_jaccard: the skeleton alphabet, both
           compute_sequence_length_bound directions on it (k_reach_rows + one
           k_length_exact replay per spectrum), the Jaccard length and the
           combined skeleton (k_jaccard)
  gather   (N > 1) every rank's per-spectrum outcomes to rank 0
           (pipeline_device.pack_outcomes, one agreed-size gather)

One process per GPU (torch.distributed.run for N > 1, spectra sharded by
rank, no collective in the data path); every stage is timed over all of this
rank's spectra with barriers around it, max over ranks.  The full alphabet's
table serves every spectrum; the per-spectrum reduced alphabets are row
masks over it (no table is rebuilt; a reference-style rebuild is timed
separately: `reduction_rebuild_ms`).  Results
come back to the host (status, counts, payload: PCIe included).  The
reference Python cannot run on the GPU box; `reference_estimate_s` prices the
same query counts at its measured single-core rates (is_valid
70 k/s, sliding-window explain 3.6-4.5 k/s).

All three stages run device-resident by default (pipeline_device: classify,
every fixpoint round and the bin queries in HBM; the host reads one counter
per round and the bins' total); with --host-driven through the host-driven
batched path (pipeline.classify / filter_fixpoint / bin_queries +
k_pairs_alpha).  Every stage reports its event-timed kernel time and the
GPU-busy share of its wall time.

Usage: python tools/pipeline_bench.py [--spectra 100000] [--seed 7] [--host-driven]
       [--backend nccl|gloo] [--dump-outcomes DIR] [--as-rank R] [--handoff [--handoff-repeats 3]]
       [--align | --align-split] [--align-caps | --align-keep] [--align-final] [--align-robust | --align-search] [--length-program] [--modification-rate 0.5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def length_cpu_baseline(dp, ln, su_seq, obs_seq, max_len, n_len, budget_s):
    """Stage 5 on the host: for spectra of the stage (in order, until about
    budget_s seconds of wall time), what the reference does per spectrum
    after the skeleton -- rebuild the table on the skeleton alphabet
    (skeleton_building.py:324, mass_table.py:94-121) and run
    compute_sequence_length_bound both ways (:335-336) -- by the CPU oracle
    (oracle/sst_oracle.c, the literal restatement; TEST INFRASTRUCTURE, used
    here as the baseline only, after the GPU timing), one spectrum per host
    thread.  Every sampled spectrum's bounds are also compared with the GPU's."""
    import concurrent.futures as cf

    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _oracle as oracle
    from spectrseqtools_amd.pipeline import mask_rows

    threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    threads = max(1, min(threads, 16))  # the box's CPU share for one GPU
    masses = dp.masses
    kept = mask_rows(ln.alpha[:n_len], len(masses))
    tol, prec = dp.tolerance, dp.precision

    def one(g):
        full = [0] + [r for r in range(1, len(masses)) if kept[g, r]]
        ms = [masses[r].mass for r in full]
        L = int(max_len[g])
        t0 = time.perf_counter()
        tab = oracle.build_table(ms, max(ms) * 35, 32)
        t1 = time.perf_counter()
        alph = oracle.Alphabet(ms, [masses[r].is_modification for r in full],
                               [round(L * masses[r].modification_rate) for r in full])
        a0 = round(dp.seq.modification_rate * L)
        b = [oracle.length_bound(tab, 32, alph, float(su_seq[g]), float(obs_seq[g]), tol, L, a0, d, precision=prec)
             for d in ("lower", "upper")]
        return g, t1 - t0, time.perf_counter() - t1, b

    done, build_s, dfs_s, mism = [], 0.0, 0.0, 0
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(threads) as ex:  # ctypes releases the GIL
        it = iter(range(n_len))
        futs = set()
        for _ in range(2 * threads):
            g = next(it, None)
            if g is not None:
                futs.add(ex.submit(one, g))
        while futs:
            fin, futs = cf.wait(futs, return_when=cf.FIRST_COMPLETED)
            for f in fin:
                g, tb, td, b = f.result()
                done.append(g)
                build_s += tb
                dfs_s += td
                if b[0] is None:
                    mism += int(ln.lb_status[g]) == 0
                else:
                    mism += (int(ln.lb_status[g]), int(ln.lower[g]), int(ln.upper[g])) != (0, b[0], b[1])
            if time.perf_counter() - t0 < budget_s:
                for _ in range(len(fin)):
                    g = next(it, None)
                    if g is not None:
                        futs.add(ex.submit(one, g))
    wall = time.perf_counter() - t0
    n = len(done)
    return {"kind": "port", "what": "oracle table rebuild + length_bound lower and upper per spectrum",
            "threads": threads, "spectra": n, "sample": f"the first {n} of the stage's {n_len} spectra (in order)",
            "wall_s": wall, "spectra_per_s": n / wall if wall > 0 else 0.0,
            "thread_s_table_rebuild": build_s, "thread_s_length_bounds": dfs_s,
            "est_s_all_spectra": n_len * wall / n if n else None,
            "mismatches_vs_gpu": int(mism)}


CHASE_LINES_PER_S = 50e9  # tools/chase_probe.hip: random 64-B line fetches per second chip-wide (r3_chase_probe.txt)


def frontier_roofline(fr, kernels):
    """Stage 5's dominant kernels (the first-visit frontier: k_lbf_groups,
    k_lbf_nodes, k_lbf_values, all under the k_length_bound profile id) against
    the per-unit model of DESIGN.md §4: algorithmic bytes at their natural
    sizes per node N, group G and edge E (a left move onto a mass > 0: one
    candidate insert and find, the child's value pushed to the parent), and
    the random lines they touch -- the kernels' real bound, priced against the
    chip's random-line rate."""
    N, G, E, kw = fr["nodes"], fr.get("groups", 0), fr.get("edges", 0), max(1, fr.get("key_words", 1))
    cand = {1: 24, 2: 32, 4: 48}[kw]
    per_node, per_group, per_edge = 17, 97, 36 + 2 * cand
    algo = per_node * N + per_group * G + per_edge * E
    lines = N + G + 4 * E  # lowest-rank byte per node; group entry per group; per edge the child's group entry,
    # its candidate slot (insert, then find) and the value pushed into the parent's slot
    ms = kernels.get("k_length_bound", [0.0])[0]
    s = ms / 1e3
    achieved = algo / s / 1e9 if s > 0 else 0.0
    # HBM bytes per node from the matched counter record (tools/gpu_frontier_record.sh, 16 k spectra)
    rec_path = os.path.join(REPO, "profiles", "r6_frontier_16k_record.json")
    traffic = None
    if os.path.exists(rec_path):
        rec = json.load(open(rec_path))["frontier_band_kernels"]
        traffic = {"bytes_per_node": rec["hbm_bytes_per_node"], "bytes": rec["hbm_bytes_per_node"] * N,
                   "GBps": rec["hbm_bytes_per_node"] * N / s / 1e9 if s > 0 else 0.0,
                   "frac_hbm": rec["hbm_bytes_per_node"] * N / s / 8e12 if s > 0 else 0.0,
                   "source": "profiles/r6_frontier_16k_record.json (2 FETCH_SIZE + WRITE_SIZE per node, gfx950)"}
    return {"bound": "random lines (HBM / fabric)", "kernels": "k_lbf_* (profile id k_length_bound)",
            "nodes": N, "groups": G, "edges": E, "key_words": kw,
            "model_bytes_per": {"node": per_node, "group": per_group, "edge": per_edge},
            "algorithmic_bytes": algo, "algorithmic_bytes_per_node": algo / N if N else 0.0,
            "kernel_s": s, "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
            "random_lines": lines, "random_lines_per_node": lines / N if N else 0.0,
            "random_lines_per_s": lines / s if s > 0 else 0.0,
            "frac_random_line_rate": lines / s / CHASE_LINES_PER_S if s > 0 else 0.0,
            "line_rate_peak": CHASE_LINES_PER_S, "nodes_per_s": N / s if s > 0 else 0.0, "traffic": traffic}


def stages_cpu_baseline(dp, rows, fx, sk, args, data_rank, budget_s):
    """Stages 1-4 on the host (tools/cpu_stages_leg.py, a child process that
    never touches the GPU): A7 on every peak x 4 breakages by the oracle
    (OpenMP), then the host mirrors of classify_fragments /
    filter_by_explanation / _predict_skeleton with the oracle answering every
    query, one spectrum per process, spectra in order for about budget_s.
    Every sampled spectrum's final alphabet and kept rows are compared with
    the device's, and both sides' skeletons too when PYTHONHASHSEED is fixed
    (the walk's set order is this interpreter's, the child's must equal it)."""
    import subprocess

    from spectrseqtools_amd import pipeline_device as pd
    from spectrseqtools_amd.pipeline import mask_rows

    threads = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    threads = max(1, min(threads, 16))  # the box's CPU share for one GPU
    cmd = [sys.executable, os.path.join(REPO, "tools", "cpu_stages_leg.py"), "--spectra", str(args.spectra),
           "--seed", str(args.seed), "--rank", str(data_rank), "--procs", str(threads), "--budget-s", str(budget_s)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=budget_s + 600)
    if p.returncode != 0:
        return {"error": p.stderr[-2000:]}
    res = json.loads(p.stdout.strip().splitlines()[-1])
    outs = res.pop("outcomes")
    seeded = os.environ.get("PYTHONHASHSEED") is not None and args.name_hashes is None
    n_rows = len(dp.masses)
    mism = {"alphabet": 0, "kept": 0, "skeleton": 0}
    alive = rows.alive.cpu().numpy()
    for o in outs:
        g = o["g"]
        kept = mask_rows(fx.alpha[g:g + 1], n_rows)[0]
        mism["alphabet"] += [0] + [dp.masses[r].mass for r in range(1, n_rows) if kept[r]] != o["masses"]
        o4 = int(rows.peak_off[g].item()) * 4
        mism["kept"] += np.flatnonzero(alive[o4:o4 + int(rows.rows[g].item())]).tolist() != o["kept"]
        if seeded:
            got = pd.skeleton_frames(dp, rows, sk, g)
            mism["skeleton"] += any(got[sd] != o[sd] for sd in ("START", "END"))
    st = res["stages1to4"]
    st["mismatches_vs_gpu"] = mism
    st["skeletons_compared"] = seeded
    res["stages1to4"] = st
    return res


def handoff_timings(pd, dp, rows, ln, post, repeats):
    """--handoff: seconds and bytes moved of the dense hand-off
    (pipeline_device.handoff_device: count, emit, one download per output
    array) and of getting the same data the way to_classified does --
    downloading rows.su / obs / meta, post.alive / min_end / max_end and the
    combined skeleton whole and compacting them with numpy.  One untimed run
    of each first; both must deliver the same arrays."""
    import torch

    dev = rows.su.device
    S = len(ln.seq_len)

    def whole_arrays():
        off = rows.peak_off.cpu().numpy()
        cnt = rows.rows.cpu().numpy().astype(np.int64)[:S]
        host = [t.cpu().numpy() for t in (rows.su, rows.obs, rows.meta, post.alive, post.min_end, post.max_end,
                                          ln.comb)]
        su, ob, meta, alive, lo, hi, comb = host
        moved = off.nbytes + rows.rows.numel() * 4 + sum(a.nbytes for a in host)
        act = np.asarray(post.active[:S]) != 0
        cnt = np.where(act, cnt, 0)
        spec = np.repeat(np.arange(S), cnt)
        local = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        slot = 4 * off[:-1][spec] + local
        keep = alive[slot] != 0
        slot, spec, local = slot[keep], spec[keep], local[keep]
        n_pos = np.where(act, ln.seq_len[:S], 0).astype(np.int64)
        pos = np.repeat(np.asarray(ln.comb_off[:S], dtype=np.int64), n_pos) + \
            (np.arange(int(n_pos.sum())) - np.repeat(np.cumsum(n_pos) - n_pos, n_pos))
        return {"frag_off": np.searchsorted(spec, np.arange(S + 1)), "pos_off": np.concatenate([[0], np.cumsum(n_pos)]),
                "index": local.astype(np.int32), "code": (meta[slot] & 0x1f).astype(np.uint8), "su": su[slot],
                "obs": ob[slot], "min_end": lo[slot], "max_end": hi[slot],
                "skeleton": comb[pos].view(np.uint64), "bytes": int(moved)}

    def timed(fn):
        out, ts = fn(), []  # untimed
        for _ in range(repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return out, ts

    a, ta = timed(lambda: pd.handoff_device(dp, rows, ln, post))
    b, tb = timed(whole_arrays)
    same = all(np.array_equal(a[k], b[k]) for k in a if k != "bytes")
    return {"spectra": S, "row_slots": int(rows.su.numel()), "fragments": int(a["frag_off"][-1]),
            "positions": int(a["pos_off"][-1]), "repeats": repeats, "same_arrays": bool(same),
            "kernels": {"s": ta, "s_min": min(ta), "s_median": float(np.median(ta)), "bytes": a["bytes"],
                        "path": "sst_handoff_count_device + sst_handoff_emit_device + one download per output array"},
            "whole_arrays": {"s": tb, "s_min": min(tb), "s_median": float(np.median(tb)), "bytes": b["bytes"],
                             "path": "rows.su/obs/meta, post.alive/min_end/max_end and the combined skeleton "
                                     "downloaded whole, compacted with numpy"}}


def position_rows(out):
    """|A_i| of every position of a BatchOutcome (alignment.position_sets'
    rule: P_i & alpha where P_i != 0, else alpha; row 0 excluded), and which
    positions are unconstrained (an all-zero mask)."""
    spec = np.repeat(np.arange(len(out.seq_len)), np.diff(out.pos_off))
    free = (out.skeleton[:, 0] | out.skeleton[:, 1]) == 0
    n = np.zeros(len(spec), np.int64)
    for w in (0, 1):
        a = out.alpha[spec, w]
        m = np.where(free, a, out.skeleton[:, w] & a) & (~np.uint64(1) if w == 0 else ~np.uint64(0))
        n += np.unpackbits(np.ascontiguousarray(m).view(np.uint8)).reshape(-1, 64).sum(axis=1, dtype=np.int64)
    return n, free


def unconstrained_runs(out, spectra, free=None):
    """Per spectrum of `spectra`: its longest run of unconstrained positions
    (an all-zero position mask: the whole alphabet) and their number."""
    free = (out.skeleton[:, 0] | out.skeleton[:, 1]) == 0 if free is None else free
    longest, count = [], []
    for g in spectra.tolist():
        f = free[int(out.pos_off[g]):int(out.pos_off[g + 1])]
        edge = np.flatnonzero(np.diff(np.concatenate([[0], f.view(np.int8), [0]])))
        longest.append(int((edge[1::2] - edge[::2]).max()) if len(edge) else 0)
        count.append(int(f.sum()))
    return np.array(longest, dtype=np.int64), np.array(count, dtype=np.int64)


def keep_record(dp, out, al, split, kern):
    """--align-keep: the three-way answer of the timed certificate `al` (keep
    mode) -- the shares of DROP, KEEP and SOLVE over all fragments, the share of
    row-free spectra among those with fragments -- and why a FIT fragment is
    left without keep: its spectrum is not row-free; or it is and no sum of any
    decided interval lies in the inner window (the fragment fits only in the
    band between W_in and W); or one does, in a split-closed interval the split
    did not visit (the fragment was FIT at base); or the inner window only
    meets an undecided interval.  The last three come from an untimed caps
    certificate (same split) of the same fragments with observed masses whose
    W is the fragment's W_in."""
    import copy

    from spectrseqtools_amd import _native, alignment

    tol, prec = float(dp.tolerance), float(dp.precision)
    dec = alignment.lp_decisions(al)
    n = max(1, len(dec))
    n_frag = np.diff(out.frag_off)
    spec_of = np.repeat(np.arange(len(n_frag)), n_frag)
    has = n_frag > 0
    q = tol * out.frag_obs / prec
    w_in = np.where(np.isfinite(q) & (q >= 1), np.floor(q) - 1, -1.0)
    inner = copy.copy(out)
    inner.frag_obs = np.where(w_in >= 0, (w_in - 0.5) * prec / tol, -1.5 * prec / tol)  # ceil(q') == W_in (-1: nothing fits)
    reproduced = bool((np.maximum(np.ceil(tol * inner.frag_obs / prec), -1.0) == w_in).all())
    al_in = alignment.align_device(dp, inner, split=split, caps=True)
    left = (al.status == _native.ALIGN_FIT) & (al.keep == 0)
    free = al.spec_free[spec_of] != 0
    n_left = max(1, int(left.sum()))
    cause = {"spectrum_not_row_free": left & ~free,
             "fits_only_between_w_in_and_w": left & free & (al_in.status == _native.ALIGN_NONE),
             "inner_fit_in_an_interval_the_split_did_not_visit": left & free & (al_in.status == _native.ALIGN_FIT),
             "inner_window_meets_an_undecided_interval_only": left & free & (al_in.status == _native.ALIGN_OPEN)}
    return {"decision_shares": {name: float((dec == v).sum()) / n
                                for name, v in (("DROP", alignment.LP_DROP), ("KEEP", alignment.LP_KEEP),
                                                ("SOLVE", alignment.LP_SOLVE))},
            "row_free_spectra_share": float(al.spec_free[has].mean()) if has.any() else 0.0,
            "spectra_with_fragments": int(has.sum()),
            "fit_share": float((al.status == _native.ALIGN_FIT).sum()) / n,
            "fit_kept_share": float(((al.status == _native.ALIGN_FIT) & (al.keep != 0)).sum())
            / max(1, int((al.status == _native.ALIGN_FIT).sum())),
            "fit_without_keep": int(left.sum()),
            "fit_without_keep_share_of_fit": float(left.sum()) / max(1, int((al.status == _native.ALIGN_FIT).sum())),
            "fit_without_keep_by_cause": {k: float(v.sum()) / n_left for k, v in cause.items()},
            "causes_cover_every_such_fragment": bool(sum(int(v.sum()) for v in cause.values()) == int(left.sum())),
            "inner_window_reproduced": reproduced,
            "keep_implies_fit": bool((al.status[al.keep != 0] == _native.ALIGN_FIT).all()),
            "kernel_ms": {str(k): kern.get(_native.KERNEL_NAMES[k], (0.0, 0))[0]
                          for k in (_native.K_ALIGN_KEEP, _native.K_ALIGN_SPLIT_KEEP)}}


def final_stage(dp, out, al, kernels, max_combos):
    """--align-final: the final program by exact enumeration (final_program.
    final_device) over the certificate's KEEP fragments, spectra that hold an
    LP_SOLVE fragment left out (final_program.final_use).  Its seconds run from
    the host arrays in to the host arrays out (uploads, k_final_program,
    downloads); it records the share of each status over all spectra and over
    the spectra that have fragments, the TAKE share (final_decisions), and the
    percentiles of log2(combos) of the SOLVED and of the TOO_LARGE spectra."""
    from spectrseqtools_amd import final_program as fp

    use, undecided = fp.final_use(al)
    kernels()
    t0 = time.perf_counter()
    fo = fp.final_device(dp, out, use=use, max_combos=max_combos, undecided=undecided)
    s = time.perf_counter() - t0
    kern = kernels()
    live = np.diff(out.frag_off) > 0
    dec = fp.final_decisions(fo)
    pct = lambda x: {str(p): float(np.percentile(x, p)) for p in (50, 90, 99, 100)} if len(x) else {}  # noqa: E731
    log2 = lambda st: pct(np.log2(np.maximum(fo.combos[fo.status == st].astype(np.float64), 1.0)))  # noqa: E731
    n_live = max(1, int(live.sum()))
    solved = fo.status == fp.FINAL_SOLVED
    return {"s": s, "spectra": int(len(fo)), "spectra_with_fragments": int(live.sum()), "max_combos": int(max_combos),
            "used_fragments_share": float(use.mean()) if len(use) else 0.0,
            "status_shares": fo.shares(),
            "status_shares_with_fragments": {name: float(np.count_nonzero((fo.status == st) & live)) / n_live
                                             for st, name in fp.STATUS_NAMES.items()},
            "take_share": float(dec.mean()) if len(dec) else 0.0,
            "take_share_with_fragments": float(dec[live].sum()) / n_live,
            "take_share_of_solved": float(dec[solved].mean()) if solved.any() else 0.0,
            "solved_with_several_optima_share": float((fo.n_opt[solved] > 1).mean()) if solved.any() else 0.0,
            "log2_combos_solved": log2(fp.FINAL_SOLVED), "log2_combos_too_large": log2(fp.FINAL_TOO_LARGE),
            "assignments_enumerated": int(fo.combos[solved].sum()),
            "path": "device (sst_final_program_device), host arrays in and out", "kernels": kern,
            "kernel_ms": {"k_final_program": kern.get("k_final_program", (0.0, 0))[0]}}


def length_program_stage(pd, dp, rows, sk, ln, su_seq, kernels, max_combos):
    """--length-program: the length program (length_program.length_cases +
    length_program_device) over every candidate length of every spectrum: the
    optimum of the program select_sequence_length_with_lp builds, by exact
    enumeration.  Its seconds run from the device stages' arrays to the host
    arrays out (downloads and the gather, the validation's f64 sums on the host,
    uploads, k_length_program, downloads), with the gather's and the
    validation's share beside them.  It records per decision (length_decisions)
    the spectra and how many of them have terminal fragments, the share of
    candidates per status, log2(combos) of the SOLVED and TOO_LARGE candidates,
    and among the LENGTH_TAKE spectra how many take a length other than the
    Jaccard seq_len: the number this stage exists for."""
    from spectrseqtools_amd import length_program as lp

    kernels()
    times = {}
    t0 = time.perf_counter()
    cases = lp.length_cases(dp, rows, sk, ln, su_seq)
    t1 = time.perf_counter()
    lo = lp.length_program_device(dp, cases, max_combos=max_combos, times=times)
    s = time.perf_counter() - t0
    kern = kernels()
    decision, length = lp.length_decisions(lo)
    S = max(1, len(lo))
    has = lo.n_frag > 0
    jac = np.asarray(ln.seq_len)[:len(lo)]
    jac_ok = np.asarray(ln.status)[:len(lo)] == 0
    take = decision == lp.LENGTH_TAKE
    n_cand = np.diff(lo.cand_off)
    pct = lambda x: {str(p): float(np.percentile(x, p)) for p in (50, 90, 99, 100)} if len(x) else {}  # noqa: E731
    log2 = lambda st: pct(np.log2(np.maximum(lo.combos[lo.status == st].astype(np.float64), 1.0)))  # noqa: E731
    solved = lo.status == lp.LEN_SOLVED
    return {"s": s, "gather_s": t1 - t0, "valid_s": times.get("valid_s", 0.0), "spectra": int(len(lo)),
            "candidates": int(len(lo.status)), "max_combos": int(max_combos),
            "candidates_per_spectrum": pct(n_cand), "spectra_with_fragments": int(has.sum()),
            "decisions": {name: {"spectra": int((decision == d).sum()), "share": float((decision == d).sum()) / S,
                                 "with_fragments_share": float(has[decision == d].mean()) if (decision == d).any() else 0.0}
                          for d, name in lp.DECISION_NAMES.items()},
            "status_shares": lo.shares(),
            "status_counts": {name: int((lo.status == st).sum()) for st, name in lp.STATUS_NAMES.items()},
            "take_spectra": int(take.sum()),
            "take_differs_from_jaccard": int((take & (length != jac)).sum()),
            "take_where_jaccard_found_no_length": int((take & ~jac_ok).sum()),
            "jaccard_decisions_where_jaccard_found_a_length": int(((decision == lp.LENGTH_JACCARD) & jac_ok).sum()),
            "log2_combos_solved": log2(lp.LEN_SOLVED), "log2_combos_too_large": log2(lp.LEN_TOO_LARGE),
            "assignments_enumerated": int(lo.combos[solved].sum()), "spectra_are": "synthetic (spectrseqtools_amd.synthetic)",
            "path": "device (sst_length_program_device), the stages' device arrays in, host arrays out",
            "kernels": kern, "kernel_ms": {"k_length_program": kern.get("k_length_program", (0.0, 0))[0]}}


def free_positions(out):
    """Free positions (|A_i| > 1) per spectrum of a BatchOutcome (i64)."""
    spec = np.repeat(np.arange(len(out)), np.diff(out.pos_off))
    skel = np.asarray(out.skeleton, dtype=np.uint64).reshape(-1, 2)
    alpha = np.asarray(out.alpha, dtype=np.uint64).reshape(-1, 2)[spec]
    sets = np.where((skel != 0).any(axis=1)[:, None], skel & alpha, alpha)
    n_rows = len(out.row_mass)
    sets[:, 0] &= np.uint64(((1 << min(n_rows, 64)) - 1) & ~1)  # rows below n_rows; row 0 is no row of a set
    sets[:, 1] &= np.uint64((1 << min(max(0, n_rows - 64), 64)) - 1)
    size = np.unpackbits(np.ascontiguousarray(sets).view(np.uint8), axis=1).sum(axis=1)
    return np.bincount(spec, weights=size > 1, minlength=len(out)).astype(np.int64)


def search_record(dp, out, use, fo, ro, so, max_combos, max_width, sample=64):
    """--align-search: what the bounded search did.  The counts of enumerated
    and searched spectra; among the searched SOLVED, TOO_LARGE by cause (more
    than 48 free positions, or a level wider than max_width) and TAKE;
    percentiles of rounds and nodes over the searched SOLVED ones, and of the
    widest level over an evenly spaced sample of at most 64 of them (the host
    model's at the run's max_width: the entry point has no output for it, and
    the model's time grows with the nodes it keeps); whether every spectrum the robust program alone solves has
    identical arrays."""
    from spectrseqtools_amd import alignment
    from spectrseqtools_amd import final_program as fp

    live = ~np.isin(fo.status, (fp.FINAL_NONE, fp.FINAL_SKIPPED, fp.FINAL_NOT_FREE)) & (fo.combos > 0)
    searched = live & (fo.combos > np.uint64(max_combos))
    solved = searched & (fo.status == fp.FINAL_SOLVED)
    too_large = searched & (fo.status == fp.FINAL_TOO_LARGE)
    many_free = too_large & (free_positions(out) > fp.SEARCH_MAX_FREE)
    dec = fp.robust_decisions(fo, ro)
    pct = lambda x: {f"p{q}": float(np.percentile(x, q)) for q in (50, 90, 99, 100)} if len(x) else {}  # noqa: E731
    at = np.flatnonzero(solved)
    at = at[np.unique(np.linspace(0, len(at) - 1, min(sample, len(at))).astype(np.int64))] if len(at) else at
    widest = np.zeros(0)
    if len(at):
        src, _ = pipeline_segments(out.frag_off, at)
        sub = out.take(at)
        host = fp.final_search_host(sub, dp.precision, alignment.lp_caps(dp, sub), alignment.lp_row_caps(dp, sub),
                                    use=use[src], max_combos=max_combos, horizon=so.horizon, max_width=max_width)
        widest = host[2].widest[host[2].mode == fp.SEARCH_SEARCHED]
    r_fo, r_ro = fp.final_robust_device(dp, out, use=use, max_combos=max(1, max_combos))
    was = np.flatnonzero(r_fo.status == fp.FINAL_SOLVED)
    return {"horizon": int(so.horizon), "enumerated": int((so.mode == fp.SEARCH_ENUMERATED).sum()),
            "searched": int(searched.sum()), "searched_solved": int(solved.sum()),
            "searched_infeasible": int((searched & (fo.status == fp.FINAL_INFEASIBLE)).sum()),
            "searched_too_large_free_positions": int(many_free.sum()),
            "searched_too_large_width": int((too_large & ~many_free).sum()),
            "searched_take": int(dec[solved].sum()), "rounds": pct(so.rounds[solved]), "nodes": pct(so.nodes[solved]),
            "widest_level_sample": dict(pct(widest), spectra=int(len(widest))),
            "robust_too_large": int((r_fo.status == fp.FINAL_TOO_LARGE).sum()),
            "robust_solved": int(len(was)),
            "robust_solved_identical": bool(fo.take(was).equals(r_fo.take(was)) and ro.take(was).equals(r_ro.take(was)))}


def pipeline_segments(off, idx):
    from spectrseqtools_amd.pipeline_device import _segments

    return _segments(np.asarray(off, dtype=np.int64), np.asarray(idx, dtype=np.int64))


def robust_stage(dp, out, al, kernels, max_combos, search=None):
    """--align-search (search = (horizon, max_width)): the same stage through
    final_program.final_search_device, with a "search" record (search_record)
    and k_final_search's time.
    --align-robust: the robust final program (final_program.
    final_robust_device) with the certificate's KEEP fragments required and its
    LP_SOLVE fragments optional, so that no spectrum is left out.  Its seconds
    run from the host arrays in to the host arrays out (uploads, k_final_robust,
    downloads); it records the status shares, the TAKE share (robust_decisions)
    over all spectra and over those with fragments, and among the spectra that
    hold an LP_SOLVE fragment (UNDECIDED under --align-final): their TAKE share,
    the share that fails each of the three conditions, and the distribution of
    n_optional."""
    from spectrseqtools_amd import final_program as fp

    use, _ = fp.final_use(al, optional=True)
    _, was_undecided = fp.final_use(al)
    kernels()
    t0 = time.perf_counter()
    if search:
        fo, ro, so = fp.final_search_device(dp, out, use=use, max_combos=max_combos, horizon=search[0], max_width=search[1])
    else:
        fo, ro = fp.final_robust_device(dp, out, use=use, max_combos=max_combos)
    s = time.perf_counter() - t0
    kern = kernels()
    more = {"search": dict(search_record(dp, out, use, fo, ro, so, max_combos, int(search[1])), max_width=int(search[1]))} if search else {}
    live = np.diff(out.frag_off) > 0
    n_live = max(1, int(live.sum()))
    dec = fp.robust_decisions(fo, ro)
    solved = fo.status == fp.FINAL_SOLVED
    need = np.maximum(2 * fo.n_used() + 1, fp.FIX // 2).astype(np.uint64)
    open_solved = was_undecided & solved
    share = lambda m, of: float(np.count_nonzero(m & of)) / max(1, int(of.sum()))  # noqa: E731
    n_opt_of = ro.n_optional[open_solved]
    return {"s": s, "spectra": int(len(fo)), "spectra_with_fragments": int(live.sum()), "max_combos": int(max_combos),
            "required_fragments_share": float((use == 1).mean()) if len(use) else 0.0,
            "optional_fragments_share": float((use == 2).mean()) if len(use) else 0.0,
            "status_shares": fo.shares(),
            "status_shares_with_fragments": {name: float(np.count_nonzero((fo.status == st) & live)) / n_live
                                             for st, name in fp.STATUS_NAMES.items()},
            "take_share": float(dec.mean()) if len(dec) else 0.0,
            "take_share_with_fragments": float(dec[live].sum()) / n_live,
            "take_share_of_solved": float(dec[solved].mean()) if solved.any() else 0.0,
            "formerly_undecided": {
                "spectra": int(was_undecided.sum()), "share_with_fragments": float((was_undecided & live).sum()) / n_live,
                "status_shares": {name: share(fo.status == st, was_undecided) for st, name in fp.STATUS_NAMES.items()},
                "take_share": share(dec == fp.FINAL_TAKE, was_undecided),
                "take_share_of_solved": share(dec == fp.FINAL_TAKE, open_solved),
                "of_solved_fails_rbest": share(ro.rbest != fo.best + ro.cstar, open_solved),
                "of_solved_fails_rn_opt": share(ro.rn_opt != 1, open_solved),
                "of_solved_fails_rgap": share(ro.rgap < need, open_solved),
                "n_optional_counts": {str(int(k)): int(v) for k, v in zip(*np.unique(np.minimum(n_opt_of, 8),
                                                                                   return_counts=True))},
                "n_optional_max": int(n_opt_of.max(initial=0))},
            "assignments_enumerated": int(fo.combos[solved].sum() + fo.combos[solved & (ro.n_optional > 0)].sum()),
            "path": f"device ({'sst_final_search_device' if search else 'sst_final_robust_device'}), host arrays in and out",
            "kernels": kern,
            "kernel_ms": {k: kern.get(k, (0.0, 0))[0] for k in ("k_final_robust",) + (("k_final_search",) if search else ())},
            **more}


def align_stage(pd, dp, rows, ln, post, kernels, split=False, caps=False, keep=False, hold=None):
    """--align: the alignment certificate (alignment.align_device) over the
    hand-off of the spectra the stages ran -- wall seconds from the host
    arrays in to the host arrays out (uploads, k_align_windows, downloads), the
    kernel's event time, and the share of each status over all fragments.
    The hand-off itself is not part of the time.
    --align-split (split=True): the timed call is align_device(split=True)
    (k_align_split follows k_align_windows on the stream, one download); the
    base certificate is then taken again, untimed, for the shares before the
    split, what became of the base-OPEN fragments, and what the spectra that
    are still OPEN look like.
    --align-caps (caps=True): the timed call runs under the universal
    modification cap (align_device(caps=True): k_align_windows_caps and, with
    --align-split, k_align_split_caps); the split's base is then the caps base.
    The uncapped certificate of the same run (same split) is taken again,
    untimed, for its shares, the fragments the cap moved, the spectra it makes
    INFEASIBLE and the mod_cap distribution ("caps").
    --align-keep (keep=True, implies caps): the timed call runs in keep mode
    (align_device(caps=True, keep=True): k_align_windows_keep and, with
    --align-split, k_align_split_keep); "keep" holds keep_record's shares.
    hold: a dict that receives the outcome and its certificate (--align-final)."""
    from spectrseqtools_amd import _native, alignment

    S = len(ln.seq_len)
    act = np.asarray(post.active[:S]) != 0
    h = pd.handoff_device(dp, rows, ln, post, active=act)
    empty = pd._empty_outcome(dp, rows.names, 0)
    out = pd.BatchOutcome(default=~act, route=np.zeros(S, np.uint8), reason=np.zeros(S, np.uint8),
                          alpha=np.where(act[:, None], post.alpha[:S], np.uint64(0)),
                          seq_len=np.where(act, ln.seq_len[:S], 0), pos_off=h["pos_off"], skeleton=h["skeleton"],
                          frag_off=h["frag_off"], frag_index=h["index"], frag_code=h["code"], frag_su=h["su"],
                          frag_obs=h["obs"], frag_min_end=h["min_end"], frag_max_end=h["max_end"],
                          breakage_names=rows.names, row_names=empty.row_names, row_mass=empty.row_mass)
    kernels()  # (the hand-off's launches are not this stage's)
    t0 = time.perf_counter()
    al = alignment.align_device(dp, out, split=split, caps=caps, keep=keep)
    s = time.perf_counter() - t0
    kern = kernels()
    if hold is not None:
        hold.update(outcome=out, certificate=al)
    n = np.diff(out.frag_off)
    internal = (out.frag_code >> 2) & 3 == 0
    rec = {"s": s, "spectra": int(act.sum()), "fragments": int(out.frag_off[-1]), "positions": int(out.pos_off[-1]),
           "fragments_per_spectrum_max": int(n.max()) if S else 0, "seq_len_max": int(out.seq_len.max()) if S else 0,
           "internal_fragments": int(internal.sum()), "capacity": alignment.ALIGN_CAPACITY,
           "status_shares": al.shares(), "not_alignable_share": float(1.0 - al.alignable.mean()) if len(al.status) else 0.0,
           "not_alignable_share_internal": float(1.0 - al.alignable[internal].mean()) if internal.any() else 0.0,
           "path": "device (sst_align_windows_device), host arrays in and out", "kernels": kern}
    if caps:
        rec["path"] = "device (sst_align_windows_caps_device), host arrays in and out"
        plain = alignment.align_device(dp, out, split=split)  # untimed: the same run without the cap
        kernels()
        st = _native
        was = lambda a, b: int(((plain.status == a) & (al.status == b)).sum())  # noqa: E731
        by_cap = (plain.status != st.ALIGN_INFEASIBLE) & (al.status == st.ALIGN_INFEASIBLE)
        mod_cap = alignment.lp_caps(dp, out)[1][act]
        rec["caps"] = {"modification_rate": float(dp.seq.modification_rate),
                       "status_shares_uncapped": plain.shares(),
                       "not_alignable_share_uncapped": float(1.0 - plain.alignable.mean()) if len(plain.status) else 0.0,
                       "solver_calls_saved_by_the_cap": int((plain.alignable != 0).sum() - (al.alignable != 0).sum()),
                       "alignable_never_raised": bool((al.alignable <= plain.alignable).all()),
                       "fit_to_none": was(st.ALIGN_FIT, st.ALIGN_NONE), "fit_to_open": was(st.ALIGN_FIT, st.ALIGN_OPEN),
                       "open_to_fit": was(st.ALIGN_OPEN, st.ALIGN_FIT), "open_to_none": was(st.ALIGN_OPEN, st.ALIGN_NONE),
                       "open_uncapped": int((plain.status == st.ALIGN_OPEN).sum()),
                       "open_capped": int((al.status == st.ALIGN_OPEN).sum()),
                       "fragments_infeasible_by_cap": int(by_cap.sum()),
                       "spectra_infeasible_by_cap": int(len(np.unique(np.repeat(np.arange(S), np.diff(out.frag_off))[by_cap]))),
                       "mod_cap_counts": {str(int(v)): int(c) for v, c in zip(*np.unique(mod_cap, return_counts=True))},
                       "kernel_ms": {str(k): kern.get(_native.KERNEL_NAMES[k], (0.0, 0))[0]
                                     for k in (_native.K_ALIGN_CAPS, _native.K_ALIGN_SPLIT_CAPS)}}
    if keep:
        rec["keep"] = keep_record(dp, out, al, split, kern)
        kernels()
    if not split:
        return rec
    base = alignment.align_device(dp, out, caps=caps)  # untimed: what the split started from
    kernels()
    was_open = base.status == _native.ALIGN_OPEN
    still = al.status == _native.ALIGN_OPEN
    n_open = max(1, int(was_open.sum()))
    spec_of = np.repeat(np.arange(S), n)
    pct = lambda x: {str(p): float(np.percentile(x, p)) for p in (50, 90, 99, 100)} if len(x) else {}  # noqa: E731
    rows_of = lambda g: np.array([bin(int(a0)).count("1") + bin(int(a1)).count("1") for a0, a1 in out.alpha[g]])  # noqa: E731

    n_rows, free = position_rows(out)

    def describe(mask):  # the spectra that hold a fragment of `mask`
        g = np.unique(spec_of[mask])
        longest, count = unconstrained_runs(out, g, free)
        per = [n_rows[int(out.pos_off[x]):int(out.pos_off[x + 1])] for x in g.tolist()]
        return {"spectra": int(len(g)), "fragments": int(mask.sum()), "seq_len": pct(out.seq_len[g]),
                "alphabet_rows": pct(rows_of(g)), "unconstrained_positions": pct(count),
                "longest_unconstrained_run": pct(longest),
                "rows_per_position_mean": pct([float(x.mean()) for x in per if len(x)]),
                "rows_per_position_max": pct([int(x.max()) for x in per if len(x)]),
                "positions_of_several_rows": pct([int((x > 1).sum()) for x in per]),
                # log2 of the product of |A_i| over the whole skeleton: the sums [0, L - 1] could have at most
                "log2_combinations": pct([float(np.log2(np.maximum(x, 1)).sum()) for x in per])}

    unchanged = all(np.array_equal(getattr(al, k)[~was_open], getattr(base, k)[~was_open]) for k in al.FRAGMENT_FIELDS)
    rec.update({"path": "device (sst_align_windows_keep_device + sst_align_split_keep_device), host arrays in and out"
                if keep else
                "device (sst_align_windows_caps_device + sst_align_split_caps_device), host arrays in and out"
                if caps else "device (sst_align_windows_device + sst_align_split_device), host arrays in and out",
                "status_shares_base": base.shares(),
                "open_decided_share": float((was_open & ~still).sum()) / n_open,
                "open_to_fit_share": float((was_open & (al.status == _native.ALIGN_FIT)).sum()) / n_open,
                "open_to_none_share": float((was_open & (al.status == _native.ALIGN_NONE)).sum()) / n_open,
                "none_share_added": float((was_open & (al.status == _native.ALIGN_NONE)).sum()) / max(1, len(al.status)),
                "not_alignable_share_base": float(1.0 - base.alignable.mean()) if len(base.status) else 0.0,
                "other_fragments_unchanged": bool(unchanged),
                "kernel_ms": {str(k): kern.get(_native.KERNEL_NAMES[k], (0.0, 0))[0]
                              for k in ((_native.K_ALIGN_KEEP, _native.K_ALIGN_SPLIT_KEEP) if keep else
                                        (_native.K_ALIGN_CAPS, _native.K_ALIGN_SPLIT_CAPS) if caps else
                                        (_native.K_ALIGN, _native.K_ALIGN_SPLIT))},
                "split_spectra": describe(was_open),  # the spectra k_align_split swept (a base-OPEN fragment)
                "open_after_split": describe(still)})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=100000, help="spectra per GPU")
    ap.add_argument("--warmup-spectra", type=int, default=256, help="untimed warm-up spectra (all stages)")
    ap.add_argument("--length-soft-nodes", type=int, default=1 << 20,
                    help="stage 5's light pass: replays over this many nodes are deferred to the heavy pass")
    ap.add_argument("--length-spectra", type=int, default=0,
                    help="stage 5's length bounds on this many spectra of the rank (0: all); the reference's "
                         "memoised DFS visits up to ~10^7 nodes per spectrum on rich skeleton alphabets")
    ap.add_argument("--length-engine", default="frontier", choices=("frontier", "replay"),
                    help="stage 5: the first-visit frontier (default) or the round-4 per-spectrum DFS replay")
    ap.add_argument("--frontier-workspace-gb", type=float, default=0.0,
                    help="stage 5: the frontier's device workspace per call in GiB (0: its default, min(96, free/2))")
    ap.add_argument("--cpu-baseline-s", type=float, default=20.0,
                    help="stage 5's CPU baseline: the oracle's table rebuild + both length bounds per spectrum on "
                         "the host's cores, for about this many seconds (0: skip)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--host-driven", action="store_true",
                    help="stages 1-2 through the host-driven batched path (pipeline.classify / filter_fixpoint) "
                         "instead of the device-resident one (pipeline_device)")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"))
    ap.add_argument("--dump-outcomes", default=None,
                    help="rank 0 saves the gathered per-spectrum outcomes (one .npy per rank) here")
    ap.add_argument("--name-hashes", default=None,
                    help="a .npy of the rows' name hashes (the skeleton walk's set order) to use instead of this "
                         "interpreter's; a multi-rank run always uses rank 0's (saved with --dump-outcomes)")
    ap.add_argument("--handoff", action="store_true",
                    help="after the timed stages, also time the dense hand-off (the two sst_handoff_*_device calls "
                         "plus one download per output array) and, for the same data, downloading the row-slot "
                         "arrays whole and compacting them with numpy (to_classified's way); reported under "
                         "\"handoff\", outside the stages' total")
    ap.add_argument("--handoff-repeats", type=int, default=3, help="--handoff: timed repeats of each way (after one "
                                                                   "untimed run)")
    ap.add_argument("--align", action="store_true",
                    help="after the stages, also run the alignment certificate (alignment.align_device) over the "
                         "hand-off: a stage \"align\" with its seconds and the share of each status over all fragments")
    ap.add_argument("--align-split", action="store_true",
                    help="--align with the two-list split of the open intervals (align_device(split=True)): the "
                         "stage also reports the shares before the split, the share of the base-OPEN fragments it "
                         "decides (open_decided_share) and turns into NONE (open_to_none_share), each kernel's "
                         "milliseconds, and what the spectra that stay OPEN look like")
    ap.add_argument("--align-caps", action="store_true",
                    help="--align under the program's universal modification cap (align_device(caps=True)); alone or "
                         "with --align-split.  The stage also reports the uncapped shares of the same run (untimed), "
                         "the fragments the cap moved (FIT -> NONE, OPEN -> FIT, OPEN -> NONE), the spectra it makes "
                         "INFEASIBLE and the mod_cap distribution")
    ap.add_argument("--align-keep", action="store_true",
                    help="--align-caps in keep mode (align_device(caps=True, keep=True)); alone or with --align-split.  "
                         "The stage also reports the shares of DROP, KEEP and SOLVE, the share of row-free spectra, "
                         "and the FIT fragments left without keep by cause (\"keep\")")
    ap.add_argument("--align-final", action="store_true",
                    help="--align-keep --align-split, then the final program by exact enumeration (final_program."
                         "final_device) over the KEEP fragments: a stage \"final\" with its seconds, k_final_program's "
                         "time, the status and TAKE shares and the percentiles of log2(combos)")
    ap.add_argument("--align-robust", action="store_true",
                    help="--align-keep --align-split, then the robust final program (final_program.final_robust_device): "
                         "the LP_SOLVE fragments are optional and no spectrum is UNDECIDED.  A stage \"final_robust\" "
                         "with its seconds, k_final_robust's time, the status and TAKE shares, and the formerly "
                         "undecided spectra's TAKE share, failed conditions and n_optional (n_optional_counts: 8 "
                         "stands for 8 and more)")
    ap.add_argument("--align-search", action="store_true",
                    help="--align-robust through the bounded search (final_program.final_search_device): spectra above "
                         "--final-max-combos are searched, not given up.  The stage \"final_robust\" also carries "
                         "\"search\": enumerated and searched spectra, the searched ones SOLVED, TOO_LARGE by cause and "
                         "TAKE, percentiles of rounds, nodes and the widest level")
    ap.add_argument("--search-horizon", type=int, default=1 << 17, help="--align-search: the horizon H")
    ap.add_argument("--search-width", type=int, default=1 << 12, help="--align-search: max_width (up to 2^16)")
    ap.add_argument("--final-max-combos", type=int, default=1 << 20,
                    help="--align-final, --align-robust: assignments enumerated per spectrum at most (up to 2^22; "
                         "--align-search: 0 searches every spectrum)")
    ap.add_argument("--length-program", action="store_true",
                    help="after post_skeleton: the length program (select_sequence_length_with_lp by exact enumeration) "
                         "over every candidate length of every spectrum, its decisions and how many TAKE lengths "
                         "differ from the Jaccard length")
    ap.add_argument("--length-max-combos", type=int, default=1 << 20,
                    help="--length-program: assignments enumerated per candidate at most (up to 2^22)")
    ap.add_argument("--modification-rate", type=float, default=0.5,
                    help="the sequences' universal modification rate: the synthetic spectra's and the table's "
                         "SequenceInformation's (0.05: the low-modification-rate variant)")
    ap.add_argument("--as-rank", type=int, default=None,
                    help="single process: generate the spectra rank R of a multi-rank run would get")
    args = ap.parse_args()
    args.align_robust = args.align_robust or args.align_search
    args.align_keep = args.align_keep or args.align_final or args.align_robust
    args.align_split = args.align_split or args.align_final or args.align_robust
    args.align_caps = args.align_caps or args.align_keep
    args.align = args.align or args.align_split or args.align_caps

    import torch

    from spectrseqtools_amd import _native, pipeline
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE, build_breakage_dict
    from spectrseqtools_amd.parallel import dist_env
    from spectrseqtools_amd.synthetic import make_spectra

    rank, world, local = dist_env()
    gpu = int(os.environ.get("SST_DEVICE", local))
    dist = None
    if world > 1:
        import torch.distributed as dist

        torch.cuda.set_device(gpu)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", gpu))
        else:
            dist.init_process_group("gloo")
    engine = _native.get_engine(gpu)

    def barrier():
        if dist:
            dist.barrier()

    def tmax(x):
        if not dist:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=comm_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    comm_dev = torch.device("cuda", gpu) if args.backend == "nccl" else torch.device("cpu")
    t0 = time.perf_counter()
    data_rank = rank if args.as_rank is None else args.as_rank
    batch = make_spectra(args.spectra, seed=args.seed + 1_000_003 * data_rank, mod_rate=args.modification_rate)
    gen_s = time.perf_counter() - t0
    bd = build_breakage_dict(555.1294, 455.1491)
    w_full = [k for k, v in bd.items() if "START_END" in v][0]
    su_seq = batch.seq_mass - w_full * TOLERANCE  # cli.py:149-156
    seq0 = SequenceInformation(max_len=20, su_mass=float(su_seq[0]), obs_mass=float(batch.seq_mass[0]),
                               modification_rate=args.modification_rate)
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq0, engine=engine)
    min_int = min(m.mass for m in dp.masses[1:])
    # the skeleton walk orders explanations as the reference's CPython sets do,
    # by the names' str hashes: one interpreter's for every rank (rank 0's)
    from spectrseqtools_amd.pipeline_device import name_hashes

    nh = name_hashes(dp) if args.name_hashes is None else np.load(args.name_hashes)
    if dist:
        t = torch.as_tensor(nh, device=comm_dev)
        dist.broadcast(t, src=0)
        nh = t.cpu().numpy()
    if rank == 0 and args.dump_outcomes:
        os.makedirs(args.dump_outcomes, exist_ok=True)
        np.save(os.path.join(args.dump_outcomes, "name_hashes.npy"), nh)
    max_len = pipeline.max_len_of(su_seq, TOLERANCE, min_int)  # cli.py:158-170

    def kernels():
        return {_native.KERNEL_NAMES.get(k, str(k)): v for k, v in engine.profile_read().items()}

    def progress(*names):  # one line per finished stage on stderr (a long run shows it is alive)
        if rank == 0:
            print(" ".join(f"[{n}] {stages[n]['s']:.3f}s" for n in names), file=sys.stderr, flush=True)

    def busy(st):  # GPU-busy share of a stage: event-timed kernel time over its wall time
        st["gpu_busy_frac"] = sum(v[0] for v in st["kernels"].values()) / 1e3 / st["s"]

    # warm-up on the first 256 spectra (untimed): loads every kernel and the
    # torch ops the stages use, as a serving process would have
    S0 = min(args.warmup_spectra, args.spectra)
    o0, s0, m0 = batch.observed[:batch.offsets[S0]], batch.offsets[:S0 + 1], max_len[:S0]
    if args.host_driven:
        cw = pipeline.classify(o0, s0, su_seq[:S0], dp, bd)
        fw = pipeline.filter_fixpoint(cw, dp, m0, EXPLANATION_MASSES)
        qw = pipeline.bin_queries(pipeline.subset(cw, fw.alive))
        dp.device_table.explain_pairs_alpha(qw.diff, qw.thr, qw.spec, fw.alpha, dp.tolerance, dp.precision)
    else:
        from spectrseqtools_amd import pipeline_device as pd

        rw = pd.classify_device(dp, o0, s0, su_seq[:S0], bd)
        fw = pd.fixpoint_device(dp, rw, m0)
        bw = pd.bins_device(dp, rw, fw.alpha, max_len=m0)
        sw = bw.status == 2
        int(sw.sum().item()), int((bw.status == -10).sum().item()), int(bw.count[sw].sum().item())
        kw = pd.skeleton_device(dp, rw, fw.alpha, m0, bins=bw, name_hash=nh)
        # (trim=False: a serving process keeps the frontier's workspace across
        # batches; the timed stage reuses the warm-up's, as round 5 did)
        lw = pd.length_device(dp, kw, bw.alpha_dev, su_seq[:S0], batch.seq_mass[:S0], trim=False)
        pw = pd.post_skeleton_device(dp, rw, kw, lw)
        if args.length_program:
            length_program_stage(pd, dp, rw, kw, lw, su_seq[:S0], lambda: {}, args.length_max_combos)
        if args.align:
            held = {}
            align_stage(pd, dp, rw, lw, pw, lambda: {}, split=args.align_split, caps=args.align_caps, keep=args.align_keep,
                        hold=held)
            if args.align_final:
                final_stage(dp, held["outcome"], held["certificate"], lambda: {}, args.final_max_combos)
            if args.align_robust:
                robust_stage(dp, held["outcome"], held["certificate"], lambda: {}, args.final_max_combos,
                             (args.search_horizon, args.search_width) if args.align_search else None)
        # the reach buffer at length_device's batch budget, as a serving
        # process holds it: the timed stage allocates nothing (its hipMalloc /
        # hipFree of tens of GB took 0.1-3 s from run to run)
        pd.reserve_length_buffer(torch.device("cuda", gpu))
    engine.synchronize()
    if rank == 0:
        print(f"[warm-up] {S0} spectra done", file=sys.stderr, flush=True)

    stages = {}
    engine.profile(True)
    n_valid_q = 0
    if args.host_driven:
        barrier()
        t0 = time.perf_counter()
        c = pipeline.classify(batch.observed, batch.offsets, su_seq, dp, bd)
        barrier()
        stages["classify"] = {"s": tmax(time.perf_counter() - t0), "is_valid_queries": c.n_valid_queries,
                              "is_singleton_queries": c.n_singleton_queries, "rows_kept": int(c.offsets[-1])}
        stages["classify"]["kernels"] = kernels()
        n_valid_q = c.n_valid_queries

        barrier()
        t0 = time.perf_counter()
        fx = pipeline.filter_fixpoint(c, dp, max_len, EXPLANATION_MASSES)
        barrier()
        alpha_u = np.unique(fx.alpha, axis=0)
        stages["fixpoint"] = {"s": tmax(time.perf_counter() - t0), "rounds_max": int(fx.rounds.max()),
                              "rounds_histogram": {int(k): int(v) for k, v in zip(*np.unique(fx.rounds, return_counts=True))},
                              "final_round_queries": int(len(fx.last.get("diff", []))),
                              "explain_queries_per_round": [int(x[0]) for x in fx.queries],
                              "is_valid_queries_per_round": [int(x[1]) for x in fx.queries],
                              "rows_kept": int(fx.alive.sum()), "rows_in": int(len(fx.alive)),
                              "distinct_alphabets": int(len(alpha_u)),
                              "mean_alphabet_rows": float(pipeline.mask_rows(fx.alpha, len(dp.masses)).sum(1).mean() + 1)}
        stages["fixpoint"]["kernels"] = kernels()
        fx_alpha = fx.alpha
        explain_q = sum(x[0] for x in fx.queries)
        valid_q_rounds = sum(x[1] for x in fx.queries)
        rows = None
    else:
        from spectrseqtools_amd import pipeline_device as pd

        barrier()
        t0 = time.perf_counter()  # includes the peaks' upload (PCIe)
        rows = pd.classify_device(dp, batch.observed, batch.offsets, su_seq, bd)
        barrier()
        n_valid_q = 4 * len(batch.observed)
        stages["classify"] = {"s": tmax(time.perf_counter() - t0), "is_valid_queries": n_valid_q,
                              "rows_kept": int(rows.rows.sum().item()), "path": "device (sst_classify_rows_device)"}
        stages["classify"]["kernels"] = kernels()

        barrier()
        t0 = time.perf_counter()
        fx = pd.fixpoint_device(dp, rows, max_len)
        barrier()
        alpha_u = np.unique(fx.alpha, axis=0)
        stages["fixpoint"] = {"s": tmax(time.perf_counter() - t0), "rounds": fx.n_rounds,
                              "rounds_histogram": {int(k): int(v) for k, v in zip(*np.unique(fx.rounds, return_counts=True))},
                              "explain_queries": int(fx.queries.astype(np.int64).sum()),
                              "distinct_alphabets": int(len(alpha_u)),
                              "mean_alphabet_rows": float(pipeline.mask_rows(fx.alpha, len(dp.masses)).sum(1).mean() + 1),
                              "path": "device (sst_fix_round_device + sst_valid_rows_alpha_device per round)"}
        stages["fixpoint"]["kernels"] = kernels()
        fx_alpha = fx.alpha
        explain_q = int(fx.queries.astype(np.int64).sum())
        valid_q_rounds = 0  # counted inside the explain launches' rounds; priced with the explains below

    busy(stages["classify"])
    busy(stages["fixpoint"])
    progress("classify", "fixpoint")

    barrier()
    t0 = time.perf_counter()
    if rows is None:  # host-built bin queries, answered by k_pairs_alpha
        c3 = pipeline.subset(c, fx.alive)
        q3 = pipeline.bin_queries(c3)
        st3, cnt3, _, _ = dp.device_table.explain_pairs_alpha(q3.diff, q3.thr, q3.spec, fx_alpha, dp.tolerance,
                                                              dp.precision)
        n_bins_q = len(q3.diff)
        n_some, n_pend, n_cand = int((st3 == 2).sum()), int((st3 == -10).sum()), int(cnt3[st3 == 2].sum())
    else:  # device-resident: bins formed and answered in HBM, only the tallies read back
        from spectrseqtools_amd import pipeline_device as pd

        db = pd.bins_device(dp, rows, fx_alpha, max_len=max_len)
        some = db.status == 2
        n_bins_q = int(db.q_off[-1])
        n_def = db.deferred["queries"]
        n_some, n_pend = int(some.sum().item()), int((db.status == -10).sum().item())
        n_cand = int(db.count[some].sum().item())
    barrier()
    stages["bins"] = {"s": tmax(time.perf_counter() - t0), "queries": n_bins_q,
                      "pair_class": n_bins_q - (n_pend if rows is None else n_def),
                      "not_pair_class": n_pend if rows is None else n_def,
                      "not_pair_class_unanswered": n_pend,
                      "with_candidates": n_some, "candidates": n_cand}
    if rows is not None:
        stages["bins"]["masked_explain_groups"] = [list(x) for x in db.deferred["groups"]]
    stages["bins"]["kernels"] = kernels()
    busy(stages["bins"])
    progress("bins")
    outcome = None
    if rows is not None:  # stages 4-5 (device-resident path)
        barrier()
        t0 = time.perf_counter()
        sk = pd.skeleton_device(dp, rows, fx_alpha, max_len, bins=db, name_hash=nh)
        barrier()
        wst = {int(k): int(v) for k, v in zip(*np.unique(sk.status, return_counts=True))}
        stages["skeleton"] = {"s": tmax(time.perf_counter() - t0), "sides": 2 * len(max_len),
                              "walk_status": wst, "walk_launches": sk.launches, "requery_windows": sk.requeries,
                              "dict_entries": sk.dict_entries, "kernels": kernels()}
        busy(stages["skeleton"])
        progress("skeleton")
        barrier()
        t0 = time.perf_counter()
        n_len = len(max_len) if args.length_spectra <= 0 else min(args.length_spectra, len(max_len))
        ln = pd.length_device(dp, sk, db.alpha_dev, su_seq, batch.seq_mass,
                              spectra=None if n_len == len(max_len) else np.arange(n_len),
                              soft_nodes=args.length_soft_nodes, engine=args.length_engine,
                              frontier_workspace=int(args.frontier_workspace_gb * (1 << 30)), trim=False)
        barrier()
        stages["length"] = {"s": tmax(time.perf_counter() - t0), "bounds_spectra": n_len,
                            "bounds_sample": n_len < len(max_len), "reach_batches": ln.reach_batches,
                            "distinct_skeleton_alphabets": ln.distinct_alphabets,
                            "replay_nodes": {"total": int(ln.replay_nodes[:n_len].sum()),
                                             "percentiles": {str(p): int(np.percentile(ln.replay_nodes[:n_len], p))
                                                             for p in (50, 90, 99, 100)}},
                            "jaccard_status": {int(k): int(v) for k, v in zip(*np.unique(ln.status,
                                                                                         return_counts=True))},
                            "lb_status": {int(k): int(v) for k, v in zip(*np.unique(ln.lb_status,
                                                                                   return_counts=True))},
                            "mean_seq_len": float(ln.seq_len[ln.status == 0].mean()) if (ln.status == 0).any() else 0,
                            "engine": ln.engine, "frontier": ln.frontier, "kernels": kernels()}
        if ln.engine == "frontier" and ln.frontier.get("nodes"):
            stages["length"]["roofline"] = frontier_roofline(ln.frontier, stages["length"]["kernels"])
        busy(stages["length"])
        progress("length")
        barrier()
        t0 = time.perf_counter()
        post = pd.post_skeleton_device(dp, rows, sk, ln)
        barrier()
        stages["post_skeleton"] = {"s": tmax(time.perf_counter() - t0), "spectra": int(post.active.sum()),
                                   "fragments_after_skeleton": post.rows_before,
                                   "fragments_after_reduction": post.rows_after,
                                   "path": "device (sst_post_skeleton_device + sst_valid_rows_alpha_device)",
                                   "kernels": kernels()}
        busy(stages["post_skeleton"])
        progress("post_skeleton")
        barrier()
        t0 = time.perf_counter()
        buf = pd.pack_outcomes(rows, fx, sk, ln, post)
        if dist:
            from spectrseqtools_amd.parallel import Gatherer

            gth = Gatherer(dist, comm_dev)
            sizes = gth.agree(buf.numel())
            got = gth.gather(buf.to(comm_dev))
            if rank == 0:
                outcome = [x.cpu().numpy() for x in got]
        else:
            sizes = [int(buf.numel())]
            outcome = [buf.cpu().numpy()]
        barrier()
        stages["gather"] = {"s": tmax(time.perf_counter() - t0), "bytes_per_rank": sizes, "kernels": kernels(),
                            "path": "pack_outcomes + one agreed-size gather to rank 0"
                                    + (f" ({'RCCL' if args.backend == 'nccl' else 'gloo'})" if dist else " (local)")}
    if rows is not None and args.length_program:
        barrier()
        stages["length_program"] = length_program_stage(pd, dp, rows, sk, ln, su_seq, kernels, args.length_max_combos)
        stages["length_program"]["s"] = tmax(stages["length_program"]["s"])
        busy(stages["length_program"])
        progress("length_program")
    if rows is not None and args.align:
        barrier()
        held = {}
        stages["align"] = align_stage(pd, dp, rows, ln, post, kernels, split=args.align_split, caps=args.align_caps,
                                      keep=args.align_keep, hold=held)
        stages["align"]["s"] = tmax(stages["align"]["s"])
        busy(stages["align"])
        progress("align")
        if args.align_final:
            barrier()
            stages["final"] = final_stage(dp, held["outcome"], held["certificate"], kernels, args.final_max_combos)
            stages["final"]["s"] = tmax(stages["final"]["s"])
            busy(stages["final"])
            progress("final")
        if args.align_robust:
            barrier()
            stages["final_robust"] = robust_stage(dp, held["outcome"], held["certificate"], kernels, args.final_max_combos,
                                                  (args.search_horizon, args.search_width) if args.align_search else None)
            stages["final_robust"]["s"] = tmax(stages["final_robust"]["s"])
            busy(stages["final_robust"])
            progress("final_robust")
    handoff = None
    if rows is not None and args.handoff:
        engine.profile(False)  # (the hand-off is timed by the wall clock alone, outside the stages)
        handoff = handoff_timings(pd, dp, rows, ln, post, max(1, args.handoff_repeats))
    engine.profile(False)
    engine.trim()  # the frontier's workspace back to the allocator (sst_ctx_trim), after the timed stages
    if not args.host_driven:
        from spectrseqtools_amd import pipeline_device as pd_

        pd_.release_length_buffer()  # and the reach buffer
    if rows is not None and rank == 0 and args.cpu_baseline_s > 0:
        stages["length"]["cpu_baseline"] = length_cpu_baseline(dp, ln, su_seq, batch.seq_mass, max_len, n_len,
                                                               args.cpu_baseline_s)
    cpu_1to4 = None
    if rows is not None and rank == 0 and args.cpu_baseline_s > 0 and args.as_rank is None:
        cpu_1to4 = stages_cpu_baseline(dp, rows, fx, sk, args, data_rank, args.cpu_baseline_s)
        stages["classify"]["cpu_baseline"] = cpu_1to4.pop("a7")

    # per-spectrum alphabet reduction = a table rebuild (canonical + 3 mods)
    keep = {m.names[0] for m in dp.masses[1:5]} | {m.names[0] for m in dp.masses[-3:]}
    from spectrseqtools_amd.masses import EXPLANATION_MASSES as EM

    dp2 = DynamicProgrammingTable(EM, compression_rate=32, tolerance=MATCHING_THRESHOLD, precision=TOLERANCE,
                                  seq=seq0, engine=engine)
    t0 = time.perf_counter()
    dp2.adapt_individual_modification_rates_by_alphabet_reduction(keep)
    engine.synchronize()
    rebuild_ms = 1e3 * (time.perf_counter() - t0)

    peaks = len(batch.observed)
    total_s = sum(v["s"] for v in stages.values())
    if dist:
        t = torch.tensor([peaks, args.spectra], dtype=torch.int64, device=torch.device("cuda", gpu))
        dist.all_reduce(t)
        peaks_all, spectra_all = (int(x) for x in t.tolist())
    else:
        peaks_all, spectra_all = peaks, args.spectra
    ref_est = (n_valid_q + valid_q_rounds) / 70e3 + (explain_q + stages["bins"]["queries"]) / 4.0e3  # (an estimate)
    gpu_s = sum(sum(v[0] for v in st["kernels"].values()) / 1e3 for st in stages.values())
    if rank == 0 and args.dump_outcomes and outcome is not None:
        os.makedirs(args.dump_outcomes, exist_ok=True)
        for r, o in enumerate(outcome):
            np.save(os.path.join(args.dump_outcomes, f"outcome_rank{r if args.as_rank is None else args.as_rank}.npy"),
                    o)
    if rank == 0:
        print(json.dumps({
            **({"handoff": handoff} if handoff is not None else {}),
            "workload": "config5: the prediction pipeline's explanation stages (classify_fragments, the "
                        "filter_by_explanation fixpoint with per-spectrum alphabets, skeleton bin queries, the "
                        "skeleton walk, both length bounds and the Jaccard length on the skeleton alphabets; "
                        "MILP stages excluded) over synthetic spectra",
            "n_gpus": world, "spectra": spectra_all, "peaks": peaks_all,
            "path": "host-driven" if args.host_driven else "device-resident",
            "stages": stages, "total_s": total_s, "gpu_busy_frac": gpu_s / total_s,
            "total_s_without_length": total_s - stages.get("length", {}).get("s", 0.0),
            "spectra_per_s": spectra_all / total_s, "peaks_per_s": peaks_all / total_s,
            "reduction_rebuild_ms": rebuild_ms, "generation_s": gen_s,
            "cpu_baseline_stages1to4": cpu_1to4,
            "reference_estimate_s_per_gpu_share": ref_est,
            "reference_estimate_basis": "an ESTIMATE, not timed: BASELINE.md single-core rates of the reference "
                                        "Python (is_valid 70k/s, explain 4.0k/s) times this GPU's query counts "
                                        "(1 core); cpu_baseline_stages1to4 is the measured leg",
        }), flush=True)
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
