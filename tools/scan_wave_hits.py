"""Hit records per scan wave on the plain bench line's batches (bench.py,
config 3, sst_step_device), against the capacity of the waves' LDS hit-record
slots (sst_table_scan_lds_hits): a wave above it writes its later
records to its worklist region in HBM.  Prints one JSON line.
usage: scan_wave_hits.py [--spectra N] [--batches R] [--seed S]"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=10000)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000)
    args = ap.parse_args()
    import torch

    from spectrseqtools_amd import _native
    from spectrseqtools_amd.masses import EXPLANATION_MASSES, MATCHING_THRESHOLD, TOLERANCE
    from spectrseqtools_amd.mass_table import DynamicProgrammingTable, SequenceInformation
    from spectrseqtools_amd.parallel import device_bytes

    engine = _native.get_engine(0)
    dev_t = torch.device("cuda", engine.device)
    seq = SequenceInformation(max_len=20, su_mass=6500.0, obs_mass=6500.0, modification_rate=0.5)
    dp = DynamicProgrammingTable(EXPLANATION_MASSES, compression_rate=32, tolerance=MATCHING_THRESHOLD,
                                 precision=TOLERANCE, seq=seq, engine=engine)
    A = round(seq.modification_rate * seq.max_len)
    tdev = dp.device_table
    K = tdev.scan_lds_hits()
    out = {"lds_hits_per_wave": K, "batches": []}
    for b in range(args.batches):
        w = bench.build_workload(args.spectra, args.seed + 7919 * b, dp)
        obs, m, t = (torch.from_numpy(w[k]).to(dev_t) for k in ("obs", "a8_mass", "a8_thr"))
        n = len(w["a8_mass"])
        out7 = torch.empty(len(w["a7_mass"]), dtype=torch.int8, device=dev_t)
        torch.cuda.synchronize()
        res = tdev.step_device(obs.data_ptr(), len(w["obs"]), w["shifts"], out7.data_ptr(), m.data_ptr(), t.data_ptr(),
                               n, dp.tolerance, dp.precision, A)
        hits_p, n_hits = res.hit_list_device()
        _, n_pair, pair_bytes, n_wg = res.pair_hits_device()
        h = device_bytes(hits_p, 16 * n_hits, dev_t).cpu().numpy().view(np.uint32).reshape(-1, 4)
        engine.synchronize()
        waves = 16 * n_wg
        per_wave = np.bincount((h[:n_pair, 0].astype(np.int64) >> 6) % waves, minlength=waves)
        cnt = h[:n_pair, 1]
        out["batches"].append({
            "queries": n, "scan_workgroups": n_wg, "pair_hits": n_pair, "pair_payload_bytes": pair_bytes,
            "hits_per_wave": {"min": int(per_wave.min()), "median": float(np.median(per_wave)),
                              "p99": float(np.percentile(per_wave, 99)), "max": int(per_wave.max())},
            "waves_above_capacity": int((per_wave > K).sum()),
            "share_of_waves_above_capacity": float((per_wave > K).mean()),
            "hits_with_count_above_255": int((cnt > 255).sum()),
            # a 4-B record would hold a 3-bit count (the wire format's): under the sticky
            # rule a wave would leave its LDS slot at its first count above 7
            "hits_with_count_above_7": int((cnt > 7).sum()),
            "waves_with_a_count_above_7": int(len(np.unique(((h[:n_pair, 0].astype(np.int64) >> 6) % waves)[cnt > 7]))),
            "tiles_per_wave": -(-((n + 63) // 64) // waves)})
        res.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
