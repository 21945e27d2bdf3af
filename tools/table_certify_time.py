#!/usr/bin/env python3
"""Cost of certifying an uploaded table (sst_table_certify) on the full 105-row
alphabet, compression 32: the upload (host to device copy, index, valid
bitset), the certify kernel by its profile id, the bytes it checks and the
rate, beside the same run's sst_table_build and a device-to-device copy of a
buffer of the packed table's size (the yardstick: the copy moves twice the
bytes the check has to read).  Each figure is the median of `--rounds` fresh
uploads (a table is certified once).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
from conftest import load_golden  # noqa: E402
from spectrseqtools_amd import _native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch

    rows = sorted({r["tolerated_integer_masses"] for r in load_golden("alphabet.json")["rows"]} | {0})
    eng = _native.get_engine(0)
    _native.DeviceTable.build(rows, max(rows) * 35, 32, engine=eng).close()  # warm: module load, allocator
    t0 = time.perf_counter()
    built = _native.DeviceTable.build(rows, max(rows) * 35, 32, engine=eng)
    build_s = time.perf_counter() - t0
    words = built.download()
    n_bytes = int(words.nbytes)
    upload_s, certify_ms, certify_wall_s = [], [], []
    eng.profile(True, kernels=[_native.K_TABLE_CERTIFY])
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        up = _native.DeviceTable.upload(rows, words, 32, engine=eng)
        upload_s.append(time.perf_counter() - t0)
        eng.profile_read()
        t0 = time.perf_counter()
        assert up.certify() is True
        certify_wall_s.append(time.perf_counter() - t0)  # kernel + pair list, census, limits
        ms, n = eng.profile_read()[_native.K_TABLE_CERTIFY]
        assert n == 1
        certify_ms.append(ms)
        assert (up.pair_records() == built.pair_records()).all()
        up.close()
    eng.profile(False)
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    src.fill_(1)
    copy_ms = []
    for _ in range(args.rounds + 1):  # the first is a warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        copy_ms.append(a.elapsed_time(b))
    med = statistics.median
    k_ms, c_ms = med(certify_ms), med(copy_ms[1:])
    print(json.dumps({
        "workload": "certify an uploaded table: 105 rows, compression 32", "shape": list(words.shape),
        "bytes": n_bytes, "rounds": args.rounds, "table_build_s": build_s, "upload_s": med(upload_s),
        "certify_kernel_ms": k_ms, "certify_kernel_ms_all": certify_ms, "certify_gb_per_s": n_bytes / k_ms / 1e6,
        "certify_call_s": med(certify_wall_s), "d2d_copy_ms": c_ms, "d2d_copy_ms_all": copy_ms[1:],
        "d2d_copy_gb_per_s_moved": 2 * n_bytes / c_ms / 1e6, "certify_over_copy": k_ms / c_ms}))


if __name__ == "__main__":
    main()
