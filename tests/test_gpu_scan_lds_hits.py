"""GPU tests of the scan waves' LDS hit-record slots: a wave keeps the hit
records of its tiles in LDS while they fit its slot and the record's fields,
and from the first tile that does not it writes that tile's and every later
tile's records to its worklist region in device memory (sticky, decided per
tile).  Where a wave switches must not show in the result.

Each capacity (SST_SCAN_LDS_HITS, read once per process) runs in a child
process (_scan_lds_hits_check.py) over the same cases, through
sst_step_device (256 scan workgroups) and sst_explain_batch_device (512):
every query a hit ("all": 64 records per tile), "mixed", "routed", and
"wide" (windows whose counts do not fit the record's u8 count), with query
counts that give each wave 1, 2 or 3-4 tiles.

The kinds are those of test_gpu_step_shapes._queries with three departures,
made in _scan_lds_hits_check.build_queries.  At these batch sizes (0.26 M to
1.57 M queries) the shapes test's "mixed" thresholds (up to 140 mDa) and its
two-row sums past 3 w_min = 915 Da give 39 B of payload per query, more than
the 16 B per query the first pass allows, so the engine re-runs the pass
unfused -- and a re-run keeps no record in LDS and reports no pair hits, i.e.
it would not run the code under test (measured: n_pair = 0 on every such
case).  So "mixed" keeps the shapes test's masses but takes thresholds of 3
to 20 mDa and replaces two-row sums past 900 Da by one-row masses; "routed"
is that plus 100 three-row sums (the deferred DFS is slow); and the wide
windows are 20 000 masses wide, not hundreds: the pair list holds about one
sum per 100 masses, so nothing narrower reaches a count of 255.  The child
asserts for every case that the fused scan answered (pair hits present and
all but the routed windows' hits among them).

K = 1 switches inside the
first tile, K = 64 is exactly filled by one all-hit tile, K = 100 switches at
a later tile boundary; crafted tiles make one wave end exactly on each.

For every capacity the status bytes, the pair hits' dense records, hit_refs,
their payload, the totals, the is_valid bytes and the canonical digest of all
answers equal the K = 0 run's.  The K = 0 run itself is compared per query
with the two separate calls and on a sample with the CPU oracle (in the
child).  A case cannot pass by never spilling: the waves' hit counts, taken
from the result and the scan order, must exceed every forced capacity and
meet it exactly on a tile boundary; the default must hold every wave of
"mixed"."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SAME = ("n", "n_hits", "n_pair", "pair_bytes", "payload_bytes", "status", "pair_hits", "refs", "pair_payload",
        "answers", "valid", "max_wave_hits", "max_count")


def _child(tmp, k, *flags):
    env = dict(os.environ)
    env.pop("SST_SCAN_LDS_HITS", None)
    if k is not None:
        env["SST_SCAN_LDS_HITS"] = str(k)
    out = os.path.join(str(tmp), f"k_{k}.json")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_scan_lds_hits_check.py"), out, *flags], env=env,
                       capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "scan lds hits ok" in p.stdout
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """The K = 0 run: every record through the worklist region."""
    ref = _child(tmp_path_factory.mktemp("scan_lds_hits"), 0, "--reference")
    assert ref["K"] == 0
    return ref


def test_reference_has_the_cases(reference):
    c = reference["cases"]
    for api in ("step", "plain"):
        assert c[f"{api}_all_3"]["n_pair"] == c[f"{api}_all_3"]["n"]
        assert c[f"{api}_wide_3"]["max_count"] > 254
        assert c[f"{api}_routed_3"]["n_hits"] > c[f"{api}_routed_3"]["n_pair"]
        assert c[f"{api}_mixed_1"]["max_wave_hits"] <= 2 * 64


@pytest.mark.parametrize("k", (1, 64, 100, None))
def test_capacity_does_not_show(reference, tmp_path, k):
    got = _child(tmp_path, k)
    if k is not None:
        assert got["K"] == k  # (below the largest the LDS holds)
    else:
        assert got["K"] > 300  # what the budget rule leaves behind a <= 44 KB image
    assert got["cases"].keys() == reference["cases"].keys()
    for name, c in got["cases"].items():
        want = reference["cases"][name]
        for key in SAME:
            assert c[key] == want[key], (name, key)
    for api in ("step", "plain"):
        c = got["cases"]
        if k is None:
            for rounds in (1, 2, 3):  # the default holds every wave of "mixed"
                assert not c[f"{api}_mixed_{rounds}"]["exceeds"], (api, rounds, c[f"{api}_mixed_{rounds}"])
            continue
        for kind in ("all", "mixed", "routed", "wide"):  # three tiles and more per wave: some wave spills
            assert c[f"{api}_{kind}_3"]["exceeds"], (api, kind)
        for kind in ("mixed", "routed", "wide") + (("all",) if k == 64 else ()):
            assert c[f"{api}_{kind}_3"]["boundary"], (api, kind)  # a wave ends a tile exactly at the capacity
