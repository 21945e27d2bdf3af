"""GPU tests of the final program's limits (k_final_program in
csrc/sst_final.hip): the branches no other test reaches.  Every case is the
device equal to final_program.final_host in all nine arrays (test_gpu_final.run)
-- tests/test_final_model.py holds the host model to the brute force on the same
kinds of input at a size it can enumerate -- and the facts below are pinned as
well: 22 and 23 free positions and the digit table's 512 entries, combos up to
and at saturation, record chunks times passes under a use mask that empties the
middle chunk, 16384 and 16385 used fragments, L == 0 and L == 1, su that is NaN,
infinite, negative or at the fixed-point range's edge, and tables of 64, 65 and
120 rows with alphabet and skeleton bits set for rows that do not exist (there
also through the alignment certificate's keep mode, base and split)."""
from types import SimpleNamespace

import numpy as np
import pytest

import _align_caps_cases as CC
import _align_cases as AC
import _align_keep_cases as KC
import _final_cases as FC
from _align_gpu import K, engine, full_table  # noqa: F401
from test_gpu_final import CHUNK, WG, masses_of, run

pytestmark = pytest.mark.gpu
MAX_COMBOS = 1 << 22  # sst_final_max_combos()
SATURATED = (1 << 64) - 1


def test_22_and_23_free_positions(full_table):  # noqa: F811
    """22 positions of two rows each are 2^22 == max_combos assignments over
    the last row of D: SOLVED, and with every digit 1 the optimum is the last
    index of the last pass.  23 are more free positions than are recorded:
    TOO_LARGE with combos == 2^23; 22 at max_combos == 2^22 - 1 likewise."""
    dp = full_table
    rm = masses_of(dp)
    pairs = FC.distinct_pairs(rm, 23)
    s22, y = FC.pinned_binary_spec(rm, 22, [1] * 22, dp.precision, pairs=pairs[:22])
    s23, _ = FC.pinned_binary_spec(rm, 23, [1] * 23, dp.precision, pairs=pairs)
    o, got = run(dp, [s22, s23], rm, max_combos=MAX_COMBOS)
    assert got.status.tolist() == [FC.SOLVED, FC.TOO_LARGE] and got.combos.tolist() == [1 << 22, 1 << 23]
    assert got.n_feas.tolist() == [1 << 22, 0] and got.n_opt.tolist() == [1, 0] and got.best.tolist() == [0, 0]
    assert got.seq[:22].tolist() == y and (got.gap[0] > 0) and (got.iv[:22] == np.arange(22)).all()
    _, below = run(dp, [s22], rm, max_combos=MAX_COMBOS - 1)
    assert below.status.tolist() == [FC.TOO_LARGE] and below.combos.tolist() == [1 << 22] and below.n_feas.tolist() == [0]


def test_digit_table_edge_and_saturating_combos(full_table):  # noqa: F811
    """Four positions of all 104 rows and one of 96 fill the digit table (512),
    one of 97 passes it: TOO_LARGE with the exact product.  104^9 is below 2^64
    and exact, 104^10 and 253 unconstrained positions report 2^64 - 1, and a
    spectrum of that size that is not row-free is NOT_FREE with the saturated
    combos (NOT_FREE comes before TOO_LARGE)."""
    dp = full_table
    rm = masses_of(dp)
    rows = list(range(1, len(rm)))
    assert len(rows) == 104
    one = [(FC.START_END, rm[1] * dp.precision, 100.0, 0, 0), (FC.INTERNAL, rm[2] * dp.precision, 100.0, 0, 0)]
    open_spec = lambda L: {"L": L, "pos": [(0, 0)] * L, "alpha": AC.mask(rows + [0]), "frags": one,  # noqa: E731
                           "row_mod": np.zeros(len(rm), np.uint8), "mod_cap": L}
    specs = [FC.loose_spec(rm, [rows] * 4 + [rows[:96]], one), FC.loose_spec(rm, [rows] * 4 + [rows[:97]], one),
             FC.loose_spec(rm, [rows] * 9, one), open_spec(10), open_spec(253), open_spec(11), open_spec(12)]
    row_cap = KC.loose_row_cap(len(rm)).reshape(KC.MAX_LEN + 1, -1)
    row_cap[11, 7] = 10  # row 7 is in all eleven sets and unmodified: not free
    for max_combos in (1 << 20, MAX_COMBOS):
        _, got = run(dp, specs, rm, row_cap.reshape(-1), max_combos)
        assert got.status.tolist() == [FC.TOO_LARGE] * 5 + [FC.NOT_FREE, FC.TOO_LARGE]
        assert got.combos.tolist() == [104 ** 4 * 96, 104 ** 4 * 97, 104 ** 9] + [SATURATED] * 4
    assert 104 ** 4 * 96 > MAX_COMBOS and 104 ** 9 < SATURATED < 104 ** 10 and 4 * 104 + 96 == 512


def test_chunks_times_passes(full_table):  # noqa: F811
    """1100 fragments (three chunks of records) over 729 assignments (three
    passes) at a noise that lets lanes stop summing early, across chunk
    reloads, with a use mask that leaves the middle chunk entirely unused; and
    exactly 512, 513 and 1024 fragments (one chunk, one record more, two full
    chunks) at 729 assignments."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(93)
    rows = list(range(1, 19))
    sets = [rows[3 * i:3 * i + 3] for i in range(6)]
    masked = FC.chunk_mask_spec(rm, sets, 1100, dp.precision, rng, unused=(CHUNK, 2 * CHUNK))
    exact = [FC.loose_spec(rm, sets, FC.random_frags(rng, rm, sets, n, dp.precision, noise=400)) for n in (512, 513, 1024)]
    o, got = run(dp, [masked, dict(masked, use=None)] + exact, rm)
    assert got.status.tolist() == [FC.SOLVED] * 5 and got.combos.tolist() == [729] * 5 and 729 > 2 * WG
    iv = got.iv[:1100]
    assert (iv[CHUNK:2 * CHUNK] == 0xFFFE).all() and (iv[:CHUNK] != 0xFFFE).all() and (iv[2 * CHUNK:] != 0xFFFE).all()
    assert (got.iv[1100:] != 0xFFFE).all() and got.best[0] < got.best[1] and (got.gap != FC.NO_GAP).all()


def test_used_fragments_at_the_limit(full_table):  # noqa: F811
    """16390 identical START_END fragments over one position of two rows:
    16384 in use is SOLVED (the objective 16384 times one fragment's), 16385 is
    SKIPPED."""
    dp = full_table
    rm = masses_of(dp)
    specs, a, b = FC.n_used_specs(rm, dp.precision)
    o, got = run(dp, specs, rm)
    assert got.status.tolist() == [FC.SOLVED, FC.SKIPPED] and got.combos.tolist() == [2, 0]
    assert got.best[0] == 0 and got.seq.tolist() == [b, 0] and got.n_opt[0] == 1
    assert got.gap[0] == 16384 * FC.FIX * abs(rm[b] - rm[a])
    assert (got.iv[:16390] != 0xFFFE).sum() == 16384 and (got.iv[16390:] == 0xFFFE).all()


def test_zero_and_one_position(full_table):  # noqa: F811
    """L == 0 with fragments: one assignment, the empty interval everywhere,
    the objective the sum of |qfix|; a used START fragment makes it SKIPPED.
    L == 1 with one, two and three rows."""
    dp = full_table
    rm = masses_of(dp)
    rng = np.random.default_rng(94)
    zero, want, objective = FC.zero_length_specs(rm, dp.precision)
    ones = [FC.loose_spec(rm, sets, FC.random_frags(rng, rm, sets, 9, dp.precision)) for sets in ([[5]], [[1, 2]], [[3, 4, 6]])]
    o, got = run(dp, zero + ones, rm)
    assert got.status.tolist() == want + [FC.SOLVED] * 3 and got.combos.tolist() == [1, 1, 0, 1, 1, 2, 3]
    for g in (0, 1):
        assert got.best[g] == objective and got.n_opt[g] == 1 and got.n_feas[g] == 1 and got.gap[g] == FC.NO_GAP
        assert (got.iv[o.frag_off[g]:o.frag_off[g + 1]] == 0xFFFF).all() and not got.sum[o.frag_off[g]:o.frag_off[g + 1]].any()
    assert got.best[3] == objective and got.iv[o.frag_off[4] - 1] == 0xFFFE and o.pos_off[4] == 0


def test_su_values(full_table):  # noqa: F811
    """su that is NaN, +inf, -inf or +-2^32 precision units makes a spectrum
    SKIPPED where the fragment is used and leaves it SOLVED where it is not, in
    every class; +-(2^32 - 1) units and negative su stay within the model."""
    dp = full_table
    rm = masses_of(dp)
    specs, want = FC.su_value_specs(rm, dp.precision)
    _, got = run(dp, specs, rm)
    assert got.status.tolist() == want
    assert want.count(FC.SKIPPED) == 4 * len(FC.SU_OUTSIDE) and want.count(FC.SOLVED) == 4 * (len(FC.SU_OUTSIDE) + len(FC.SU_INSIDE))


@pytest.mark.parametrize("n_rows", [64, 65, 120])
def test_row_count_edges(engine, K, n_rows):  # noqa: F811
    """Tables of 64, 65 and 120 rows (the row masks' three branches are below
    64, 64 to 127 and 128): free positions over rows {63, 64} and the last two
    rows, modified rows at 64 and above, and every alphabet and constrained
    position with all bits at and above n_rows set, which the kernels ignore --
    through the final program and through keep mode's base and split kernels."""
    from spectrseqtools_amd import _native, alignment

    rm, specs, row_cap = FC.row_edge_case(n_rows, 0.001, np.random.default_rng(95))
    table = _native.DeviceTable.build(rm, max(rm) * 4, 32, engine=engine)
    dp = SimpleNamespace(masses=[SimpleNamespace(mass=m) for m in rm], device_table=table, precision=0.001, tolerance=1e-5)
    try:
        o, got = run(dp, specs, rm, row_cap)
        assert got.combos[0] == (8 if n_rows > 64 else 4) and got.status[:2].tolist() == [FC.SOLVED] * 2
        assert got.n_feas[1] < got.combos[1] and got.status[5] == FC.INFEASIBLE and got.combos[5] == 0
        assert got.status[6] == FC.NOT_FREE and (got.status[7] == FC.NOT_FREE) == (n_rows == 64)
        assert (o.alpha[:, 1] >> np.uint64(63)).all() and (o.alpha[:, 0] & np.uint64(1)).all()
        caps = CC.caps_of(specs, n_rows)
        for split in (False, True):
            host = alignment.align_host(o, dp.tolerance, dp.precision, K, split=split, caps=caps, keep=row_cap)
            dev = alignment.align_device(dp, o, split=split, caps=caps, keep=row_cap)
            KC.same7(dev, host, ("rows", n_rows, "split", split))
        assert host.spec_free[[0, 1, 3, 4]].all() and not host.spec_free[[5, 6]].any() and host.keep.sum() >= 10
        assert (host.status[o.frag_off[5]:o.frag_off[6]] == AC.INFEASIBLE).all()
    finally:
        table.close()
