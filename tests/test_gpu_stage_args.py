"""The row stages' and the length bounds' argument structs at the C boundary
(include/sst.h: sst_row_slots, sst_classify_args, sst_fix_args, sst_bins_args,
sst_dict_args, sst_length_queries): each of the eleven entry points, called
through _native.lib() directly, refuses a null struct and a null required
array with SST_E_ARG.  One spectrum of three peaks on a table of three masses,
every array at its minimum size; the refusals precede any launch, so nothing
is queued and no kernel runs here."""
import ctypes

import pytest

from spectrseqtools_amd import _native

pytestmark = pytest.mark.gpu

SST_E_ARG = -1
MASSES = [0, 305042, 329053, 345048]
PEAKS, SLOTS = 3, 12  # row slots: 4 per peak
ROWS = ("peak_off", "su", "obs", "meta", "alive", "cnt")
FIX = ("alpha", "alpha_next", "active", "active_next", "rounds", "queries", "n_active")
QUERIES = ("su", "obs", "spec", "alpha", "lower", "upper", "status")

# entry point -> (its positional arguments after the table, the arrays it requires with n_spec = 1 / n = 1).
# An argument is a struct ("rows", "args", "x": passed by reference) or a loose pointer / value (by name).
STAGES = {
    "sst_classify_rows_device": (("rows", "args", "d_err"),
                                 [f"rows.{f}" for f in ROWS] + ["args.obs", "args.su_seq", "args.shifts", "args.sides",
                                                                "d_err"]),
    "sst_fix_round_device": (("rows", "args", "d_err", "no_x"),
                             [f"rows.{f}" for f in ROWS] + [f"args.{f}" for f in FIX] + ["d_err"]),
    "sst_fix_finish_device": (("rows", "args", "d_err", "x"),
                              ["rows.cnt"] + [f"args.{f}" for f in FIX] + ["d_err", "x.xa_st", "x.xa_n", "x.xa_ptr"]),
    "sst_valid_rows_alpha_device": (("rows", "d_alpha", "d_active", "tol", "prec", "d_err"),
                                    [f"rows.{f}" for f in ROWS if f != "meta"] + ["d_alpha", "d_err"]),
    "sst_bins_count_device": (("rows", "args", "d_err"),
                              [f"rows.{f}" for f in ROWS] + ["args.q_off", "args.n_q", "d_err"]),
    "sst_bins_emit_device": (("rows", "args", "d_err"),
                             [f"rows.{f}" for f in ROWS] + ["args.q_off", "args.alpha", "args.status", "args.count",
                                                            "d_err"]),
    "sst_dict_count_device": (("rows", "args", "d_err"), [f"rows.{f}" for f in ROWS] + ["args.off", "args.n_q", "d_err"]),
    "sst_dict_build_device": (("rows", "args", "d_err", "no_x"),
                              [f"rows.{f}" for f in ROWS] + ["args.alpha", "args.off", "args.n_ent", "d_err"]),
    "sst_dict_list_device": (("rows", "args", "d_err", "x"), [f"rows.{f}" for f in ROWS] + ["d_err"]),
    "sst_length_bounds_reach_device": (("args", "d_reach_bits", "d_reach_off", "d_reach_words", "soft_nodes",
                                        "memo_first", "fuse"),
                                       [f"args.{f}" for f in QUERIES] + ["d_reach_bits", "d_reach_off", "d_reach_words"]),
    "sst_length_bounds_frontier_device": (("args", "d_lr", "d_lr_off", "workspace_bytes", "no_stats"),
                                          [f"args.{f}" for f in QUERIES] + ["d_lr", "d_lr_off"]),
}
ARGS_STRUCT = {"sst_classify_rows_device": _native.ClassifyArgs, "sst_fix_round_device": _native.FixArgs,
               "sst_fix_finish_device": _native.FixArgs, "sst_bins_count_device": _native.BinsArgs,
               "sst_bins_emit_device": _native.BinsArgs, "sst_dict_count_device": _native.DictArgs,
               "sst_dict_build_device": _native.DictArgs, "sst_dict_list_device": _native.DictArgs,
               "sst_length_bounds_reach_device": _native.LengthQueries,
               "sst_length_bounds_frontier_device": _native.LengthQueries}
VALUES = {"tol": 1e-5, "prec": 1e-3, "soft_nodes": 0, "memo_first": 0, "fuse": 0, "workspace_bytes": 1 << 20,
          "no_x": None, "no_stats": None}


@pytest.fixture(scope="module")
def table():
    t = _native.DeviceTable.build(MASSES, max(MASSES) * 35, 32, engine=_native.get_engine(0))
    yield t
    t.close()


@pytest.fixture(scope="module")
def arrays(table):
    """One small zeroed device array per pointer the entry points take, and two host arrays (shifts, sides)."""
    import numpy as np
    import torch

    dev = torch.device("cuda", table.engine.device)
    keep = []

    def ptr(nbytes):
        keep.append(torch.zeros(nbytes, dtype=torch.uint8, device=dev))
        return keep[-1].data_ptr()

    host = [np.zeros(1, np.float64), np.zeros(1, np.uint8)]
    structs = {
        "rows": _native.RowSlots(1, ptr(16), ptr(8 * SLOTS), ptr(8 * SLOTS), ptr(4 * SLOTS), ptr(SLOTS), ptr(4)),
        _native.ClassifyArgs: _native.ClassifyArgs(ptr(8 * PEAKS), PEAKS, None, 0.5e6, 1000.0, ptr(8),
                                                   host[0].ctypes.data, host[1].ctypes.data, 1, 400.0, 1e-5, 1e-3,
                                                   None),
        _native.FixArgs: _native.FixArgs(ptr(16), ptr(16), ptr(1), ptr(1), ptr(4), ptr(4), ptr(4), 400.0, 1e-5, 1e-3),
        _native.BinsArgs: _native.BinsArgs(alpha=ptr(16), tol=1e-5, prec=1e-3, n_q=ptr(4), n_q0=ptr(4), q_off=ptr(16),
                                           status=ptr(1), count=ptr(4)),
        _native.DictArgs: _native.DictArgs(ptr(16), 400.0, 1e-5, 1e-3, ptr(4), ptr(16), ptr(8), ptr(8), ptr(4)),
        _native.LengthQueries: _native.LengthQueries(ptr(8), ptr(8), ptr(4), ptr(16), 1, 1e-5, 1e-3, 4, 2, ptr(8),
                                                     ptr(8), ptr(1)),
        "x": _native.ExactIO(ptr(1), ptr(8), ptr(8), ptr(4), ptr(1), ptr(4), 1, ptr(8), ptr(1), ptr(4), ptr(8)),
    }
    loose = {n: ptr(16) for n in ("d_err", "d_alpha", "d_active", "d_reach_bits", "d_reach_off", "d_reach_words",
                                  "d_lr", "d_lr_off")}
    torch.cuda.synchronize(dev)
    yield structs, loose
    del keep, host


def call(table, arrays, name, null):
    """The entry point with the array or struct `null` (as in STAGES) passed as NULL; (return code, whether the
    context's error text changed: a refusal of a null argument sets none)."""
    structs, loose = arrays
    given = {"rows": structs["rows"], "args": structs[ARGS_STRUCT[name]] if name in ARGS_STRUCT else None,
             "x": structs["x"]}
    where, _, field = null.partition(".")
    if field:  # a copy of the struct without that array
        given[where] = type(given[where]).from_buffer_copy(given[where])
        assert getattr(given[where], field), null
        setattr(given[where], field, None)
    argv = []
    for a in STAGES[name][0]:
        if a == null:
            argv.append(None)
        elif a in given:
            argv.append(ctypes.byref(given[a]))
        else:
            argv.append(VALUES[a] if a in VALUES else loose[a])
    L = _native.lib()
    before = L.sst_last_error(table.engine.handle)
    rc = getattr(L, name)(table.handle, *argv)
    return rc, L.sst_last_error(table.engine.handle) != before


@pytest.mark.parametrize("name,null", [(n, r) for n, (_, req) in STAGES.items() for r in req])
def test_null_required_array_is_refused(table, arrays, name, null):
    assert call(table, arrays, name, null) == (SST_E_ARG, False)


@pytest.mark.parametrize("name,null", [(n, s) for n, (argv, _) in STAGES.items() for s in ("rows", "args", "x")
                                       if s in argv])
def test_null_struct_is_refused(table, arrays, name, null):
    assert call(table, arrays, name, null) == (SST_E_ARG, False)


def test_every_reworked_entry_point_is_covered():
    assert len(STAGES) == 11 and set(STAGES) <= set(_native.EXPORTS)
