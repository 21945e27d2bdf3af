"""The drop-in boundary: libsstgpu.so loads on a GPU-less host, exports every
function include/sst.h declares, and fails loudly (no CPU fallback) when no
HIP device is visible.  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from spectrseqtools_amd import _native

HEADER = os.path.join(REPO, "include", "sst.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sst_[a-z_]+)\s*\(", src)))


def test_header_and_exports_agree():
    assert header_functions() == sorted(_native.EXPORTS)


def test_library_exports_every_header_symbol():
    lib = _native.load_library()
    for name in header_functions():
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (sst_\w+)", out))
    assert set(header_functions()) <= exported


def test_library_targets_gfx950(tmp_path):
    # llvm-objdump --offloading writes the code objects it lists next to its
    # input: run it on a copy in a scratch directory, not on the in-tree library
    lib = tmp_path / "libsstgpu.so"
    shutil.copyfile(_native.LIB_PATH, lib)
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", str(lib)],
                         capture_output=True, text=True, cwd=tmp_path)
    text = out.stdout + out.stderr
    if "gfx" not in text:  # older objdump: fall back to the raw bundle id string
        text = open(_native.LIB_PATH, "rb").read().decode("latin-1")
    assert "gfx950" in text


def header_struct_fields(name):
    """[(field, base type, is pointer, array length or None)] of a header struct, in its order."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", src, flags=re.S).group(1)
    out = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        base, rest = re.fullmatch(r"(?:const\s+)?(\w+)\b\s*(.*)", stmt, flags=re.S).groups()
        for decl in rest.split(","):
            star, field, length = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[(\w+)\])?\s*", decl).groups()
            if length is not None and not length.isdigit():
                length = re.search(rf"#define\s+{length}\s+(\d+)", src).group(1)
            out.append((field, base, bool(star), None if length is None else int(length)))
    return out


SCALARS = {"double": ctypes.c_double, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}


def native_mirrors():
    """{header struct: ctypes mirror} of every Structure in _native whose docstring names its header struct."""
    out = {}
    for obj in vars(_native).values():
        if isinstance(obj, type) and issubclass(obj, ctypes.Structure) and obj is not ctypes.Structure:
            m = re.match(r"(sst_\w+) \(include/sst\.h\)", obj.__doc__ or "")
            if m:
                out[m.group(1)] = obj
    return out


def test_mirrors_cover_the_stage_structs():
    assert {"sst_row_slots", "sst_classify_args", "sst_fix_args", "sst_bins_args", "sst_dict_args",
            "sst_length_queries", "sst_walk_args", "sst_handoff_args", "sst_exact_io"} <= set(native_mirrors())


@pytest.mark.parametrize("name", sorted(native_mirrors()))
def test_ctypes_mirror_matches_header_struct(name):
    """The mirror has the header struct's fields, in its order, each of the
    header's kind: any pointer a c_void_p, a scalar its ctypes twin, T x[N]
    an array of N of them."""
    want = []
    for field, base, pointer, length in header_struct_fields(name):
        kind = ctypes.c_void_p if pointer else SCALARS[base]
        want.append((field, kind if length is None else kind * length))
    assert [(n, t) for n, t, *_ in native_mirrors()[name]._fields_] == want
    if name == "sst_walk_args":  # the array fields are seen
        assert ("rq_block", ctypes.c_void_p * 16) in want


def test_no_cpu_fallback_without_device():
    lib = _native.load_library()
    if lib.sst_device_count() > 0:
        pytest.skip("a HIP device is visible")
    with pytest.raises(_native.EngineError):
        _native.Engine(0)
    h = ctypes.c_void_p()
    assert lib.sst_ctx_create(0, ctypes.byref(h)) != 0


def test_null_arguments_rejected():
    lib = _native.load_library()
    assert lib.sst_table_build(None, None, 0, 0, 32, None) < 0
    assert lib.sst_is_valid_batch(None, None, None, 0, 1e-5, 1e-3, None) < 0
    assert lib.sst_explain_batch(None, None, None, 0, 1e-5, 1e-3, None, 0, 1, 1, None) < 0
    assert lib.sst_result_stats(None, None) < 0
    assert lib.sst_profile_sample(None, 1) < 0
    assert lib.sst_last_error(None) == b"null context"


def test_budget_conversion():
    # the reference only tests `A > 0` and decrements by one (mass_explanation.py:166-172)
    assert _native._budget(np.inf) == -1
    assert _native._budget(None) == -1
    assert _native._budget(3) == 3
    assert _native._budget(2.5) == 3
    assert _native._budget(-2) == 0
    assert _native._budget(-np.inf) == 0
    arr, s = _native._mods([1, np.inf, 0], 3)
    assert arr.tolist() == [1, -1, 0] and s == 0


def test_library_matches_its_build_record():
    """The shipped libsstgpu.so is the one built from this tree's sources
    (spectrseqtools_amd/build_record.json: the Makefile writes it after every
    link; the loader refuses a library or sources that no longer match)."""
    import json
    import os

    from spectrseqtools_amd import build_record

    if not os.path.exists(build_record.LIB):
        pytest.skip("libsstgpu.so not built")
    assert build_record.check() is None, build_record.check()
    rec = json.load(open(build_record.RECORD))
    assert rec["arch"] == "gfx950" and rec["library"]["bytes"] == os.path.getsize(build_record.LIB)
    assert set(rec["sources"]) >= {"spectrseqtools_amd/csrc/sst_kernels.hip", "include/sst.h"}
