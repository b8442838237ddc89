"""CPU: the C-ABI surface of SemanticKITTI's training-time validation loops (csrc/kitti_block_test.hip): the five entry points
are declared in include/pasnl.h, listed in pointasnl_amd._hip.SYMBOLS, exported by the built library, and answer bad arguments
with their error code before any launch -- no GPU is needed for any of it."""
import ctypes
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["pasnl_kblock_crop_stats", "pasnl_kblock_grid_count", "pasnl_kblock_fill", "pasnl_kblock_gather", "pasnl_kblock_rotate"]
OK, EINVAL, ENULL, EUNSUPPORTED = 0, -1, -2, -5  # include/pasnl.h
L, D, NULL = ctypes.c_long, ctypes.c_double, ctypes.c_void_p(0)
SOME = ctypes.c_void_p(64)  # a non-NULL pointer: never dereferenced, the calls below all return before any launch


def test_the_five_entries_are_declared_in_the_header_under_their_own_section():
    header = open(os.path.join(os.path.dirname(HERE), "include", "pasnl.h")).read()
    section = header[header.index("SemanticKITTI's training-time validation loops"):]
    for cite in ("semantic_kitti_dataset.py (D) :68-109", ":164-211", "(T) :267-328", ":331-418", "(P) :71-89"):
        assert cite in section.split("*/")[0], cite
    code = re.sub(r"/\*.*?\*/", "", section, flags=re.S)
    assert re.findall(r"\b(pasnl_kblock_[a-z_]+)\s*\(", code) == NAMES


def test_the_five_entries_are_exported_by_the_built_library():
    from pointasnl_amd import _hip

    lib = _hip.lib()
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pasnl_\w+)", nm))
    for name in NAMES:
        assert name in _hip.SYMBOLS and hasattr(lib, name) and name in exported


def test_bad_arguments_are_refused_before_any_launch():
    from pointasnl_amd import _hip

    lib = _hip.lib()
    # n <= 0, a centre outside the scan
    assert lib.pasnl_kblock_crop_stats(L(0), SOME, SOME, SOME, L(0), D(5.0), SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_crop_stats(L(100), SOME, SOME, SOME, L(100), D(5.0), SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_crop_stats(L(100), SOME, SOME, SOME, L(-1), D(5.0), SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_crop_stats(L((1 << 30) + 1), SOME, SOME, SOME, L(0), D(5.0), SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_grid_count(L(0), SOME, SOME, 3, 3, D(10.0), SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_grid_count(L(100), SOME, SOME, 0, 3, D(10.0), SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_grid_count(L(100), SOME, SOME, 3, 3, D(0.0), SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_fill(L(0), SOME, SOME, L(-1), D(5.0), 3, 3, D(10.0), D(0.01), SOME, SOME, L(5), SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_fill(L(100), SOME, SOME, L(-1), D(5.0), 3, 3, D(10.0), D(0.01), SOME, SOME, L(0), SOME, SOME, NULL) == EINVAL
    # the chopped column is one column
    assert lib.pasnl_kblock_fill(L(100), SOME, SOME, L(7), D(5.0), 2, 1, D(10.0), D(0.01), SOME, SOME, L(5), SOME, SOME, NULL) == EINVAL
    # nx * ny past INT_MAX: no limit per axis, but the positions must fit
    assert lib.pasnl_kblock_grid_count(L(100), SOME, SOME, 50000, 50000, D(10.0), SOME, SOME, NULL) == EUNSUPPORTED
    assert lib.pasnl_kblock_fill(L(100), SOME, SOME, L(-1), D(5.0), 50000, 50000, D(10.0), D(0.01), SOME, SOME, L(5), SOME, SOME,
                                 NULL) == EUNSUPPORTED
    assert lib.pasnl_kblock_grid_count(L(100), NULL, NULL, 83, 19, D(0.5), NULL, NULL, NULL) == ENULL  # 83 columns: only the NULLs
    # nfeat is 0 or 1; c <= 256
    gather = (SOME, SOME, L(5), SOME, SOME, L(100), SOME, SOME)
    assert lib.pasnl_kblock_gather(1, 8, *gather, 2, SOME, 20, SOME, 1, SOME, SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_gather(1, 8, *gather, -1, SOME, 20, SOME, 1, SOME, SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_gather(1, 8, *gather, 1, SOME, 257, SOME, 1, SOME, SOME, SOME, NULL) == EUNSUPPORTED
    assert lib.pasnl_kblock_gather(1, 0, *gather, 1, SOME, 20, SOME, 1, SOME, SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_gather(0, 8, *gather, 1, SOME, 20, SOME, 1, SOME, SOME, SOME, NULL) == OK  # no rows: a no-op
    assert lib.pasnl_kblock_rotate(1, 8, 2, SOME, SOME, SOME, NULL) == EINVAL
    assert lib.pasnl_kblock_rotate(0, 8, 3, NULL, NULL, NULL, NULL) == OK
    # NULL where a pointer is required (remission only with nfeat == 1)
    assert lib.pasnl_kblock_crop_stats(L(100), SOME, NULL, SOME, L(0), D(5.0), SOME, SOME, NULL) == ENULL
    assert lib.pasnl_kblock_crop_stats(L(100), SOME, SOME, SOME, L(0), D(5.0), SOME, NULL, NULL) == ENULL
    assert lib.pasnl_kblock_grid_count(L(100), SOME, SOME, 3, 3, D(10.0), NULL, SOME, NULL) == ENULL
    assert lib.pasnl_kblock_fill(L(100), SOME, SOME, L(-1), D(5.0), 3, 3, D(10.0), D(0.01), SOME, NULL, L(5), SOME, SOME, NULL) == ENULL
    assert lib.pasnl_kblock_fill(L(100), SOME, SOME, L(7), D(5.0), 1, 1, D(10.0), D(0.01), SOME, SOME, L(5), SOME, NULL, NULL) == ENULL
    assert lib.pasnl_kblock_gather(1, 8, SOME, SOME, L(5), SOME, SOME, L(100), SOME, NULL, 1, SOME, 20, SOME, 1, SOME, SOME, SOME,
                                   NULL) == ENULL
    assert lib.pasnl_kblock_gather(1, 8, SOME, NULL, L(5), SOME, SOME, L(100), SOME, NULL, 0, SOME, 20, SOME, 1, SOME, SOME, SOME,
                                   NULL) == ENULL
    assert lib.pasnl_kblock_gather(1, 8, SOME, SOME, L(5), SOME, SOME, L(100), SOME, NULL, 0, SOME, 20, NULL, 0, SOME, SOME, SOME,
                                   NULL) == ENULL
    assert lib.pasnl_kblock_rotate(1, 8, 3, SOME, NULL, SOME, NULL) == ENULL
