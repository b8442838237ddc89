"""CPU: the backward of the input-space non-local cell before any device is involved.  tests/nl_cell_input_grad_ref.py (the
formulas of include/pasnl.h in float64) equals torch's float64 autograd of the projected op-by-op chain, whose dbk vanishes;
the two entries pasnl_cls_nl_cell_input_grad / _workspace_bytes are declared, listed, exported and outside the scope of
tests/abi_cases.py; the header's validation order is answered on the host with null (or never dereferenced) pointers; the
workspace is the header's formula."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_cases
import nl_cell_input_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("pasnl_cls_nl_cell_input_grad_workspace_bytes", "pasnl_cls_nl_cell_input_grad")
OK, EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3, -5  # include/pasnl.h


@pytest.mark.parametrize("shape", R.SHAPES_FLOW)
def test_reference_equals_float64_autograd_of_the_chain(shape):
    h, g = R.problem(*shape)
    cb = shape[-1]
    out, chain = R.chain_autograd(h, g, torch.float64)
    want = R.backward(h, g)
    assert R.err(R.forward(h)[3], out) <= 1e-12
    for name in R.NAMES:
        assert want[name].shape == h[name].shape
        e = R.err(want[name], chain[name])
        print(f"{shape} {name}: {e:.3g}")
        assert e <= 1e-12, name
    # the chain's own dbk is rounding noise beside dbv: Q . bk is constant over the keys -- the kernel writes exact zeros
    assert np.abs(chain["bkv"][:cb]).max() <= 1e-12 * np.abs(chain["bkv"][cb:]).max()
    assert (want["bkv"][:cb] == 0).all()


def test_both_symbols_are_declared_listed_exported_and_out_of_abi_scope():
    from pointasnl_amd import _hip

    header = open(os.path.join(ROOT, "include", "pasnl.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pasnl_\w+)", nm))
    lib = _hip.lib()
    for name in SYMS:
        assert re.search(r"\b%s\s*\(" % name, decl), name
        assert name in _hip.SYMBOLS and name in exported and hasattr(lib, name)
        assert not abi_cases.in_scope(name)
    assert lib.pasnl_cls_nl_cell_input_grad_workspace_bytes.restype is ctypes.c_size_t


INPUTS = ("feature", "new_point", "wkv", "bkv", "wq", "bq", "g")
GRADS = ("gx", "gz", "gwkv", "gbkv", "gwq", "gbq")
A = {name: 4096 * (i + 1) for i, name in enumerate(INPUTS + GRADS + ("ws",))}  # 16-byte aligned, never touched


def grad(b, p, n, c, cz, cb, ws_bytes=0, **ptrs):
    from pointasnl_amd import _hip

    args = [ctypes.c_void_p(ptrs.get(k, 0)) for k in INPUTS + GRADS + ("ws",)]
    return _hip.lib().pasnl_cls_nl_cell_input_grad(b, p, n, c, cz, cb, *args, ctypes.c_size_t(ws_bytes), ctypes.c_void_p(0))


def formula(b, p, n, c, cz, cb):
    """the header's: 4 * ((2c + 2) b p + b ceil(p / 64) ((cz + 1) c + (c + 1) cb))"""
    return 4 * ((2 * c + 2) * b * p + b * ((p + 63) // 64) * ((cz + 1) * c + (c + 1) * cb))


def test_validation_happens_before_any_launch_and_in_the_headers_order():
    """pointers are null, or addresses that are never dereferenced: every call here is answered on the host"""
    S = (2, 5, 7, 3, 6, 32)
    need = formula(*S)
    # 1. dimensions, whatever the widths and the pointers
    for bad in [(-1, 5, 7, 3, 6, 32), (2, -1, 7, 3, 6, 32), (2, 5, 0, 3, 6, 32), (2, 5, 7, 0, 6, 32), (2, 5, 7, 3, 0, 32),
                (2, 5, 7, 3, 6, 0), (0, 5, 0, 3, 6, 32), (2, 5, -3, 9, 6, 48)]:
        assert grad(*bad) == EINVAL, bad
    # 2. unsupported widths, before the empty shapes and the pointers
    for bad in [(2, 5, 7, 9, 6, 32), (2, 5, 7, 3, 17, 32), (2, 5, 7, 3, 6, 16), (2, 5, 7, 3, 6, 48), (2, 5, 7, 3, 6, 256),
                (0, 5, 7, 9, 6, 32), (2, 0, 7, 3, 6, 96)]:
        assert grad(*bad) == EUNSUPPORTED, bad
    # 3. empty shapes succeed, with nothing given (zero-filling what is given: tests/test_gpu_nl_cell_input_grad.py)
    assert grad(0, 5, 7, 3, 6, 32) == OK and grad(2, 0, 7, 3, 6, 64) == OK and grad(0, 0, 7, 8, 16, 128) == OK
    # 4. null pointers: each input, grad_out, the workspace, and all six gradients at once
    assert grad(*S) == ENULL
    for missing in INPUTS + ("ws",):
        assert grad(*S, ws_bytes=need, **{k: v for k, v in A.items() if k != missing}) == ENULL, missing
    assert grad(*S, ws_bytes=need, **{k: v for k, v in A.items() if k not in GRADS}) == ENULL
    # 5. alignment (grad_out and the workspace: 16 bytes) and the batch limit, before the workspace size
    for name in ("g", "ws"):
        assert grad(*S, ws_bytes=0, **dict(A, **{name: A[name] + 4})) == EUNSUPPORTED, name
    assert grad(65536, 5, 7, 3, 6, 32, ws_bytes=0, **A) == EUNSUPPORTED
    # 6. a short workspace last -- whichever gradients are skipped
    assert grad(*S, ws_bytes=need - 1, **A) == EWORKSPACE
    assert grad(*S, ws_bytes=0, **A) == EWORKSPACE
    for only in GRADS:
        assert grad(*S, ws_bytes=need - 1, **{k: v for k, v in A.items() if k not in GRADS or k == only}) == EWORKSPACE, only
    big = (65535, 5, 7, 8, 16, 128)
    assert grad(*big, ws_bytes=formula(*big) - 1, **A) == EWORKSPACE


def test_workspace_is_the_headers_formula():
    from pointasnl_amd import _hip

    size = _hip.lib().pasnl_cls_nl_cell_input_grad_workspace_bytes
    for shape in [(1, 1, 1, 3, 6, 32), (2, 70, 45, 3, 6, 32), (2, 33, 77, 6, 9, 64), (1, 40, 200, 8, 16, 128),
                  (512, 1, 1100, 3, 6, 32), (64, 512, 1024, 3, 3, 32), (16, 1024, 8192, 6, 6, 32), (8, 1280, 10240, 3, 3, 32),
                  (65535, 8192, 1, 8, 16, 128)]:
        b, p, n, c, cz, cb = shape
        nbytes = int(size(*shape))
        assert nbytes == formula(*shape), shape
        assert nbytes == int(size(b, p, 1, c, cz, cb)) == int(size(b, p, 2 ** 30, c, cz, cb))  # no term in n
        # the per-query records and the per-workgroup partial moments: nothing proportional to p * n, n * cb or p * cb
        assert nbytes <= 4 * (2 * c + 2) * b * p + 4 * b * ((p + 63) // 64) * 25 * cb
    for shape in [(0, 5, 7, 3, 6, 32), (2, 0, 7, 3, 6, 32), (2, 5, 0, 3, 6, 32), (-1, 5, 7, 3, 6, 32), (2, 5, 7, 0, 6, 32),
                  (2, 5, 7, 9, 6, 32), (2, 5, 7, 3, 17, 32), (2, 5, 7, 3, 0, 32), (2, 5, 7, 3, 6, 48), (0, 0, 0, 3, 6, 64)]:
        assert int(size(*shape)) == 0, shape
