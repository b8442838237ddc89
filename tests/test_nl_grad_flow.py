"""CPU: the backward of the non-local attention core before any device is involved.  tests/nl_grad_ref.py (the six formulas of
include/pasnl.h in float64) equals torch's float64 autograd of the op-by-op chain; the two entries pasnl_cls_nl_attention_grad /
_workspace_bytes are declared, listed, exported and outside the scope of tests/abi_cases.py; the header's validation order is
answered on the host with null (or never dereferenced) pointers; the workspace is the rows' statistics and nothing more."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_cases
import nl_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pasnl_cls_nl_attention_grad_workspace_bytes", "pasnl_cls_nl_attention_grad")
OK, EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3, -5  # include/pasnl.h


@pytest.mark.parametrize("shape", R.SHAPES_FLOW)
def test_reference_equals_float64_autograd_of_the_chain(shape):
    q, kv, g = R.problem(*shape)
    out, dq, dkv = R.chain_autograd(q, kv, g, torch.float64)
    _, o = R.forward(q, kv)
    want_q, want_kv = R.backward(q, kv, g)
    assert want_q.shape == q.shape and want_kv.shape == kv.shape
    for got, want in ((out, o), (dq, want_q), (dkv, want_kv)):
        assert np.abs(got - want).max() <= 1e-12


def test_both_symbols_are_declared_listed_exported_and_out_of_abi_scope():
    from pointasnl_amd import _hip

    header = open(os.path.join(ROOT, "include", "pasnl.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (pasnl_\w+)", nm))
    lib = _hip.lib()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, decl), name
        assert name in _hip.SYMBOLS and name in exported and hasattr(lib, name)
        assert not abi_cases.in_scope(name)
    assert "pasnl_cls_" in abi_cases.EXCLUDED_PREFIXES and "tests/abi_cases.py" in header  # the header says why the prefix


def grad(b, p, n, cb, q=0, kv=0, out=0, g=0, gq=0, gkv=0, ws=0, ws_bytes=0):
    from pointasnl_amd import _hip

    ptrs = [ctypes.c_void_p(x) for x in (q, kv, out, g, gq, gkv, ws)]
    return _hip.lib().pasnl_cls_nl_attention_grad(b, p, n, cb, *ptrs, ctypes.c_size_t(ws_bytes), ctypes.c_void_p(0))


def test_validation_happens_before_any_launch_and_in_the_headers_order():
    """pointers are null, or addresses that are never dereferenced: every call here is answered on the host"""
    A = dict(q=4096, kv=8192, out=12288, g=16384, gq=20480, gkv=24576, ws=28672)  # 16-byte aligned, never touched
    need = 8 * 2 * 5
    # dimensions first, whatever the pointers and cb
    assert grad(-1, 5, 7, 32) == EINVAL and grad(2, -1, 7, 32) == EINVAL
    assert grad(2, 5, 0, 32) == EINVAL and grad(2, 5, -3, 48) == EINVAL and grad(0, 5, 0, 32) == EINVAL
    # then cb, before the empty shapes and the pointers
    for cb in (16, 48, 96, 256):
        assert grad(2, 5, 7, cb) == EUNSUPPORTED and grad(0, 5, 7, cb) == EUNSUPPORTED
    # empty shapes: success with nothing to do (p == 0 with grad_kv given zero-fills it: tests/test_gpu_nl_grad.py)
    assert grad(0, 5, 7, 32) == OK and grad(2, 0, 7, 64) == OK and grad(0, 0, 7, 128) == OK
    # null pointers: each required operand, the workspace, and both gradients at once
    assert grad(2, 5, 7, 32) == ENULL
    for missing in ("q", "kv", "out", "g", "ws"):
        assert grad(2, 5, 7, 32, ws_bytes=need, **{k: v for k, v in A.items() if k != missing}) == ENULL, missing
    assert grad(2, 5, 7, 32, ws_bytes=need, **{k: v for k, v in A.items() if k not in ("gq", "gkv")}) == ENULL
    # alignment and the batch limit, before the workspace size
    for name in A:
        assert grad(2, 5, 7, 32, ws_bytes=0, **dict(A, **{name: A[name] + 4})) == EUNSUPPORTED, name
    assert grad(65536, 5, 7, 32, ws_bytes=0, **A) == EUNSUPPORTED
    # a short workspace last -- with either gradient skipped too
    assert grad(2, 5, 7, 32, ws_bytes=need - 1, **A) == EWORKSPACE
    assert grad(2, 5, 7, 32, ws_bytes=0, **dict(A, gq=0)) == EWORKSPACE
    assert grad(2, 5, 7, 32, ws_bytes=need - 1, **dict(A, gkv=0)) == EWORKSPACE
    assert grad(65535, 5, 7, 128, ws_bytes=8 * 65535 * 5 - 1, **A) == EWORKSPACE


def test_workspace_is_the_row_statistics_only():
    from pointasnl_amd import _hip

    size = _hip.lib().pasnl_cls_nl_attention_grad_workspace_bytes
    assert size.restype is ctypes.c_size_t
    for b, p, n, cb in [(1, 1, 1, 64), (2, 45, 77, 32), (2, 40, 80, 128), (64, 512, 1024, 32), (16, 1024, 8192, 32),
                        (8, 40, 80, 128), (65535, 8192, 1, 32)]:
        nbytes = int(size(b, p, n, cb))
        assert 0 < nbytes <= 8 * b * p + 256, (b, p, n, cb, nbytes)
        assert nbytes >= 8 * b * p  # lse2[b,p] and delta[b,p] do have to fit
    for b, p, n, cb in [(0, 5, 7, 32), (2, 0, 7, 32), (2, 5, 0, 32), (-1, 5, 7, 32), (0, 0, 0, 64)]:
        assert int(size(b, p, n, cb)) == 0
