"""CPU: the backward of a set-abstraction layer's grouping and local cell before any device is involved.  tests/sa_grad_ref.py
(the formulas of include/pasnl.h in float64) equals torch's float64 autograd of the op-by-op chain; every problem the GPU tests
use keeps its ReLU margin and has no ambiguous maximum; the four new entries are declared, listed, exported and outside the scope
of tests/abi_cases.py; both header validation orders are answered on the host with null (or never dereferenced) pointers; both
workspaces are the header's formulas."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_cases
import sa_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pasnl_cls_sa_local_cell_grad_workspace_bytes", "pasnl_cls_sa_local_cell_grad", "pasnl_cls_sa_group_grad_workspace_bytes",
         "pasnl_cls_sa_group_grad")
OK, EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3, -5  # include/pasnl.h
TOL = 1e-12


@pytest.mark.parametrize("shape", R.CELL_FLOW)
def test_cell_reference_equals_float64_autograd(shape):
    x, p, gout = R.cell_problem(*shape)
    out, grads = R.cell_chain(x, p, gout, torch.float64)
    assert R.err(out, R.cell_forward(x, p)) <= TOL
    want = R.cell_backward(x, p, gout)
    assert set(want) == set(R.CELL_NAMES)
    for name in R.CELL_NAMES:
        assert want[name].shape == grads[name].shape and R.err(grads[name], want[name]) <= TOL, name


@pytest.mark.parametrize("shape", R.GROUP_SHAPES + ["tie"])
def test_group_reference_equals_float64_autograd(shape):
    prob = R.group_tie_problem() if shape == "tie" else R.group_problem(*shape)
    xyz, feature, idx, new_xyz, gnp, gskip = prob
    new_point, skip, grads = R.group_chain(*prob, torch.float64)
    fwd = R.group_forward(xyz.astype(np.float64), feature.astype(np.float64), idx, new_xyz.astype(np.float64))
    assert np.abs(new_point - fwd[0]).max() <= TOL and np.abs(skip - fwd[1]).max() <= TOL
    want = R.group_backward(*prob)
    for got, w_ in zip(grads, want):
        assert got.shape == w_.shape and R.err(got, w_) <= TOL
    # either gradient alone: the chain is linear in them
    only_np = R.group_backward(xyz, feature, idx, new_xyz, gnp, None)
    only_skip = R.group_backward(xyz, feature, idx, new_xyz, None, gskip)
    for a, b_, w_ in zip(only_np, only_skip, want):
        assert np.abs(a + b_ - w_).max() <= 1e-12 * max(1.0, np.abs(w_).max())


@pytest.mark.parametrize("shape", R.CELL_SHAPES + [R.CELL_WIDE])
def test_every_gpu_cell_problem_keeps_its_relu_margin(shape):
    x, p, gout = R.cell_problem(*shape)
    g, k, c, c1 = shape
    assert x.shape == (g, k, 6 + c) and gout.shape == (g, c1, 32) and x.dtype == np.float32
    margins = R.relu_margins(x, p)
    print(f"{shape}: margins {margins}")
    assert min(margins) >= R.MARGIN


@pytest.mark.parametrize("shape", R.GROUP_SHAPES)
def test_every_gpu_group_problem_has_no_ambiguous_maximum(shape):
    xyz, feature, idx, new_xyz, gnp, gskip = R.group_problem(*shape)
    b, n, c, m, k = shape
    assert R.ties_ok(xyz, feature, idx, new_xyz)
    assert (idx[:, 0, k - 1] == idx[:, 0, 0]).all() and not (idx == n - 1).any()  # a neighbour drawn twice; a point nobody drew
    want = R.group_backward(xyz, feature, idx, new_xyz, gnp, gskip)
    assert (want[0][:, n - 1] == 0).all() and (want[1][:, n - 1] == 0).all()


def test_the_tie_case_shares_equally():
    xyz, feature, idx, new_xyz, gnp, gskip = R.group_tie_problem()
    assert not R.ties_ok(xyz, feature, idx, new_xyz)
    assert (xyz[0, 3].view(np.uint32) == xyz[0, 7].view(np.uint32)).all()
    assert (feature[0, 3].view(np.uint32) == feature[0, 7].view(np.uint32)).all()
    gx, gf, gn = R.group_backward(xyz, feature, idx, new_xyz, None, gskip)
    half = gskip[0, 0].astype(np.float64) / 2
    np.testing.assert_allclose(gf[0, 3], half[6:], rtol=0, atol=1e-15)
    np.testing.assert_allclose(gf[0, 7], half[6:], rtol=0, atol=1e-15)
    np.testing.assert_allclose(gx[0, 3], half[0:3] + half[3:6], rtol=0, atol=1e-15)
    np.testing.assert_allclose(gn[0, 0], -2 * half[0:3], rtol=0, atol=1e-15)
    assert (np.delete(gf[0], (3, 7), axis=0) == 0).all()


def test_every_symbol_is_declared_listed_exported_and_out_of_abi_scope():
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


def P(*addresses):
    return [ctypes.c_void_p(a) for a in addresses]


NOSTREAM = ctypes.c_void_p(0)
CELL_PTRS = ("x", "w0", "b0", "w1", "b1", "ww", "bw", "grad_out", "gx", "gw0", "gb0", "gw1", "gb1", "gww", "gbw", "ws")
CELL_A = {name: 4096 * (i + 1) for i, name in enumerate(CELL_PTRS)}


def cell_grad(groups, k, w, c1, c2, ws_bytes=0, **ptrs):
    from pointasnl_amd import _hip

    return _hip.lib().pasnl_cls_sa_local_cell_grad(groups, k, w, c1, c2, *P(*(ptrs.get(n, 0) for n in CELL_PTRS)),
                                                   ctypes.c_size_t(ws_bytes), NOSTREAM)


def test_cell_validation_order_and_workspace_formula():
    """pointers are null, or addresses that are never dereferenced: every call here is answered on the host"""
    from pointasnl_amd import _hip

    size = _hip.lib().pasnl_cls_sa_local_cell_grad_workspace_bytes
    assert size.restype is ctypes.c_size_t
    for groups, w, c1 in [(1, 9, 32), (5, 9, 64), (1024, 9, 64), (1025, 9, 64), (64 * 512, 9, 64), (4102, 32, 64), (3, 70, 32)]:
        assert int(size(groups, w, c1, c1)) == 4 * min(groups, 1024) * (w * c1 + c1 + c1 * c1 + c1 + 96 + 32)
    for bad in [(0, 9, 64, 64), (-1, 9, 64, 64), (5, 2, 64, 64), (5, 9, 0, 64), (5, 9, 64, 0)]:
        assert int(size(*bad)) == 0
    need = int(size(5, 9, 64, 64))
    A = CELL_A
    for bad in [(-1, 32, 9, 64, 64), (5, 0, 9, 64, 64), (5, 32, 2, 64, 64), (5, 32, 9, 0, 64), (5, 32, 9, 64, 0),
                (5, 0, 9, 128, 128), (-1, 33, 9, 64, 64)]:                                   # dimensions first
        assert cell_grad(*bad, ws_bytes=need, **A) == EINVAL
    for bad in [(5, 32, 9, 128, 128), (5, 33, 9, 64, 64), (5, 32, 9, 32, 64), (5, 32, 9, 256, 256), (5, 32, 9, 16, 16),
                (5, 32, 97, 64, 64), (5, 32, 97, 32, 32), (0, 32, 9, 128, 128)]:              # then the supported set, before groups == 0
        assert cell_grad(*bad) == EUNSUPPORTED
    for good in [(5, 32, 96, 64, 64), (5, 64, 96, 32, 32), (5, 96, 3, 32, 32)]:               # the limits themselves pass that check
        assert cell_grad(*good) == ENULL
    assert cell_grad(0, 32, 9, 64, 64) == OK                                                 # nothing to zero-fill, nothing enqueued
    assert cell_grad(5, 32, 9, 64, 64) == ENULL
    for missing in CELL_PTRS[:8]:                                                             # null operands
        assert cell_grad(5, 32, 9, 64, 64, ws_bytes=need, **{k: v for k, v in A.items() if k != missing}) == ENULL
    assert cell_grad(5, 32, 9, 64, 64, ws_bytes=need, **{k: v for k, v in A.items() if not k.startswith("g") or k == "grad_out"}) == ENULL
    assert cell_grad(5, 32, 9, 64, 64, ws_bytes=need, **dict(A, ws=A["ws"] + 2)) == EUNSUPPORTED  # alignment before the size
    assert cell_grad(5, 32, 9, 64, 64, ws_bytes=need - 1, **dict(A, ws=A["ws"] + 2)) == EUNSUPPORTED
    assert cell_grad(5, 32, 9, 64, 64, ws_bytes=need, **dict(A, ws=0)) == EWORKSPACE
    assert cell_grad(5, 32, 9, 64, 64, ws_bytes=need - 1, **A) == EWORKSPACE
    only_bw = {k: v for k, v in A.items() if not k.startswith("g") or k in ("grad_out", "gbw")}
    assert cell_grad(5, 32, 9, 64, 64, ws_bytes=need - 1, **only_bw) == EWORKSPACE             # one weight gradient needs it all


GROUP_PTRS = ("xyz", "feature", "idx", "new_xyz", "gnp", "gskip", "gxyz", "gfeat", "gnew", "ws")
GROUP_A = {name: 4096 * (i + 1) for i, name in enumerate(GROUP_PTRS)}


def group_grad(b, n, c, m, k, ws_bytes=0, **ptrs):
    from pointasnl_amd import _hip

    return _hip.lib().pasnl_cls_sa_group_grad(b, n, c, m, k, *P(*(ptrs.get(name, 0) for name in GROUP_PTRS)),
                                              ctypes.c_size_t(ws_bytes), NOSTREAM)


def test_group_validation_order_and_workspace_formula():
    from pointasnl_amd import _hip

    size, lists = _hip.lib().pasnl_cls_sa_group_grad_workspace_bytes, _hip.lib().pasnl_grad_workspace_bytes
    assert size.restype is ctypes.c_size_t
    for b, n, c, m, k in [(2, 50, 3, 7, 32), (1, 64, 64, 1, 32), (64, 1024, 3, 512, 32), (3, 38400, 5, 0, 2)]:
        assert int(size(b, n, c, m, k)) == int(lists(b, n, ctypes.c_long(m * k))) + 4 * b * m * k * (3 + c)
    for bad in [(0, 50, 3, 7, 32), (2, 0, 3, 7, 32), (2, 50, 0, 7, 32), (2, 50, 3, -1, 32), (2, 50, 3, 7, 0)]:
        assert int(size(*bad)) == 0
    A = GROUP_A
    need = int(size(2, 50, 3, 7, 32))
    for bad in [(-1, 50, 3, 7, 32), (2, 0, 3, 7, 32), (2, 50, 0, 7, 32), (2, 50, 3, -1, 32), (2, 50, 3, 7, 0), (2, 38401, 3, 7, 0)]:
        assert group_grad(*bad, ws_bytes=need, **A) == EINVAL
    assert group_grad(2, 38401, 3, 7, 32) == EUNSUPPORTED and group_grad(0, 38401, 3, 7, 32) == EUNSUPPORTED
    assert group_grad(1, 50, 3, 1 << 27, 32) == EUNSUPPORTED
    assert group_grad(0, 50, 3, 7, 32) == OK
    assert group_grad(2, 50, 3, 7, 32) == ENULL
    for missing in ("xyz", "feature", "idx", "new_xyz"):
        assert group_grad(2, 50, 3, 7, 32, ws_bytes=need, **{k: v for k, v in A.items() if k != missing}) == ENULL
    assert group_grad(2, 50, 3, 7, 32, ws_bytes=need, **dict(A, gxyz=0, gfeat=0, gnew=0)) == ENULL
    assert group_grad(2, 50, 3, 7, 32, ws_bytes=need, **dict(A, ws=A["ws"] + 2)) == EUNSUPPORTED
    assert group_grad(2, 50, 3, 7, 32, ws_bytes=need, **dict(A, ws=0)) == EWORKSPACE
    assert group_grad(2, 50, 3, 7, 32, ws_bytes=need - 1, **A) == EWORKSPACE
    assert group_grad(2, 50, 3, 7, 32, ws_bytes=need - 1, **dict(A, gfeat=0, gnew=0)) == EWORKSPACE
