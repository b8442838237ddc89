"""CPU: the backward of the AdaptiveSampling cell's fused parts before any device is involved.  tests/as_grad_ref.py (the
formulas of include/pasnl.h in float64) equals torch's float64 autograd of the op-by-op chain; the six new entries are declared,
listed, exported and outside the scope of tests/abi_cases.py; each header validation order is answered on the host with null (or
never dereferenced) pointers; the gather's workspace is the header's formula."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_cases
import as_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pasnl_cls_as_attention_grad", "pasnl_cls_as_attention_qkv_grad", "pasnl_cls_as_reweight_grad",
         "pasnl_cls_as_reweight_x_grad", "pasnl_cls_as_gather_grad_workspace_bytes", "pasnl_cls_as_gather_grad")
OK, EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3, -5  # include/pasnl.h
TOL = 1e-12


@pytest.mark.parametrize("shape", R.SHAPES_FLOW)
def test_attention_reference_equals_float64_autograd(shape):
    q, kv, g = R.attention_problem(*shape)
    out, dq, dkv = R.attention_chain(q, kv, g, torch.float64)
    want_q, want_kv = R.attention_backward(q, kv, g)
    assert want_q.shape == q.shape and want_kv.shape == kv.shape
    for got, want in ((out, R.attention_forward(q, kv)), (dq, want_q), (dkv, want_kv)):
        assert np.abs(got - want).max() <= TOL
    if shape[1] == 1:  # the softmax is the constant 1: no gradient reaches the scores
        assert np.abs(want_q).max() <= 1e-15 and np.abs(want_kv[..., :shape[2]]).max() <= 1e-15


@pytest.mark.parametrize("shape", R.SHAPES_FLOW)
def test_reweight_reference_equals_float64_autograd(shape):
    g, as_, cb = shape
    ch, nsample = cb, as_ + 3
    h = R.reweight_problem(g, as_, nsample, ch)
    chain = R.reweight_chain(dtype=torch.float64, **h)
    nx, nf = R.reweight_forward(h["logits"], h["X"], h["F"])
    dl, dx, df = R.reweight_backward(**h)
    for got, want in ((chain["new_xyz"], nx), (chain["new_feature"], nf), (chain["logits"], dl), (chain["X"], dx), (chain["F"], df)):
        assert got.shape == want.shape and np.abs(got - want).max() <= TOL
    assert (dx[:, as_:] == 0).all() and (df[:, as_:] == 0).all()
    # the x form: one tensor serves as coordinates and as features
    x = np.concatenate([h["X"][:, :as_], h["X"][:, :as_], h["F"][:, :as_, : ch]], axis=-1)  # (g, as, 3 + (3 + ch))
    rng = np.random.default_rng(3)
    logits = rng.standard_normal((g, as_, 1 + 3 + ch)).astype(np.float32)
    gfeat = rng.standard_normal((g, 3 + ch)).astype(np.float32)
    chain = R.reweight_x_chain(logits, x, h["gxyz"], gfeat, torch.float64)
    dl, gx = R.reweight_x_backward(logits, x, h["gxyz"], gfeat)
    assert np.abs(chain["logits"] - dl).max() <= TOL and np.abs(chain["x"] - gx).max() <= TOL
    assert (gx[:, :, :3] == 0).all()


def test_gather_reference_equals_float64_autograd():
    b, n, c, m, k, as_ = R.GATHER_FLOW
    xyz, feature, idx, gx = R.gather_problem(*R.GATHER_FLOW)
    assert (idx[:, 0, as_ - 1] == idx[:, 0, 0]).all() and (idx[:, :, 1] == 1).all() and not (idx[:, :, :as_] == n - 1).any()
    x, dxyz, dfeat = R.gather_chain(xyz, feature, idx, gx, torch.float64)
    want_xyz, want_feat = R.gather_backward(gx, idx, n)
    assert np.abs(x - R.gather_forward(xyz.astype(np.float64), feature.astype(np.float64), idx, as_)).max() <= TOL
    assert np.abs(dxyz - want_xyz).max() <= TOL and np.abs(dfeat - want_feat).max() <= TOL
    assert (want_xyz[:, n - 1] == 0).all() and (want_feat[:, n - 1] == 0).all()


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


def test_attention_validation_order():
    """pointers are null, or addresses that are never dereferenced: every call here is answered on the host"""
    from pointasnl_amd import _hip

    f, fq = _hip.lib().pasnl_cls_as_attention_grad, _hip.lib().pasnl_cls_as_attention_qkv_grad
    A = (4096, 8192, 12288, 16384, 20480)  # q, kv, grad_out, grad_q, grad_kv
    for bad in ((-1, 12, 32), (5, 0, 32), (5, 12, 0), (5, -1, 300), (0, 17, 0)):  # dimensions first
        assert f(*bad, *P(*A), NOSTREAM) == EINVAL and fq(*bad, *P(*A[:3]), NOSTREAM) == EINVAL
    for bad in ((5, 17, 32), (5, 12, 257), (0, 17, 32)):                            # then the limits, before g == 0
        assert f(*bad, *P(0, 0, 0, 0, 0), NOSTREAM) == EUNSUPPORTED and fq(*bad, *P(0, 0, 0), NOSTREAM) == EUNSUPPORTED
    assert f(0, 12, 32, *P(0, 0, 0, 0, 0), NOSTREAM) == OK and fq(0, 16, 256, *P(0, 0, 0), NOSTREAM) == OK
    for missing in range(3):                                                       # null operands
        assert f(5, 12, 32, *P(*(0 if i == missing else a for i, a in enumerate(A))), NOSTREAM) == ENULL
        assert fq(5, 12, 32, *P(*(0 if i == missing else a for i, a in enumerate(A[:3]))), NOSTREAM) == ENULL
    assert f(5, 12, 32, *P(A[0], A[1], A[2], 0, 0), NOSTREAM) == ENULL             # both gradients NULL


def test_reweight_validation_order():
    from pointasnl_amd import _hip

    f, fx = _hip.lib().pasnl_cls_as_reweight_grad, _hip.lib().pasnl_cls_as_reweight_x_grad
    A = tuple(4096 * (i + 1) for i in range(8))  # logits, X, F, gxyz, gfeat, grad_logits, grad_X, grad_F
    AX = tuple(4096 * (i + 1) for i in range(6))  # logits, x, gxyz, gfeat, grad_logits, grad_x
    for bad in ((-1, 12, 32, 6), (5, 0, 32, 6), (5, 12, 11, 6), (5, 12, 32, 0), (5, 17, 16, 6)):
        assert f(*bad, *P(*A), NOSTREAM) == EINVAL
    for bad in ((-1, 12, 6), (5, 0, 6), (5, 12, 3), (5, 17, 0)):
        assert fx(*bad, *P(*AX), NOSTREAM) == EINVAL
    assert f(5, 17, 32, 6, *P(*[0] * 8), NOSTREAM) == EUNSUPPORTED and f(0, 17, 32, 6, *P(*[0] * 8), NOSTREAM) == EUNSUPPORTED
    assert fx(5, 17, 6, *P(*[0] * 6), NOSTREAM) == EUNSUPPORTED and fx(0, 17, 6, *P(*[0] * 6), NOSTREAM) == EUNSUPPORTED
    assert f(0, 12, 32, 6, *P(*[0] * 8), NOSTREAM) == OK and fx(0, 12, 6, *P(*[0] * 6), NOSTREAM) == OK
    for missing in (0, 3, 4):
        assert f(5, 12, 32, 6, *P(*(0 if i == missing else a for i, a in enumerate(A))), NOSTREAM) == ENULL
    for missing in (1, 2):  # the grouped tensors are needed for grad_logits
        assert f(5, 12, 32, 6, *P(*(0 if i == missing else a for i, a in enumerate(A))), NOSTREAM) == ENULL
    assert f(5, 12, 32, 6, *P(*A[:5], 0, 0, 0), NOSTREAM) == ENULL
    for missing in (0, 1, 2, 3):
        assert fx(5, 12, 6, *P(*(0 if i == missing else a for i, a in enumerate(AX))), NOSTREAM) == ENULL
    assert fx(5, 12, 6, *P(*AX[:4], 0, 0), NOSTREAM) == ENULL


def gather_grad(b, n, c, m, k, as_, gx=0, idx=0, gxyz=0, gfeat=0, ws=0, ws_bytes=0):
    from pointasnl_amd import _hip

    return _hip.lib().pasnl_cls_as_gather_grad(b, n, c, m, k, as_, *P(gx, idx, gxyz, gfeat, ws), ctypes.c_size_t(ws_bytes), NOSTREAM)


def test_gather_validation_order_and_workspace_formula():
    from pointasnl_amd import _hip

    size, lists = _hip.lib().pasnl_cls_as_gather_grad_workspace_bytes, _hip.lib().pasnl_grad_workspace_bytes
    assert size.restype is ctypes.c_size_t
    for b, n, c, m, as_ in [(2, 50, 3, 7, 12), (1, 1, 64, 1, 1), (64, 1024, 3, 512, 12), (16, 1024, 64, 256, 4), (3, 38400, 5, 0, 2)]:
        assert int(size(b, n, c, m, as_)) == int(lists(b, n, ctypes.c_long(m * as_))) + 4 * b * m * as_ * (1 + 3 + c)
        assert int(size(b, n, c, m, as_)) == 4 * (b * (n + 1) + b * m * as_) + 4 * b * m * as_ * (4 + c)
    for bad in [(0, 50, 3, 7, 12), (2, 0, 3, 7, 12), (2, 50, 0, 7, 12), (2, 50, 3, -1, 12), (2, 50, 3, 7, 0)]:
        assert int(size(*bad)) == 0
    A = dict(gx=4096, idx=8192, gxyz=12288, gfeat=16384, ws=20480)
    need = int(size(2, 50, 3, 7, 12))
    for bad in [(-1, 50, 3, 7, 20, 12), (2, 0, 3, 7, 20, 12), (2, 50, 0, 7, 20, 12), (2, 50, 3, -1, 20, 12), (2, 50, 3, 7, 0, 12),
                (2, 50, 3, 7, 20, 0), (2, 50, 3, 7, 11, 12), (2, 38401, 3, 7, 11, 12)]:
        assert gather_grad(*bad, ws_bytes=need, **A) == EINVAL
    assert gather_grad(2, 38401, 3, 7, 20, 12) == EUNSUPPORTED and gather_grad(0, 38401, 3, 7, 20, 12) == EUNSUPPORTED
    assert gather_grad(1, 50, 3, 1 << 28, 20, 12) == EUNSUPPORTED
    assert gather_grad(0, 50, 3, 7, 20, 12) == OK
    assert gather_grad(2, 50, 3, 7, 20, 12) == ENULL
    for missing in ("gx", "idx"):
        assert gather_grad(2, 50, 3, 7, 20, 12, ws_bytes=need, **{k: v for k, v in A.items() if k != missing}) == ENULL
    assert gather_grad(2, 50, 3, 7, 20, 12, ws_bytes=need, **dict(A, gxyz=0, gfeat=0)) == ENULL
    assert gather_grad(2, 50, 3, 7, 20, 12, ws_bytes=need, **dict(A, ws=0)) == EWORKSPACE
    assert gather_grad(2, 50, 3, 7, 20, 12, ws_bytes=need - 1, **A) == EWORKSPACE
    assert gather_grad(2, 50, 3, 7, 20, 12, ws_bytes=need - 1, **dict(A, gfeat=0)) == EWORKSPACE
    assert gather_grad(2, 50, 3, 7, 20, 12, ws_bytes=need, **dict(A, ws=A["ws"] + 2)) == EUNSUPPORTED
