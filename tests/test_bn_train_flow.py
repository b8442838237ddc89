"""CPU: training-mode batch norm and dropout before any device is involved.  tests/bn_train_ref.py (the formulas of
include/pasnl.h in float64) equals torch's float64 autograd of the formula; every ReLU problem the GPU tests use keeps its margin;
the case list reaches every dispatch branch of csrc/bn_train.hip and every case is ragged against the widths it names; the five
new entries are declared, listed, exported and outside the scope of tests/abi_cases.py; the header's validation order is answered
on the host with null (or never dereferenced) pointers; the workspaces are the header's formula; the dropout mask keeps its share
and depends on its whole address; VariableStore.trainable() and the version-checked fold cache on a CPU store."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_cases
import bn_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pasnl_cls_bn_train_workspace_bytes", "pasnl_cls_bn_train", "pasnl_cls_bn_train_grad_workspace_bytes",
         "pasnl_cls_bn_train_grad", "pasnl_cls_dropout")
OK, EINVAL, ENULL, EWORKSPACE, EUNSUPPORTED = 0, -1, -2, -3, -5  # include/pasnl.h
TOL = 1e-12


@pytest.mark.parametrize("rows,c", [(1, 5), (2, 4), (37, 9), (300, 3)])
@pytest.mark.parametrize("act", [0, 1])
def test_reference_equals_float64_autograd(rows, c, act):
    x, gamma, beta, mm, mv, gy = R.problem(rows, c, act, seed=5)
    y, mean, var, rstd = R.forward(x, gamma, beta, act)
    t = R.chain(x, gamma, beta, act, gy, torch.float64)
    assert R.err(t["y"], y) <= TOL and R.err(t["rstd"], rstd) <= TOL and np.abs(t["mean"] - mean).max() <= TOL
    if rows == 1:
        assert (var == 0).all()
    got = R.backward(x, gamma, beta, act, gy)
    for name, g in zip(("grad_x", "grad_gamma", "grad_beta"), got):
        scale = max(np.abs(t[name]).max(), np.abs(gy).max())  # (rows == 1: grad_x is exactly 0)
        assert g.shape == t[name].shape and np.abs(g - t[name]).max() <= TOL * scale, name
    for unbiased in (False, True):
        batch = R.batch_variance(var, rows, unbiased)
        want = x.astype(np.float64).var(axis=0, ddof=1 if (unbiased and rows > 1) else 0)
        assert np.abs(batch - want).max() <= TOL
        for decay in (0.0, 0.5, 0.99):
            d = float(np.float32(decay))
            np.testing.assert_allclose(R.moving(mv, batch, decay), d * mv.astype(np.float64) + (1 - d) * batch, rtol=0, atol=1e-15)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_relu_case_keeps_its_margin(case):
    rows, c, act, offset, _ = case
    x, gamma, beta, mm, mv, gy = R.problem(rows, c, act, offset)
    assert x.shape == (rows, c) and x.dtype == np.float32 and gy.shape == (rows, c)
    if offset:
        assert np.abs(x.mean(axis=0) - 8).max() < 0.2 and (rows < 50 or np.abs(x.std(axis=0) - 0.25).max() < 0.08)
    if act:
        margin = R.relu_margin(x, gamma, beta)
        print(f"{R.case_id(case)}: margin {margin:.3g}")
        assert margin >= R.MARGIN


def plan(rows, c, vec):
    """csrc/bn_train.hip's bnt_plan, restated: (one launch?, lx, ly, channel tiles, slabs, rows per slab)"""
    vw = R.VW if vec else 1
    small = rows <= R.SMALL_ROWS
    lx = 1
    while lx < (R.SMALL_LX if small else R.MAX_LX) and lx * vw < c:
        lx *= 2
    ly = 256 // lx
    ctiles = -(-c // (lx * vw))
    slabs = max(1, min(R.slabs(rows, c), R.MAX_BLOCKS // ctiles))
    slab_rows = -(-(-(-rows // slabs)) // ly) * ly
    return small, lx, ly, ctiles, -(-rows // slab_rows), slab_rows


def test_the_case_list_reaches_every_branch_and_every_case_is_ragged():
    seen = set()
    for rows, c, act, offset, why in R.CASES:
        vec = c % R.VW == 0
        small, lx, ly, ctiles, slabs, slab_rows = plan(rows, c, vec)
        assert why and slabs <= R.slabs(rows, c) and (slabs - 1) * slab_rows < rows <= slabs * slab_rows
        # ragged: rows against the ly rows of a step (or at a seam of the row dispatch), or c against the channel tile
        assert rows % ly != 0 or c % (lx * (R.VW if vec else 1)) != 0 or rows in (R.SMALL_ROWS, R.SMALL_ROWS + 1), (rows, c)
        seen.add(("one launch" if small else "three launches", "vector" if vec else "scalar"))
        seen.update(k for k, v in {"channel tiles": ctiles > 1, "slabs": slabs > 1, "partials per CU at c = 4": c == 4 and slabs > R.CUS,
                                   "a wave of slabs": slabs > 64, "offset": offset, "relu": act == 1, "rows == 1": rows == 1,
                                   "seam": rows == R.SMALL_ROWS, "seam + 1": rows == R.SMALL_ROWS + 1}.items() if v)
    assert seen >= {("one launch", "vector"), ("one launch", "scalar"), ("three launches", "vector"), ("three launches", "scalar"),
                    "channel tiles", "slabs", "partials per CU at c = 4", "a wave of slabs", "offset", "relu", "rows == 1", "seam",
                    "seam + 1"}


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
        assert getattr(lib, name).argtypes is not None
    for name in NAMES:
        assert "utils/tf_util.py:512-531" in header and "utils/tf_util.py:594-615" in header


FWD_PTRS = ("x", "gamma", "beta", "mm", "mv", "y", "mean", "rstd", "ws")
BWD_PTRS = ("x", "y", "gamma", "mean", "rstd", "gy", "gx", "gg", "gb", "ws")
A = {name: 4096 * (i + 1) for i, name in enumerate(sorted(set(FWD_PTRS + BWD_PTRS)))}


def fwd(rows, c, eps=1e-3, decay=0.9, act=1, unbiased=1, ws_bytes=0, **p):
    from pointasnl_amd import _hip

    g = lambda n: p.get(n, 0)
    return _hip.lib().pasnl_cls_bn_train(rows, c, g("x"), g("gamma"), g("beta"), eps, decay, act, unbiased, g("mm"), g("mv"), g("y"),
                                         g("mean"), g("rstd"), g("ws"), ws_bytes, 0)


def bwd(rows, c, act=1, ws_bytes=0, **p):
    from pointasnl_amd import _hip

    g = lambda n: p.get(n, 0)
    return _hip.lib().pasnl_cls_bn_train_grad(rows, c, g("x"), g("y"), g("gamma"), g("mean"), g("rstd"), act, g("gy"), g("gx"),
                                              g("gg"), g("gb"), g("ws"), ws_bytes, 0)


def test_workspace_formula():
    from pointasnl_amd import _hip

    for size in (_hip.lib().pasnl_cls_bn_train_workspace_bytes, _hip.lib().pasnl_cls_bn_train_grad_workspace_bytes):
        assert size.restype is ctypes.c_size_t
        for rows, c in [(1, 1), (128, 512), (129, 4), (256, 4), (257, 4), (64 * 512 * 32, 32), (64 * 128 * 32, 128), (4099, 129),
                        (10 ** 6, 2048), (10 ** 6, 4), (3 * 10 ** 9, 257), (70001, 4)]:
            assert int(size(rows, c)) == R.workspace_bytes(rows, c), (rows, c)
        assert int(size(1 << 20, 4)) == 16 * 4 * 2048 and int(size(1 << 20, 2048)) == 16 * 2048 * 256
        for bad in [(0, 4), (-1, 4), (5, 0), (5, -3)]:
            assert int(size(*bad)) == 0


def test_validation_order_of_the_forward():
    """pointers are null, or addresses that are never dereferenced: every call here is answered on the host"""
    need = R.workspace_bytes(300, 8)
    for bad in [dict(rows=-1, c=8), dict(rows=300, c=0), dict(rows=300, c=8, act=2), dict(rows=300, c=8, act=-1),
                dict(rows=300, c=8, eps=0.0), dict(rows=300, c=8, decay=1.5), dict(rows=300, c=8, decay=-0.1), dict(rows=0, c=0)]:
        assert fwd(ws_bytes=need, **bad, **A) == EINVAL                      # dimensions and attributes first
    assert fwd(0, 8) == OK                                                   # then rows == 0: nothing read, nothing enqueued
    assert fwd(300, 8) == ENULL
    for missing in ("x", "gamma", "beta", "y", "mean", "rstd", "mm", "mv"):  # (one of the moving pair alone is a null pointer too)
        assert fwd(300, 8, ws_bytes=need, **{k: v for k, v in A.items() if k != missing}) == ENULL, missing
    assert fwd(300, 8, ws_bytes=need - 1, **dict(A, x=A["x"] + 2)) == EUNSUPPORTED   # alignment before the workspace's size
    assert fwd(300, 8, ws_bytes=need, **dict(A, ws=A["ws"] + 4)) == EUNSUPPORTED
    assert fwd((1 << 40) + 1, 8, ws_bytes=need, **A) == EUNSUPPORTED
    assert fwd(300, 8, ws_bytes=need, **dict(A, ws=0)) == EWORKSPACE
    assert fwd(300, 8, ws_bytes=need - 1, **A) == EWORKSPACE
    assert fwd(300, 8, ws_bytes=need - 1, **{k: v for k, v in A.items() if k not in ("mm", "mv")}) == EWORKSPACE  # both null is legal


def test_validation_order_of_the_backward():
    need = R.workspace_bytes(300, 8)
    for bad in [dict(rows=-1, c=8), dict(rows=300, c=0), dict(rows=300, c=8, act=2)]:
        assert bwd(ws_bytes=need, **bad, **A) == EINVAL
    assert bwd(0, 8) == OK
    assert bwd(300, 8) == ENULL
    for missing in ("x", "y", "gamma", "mean", "rstd", "gy", "gg", "gb"):
        assert bwd(300, 8, ws_bytes=need, **{k: v for k, v in A.items() if k != missing}) == ENULL, missing
    no_y = {k: v for k, v in A.items() if k != "y"}
    assert bwd(300, 8, act=0, ws_bytes=need - 1, **no_y) == EWORKSPACE         # y is not read without the mask
    assert bwd(300, 8, ws_bytes=need - 1, **{k: v for k, v in A.items() if k != "gx"}) == EWORKSPACE  # grad_x may be null
    assert bwd(300, 8, ws_bytes=need - 1, **dict(A, gy=A["gy"] + 1)) == EUNSUPPORTED
    assert bwd(300, 8, ws_bytes=need, **dict(A, ws=A["ws"] + 4)) == EUNSUPPORTED
    assert bwd(300, 8, ws_bytes=need, **dict(A, ws=0)) == EWORKSPACE
    assert bwd(300, 8, ws_bytes=need - 1, **A) == EWORKSPACE


def test_validation_order_of_dropout():
    from pointasnl_amd import _hip

    drop = _hip.lib().pasnl_cls_dropout
    for n, keep in [(-1, 0.5), (8, 0.0), (8, -0.5), (8, 1.5), (8, float("nan"))]:
        assert drop(n, keep, 1, 2, 3, 4096, 8192, 0) == EINVAL
    assert drop(0, 0.5, 1, 2, 3, 0, 0, 0) == OK
    assert drop(8, 0.5, 1, 2, 3, 0, 8192, 0) == ENULL and drop(8, 0.5, 1, 2, 3, 4096, 0, 0) == ENULL
    assert drop(8, 0.5, 1, 2, 3, 4098, 8192, 0) == EUNSUPPORTED and drop((1 << 40) + 1, 0.5, 1, 2, 3, 4096, 8192, 0) == EUNSUPPORTED


@pytest.mark.parametrize("p", [0.4, 0.5])
def test_dropout_reference_keeps_its_share(p):
    n = 2 ** 20
    keep = R.dropout_keep(n, p, seed=11, stream_id=0x9E3779B9, call=3)
    sigma = np.sqrt(p * (1 - p) / n)
    share = keep.mean()
    print(f"keep_prob {p}: share {share:.6f}, {abs(share - p) / sigma:.2f} sigma")
    assert abs(share - p) <= 5 * sigma


def test_dropout_mask_depends_on_its_whole_address():
    n = 4099
    base = R.dropout_keep(n, 0.5, 11, 7, 3)
    assert (base == R.dropout_keep(n, 0.5, 11, 7, 3)).all()
    for other in [(11, 7, 4), (11, 8, 3), (12, 7, 3), (11 + (1 << 32), 7, 3)]:
        assert (base != R.dropout_keep(n, 0.5, *other)).mean() > 0.4, other
    assert (base[:1000] == R.dropout_keep(1000, 0.5, 11, 7, 3)).all()  # element i does not depend on n
    x = np.arange(1, n + 1, dtype=np.float32)
    y = R.dropout(x, 0.4, 11, 7, 3)
    keep = R.dropout_keep(n, 0.4, 11, 7, 3)
    assert (y[~keep] == 0).all() and (y[keep] == x[keep] / np.float32(0.4)).all()


def cpu_store():
    from pointasnl_amd.utils import tf_util

    st = tf_util.set_store(tf_util.VariableStore(seed=4, device="cpu", randomize_bn=True))
    with st.scope("net"):
        with st.scope("a"):
            st.layer(6, 8, True)
        with st.scope("b"):
            st.layer(8, 3, False)
    return tf_util, st


def test_trainable_returns_the_four_kinds_and_never_a_moving_statistic():
    tf_util, st = cpu_store()
    tr = st.trainable()
    assert set(tr) == {"net/a/weights", "net/a/biases", "net/a/bn/gamma", "net/a/bn/beta", "net/b/weights", "net/b/biases"}
    assert all(t.requires_grad and t is st.vars[n] for n, t in tr.items())
    assert not st.vars["net/a/bn/moving_mean"].requires_grad and not st.vars["net/a/bn/moving_variance"].requires_grad
    assert not any(t.requires_grad for t in st.trainable(requires_grad=False).values())


@pytest.mark.parametrize("leaf", ["weights", "biases", "bn/gamma", "bn/beta", "bn/moving_mean", "bn/moving_variance"])
def test_layer_refolds_after_an_in_place_change(leaf):
    tf_util, st = cpu_store()

    def folded():
        v = {k.split("net/a/")[1]: t.double() for k, t in st.vars.items() if k.startswith("net/a/")}
        s = v["bn/gamma"] / torch.sqrt(v["bn/moving_variance"] + tf_util.BN_EPS)
        return v["weights"] * s, (v["biases"] - v["bn/moving_mean"]) * s + v["bn/beta"]

    with st.scope("net"), st.scope("a"):
        w0, b0 = st.layer(6, 8, True)
        assert st.layer(6, 8, True)[0] is w0                      # served from the cache while nothing changed
        with torch.no_grad():
            st.vars["net/a/" + leaf].mul_(1.5).add_(0.25)         # what an optimizer's step() or the moving update does
        w1, b1 = st.layer(6, 8, True)
    want_w, want_b = folded()
    assert (w1.double() - want_w).abs().max() < 1e-6 and (b1.double() - want_b).abs().max() < 1e-6
    assert (w1 - w0).abs().max() > 1e-3 or (b1 - b0).abs().max() > 1e-3


def test_derived_entries_follow_their_layer():
    """an entry built from layers inside its own miss (the cells' concatenated / padded weights) is refreshed with them, and one
    keyed by a folded tensor's pointer does not survive it"""
    tf_util, st = cpu_store()

    def derived():
        key = st.path("cat")
        if key not in st._folded:
            with st.scope("a"):
                w, b = st.layer(6, 8, True)
            st._folded[key] = (torch.cat([w, w], dim=1).contiguous(), b)
        return st._folded[key]

    with st.scope("net"):
        first = derived()
        assert derived()[0] is first[0]
        pkey = "@T%x" % first[0].data_ptr()
        assert pkey not in st._folded
        st._folded[pkey] = (first[0].t().contiguous(), first[0])
        with torch.no_grad():
            st.vars["net/a/bn/gamma"].add_(1.0)
        second = derived()
        assert second[0] is not first[0] and (second[0] - first[0]).abs().max() > 1e-3
        assert not dict.__contains__(st._folded, pkey)
        with st.scope("a"):
            assert (second[0][:, :8] == st.layer(6, 8, True)[0]).all()


def test_is_training_must_be_a_bool():
    from pointasnl_amd.utils import tf_util

    assert tf_util._training(None) is False and tf_util._training(False) is False and tf_util._training(True) is True
    with pytest.raises(TypeError):
        tf_util._training(torch.tensor(True))
    with pytest.raises(TypeError):
        tf_util._training("yes")
    assert tf_util._bn_unbiased(2) and tf_util._bn_unbiased(4) and not tf_util._bn_unbiased(3)
    assert tf_util._bn_decay_value(None) == 0.9 and tf_util._bn_decay_value(torch.tensor(0.5)) == 0.5
    assert tf_util._bn_decay_value(lambda: 0.75) == 0.75 and tf_util._bn_decay_value(0.99) == 0.99
