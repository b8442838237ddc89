"""The fused backward of a set-abstraction layer's grouping and local cell (csrc/sa_grad.hip; include/pasnl.h:
pasnl_cls_sa_local_cell_grad, pasnl_cls_sa_group_grad) through pointasnl_util's autograd functions, through the C ABI and through
PointASNLSetAbstraction.

Reference: tests/sa_grad_ref.py, the header's formulas in float64, on problems that keep a ReLU margin and have no ambiguous
maximum (tests/test_sa_grad_flow.py asserts both).  Measure: err(X) = max |X - X64| / max |X64| per gradient.  Yardstick: the
float32 op-by-op chain differentiated by torch on the CPU, against the same float64 -- computed here, never taken from the code
under test.  Allowed: err <= max(4 * err_chain, 1e-5), the rule of tests/test_gpu_nl_grad.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import as_grad_ref as A
import sa_grad_ref as R
from guarded import ALT_BYTE, ALT_WS_BYTE, NAN_BYTE, WS_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu

OK, EWORKSPACE, EUNSUPPORTED = 0, -3, -5


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else 0 if t is None else t.data_ptr())


def allowed(chain_err):
    return max(4 * chain_err, 1e-5)


def check(what, got, want, chain):
    e, ec = R.err(got, want), R.err(chain, want)
    print(f"{what}: err {e:.3g} (chain {ec:.3g})")
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), what
    assert e <= allowed(ec), what


@pytest.fixture(scope="module")
def U():
    from pointasnl_amd.utils import pointasnl_util

    return pointasnl_util


@pytest.fixture(scope="module")
def L():
    from pointasnl_amd import _hip

    return _hip


# ---------------------------------------------------------------------------------------------------------------------------
# local cell
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cell_case(shape):
    x, p, gout = R.cell_problem(*shape)
    want = R.cell_backward(x, p, gout)
    want_out = R.cell_forward(x, p)
    chain_out, chain = R.cell_chain(x, p, gout, torch.float32)
    for a in (x, gout) + tuple(p.values()):
        a.setflags(write=False)
    return x, p, gout, want, chain, want_out, chain_out


ALL7 = (True,) * 7


def cell_public(U, case, need=ALL7, gout=None):
    """-> (out (g,c2,32), {name: gradient or None}) through sa_local_cell_w, the groups as one cloud's points"""
    x, p, gout0 = case[:3]
    t = {"x": dev(x)[None]}
    t.update({k: dev(v) for k, v in p.items()})
    for name, n in zip(R.CELL_NAMES, need):
        t[name].requires_grad_(n)
    out = U.sa_local_cell_w(*[t[name] for name in R.CELL_NAMES])
    out.backward(dev(gout0 if gout is None else gout)[None])
    grads = {name: None if t[name].grad is None else t[name].grad.cpu().numpy() for name in R.CELL_NAMES}
    if grads["x"] is not None:
        grads["x"] = grads["x"][0]
    return out.detach().cpu().numpy()[0], grads


@pytest.mark.parametrize("shape", R.CELL_SHAPES)
def test_cell_parity(U, shape):
    case = cell_case(shape)
    x, p, gout, want, chain, want_out, chain_out = case
    out, grads = cell_public(U, case)
    check(f"sa_local_cell {shape} out", out, want_out, chain_out)
    for name in R.CELL_NAMES:
        check(f"sa_local_cell {shape} grad_{name}", grads[name], want[name], chain[name])
    zeros = cell_public(U, case, gout=np.zeros_like(gout))[1]
    for name in R.CELL_NAMES:
        assert (zeros[name] == 0).all(), name


SUBSETS = [tuple(i == j for i in range(7)) for j in range(7)] + [(False,) + (True,) * 6, (True, False, True, False, False, False, False)]


@pytest.mark.parametrize("shape", [R.CELL_SHAPES[1], R.CELL_SHAPES[5], R.CELL_SHAPES[4]])  # one launch, two, three
def test_cell_needs_input_grad_subsets_give_the_full_calls_bits(U, shape):
    case = cell_case(shape)
    full = cell_public(U, case)[1]
    for need in SUBSETS:
        part = cell_public(U, case, need)[1]
        for name, n in zip(R.CELL_NAMES, need):
            if n:
                np.testing.assert_array_equal(bits(part[name]), bits(full[name]), err_msg=f"{need} {name}")
            else:
                assert part[name] is None


def cell_abi(L, shape, dx, outs, ws, ws_bytes):
    g, k, c, c1 = shape
    st = L.lib().pasnl_cls_sa_local_cell_grad(g, k, 6 + c, c1, c1, *[ptr(t) for t in dx], *[ptr(o) for o in outs], ptr(ws),
                                              ctypes.c_size_t(ws_bytes), L.stream_ptr())
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("shape", [R.CELL_SHAPES[1], R.CELL_SHAPES[3], R.CELL_SHAPES[4], R.CELL_SHAPES[5]])
def test_cell_abi_guarded_exact_workspace_two_stale_fills(L, shape):
    g, k, c, c1 = shape
    w = 6 + c
    x, p, gout, want, chain = cell_case(shape)[:5]
    dx = [dev(x)] + [dev(p[n]) for n in R.CELL_NAMES[1:]] + [dev(gout)]
    nbytes = int(L.lib().pasnl_cls_sa_local_cell_grad_workspace_bytes(g, w, c1, c1))
    assert nbytes == 4 * min(g, R.SLOT_CAP) * (w * c1 + c1 + c1 * c1 + c1 + 96 + 32)
    shapes = [(g, k, w), (w, c1), (c1,), (c1, c1), (c1,), (3, 32), (32,)]
    runs = []
    for fill, ws_fill in ((NAN_BYTE, WS_BYTE), (ALT_BYTE, ALT_WS_BYTE)):
        make = lambda: [Guarded(4 * int(np.prod(s)), fill, output_guard(4 * s[-1])) for s in shapes]
        outs = make()
        ws = Guarded(nbytes, ws_fill)
        assert cell_abi(L, shape, dx, [o.ptr for o in outs], ws.ptr, nbytes - 1) == EWORKSPACE  # refused before any launch
        assert all(o.untouched() for o in outs) and ws.untouched()
        assert cell_abi(L, shape, dx, [o.ptr for o in outs], ws.ptr, nbytes) == OK
        assert all(o.guards_intact() for o in outs) and ws.guards_intact()
        runs.append([o.floats(s) for o, s in zip(outs, shapes)])
        assert all(np.isfinite(a).all() for a in runs[-1])  # every element written
        # grad_x alone: no partials, the workspace is not touched and may be NULL
        only = make()
        assert cell_abi(L, shape, dx, [only[0].ptr] + [None] * 6, None, 0) == OK
        assert only[0].guards_intact() and all(o.untouched() for o in only[1:])
        np.testing.assert_array_equal(bits(only[0].floats(shapes[0])), bits(runs[-1][0]))
        # one weight gradient alone: the others and grad_x stay untouched
        only = make()
        assert cell_abi(L, shape, dx, [None, None, None, only[3].ptr, None, None, None], ws.ptr, nbytes) == OK
        assert only[3].guards_intact() and all(o.untouched() for i, o in enumerate(only) if i != 3) and ws.guards_intact()
        np.testing.assert_array_equal(bits(only[3].floats(shapes[3])), bits(runs[-1][3]))
    for a, b_ in zip(*runs):  # two runs over different stale bytes: the same bits
        np.testing.assert_array_equal(bits(a), bits(b_))
    for name, got in zip(R.CELL_NAMES, runs[0]):
        check(f"abi sa_local_cell_grad {shape} grad_{name}", got, want[name], chain[name])


def test_cell_no_group_zero_fills_the_weight_gradients(L):
    shapes = [(9, 64), (64,), (64, 64), (64,), (3, 32), (32,)]
    outs = [Guarded(4 * int(np.prod(s)), NAN_BYTE, output_guard(4 * s[-1])) for s in shapes]
    st = L.lib().pasnl_cls_sa_local_cell_grad(0, 32, 9, 64, 64, *[ptr(None)] * 9, *[ptr(o.ptr) for o in outs], ptr(None),
                                              ctypes.c_size_t(0), L.stream_ptr())
    torch.cuda.synchronize()
    assert st == OK
    for o, s in zip(outs, shapes):
        assert o.guards_intact() and (bits(o.floats(s)) == 0).all()


def test_wider_cells_are_unsupported_and_still_differentiable(U, L):
    from pointasnl_amd.utils import tf_util

    shape = R.CELL_WIDE
    case = cell_case(shape)
    x, p, gout, want, chain, want_out, chain_out = case
    null = [ptr(None)] * 16
    assert L.lib().pasnl_cls_sa_local_cell_grad(2, 32, 9, 128, 128, *null, ctypes.c_size_t(0), L.stream_ptr()) == EUNSUPPORTED
    out, grads = cell_public(U, case)  # the op-by-op chain, differentiated by torch
    check(f"sa_local_cell {shape} out", out, want_out, chain_out)
    for name in R.CELL_NAMES:
        check(f"sa_local_cell {shape} grad_{name}", grads[name], want[name], chain[name])
    # and through sa_local_cell itself: the variables of a 128-channel layer receive gradients
    st = tf_util.set_store(tf_util.VariableStore(seed=3, randomize_bn=True))
    xd = dev(x)[None]
    with torch.no_grad():
        plain = U.sa_local_cell(xd, [128, 128, 256], False, None, None, True)
    for v in st.vars.values():
        v.requires_grad_()
    out = U.sa_local_cell(xd, [128, 128, 256], False, None, None, True)
    assert out.grad_fn is not None
    check("sa_local_cell 128 chain forward", out.detach().cpu().numpy(), plain.cpu().numpy().astype(np.float64), plain.cpu().numpy())
    out.backward(dev(gout)[None])
    trained = [n for n in st.vars if n.split("/")[-1] in ("weights", "biases", "gamma", "beta")]
    assert len(trained) == 12
    for name in trained:
        g_ = st.vars[name].grad
        assert g_ is not None and bool(torch.isfinite(g_).all()) and float(g_.abs().max()) > 0, name


# ---------------------------------------------------------------------------------------------------------------------------
# grouping
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_case(shape):
    prob = R.group_tie_problem() if shape == "tie" else R.group_problem(*shape)
    want = R.group_backward(*prob)
    chain = R.group_chain(*prob, torch.float32)[2]
    for a in prob:
        a.setflags(write=False)
    return prob, want, chain


def group_public(U, prob, need=(True, True, True), gnp="given", gskip="given"):
    """-> (new_point, skip, (grad_xyz, grad_feature, grad_new_xyz)); gnp / gskip = None: that output takes no part in the backward"""
    xyz, feature, idx, new_xyz, gnp0, gskip0 = prob
    xt, ft, nt = dev(xyz).requires_grad_(need[0]), dev(feature).requires_grad_(need[1]), dev(new_xyz).requires_grad_(need[2])
    new_point, skip = U.sa_group(xt, ft, dev(idx), nt)
    outs, gs = [], []
    for o, g_, g0 in ((new_point, gnp, gnp0), (skip, gskip, gskip0)):
        if g_ is not None:
            outs.append(o)
            gs.append(dev(g0 if isinstance(g_, str) else g_))
    torch.autograd.backward(outs, gs)
    return (new_point.detach().cpu().numpy(), skip.detach().cpu().numpy(),
            tuple(None if t.grad is None else t.grad.cpu().numpy() for t in (xt, ft, nt)))


GROUP_WHAT = ("grad_xyz", "grad_feature", "grad_new_xyz")


@pytest.mark.parametrize("shape", R.GROUP_SHAPES + ["tie"])
def test_group_parity(U, shape):
    prob, want, chain = group_case(shape)
    xyz, feature, idx, new_xyz, gnp, gskip = prob
    n = xyz.shape[1]
    new_point, skip, grads = group_public(U, prob)
    fwd = R.group_forward(xyz, feature, idx, new_xyz)  # float32 gathers, one subtraction, a maximum: the same bits
    np.testing.assert_array_equal(bits(new_point), bits(fwd[0]))
    np.testing.assert_array_equal(bits(skip), bits(fwd[1]))
    for what, got, w_, c_ in zip(GROUP_WHAT, grads, want, chain):
        check(f"sa_group {shape} {what}", got, w_, c_)
    if shape != "tie":  # a point no group drew: exact zeros
        assert not (idx == n - 1).any() and (bits(grads[0][:, n - 1]) == 0).all() and (bits(grads[1][:, n - 1]) == 0).all()
    zeros = group_public(U, prob, gnp=np.zeros_like(gnp), gskip=np.zeros_like(gskip))[2]
    assert all((z == 0).all() for z in zeros)
    # either output alone in the backward (the other gradient is NULL at the entry point)
    for kw, ref in ((dict(gskip=None), R.group_backward(xyz, feature, idx, new_xyz, gnp, None)),
                    (dict(gnp=None), R.group_backward(xyz, feature, idx, new_xyz, None, gskip))):
        part = group_public(U, prob, **kw)[2]
        for what, got, w_ in zip(GROUP_WHAT, part, ref):
            e = R.err(got, w_)
            print(f"sa_group {shape} without {'grad_skip' if 'gskip' in kw else 'grad_new_point'} {what}: err {e:.3g}")
            assert e <= 1e-5  # (sums of at most a few hundred float32 terms against float64)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False)):
        part = group_public(U, prob, need)[2]
        for i in range(3):
            if need[i]:
                np.testing.assert_array_equal(bits(part[i]), bits(grads[i]))
            else:
                assert part[i] is None


def test_group_tie_shares_equally(U):
    prob, want, chain = group_case("tie")
    xyz, feature, idx, new_xyz, gnp, gskip = prob
    gx, gf, gn = group_public(U, prob, gnp=None)[2]  # the skip maximum's gradient alone
    half = gskip[0, 0] / np.float32(2)
    np.testing.assert_array_equal(bits(gf[0, 3]), bits(half[6:]))
    np.testing.assert_array_equal(bits(gf[0, 7]), bits(half[6:]))
    np.testing.assert_array_equal(bits(gx[0, 3]), bits(half[0:3] + half[3:6]))
    np.testing.assert_array_equal(bits(gx[0, 7]), bits(half[0:3] + half[3:6]))
    assert (np.delete(gf[0], (3, 7), axis=0) == 0).all() and (np.delete(gx[0], (3, 7), axis=0) == 0).all()


@pytest.mark.parametrize("shape", R.GROUP_SHAPES[:2] + ["tie"])
def test_group_abi_guarded_exact_workspace_two_stale_fills(L, shape):
    prob, want, chain = group_case(shape)
    xyz, feature, idx, new_xyz, gnp, gskip = prob
    b, n, c = feature.shape
    _, m, k = idx.shape
    d = [dev(a) for a in prob]
    nbytes = int(L.lib().pasnl_cls_sa_group_grad_workspace_bytes(b, n, c, m, k))
    assert nbytes == int(L.lib().pasnl_grad_workspace_bytes(b, n, ctypes.c_long(m * k))) + 4 * b * m * k * (3 + c)
    shapes = [(b, n, 3), (b, n, c), (b, m, 3)]

    def call(outs, ws, ws_bytes):
        st = L.lib().pasnl_cls_sa_group_grad(b, n, c, m, k, *[ptr(t) for t in d], *[ptr(o) for o in outs], ptr(ws),
                                             ctypes.c_size_t(ws_bytes), L.stream_ptr())
        torch.cuda.synchronize()
        return st

    runs = []
    for fill, ws_fill in ((NAN_BYTE, WS_BYTE), (ALT_BYTE, ALT_WS_BYTE)):
        make = lambda: [Guarded(4 * int(np.prod(s)), fill, output_guard(4 * s[-1])) for s in shapes]
        outs = make()
        ws = Guarded(nbytes, ws_fill)
        assert call([o.ptr for o in outs], ws.ptr, nbytes - 1) == EWORKSPACE  # one byte short: refused before any launch
        assert all(o.untouched() for o in outs) and ws.untouched()
        assert call([o.ptr for o in outs], ws.ptr, nbytes) == OK
        assert all(o.guards_intact() for o in outs) and ws.guards_intact()
        runs.append([o.floats(s) for o, s in zip(outs, shapes)])
        assert all(np.isfinite(a).all() for a in runs[-1])  # every destination row written
        for keep in range(3):
            only = make()
            assert call([o.ptr if i == keep else None for i, o in enumerate(only)], ws.ptr, nbytes) == OK
            assert only[keep].guards_intact() and all(o.untouched() for i, o in enumerate(only) if i != keep) and ws.guards_intact()
            np.testing.assert_array_equal(bits(only[keep].floats(shapes[keep])), bits(runs[-1][keep]))
        only = make()  # grad_new_xyz alone needs no workspace
        assert call([None, None, only[2].ptr], None, 0) == OK
        np.testing.assert_array_equal(bits(only[2].floats(shapes[2])), bits(runs[-1][2]))
    for a, b_ in zip(*runs):  # two runs over different stale bytes: the same bits
        np.testing.assert_array_equal(bits(a), bits(b_))
    for what, got, w_, c_ in zip(GROUP_WHAT, runs[0], want, chain):
        check(f"abi sa_group_grad {shape} {what}", got, w_, c_)


# ---------------------------------------------------------------------------------------------------------------------------
# the forward is what it was
# ---------------------------------------------------------------------------------------------------------------------------
def same_forward(fn, direct, tensors):
    """fn(*tensors) without a gradient, under no_grad with leaves, and tracked: grad_fn only when tracked, always direct's bits"""
    want = [t.cpu().numpy() for t in direct]
    listed = lambda r: list(r) if isinstance(r, tuple) else [r]
    plain = listed(fn(*tensors))
    leaves = [t.clone().requires_grad_() if t.is_floating_point() else t for t in tensors]
    with torch.no_grad():
        quiet = listed(fn(*leaves))
    tracked = listed(fn(*leaves))
    for outs, has_fn in ((plain, False), (quiet, False), (tracked, True)):
        for o, w_ in zip(outs, want):
            assert (o.grad_fn is not None) == has_fn and o.requires_grad == has_fn
            np.testing.assert_array_equal(bits(o.detach().cpu().numpy()), bits(w_))


def test_forward_unchanged(U, L):
    lib, sp = L.lib(), L.stream_ptr
    b, n, c, m, k = R.GROUP_SHAPES[0]
    xyz, feature, idx, new_xyz = (dev(a) for a in group_case(R.GROUP_SHAPES[0])[0][:4])
    new_point, skip = torch.empty((b, m, k, 6 + c), device="cuda"), torch.empty((b, m, 6 + c), device="cuda")
    assert lib.pasnl_sa_group(b, n, c, m, k, ptr(xyz), ptr(feature), ptr(idx), ptr(new_xyz), ptr(new_point), ptr(skip), sp()) == OK
    same_forward(lambda a, f, z: U.sa_group(a, f, idx, z), [new_point, skip], [xyz, feature, new_xyz])

    shape = R.CELL_SHAPES[1]
    g, k, c, c1 = shape
    x, p = cell_case(shape)[:2]
    t = [dev(x)[None]] + [dev(p[name]) for name in R.CELL_NAMES[1:]]
    out = torch.empty((1, g, c1, 32), device="cuda")
    assert lib.pasnl_sa_local_cell(g, k, 6 + c, c1, c1, *[ptr(a) for a in t], ptr(out), sp()) == OK
    same_forward(U.sa_local_cell_w, [out], t)


# ---------------------------------------------------------------------------------------------------------------------------
# one whole layer: PointASNLSetAbstraction, BN folding differentiated by torch
# ---------------------------------------------------------------------------------------------------------------------------
LAYER = dict(b=2, n=256, npoint=64, nsample=32, mlp=[32, 32, 64], c=3, as_neighbor=8)
SCOPE = "sa"
LEAVES = ("weights", "biases", "bn/gamma", "bn/beta")


def layer_chain(vars_, xyz, feature, idx, g_xyz, g_out, dtype):
    """the layer op by op on the CPU from the store's own variables (BN folded as VariableStore.layer folds it), built from the
    reference functions; the neighbour lists are given -> (new_xyz, out, {name: gradient})"""
    from pointasnl_amd.utils import tf_util

    leaves = {}

    def fold(scope):
        v = {leaf: torch.from_numpy(vars_[f"{scope}/{leaf}"]).to(dtype) for leaf in LEAVES + ("bn/moving_mean", "bn/moving_variance")}
        for leaf in LEAVES:
            leaves[f"{scope}/{leaf}"] = v[leaf].requires_grad_()
        s = v["bn/gamma"] / torch.sqrt(v["bn/moving_variance"] + tf_util.BN_EPS)
        return v["weights"] * s, (v["biases"] - v["bn/moving_mean"]) * s + v["bn/beta"]

    S = SCOPE
    leaves["xyz"] = xt = torch.from_numpy(xyz).to(dtype).requires_grad_()
    leaves["feature"] = ft = torch.from_numpy(feature).to(dtype).requires_grad_()
    new_xyz, new_feature = A.cell_tensors(xt, ft, idx, LAYER["as_neighbor"], {conv: fold(f"{S}/{S}/{S}/{conv}") for conv in A.CELL_LAYERS})
    new_point, skip = R.group_tensors(xt, ft, idx, new_xyz)
    b, p, k, w = new_point.shape
    (w0, b0), (w1, b1), (ww, bw) = fold(f"{S}/conv0"), fold(f"{S}/conv1"), fold(f"{S}/weight_net/wconv0")
    cell = R.cell_tensors(new_point.reshape(b * p, k, w), dict(w0=w0, b0=b0, w1=w1, b1=b1, ww=ww, bw=bw)).reshape(b, p, -1)
    (wkv, bkv), (wq, bq), (wb, bb) = fold(f"{S}/{S}/conv_kv"), fold(f"{S}/{S}/conv_query"), fold(f"{S}/{S}/conv_back_project")
    cb = wq.shape[1]
    kv, q = ft @ wkv + bkv, new_feature @ wq + bq
    att = torch.softmax(q @ kv[..., :cb].transpose(1, 2) / (float(cb) ** 0.5), dim=-1) @ kv[..., cb:]
    (ws, bs), (wa, ba), (wg, bg) = fold(f"{S}/skip"), fold(f"{S}/after_conv"), fold(f"{S}/aggregation")
    tail = torch.relu(cell @ wa + ba) + torch.relu(skip @ ws + bs) + torch.relu(att @ wb + bb)
    out = torch.relu(tail @ wg + bg)
    torch.autograd.backward([new_xyz, out], [torch.from_numpy(g_xyz).to(dtype), torch.from_numpy(g_out).to(dtype)])
    return new_xyz.detach().numpy(), out.detach().numpy(), {k_: v.grad.numpy() for k_, v in leaves.items()}


def test_the_whole_layer(U, L, monkeypatch):
    from pointasnl_amd.utils import tf_util

    b, n, c = LAYER["b"], LAYER["n"], LAYER["c"]
    npoint, nsample, mlp = LAYER["npoint"], LAYER["nsample"], LAYER["mlp"]
    rng = np.random.default_rng(11)
    xyz = rng.standard_normal((b, n, 3)).astype(np.float32)
    feature = rng.standard_normal((b, n, c)).astype(np.float32)
    g_xyz = rng.standard_normal((b, npoint, 3)).astype(np.float32)
    g_out = rng.standard_normal((b, npoint, mlp[-1])).astype(np.float32)
    st = tf_util.set_store(tf_util.VariableStore(seed=5, randomize_bn=True))
    xd, fd = dev(xyz), dev(feature)
    with torch.no_grad():
        search = tuple(None if t is None else t.clone() for t in U.sa_search(xd, fd, npoint, nsample))
    idx = search[2].cpu().numpy()

    def layer():
        return U.PointASNLSetAbstraction(xd, fd, npoint, nsample, mlp, False, None, None, SCOPE, bn=True,
                                         as_neighbor=LAYER["as_neighbor"], NL=True, search=search)

    seen = []
    real = L.launch
    monkeypatch.setattr(L, "launch", lambda symbol, *a: (seen.append(symbol), real(symbol, *a))[1])
    with torch.no_grad():  # the first call creates the variables; without a gradient: the fused cell, as before
        layer()
        del seen[:]
        inf_xyz, inf_out = layer()
    assert inf_out.grad_fn is None and "pasnl_sa_cell" in "".join(seen) and "pasnl_sa_group" not in seen
    before = list(seen)
    del seen[:]
    plain_xyz, plain_out = layer()  # gradients enabled, nothing requires one: the same dispatch, the same bits
    assert plain_out.grad_fn is None and seen == before
    np.testing.assert_array_equal(bits(plain_out.cpu().numpy()), bits(inf_out.cpu().numpy()))

    names = [name for name in st.vars if name.split("/")[-1] in ("weights", "biases", "gamma", "beta")]
    assert len(names) == 4 * 13  # 4 AdaptiveSampling layers, conv0, conv1, wconv0, 3 non-local, skip, after_conv, aggregation
    for name in names:
        st.vars[name].requires_grad_()
    st._folded.clear()
    xd.requires_grad_(), fd.requires_grad_()
    del seen[:]
    new_xyz, out = layer()
    assert out.grad_fn is not None and new_xyz.grad_fn is not None
    assert "pasnl_sa_group" in seen and "pasnl_sa_local_cell" in seen
    assert not any(s.startswith(("pasnl_sa_cell", "pasnl_sa_tail", "pasnl_take_neighbor0")) for s in seen)
    for conv in ("conv0", "conv1", "weight_net/wconv0"):  # no graph-carrying fold stays behind
        assert f"{SCOPE}/{conv}/" not in st._folded
    del seen[:]
    torch.autograd.backward([new_xyz, out], [dev(g_xyz), dev(g_out)])
    assert "pasnl_cls_sa_group_grad" in seen and "pasnl_cls_sa_local_cell_grad" in seen

    vars_ = {k_: v.detach().cpu().numpy() for k_, v in st.vars.items()}
    want = layer_chain(vars_, xyz, feature, idx, g_xyz, g_out, torch.float64)
    chain = layer_chain(vars_, xyz, feature, idx, g_xyz, g_out, torch.float32)
    # (mlp2_1's biases and beta: the softmax over the neighbours ignores a per-column shift, so their float64 gradient is rounding
    # noise of 1e-17 and `err` compares two noises -- measured 5.05e8 against the chain's 1.59e9, as in tests/test_gpu_as_grad.py)
    check("layer new_xyz", new_xyz.detach().cpu().numpy(), want[0], chain[0])
    check("layer out", out.detach().cpu().numpy(), want[1], chain[1])
    assert set(want[2]) == set(names) | {"xyz", "feature"}
    for name in names:
        assert st.vars[name].grad is not None, name
        check(f"layer {name}", st.vars[name].grad.cpu().numpy(), want[2][name], chain[2][name])
    check("layer xyz", xd.grad.cpu().numpy(), want[2]["xyz"], chain[2]["xyz"])
    check("layer feature", fd.grad.cpu().numpy(), want[2]["feature"], chain[2]["feature"])

    # requires_grad off again: the inference dispatch and its bits are back
    for name in names:
        st.vars[name].requires_grad_(False)
        st.vars[name].grad = None
    st._folded.clear()
    xd.requires_grad_(False), fd.requires_grad_(False)
    del seen[:]
    again_xyz, again_out = layer()
    assert again_out.grad_fn is None and seen == before
    np.testing.assert_array_equal(bits(again_out.cpu().numpy()), bits(inf_out.cpu().numpy()))
    np.testing.assert_array_equal(bits(again_xyz.cpu().numpy()), bits(inf_xyz.cpu().numpy()))


def test_layer_without_adaptive_sampling_takes_its_centres_by_group_point(U, L, monkeypatch):
    """as_neighbor == 0: the differentiable route gathers neighbour 0 with group_point, not with pasnl_take_neighbor0 or the
    centre-producing fused cell; the centres are the inference route's bits and the gradients reach xyz and the variables"""
    from pointasnl_amd.utils import tf_util

    b, n, c, npoint, nsample, mlp = 2, 256, 3, 64, 32, [32, 32, 64]
    rng = np.random.default_rng(12)
    xd, fd = dev(rng.standard_normal((b, n, 3)).astype(np.float32)), dev(rng.standard_normal((b, n, c)).astype(np.float32))
    st = tf_util.set_store(tf_util.VariableStore(seed=6, randomize_bn=True))
    with torch.no_grad():
        search = tuple(None if t is None else t.clone() for t in U.sa_search(xd, fd, npoint, nsample))
    layer = lambda: U.PointASNLSetAbstraction(xd, fd, npoint, nsample, mlp, False, None, None, SCOPE, bn=True, as_neighbor=0,
                                              NL=True, search=search)
    with torch.no_grad():
        inf_xyz, inf_out = layer()
    for v in st.vars.values():
        v.requires_grad_()
    st._folded.clear()
    xd.requires_grad_()
    seen = []
    real = L.launch
    monkeypatch.setattr(L, "launch", lambda symbol, *a: (seen.append(symbol), real(symbol, *a))[1])
    new_xyz, out = layer()
    assert out.grad_fn is not None and new_xyz.grad_fn is not None
    assert "pasnl_sa_group" in seen and "pasnl_sa_local_cell" in seen
    assert not any(s.startswith(("pasnl_sa_cell", "pasnl_sa_tail", "pasnl_take_neighbor0")) for s in seen)
    np.testing.assert_array_equal(bits(new_xyz.detach().cpu().numpy()), bits(inf_xyz.cpu().numpy()))
    # the same layer through other kernels and vendor GEMMs: float32 rounding apart (1e-5 per cell, include/pasnl.h)
    assert R.err(out.detach().cpu().numpy(), inf_out.cpu().numpy().astype(np.float64)) <= 1e-4
    torch.autograd.backward([new_xyz, out], [torch.ones_like(new_xyz), torch.ones_like(out)])
    assert xd.grad is not None and bool(torch.isfinite(xd.grad).all()) and float(xd.grad.abs().max()) > 0
    for name, v in st.vars.items():
        if name.split("/")[-1] in ("weights", "biases", "gamma", "beta"):
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()), name
