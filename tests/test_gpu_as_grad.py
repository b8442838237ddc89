"""The fused backward of the AdaptiveSampling cell (csrc/as_grad.hip, on csrc/as_core.hpp with the forward in csrc/as_cell.hip;
include/pasnl.h: pasnl_cls_as_attention_grad / _qkv_grad, pasnl_cls_as_reweight_grad / _x_grad, pasnl_cls_as_gather_grad) through pointasnl_util's autograd functions, through the C ABI
and through adaptive_sampling_fused.

Reference: tests/as_grad_ref.py, the header's formulas in float64.  Measure: err(X) = max |X - X64| / max |X64| per gradient.
Yardstick: the float32 op-by-op chain (bmm, softmax, bmm, softmax(dim=2), sums) differentiated by torch on the CPU, against the
same float64 -- computed here, never taken from the code under test.  Allowed: err <= max(4 * err_chain, 1e-5), the rule of
tests/test_gpu_nl_grad.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import as_grad_ref as R
from guarded import ALT_BYTE, ALT_WS_BYTE, NAN_BYTE, WS_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu

OK, EWORKSPACE = 0, -3
GROUPS = (1, 5, 1030)  # a workgroup with idle waves; more than one workgroup (four groups each)


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
# micro attention
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def att_case(g, as_, cb):
    q, kv, go = R.attention_problem(g, as_, cb)
    want = R.attention_backward(q, kv, go)
    _, cq, ckv = R.attention_chain(q, kv, go, torch.float32)
    for a in (q, kv, go) + tuple(want):
        a.setflags(write=False)
    return q, kv, go, want, (cq, ckv)


def att_public(U, q, kv, go, need=(True, True)):
    qt, kvt = dev(q).requires_grad_(need[0]), dev(kv).requires_grad_(need[1])
    out = U.as_attention(qt, kvt)
    out.backward(dev(go))
    return tuple(None if t.grad is None else t.grad.cpu().numpy() for t in (qt, kvt))


def att_public_qkv(U, q, kv, go):
    cb = q.shape[-1]
    t = dev(R.pack_kvq(q, kv)).requires_grad_()
    U.as_attention_qkv(t, cb).backward(dev(go))
    g = t.grad.cpu().numpy()
    return np.ascontiguousarray(g[..., 2 * cb:]), np.ascontiguousarray(g[..., :2 * cb])


@pytest.mark.parametrize("cb", [32, 33, 64, 65])
@pytest.mark.parametrize("as_", [1, 4, 8, 12, 16])
def test_attention_parity_both_forms(U, as_, cb):
    for g in GROUPS:
        q, kv, go, want, chain = att_case(g, as_, cb)
        for form, run in (("q,kv", att_public), ("kvq", att_public_qkv)):
            gq, gkv = run(U, q, kv, go)
            check(f"as_attention[{form}] g={g} as={as_} cb={cb} grad_q", gq, want[0], chain[0])
            check(f"as_attention[{form}] g={g} as={as_} cb={cb} grad_kv", gkv, want[1], chain[1])
            if as_ == 1:  # the softmax is the constant 1
                assert (bits(gq) == 0).all() and (bits(gkv[..., :cb]) == 0).all()
                np.testing.assert_array_equal(gkv[..., cb:], go)  # dV = g


def test_attention_zero_grad_out_gives_exact_zeros(U):
    q, kv, go = att_case(5, 12, 33)[:3]
    for run in (att_public, att_public_qkv):
        gq, gkv = run(U, q, kv, np.zeros_like(go))
        assert (gq == 0).all() and (gkv == 0).all()


@pytest.mark.parametrize("need", [(True, False), (False, True)], ids=["q", "kv"])
def test_attention_needs_input_grad(U, need):
    q, kv, go = att_case(5, 12, 65)[:3]
    full, part = att_public(U, q, kv, go), att_public(U, q, kv, go, need)
    for i in range(2):
        if need[i]:
            np.testing.assert_array_equal(bits(part[i]), bits(full[i]))
        else:
            assert part[i] is None
    fq, fkv = att_public_qkv(U, q, kv, go)  # the packed form: the same kernel on other strides
    np.testing.assert_array_equal(bits(fq), bits(full[0]))
    np.testing.assert_array_equal(bits(fkv), bits(full[1]))


@pytest.mark.parametrize("shape", [(5, 12, 33), (1030, 16, 65), (3, 1, 32)])
def test_attention_abi_guarded_and_null_outputs(L, shape):
    g, as_, cb = shape
    q, kv, go, want, chain = att_case(*shape)
    qd, kvd, gd, kvqd = dev(q), dev(kv), dev(go), dev(R.pack_kvq(q, kv))
    runs = []
    for fill in (NAN_BYTE, ALT_BYTE):
        gq = Guarded(4 * q.size, fill, output_guard(4 * cb))
        gkv = Guarded(4 * kv.size, fill, output_guard(8 * cb))
        gkvq = Guarded(4 * 3 * q.size, fill, output_guard(12 * cb))
        assert L.lib().pasnl_cls_as_attention_grad(g, as_, cb, ptr(qd), ptr(kvd), ptr(gd), ptr(gq.ptr), ptr(gkv.ptr), L.stream_ptr()) == OK
        assert L.lib().pasnl_cls_as_attention_qkv_grad(g, as_, cb, ptr(kvqd), ptr(gd), ptr(gkvq.ptr), L.stream_ptr()) == OK
        torch.cuda.synchronize()
        assert gq.guards_intact() and gkv.guards_intact() and gkvq.guards_intact()
        runs.append((gq.floats(q.shape), gkv.floats(kv.shape), gkvq.floats(q.shape[:2] + (3 * cb,))))
        assert all(np.isfinite(a).all() for a in runs[-1])  # every element written
        # a NULL output leaves the other one as it is, bit for bit, and its own buffer untouched
        for skip in (0, 1):
            outs = [Guarded(4 * q.size, fill, output_guard(4 * cb)), Guarded(4 * kv.size, fill, output_guard(8 * cb))]
            ptrs = [None if i == skip else outs[i].ptr for i in range(2)]
            assert L.lib().pasnl_cls_as_attention_grad(g, as_, cb, ptr(qd), ptr(kvd), ptr(gd), ptr(ptrs[0]), ptr(ptrs[1]), L.stream_ptr()) == OK
            torch.cuda.synchronize()
            assert outs[skip].untouched() and outs[1 - skip].guards_intact()
            kept = outs[1 - skip].floats((q, kv)[1 - skip].shape)
            np.testing.assert_array_equal(bits(kept), bits(runs[-1][1 - skip]))
    for a, b in zip(*runs):  # a pure function of the inputs, whatever the outputs held
        np.testing.assert_array_equal(bits(a), bits(b))
    np.testing.assert_array_equal(bits(runs[0][2][..., 2 * cb:]), bits(runs[0][0]))
    np.testing.assert_array_equal(bits(runs[0][2][..., :2 * cb]), bits(runs[0][1]))
    check(f"abi as_attention_grad {shape} grad_q", runs[0][0], want[0], chain[0])
    check(f"abi as_attention_grad {shape} grad_kv", runs[0][1], want[1], chain[1])


# ---------------------------------------------------------------------------------------------------------------------------
# re-weighting tail
# ---------------------------------------------------------------------------------------------------------------------------
RW_G, RW_NSAMPLE = 70, 32  # 70 (1 + ch) threads: more than one workgroup at every width


@functools.lru_cache(maxsize=None)
def rw_case(as_, ch):
    h = R.reweight_problem(RW_G, as_, RW_NSAMPLE, ch)
    want = R.reweight_backward(**h)
    chain = R.reweight_chain(dtype=torch.float32, **h)
    # the x form on rows [centred | X | F[:, :, 3:]]: ch channels = the coordinates and ch - 3 more
    x = np.ascontiguousarray(np.concatenate([h["X"][:, :as_] - h["X"][:, :1], h["X"][:, :as_], h["F"][:, :as_, 3:]], axis=-1))
    want_x = R.reweight_x_backward(h["logits"], x, h["gxyz"], h["gfeat"])
    chain_x = R.reweight_x_chain(h["logits"], x, h["gxyz"], h["gfeat"], torch.float32)
    for a in tuple(h.values()) + (x,):
        a.setflags(write=False)
    return h, want, chain, x, want_x, chain_x


def rw_public(U, h, as_, need=(True, True, True), gxyz=None, gfeat=None):
    t = [dev(h[k])[None].requires_grad_(n) for k, n in zip(("logits", "X", "F"), need)]
    nx, nf = U.as_reweight(t[0], t[1], t[2], as_)
    torch.autograd.backward([nx, nf], [dev(h["gxyz"] if gxyz is None else gxyz)[None], dev(h["gfeat"] if gfeat is None else gfeat)[None]])
    return tuple(None if v.grad is None else v.grad[0].cpu().numpy() for v in t)


def rw_public_x(U, h, x, need=(True, True), gxyz=None, gfeat=None):
    t = [dev(h["logits"])[None].requires_grad_(need[0]), dev(x)[None].requires_grad_(need[1])]
    nx, nf = U.as_reweight_x(t[0], t[1])
    torch.autograd.backward([nx, nf], [dev(h["gxyz"] if gxyz is None else gxyz)[None], dev(h["gfeat"] if gfeat is None else gfeat)[None]])
    return tuple(None if v.grad is None else v.grad[0].cpu().numpy() for v in t)


@pytest.mark.parametrize("ch", [4, 6, 67, 131])
@pytest.mark.parametrize("as_", [1, 4, 12, 16])
def test_reweight_parity_both_forms(U, as_, ch):
    h, want, chain, x, want_x, chain_x = rw_case(as_, ch)
    got = rw_public(U, h, as_)
    for name, a, w_, key in zip(("grad_logits", "grad_xyz", "grad_feature"), got, want, ("logits", "X", "F")):
        check(f"as_reweight as={as_} ch={ch} {name}", a, w_, chain[key])
    assert (bits(got[1][:, as_:]) == 0).all() and (bits(got[2][:, as_:]) == 0).all()  # rows past `as`: exact zeros
    gl, gx = rw_public_x(U, h, x)
    check(f"as_reweight_x as={as_} ch={ch} grad_logits", gl, want_x[0], chain_x["logits"])
    check(f"as_reweight_x as={as_} ch={ch} grad_x", gx, want_x[1], chain_x["x"])
    assert (bits(gx[:, :, :3]) == 0).all()
    if as_ == 1:  # the softmax is the constant 1
        assert (bits(got[0]) == 0).all() and (bits(gl) == 0).all()


def test_reweight_zero_grad_out_gives_exact_zeros(U):
    h, _, _, x, _, _ = rw_case(12, 67)
    z3, zf = np.zeros_like(h["gxyz"]), np.zeros_like(h["gfeat"])
    for a in rw_public(U, h, 12, gxyz=z3, gfeat=zf) + rw_public_x(U, h, x, gxyz=z3, gfeat=zf):
        assert (a == 0).all()


def test_reweight_needs_input_grad(U):
    h, _, _, x, _, _ = rw_case(12, 6)
    full, full_x = rw_public(U, h, 12), rw_public_x(U, h, x)
    for need in [(True, False, False), (False, True, False), (False, False, True), (False, True, True)]:
        part = rw_public(U, h, 12, need)
        for i in range(3):
            if need[i]:
                np.testing.assert_array_equal(bits(part[i]), bits(full[i]))
            else:
                assert part[i] is None
    for need in [(True, False), (False, True)]:
        part = rw_public_x(U, h, x, need)
        for i in range(2):
            if need[i]:
                np.testing.assert_array_equal(bits(part[i]), bits(full_x[i]))
            else:
                assert part[i] is None


@pytest.mark.parametrize("as_,ch", [(12, 6), (16, 131), (1, 4)])
def test_reweight_abi_guarded_and_null_outputs(L, as_, ch):
    h, want, chain, x, want_x, chain_x = rw_case(as_, ch)
    d = {k: dev(v) for k, v in h.items()}
    xd = dev(x)
    g, w = RW_G, 1 + ch
    sizes = (h["logits"].shape, h["X"].shape, h["F"].shape)
    sizes_x = (h["logits"].shape, x.shape)

    def call(ptrs):
        st = L.lib().pasnl_cls_as_reweight_grad(g, as_, RW_NSAMPLE, ch, ptr(d["logits"]), ptr(d["X"]), ptr(d["F"]), ptr(d["gxyz"]),
                                                ptr(d["gfeat"]), *(ptr(p) for p in ptrs), L.stream_ptr())
        torch.cuda.synchronize()
        return st

    def call_x(ptrs):
        st = L.lib().pasnl_cls_as_reweight_x_grad(g, as_, ch, ptr(d["logits"]), ptr(xd), ptr(d["gxyz"]), ptr(d["gfeat"]),
                                                  *(ptr(p) for p in ptrs), L.stream_ptr())
        torch.cuda.synchronize()
        return st

    for fn, shapes in ((call, sizes), (call_x, sizes_x)):
        runs = []
        for fill in (NAN_BYTE, ALT_BYTE):
            make = lambda: [Guarded(4 * int(np.prod(s)), fill, output_guard(4 * s[-1])) for s in shapes]
            outs = make()
            assert fn([o.ptr for o in outs]) == OK
            assert all(o.guards_intact() for o in outs)
            runs.append([o.floats(s) for o, s in zip(outs, shapes)])
            assert all(np.isfinite(a).all() for a in runs[-1])  # every element written
            for skip in range(len(shapes)):
                outs = make()
                assert fn([None if i == skip else o.ptr for i, o in enumerate(outs)]) == OK
                for i, (o, s) in enumerate(zip(outs, shapes)):
                    if i == skip:
                        assert o.untouched()
                    else:
                        assert o.guards_intact()
                        np.testing.assert_array_equal(bits(o.floats(s)), bits(runs[-1][i]))
        for a, b in zip(*runs):
            np.testing.assert_array_equal(bits(a), bits(b))
    check(f"abi as_reweight_x_grad as={as_} ch={ch} grad_x", runs[0][1], want_x[1], chain_x["x"])


# ---------------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------------
GATHER_SHAPES = [(2, 50, 3, 7, 20, 12), (2, 50, 64, 7, 20, 12), (2, 1, 3, 5, 20, 12), (1, 300, 64, 40, 20, 12)]


@functools.lru_cache(maxsize=None)
def gather_case(shape):
    xyz, feature, idx, gx = R.gather_problem(*shape)
    want = R.gather_backward(gx, idx, shape[1])
    chain = R.gather_chain(xyz, feature, idx, gx, torch.float32)[1:]
    for a in (xyz, feature, idx, gx):
        a.setflags(write=False)
    return xyz, feature, idx, gx, want, chain


def gather_public(U, c, as_, need=(True, True), gx=None):
    xyz, feature, idx, gx0 = c[:4]
    xt, ft = dev(xyz).requires_grad_(need[0]), dev(feature).requires_grad_(need[1])
    x = U.as_gather(xt, ft, dev(idx), as_)
    x.backward(dev(gx0 if gx is None else gx))
    return x.detach().cpu().numpy(), tuple(None if t.grad is None else t.grad.cpu().numpy() for t in (xt, ft))


@pytest.mark.parametrize("shape", GATHER_SHAPES)
def test_gather_parity(U, shape):
    b, n, c, m, k, as_ = shape
    case = gather_case(shape)
    xyz, feature, idx, gx, want, chain = case
    if n > 2:  # what the problem promises: a repeated neighbour 0, a point every group draws, a point none draws
        assert (idx[:, 0, as_ - 1] == idx[:, 0, 0]).all() and (idx[:, :, 1] == 1).all() and not (idx[:, :, :as_] == n - 1).any()
    x, (gxyz, gfeat) = gather_public(U, case, as_)
    np.testing.assert_array_equal(x, R.gather_forward(xyz, feature, idx, as_))  # the forward: float32 gathers and one subtraction
    check(f"as_gather {shape} grad_xyz", gxyz, want[0], chain[0])
    check(f"as_gather {shape} grad_feature", gfeat, want[1], chain[1])
    if n > 2:
        assert (bits(gxyz[:, n - 1]) == 0).all() and (bits(gfeat[:, n - 1]) == 0).all()  # drawn by no group: exact zeros
    zx, zf = gather_public(U, case, as_, gx=np.zeros_like(gx))[1]
    assert (zx == 0).all() and (zf == 0).all()
    for need in ((True, False), (False, True)):
        part = gather_public(U, case, as_, need)[1]
        for i in range(2):
            if need[i]:
                np.testing.assert_array_equal(bits(part[i]), bits((gxyz, gfeat)[i]))
            else:
                assert part[i] is None


@pytest.mark.parametrize("shape", GATHER_SHAPES[:3])
def test_gather_abi_guarded_exact_workspace_two_stale_fills(L, shape):
    b, n, c, m, k, as_ = shape
    xyz, feature, idx, gx, want, chain = gather_case(shape)
    gxd, idxd = dev(gx), dev(idx)
    nbytes = int(L.lib().pasnl_cls_as_gather_grad_workspace_bytes(b, n, c, m, as_))
    assert nbytes > 0

    def call(pxyz, pfeat, ws, ws_bytes):
        st = L.lib().pasnl_cls_as_gather_grad(b, n, c, m, k, as_, ptr(gxd), ptr(idxd), ptr(pxyz), ptr(pfeat), ptr(ws),
                                              ctypes.c_size_t(ws_bytes), L.stream_ptr())
        torch.cuda.synchronize()
        return st

    runs = []
    for fill, ws_fill in ((NAN_BYTE, WS_BYTE), (ALT_BYTE, ALT_WS_BYTE)):
        make = lambda: (Guarded(4 * b * n * 3, fill, output_guard(12)), Guarded(4 * b * n * c, fill, output_guard(4 * c)))
        ox, of = make()
        ws = Guarded(nbytes, ws_fill)
        assert call(ox.ptr, of.ptr, ws.ptr, nbytes - 1) == EWORKSPACE  # one byte short: refused before any launch
        assert ox.untouched() and of.untouched() and ws.untouched()
        assert call(ox.ptr, of.ptr, ws.ptr, nbytes) == OK
        assert ox.guards_intact() and of.guards_intact() and ws.guards_intact()
        runs.append((ox.floats((b, n, 3)), of.floats((b, n, c))))
        assert all(np.isfinite(a).all() for a in runs[-1])  # every destination row written
        for skip in (0, 1):
            outs = make()
            assert call(*(None if i == skip else o.ptr for i, o in enumerate(outs)), ws.ptr, nbytes) == OK
            assert outs[skip].untouched() and outs[1 - skip].guards_intact() and ws.guards_intact()
            np.testing.assert_array_equal(bits(outs[1 - skip].floats(runs[-1][1 - skip].shape)), bits(runs[-1][1 - skip]))
    for a, b_ in zip(*runs):  # two runs over different stale bytes: the same bits
        np.testing.assert_array_equal(bits(a), bits(b_))
    check(f"abi as_gather_grad {shape} grad_xyz", runs[0][0], want[0], chain[0])
    check(f"abi as_gather_grad {shape} grad_feature", runs[0][1], want[1], chain[1])


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
    g, as_, cb = 5, 12, 33
    q, kv, _ = R.attention_problem(g, as_, cb)
    qd, kvd, kvqd = dev(q), dev(kv), dev(R.pack_kvq(q, kv))
    out = torch.empty_like(qd)
    assert lib.pasnl_as_attention(g, as_, cb, ptr(qd), ptr(kvd), ptr(out), sp()) == OK
    same_forward(U.as_attention, [out], [qd, kvd])
    out2 = torch.empty_like(qd)
    assert lib.pasnl_as_attention_qkv(g, as_, cb, ptr(kvqd), ptr(out2), sp()) == OK
    same_forward(lambda t: U.as_attention_qkv(t, cb), [out2], [kvqd])

    h, _, _, x, _, _ = rw_case(12, 6)
    d = {k: dev(v) for k, v in h.items()}
    nx, nf = torch.empty((RW_G, 3), device="cuda"), torch.empty((RW_G, 6), device="cuda")
    assert lib.pasnl_as_reweight(RW_G, 12, RW_NSAMPLE, 6, ptr(d["logits"]), ptr(d["X"]), ptr(d["F"]), ptr(nx), ptr(nf), sp()) == OK
    same_forward(lambda a, b_, c: U.as_reweight(a, b_, c, 12), [nx[None], nf[None]], [d["logits"][None], d["X"][None], d["F"][None]])
    xd = dev(x)
    nx2, nf2 = torch.empty((RW_G, 3), device="cuda"), torch.empty((RW_G, 6), device="cuda")
    assert lib.pasnl_as_reweight_x(RW_G, 12, 6, ptr(d["logits"]), ptr(xd), ptr(nx2), ptr(nf2), sp()) == OK
    same_forward(U.as_reweight_x, [nx2[None], nf2[None]], [d["logits"][None], xd[None]])

    b, n, c, m, k, as_ = GATHER_SHAPES[1]
    xyz, feature, idx = (dev(a) for a in gather_case(GATHER_SHAPES[1])[:3])
    xo = torch.empty((b, m, as_, 6 + c), device="cuda")
    assert lib.pasnl_as_gather(b, n, c, m, k, as_, ptr(xyz), ptr(feature), ptr(idx), ptr(xo), sp()) == OK
    same_forward(lambda a, f: U.as_gather(a, f, idx, as_), [xo], [xyz, feature])


# ---------------------------------------------------------------------------------------------------------------------------
# the whole cell: adaptive_sampling_fused, BN folding differentiated by torch
# ---------------------------------------------------------------------------------------------------------------------------
CELL_SHAPES = [(2, 64, 3, 16, 16, 12), (2, 64, 64, 8, 16, 4)]  # (b, n, c, p, k, as)
CELL_KERNEL = {3: "pasnl_as_cell_narrow", 64: "pasnl_as_cell_wide_ld"}
LEAVES = ("weights", "biases", "bn/gamma", "bn/beta")
SCOPE = "as"


def cell_inputs(shape):
    b, n, c, p, k, as_ = shape
    rng = np.random.default_rng(100 + c)
    xyz = rng.standard_normal((b, n, 3)).astype(np.float32)
    feature = rng.standard_normal((b, n, c)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, p, k)).astype(np.int32)
    idx[:, 0, as_ - 1] = idx[:, 0, 0]
    gxyz = rng.standard_normal((b, p, 3)).astype(np.float32)
    gfeat = rng.standard_normal((b, p, 3 + c)).astype(np.float32)
    return xyz, feature, idx, gxyz, gfeat


def cell_chain(vars_, xyz, feature, idx, as_, gxyz, gfeat, dtype):
    """the op-by-op cell on the CPU from the store's own variables, BN folded as VariableStore.layer folds it
    -> (new_xyz, new_feature, {name: gradient})"""
    from pointasnl_amd.utils import tf_util

    leaves, layers = {}, {}
    for conv in R.CELL_LAYERS:
        pre = f"{SCOPE}/{SCOPE}/{conv}/"
        v = {leaf: torch.from_numpy(vars_[pre + leaf]).to(dtype) for leaf in LEAVES + ("bn/moving_mean", "bn/moving_variance")}
        for leaf in LEAVES:
            leaves[pre + leaf] = v[leaf].requires_grad_()
        s = v["bn/gamma"] / torch.sqrt(v["bn/moving_variance"] + tf_util.BN_EPS)
        layers[conv] = (v["weights"] * s, (v["biases"] - v["bn/moving_mean"]) * s + v["bn/beta"])
    leaves["xyz"] = torch.from_numpy(xyz).to(dtype).requires_grad_()
    leaves["feature"] = torch.from_numpy(feature).to(dtype).requires_grad_()
    nx, nf = R.cell_tensors(leaves["xyz"], leaves["feature"], idx, as_, layers)
    torch.autograd.backward([nx, nf], [torch.from_numpy(gxyz).to(dtype), torch.from_numpy(gfeat).to(dtype)])
    return nx.detach().numpy(), nf.detach().numpy(), {k: v.grad.numpy() for k, v in leaves.items()}


@pytest.mark.parametrize("shape", CELL_SHAPES)
def test_the_whole_cell(U, L, shape, monkeypatch):
    from pointasnl_amd.utils import tf_util

    b, n, c, p, k, as_ = shape
    xyz, feature, idx, gxyz, gfeat = cell_inputs(shape)
    st = tf_util.set_store(tf_util.VariableStore(seed=7, randomize_bn=True))
    xd, fd, idxd = dev(xyz), dev(feature), dev(idx)
    seen = []
    real = L.launch
    monkeypatch.setattr(L, "launch", lambda symbol, *a: (seen.append(symbol), real(symbol, *a))[1])
    with torch.no_grad():  # the first call creates the variables; without a gradient: the one-kernel cell, as before
        inf_xyz, inf_feat = U.adaptive_sampling_fused(xd, fd, idxd, as_, SCOPE, True)
    assert inf_xyz.grad_fn is None and inf_feat.grad_fn is None
    assert seen == ["pasnl_as_gather", CELL_KERNEL[c]]
    del seen[:]
    plain_xyz, plain_feat = U.adaptive_sampling_fused(xd, fd, idxd, as_, SCOPE, True)  # gradients enabled, nothing requires one
    assert plain_xyz.grad_fn is None and seen == ["pasnl_as_gather", CELL_KERNEL[c]]
    np.testing.assert_array_equal(bits(plain_xyz.cpu().numpy()), bits(inf_xyz.cpu().numpy()))
    np.testing.assert_array_equal(bits(plain_feat.cpu().numpy()), bits(inf_feat.cpu().numpy()))

    names = [f"{SCOPE}/{SCOPE}/{conv}/{leaf}" for conv in R.CELL_LAYERS for leaf in LEAVES]
    for name in names:
        st.vars[name].requires_grad_()
    st._folded.clear()
    xd.requires_grad_(), fd.requires_grad_()
    del seen[:]
    new_xyz, new_feat = U.adaptive_sampling_fused(xd, fd, idxd, as_, SCOPE, True)
    assert new_xyz.grad_fn is not None and new_feat.grad_fn is not None
    assert seen == ["pasnl_as_gather", "pasnl_as_attention_qkv", "pasnl_as_reweight_x"]
    assert not any(isinstance(key, str) and key.endswith("kvq_fused") for key in st._folded)  # no graph-carrying cache
    torch.autograd.backward([new_xyz, new_feat], [dev(gxyz), dev(gfeat)])

    vars_ = {k_: v.detach().cpu().numpy() for k_, v in st.vars.items()}
    want = cell_chain(vars_, xyz, feature, idx, as_, gxyz, gfeat, torch.float64)
    chain = cell_chain(vars_, xyz, feature, idx, as_, gxyz, gfeat, torch.float32)
    check(f"cell {shape} new_xyz", new_xyz.detach().cpu().numpy(), want[0], chain[0])
    check(f"cell {shape} new_feature", new_feat.detach().cpu().numpy(), want[1], chain[1])
    # (mlp2_1's biases and beta: the softmax over the neighbours ignores a per-column shift, so their float64 gradient is rounding
    # noise of 1e-17 and `err` compares two noises -- measured 9.2e8 against the chain's 5.4e8 and 7.5e8 against 6.5e8)
    for name in names:
        assert st.vars[name].grad is not None, name
        check(f"cell {shape} {name}", st.vars[name].grad.cpu().numpy(), want[2][name], chain[2][name])
    check(f"cell {shape} xyz", xd.grad.cpu().numpy(), want[2]["xyz"], chain[2]["xyz"])
    check(f"cell {shape} feature", fd.grad.cpu().numpy(), want[2]["feature"], chain[2]["feature"])


@pytest.mark.parametrize("shape", CELL_SHAPES)
def test_the_cells_gradient_to_xyz_alone(U, shape):
    """only xyz asks for a gradient: it flows in through the centred columns, the plain columns and the re-weighted coordinates"""
    from pointasnl_amd.utils import tf_util

    b, n, c, p, k, as_ = shape
    xyz, feature, idx, gxyz, gfeat = cell_inputs(shape)
    st = tf_util.set_store(tf_util.VariableStore(seed=7, randomize_bn=True))
    xd, fd, idxd = dev(xyz).requires_grad_(), dev(feature), dev(idx)
    new_xyz, new_feat = U.adaptive_sampling_fused(xd, fd, idxd, as_, SCOPE, True)
    assert new_xyz.grad_fn is not None
    torch.autograd.backward([new_xyz, new_feat], [dev(gxyz), dev(gfeat)])
    assert fd.grad is None and all(v.grad is None for v in st.vars.values())
    vars_ = {k_: v.detach().cpu().numpy() for k_, v in st.vars.items()}
    want = cell_chain(vars_, xyz, feature, idx, as_, gxyz, gfeat, torch.float64)[2]["xyz"]
    chain = cell_chain(vars_, xyz, feature, idx, as_, gxyz, gfeat, torch.float32)[2]["xyz"]
    check(f"cell {shape} xyz alone", xd.grad.cpu().numpy(), want, chain)
