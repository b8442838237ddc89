"""Training-mode batch norm and dropout on the device (csrc/bn_train.hip; include/pasnl.h: pasnl_cls_bn_train,
pasnl_cls_bn_train_grad, pasnl_cls_dropout) through the C ABI and through tf_util.batch_norm_train / tf_util.dropout.

Reference: tests/bn_train_ref.py, the header's formulas in float64, on problems whose ReLU cases keep a margin
(tests/test_bn_train_flow.py asserts it).  Measure: err(X) = max |X - X64| / max |X64| for y, save_rstd, both moving statistics,
grad_x, grad_gamma and grad_beta; save_mean relative to max(|mean|, std).  Yardstick: the float32 torch chain on the CPU --
centred mean / var / normalise, differentiated by torch -- against the same float64, computed here, never taken from the code
under test.  Allowed: err <= max(4 * err_chain, 1e-5), the rule of tests/test_gpu_sa_grad.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_train_ref as R
from guarded import ALT_WS_BYTE, NAN_BYTE, WS_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu

OK, EWORKSPACE, EUNSUPPORTED = 0, -3, -5
DECAY = 0.9


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def allowed(chain_err):
    return max(4 * chain_err, 1e-5)


def check(what, got, want, chain, scale=None):
    got, want = np.asarray(got), np.asarray(want, np.float64)
    scale = max(np.abs(want).max(), 1e-300) if scale is None else scale
    e = float(np.abs(got.astype(np.float64) - want).max() / scale)
    ec = float(np.abs(np.asarray(chain, np.float64) - want).max() / scale)
    print(f"{what}: err {e:.3g} (chain {ec:.3g})")
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all(), what
    assert e <= allowed(ec), what


@pytest.fixture(scope="module")
def L():
    from pointasnl_amd import _hip

    return _hip


@pytest.fixture(scope="module")
def T():
    from pointasnl_amd.utils import tf_util

    return tf_util


def moving32(m, batch, decay):
    """the float32 chain's moving update"""
    m, batch = np.asarray(m, np.float32), np.asarray(batch, np.float32)
    return (m - (m - batch) * (np.float32(1) - np.float32(decay))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_data(case, unbiased=True, decay=DECAY):
    rows, c, act, offset, _ = case
    x, gamma, beta, mm, mv, gy = R.problem(rows, c, act, offset)
    y, mean, var, rstd = R.forward(x, gamma, beta, act)
    gx, gg, gb = R.backward(x, gamma, beta, act, gy)
    want = dict(y=y, mean=mean, rstd=rstd, mm=R.moving(mm, mean, decay), mv=R.moving(mv, R.batch_variance(var, rows, unbiased), decay),
                grad_x=gx, grad_gamma=gg, grad_beta=gb, std=np.sqrt(var))
    ch = R.chain(x, gamma, beta, act, gy, torch.float32)
    ch["mm"] = moving32(mm, ch["mean"], decay)
    ch["mv"] = moving32(mv, (ch["var"] * np.float32(rows / max(rows - 1, 1))) if unbiased else ch["var"], decay)
    for a in (x, gamma, beta, mm, mv, gy):
        a.setflags(write=False)
    return (x, gamma, beta, mm, mv, gy), want, ch


def check_all(got, want, ch, names=("y", "mean", "rstd", "mm", "mv", "grad_x", "grad_gamma", "grad_beta")):
    for name in names:
        scale = max(np.abs(want["mean"]).max(), want["std"].max()) if name == "mean" else None
        if name == "grad_x" and not np.abs(want[name]).max() > 0:  # rows == 1: exactly zero
            assert (got[name] == 0).all()
            continue
        check(name, got[name], want[name], ch[name], scale)


def run_abi(L, data, act, unbiased=1, decay=DECAY, ws_fill=WS_BYTE, moving=True, want_gx=True, ws_short=0, x_offset=0):
    """both entries on guarded outputs and an exact-size guarded workspace -> (dict of numpy results, statuses, guards ok)"""
    x, gamma, beta, mm, mv, gy = data
    rows, c = x.shape
    lib = L.lib()
    if x_offset:  # the same values at an address that is 4-byte but not 16-byte aligned
        pad = np.zeros(x_offset, np.float32)
        xd = dev(np.concatenate([pad, x.reshape(-1)]))[x_offset:].view(rows, c)
        gyd = dev(np.concatenate([pad, gy.reshape(-1)]))[x_offset:].view(rows, c)
    else:
        xd, gyd = dev(x), dev(gy)
    gd, bd = dev(gamma), dev(beta)
    G = {"y": Guarded(rows * c * 4, NAN_BYTE, output_guard(c * 4)), "grad_x": Guarded(rows * c * 4, NAN_BYTE, output_guard(c * 4))}
    for name in ("mean", "rstd", "grad_gamma", "grad_beta", "mm", "mv"):
        G[name] = Guarded(c * 4, NAN_BYTE, output_guard(c * 4))
    G["mm"].inside().copy_(dev(mm).view(torch.uint8))
    G["mv"].inside().copy_(dev(mv).view(torch.uint8))
    need = int(lib.pasnl_cls_bn_train_workspace_bytes(rows, c))
    assert need == R.workspace_bytes(rows, c) == int(lib.pasnl_cls_bn_train_grad_workspace_bytes(rows, c))
    ws = Guarded(need, ws_fill)
    stream = torch.cuda.current_stream().cuda_stream
    s1 = lib.pasnl_cls_bn_train(rows, c, xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), R.EPS, decay, act, unbiased,
                                G["mm"].ptr if moving else 0, G["mv"].ptr if moving else 0, G["y"].ptr, G["mean"].ptr, G["rstd"].ptr,
                                ws.ptr, need - ws_short, stream)
    s2 = None
    if s1 == OK:
        s2 = lib.pasnl_cls_bn_train_grad(rows, c, xd.data_ptr(), G["y"].ptr, gd.data_ptr(), G["mean"].ptr, G["rstd"].ptr, act,
                                         gyd.data_ptr(), G["grad_x"].ptr if want_gx else 0, G["grad_gamma"].ptr, G["grad_beta"].ptr,
                                         ws.ptr, need - ws_short, stream)
    torch.cuda.synchronize()
    out = {name: g.floats((rows, c) if name in ("y", "grad_x") else (c,)) for name, g in G.items()}
    intact = all(g.guards_intact() for g in G.values()) and ws.guards_intact()
    return out, (s1, s2), intact, G, ws


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_parity_through_the_c_abi(L, case):
    data, want, ch = case_data(case)
    act = case[2]
    got, status, intact, G, ws = run_abi(L, data, act)
    assert status == (OK, OK) and intact
    check_all(got, want, ch)
    # the same bits over other stale workspace bytes; with null moving pointers nothing of them is written; a null grad_x
    again, status, intact, G2, _ = run_abi(L, data, act, ws_fill=ALT_WS_BYTE, moving=False, want_gx=False)
    assert status == (OK, OK) and intact
    for name in ("y", "mean", "rstd", "grad_gamma", "grad_beta"):
        assert (bits(again[name]) == bits(got[name])).all(), name
    assert (bits(again["mm"]) == bits(data[3])).all() and (bits(again["mv"]) == bits(data[4])).all()
    assert G2["grad_x"].untouched()
    # one byte less than the size function's value: refused, nothing written
    _, status, intact, G3, ws3 = run_abi(L, data, act, ws_short=1)
    assert status == (EWORKSPACE, None) and intact and ws3.untouched()
    assert all(G3[name].untouched() for name in ("y", "mean", "rstd", "grad_x", "grad_gamma", "grad_beta"))


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_parity_through_batch_norm_train(T, case):
    data, want, ch = case_data(case)
    x, gamma, beta, mm, mv, gy = data
    act = case[2]
    t = [dev(a) for a in (x, gamma, beta, mm, mv)]
    for a in t[:3]:
        a.requires_grad_(True)
    versions = (t[3]._version, t[4]._version)
    assert T.BN_TRAIN_FUSED
    y = T.batch_norm_train(t[0], t[1], t[2], t[3], t[4], DECAY, activation="relu" if act else None, unbiased=True)
    assert y.grad_fn is not None and (t[3]._version, t[4]._version) != versions
    y.backward(dev(gy))
    got = dict(y=y.detach().cpu().numpy(), mm=t[3].cpu().numpy(), mv=t[4].cpu().numpy(), grad_x=t[0].grad.cpu().numpy(),
               grad_gamma=t[1].grad.cpu().numpy(), grad_beta=t[2].grad.cpu().numpy())
    check_all(got, want, ch, names=("y", "mm", "mv", "grad_x", "grad_gamma", "grad_beta"))


def test_any_leading_shape_no_grad_and_other_activations(T):
    case = (4099, 4, 0, False, "")
    (x, gamma, beta, mm, mv, gy), want, ch = case_data(case)
    t = [dev(a) for a in (x[:4096].reshape(8, 16, 32, 4), gamma, beta, mm, mv)]
    y64, mean, var, rstd = R.forward(x[:4096], gamma, beta, 0)
    with torch.no_grad():
        y = T.batch_norm_train(t[0], t[1], t[2], t[3], t[4], lambda: 0.5, activation="sigmoid", unbiased=False)
    assert y.shape == (8, 16, 32, 4) and y.grad_fn is None
    sig = 1 / (1 + np.exp(-y64))
    assert np.abs(y.cpu().numpy().reshape(-1, 4) - sig).max() <= 1e-5                  # batch statistics under no_grad
    np.testing.assert_allclose(t[3].cpu().numpy(), R.moving(mm, mean, 0.5), rtol=1e-5, atol=1e-6)   # and the update still runs
    np.testing.assert_allclose(t[4].cpu().numpy(), R.moving(mv, var, 0.5), rtol=1e-5, atol=1e-6)
    # only gamma asks for a gradient: a grad_fn, and no grad_x pass
    g = dev(gamma).requires_grad_(True)
    y = T.batch_norm_train(dev(x), g, dev(beta), None, None, 0.9, activation="relu")
    y.sum().backward()
    assert g.grad is not None and torch.isfinite(g.grad).all()


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.99])
@pytest.mark.parametrize("unbiased", [0, 1])
@pytest.mark.parametrize("case", [R.CASES[0], R.CASES[11]], ids=R.case_id)
def test_moving_update(L, case, decay, unbiased):
    data, want, ch = case_data(case, bool(unbiased), decay)
    got, status, intact, _, _ = run_abi(L, data, case[2], unbiased=unbiased, decay=decay)
    assert status == (OK, OK) and intact
    check_all(got, want, ch, names=("mm", "mv"))
    if decay == 0.0:  # m <- batch, whatever m was
        rows = case[0]
        np.testing.assert_allclose(got["mv"], R.batch_variance(R.forward(*data[:3], 0)[2], rows, unbiased), rtol=1e-5, atol=1e-7)
    if case[0] == 1:  # one row: variance 0, and the Bessel factor's guard keeps it 0
        np.testing.assert_allclose(got["mv"], R.moving(data[4], 0.0, decay), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("case", [R.CASES[5], R.CASES[13], R.CASES[16]], ids=R.case_id)
def test_misaligned_view_takes_the_scalar_path(L, T, case):
    """c % 4 == 0 but x and grad_y start 4 bytes off a 16-byte boundary: 4-byte accesses, never a read outside the view"""
    data, want, ch = case_data(case)
    got, status, intact, _, _ = run_abi(L, data, case[2], x_offset=1)
    assert status == (OK, OK) and intact
    check_all(got, want, ch)
    # a 2-byte offset is no float pointer at all
    x = dev(data[0])
    assert L.lib().pasnl_cls_bn_train(4, 4, x.data_ptr() + 2, x.data_ptr(), x.data_ptr(), R.EPS, 0.9, 0, 1, 0, 0, x.data_ptr(),
                                      x.data_ptr(), x.data_ptr(), x.data_ptr(), 1 << 20, 0) == EUNSUPPORTED
    # the public op takes a non-contiguous view (every other column) as its values
    x2 = dev(np.repeat(data[0], 2, axis=1))[:, ::2]
    assert not x2.is_contiguous()
    y = T.batch_norm_train(x2, dev(data[1]), dev(data[2]), None, None, 0.9, activation="relu" if case[2] else None)
    check("y of a strided view", y.cpu().numpy(), want["y"], ch["y"])


# ---------------------------------------------------------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 4099, 1 << 16])
@pytest.mark.parametrize("keep", [0.4, 0.5, 1.0])
def test_dropout_bits_equal_the_host_restatement(L, n, keep):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n).astype(np.float32)
    seed, stream_id, call = (7 << 32) + 12345, 0xDEADBEEF, 41
    want = R.dropout(x, keep, seed, stream_id, call)
    stream = torch.cuda.current_stream().cuda_stream
    for offset in (0, 1):  # 16-byte aligned, and 4 bytes off
        xd = dev(np.concatenate([np.zeros(offset, np.float32), x]))[offset:]
        y = Guarded(n * 4, NAN_BYTE, 4096)
        yp = y.ptr
        assert L.lib().pasnl_cls_dropout(n, keep, seed, stream_id, call, xd.data_ptr(), yp, stream) == OK
        torch.cuda.synchronize()
        assert y.guards_intact() and (bits(y.floats((n,))) == bits(want)).all()
        assert L.lib().pasnl_cls_dropout(n, keep, seed, stream_id, call, xd.data_ptr(), xd.data_ptr(), stream) == OK  # in place
        torch.cuda.synchronize()
        assert (bits(xd.cpu().numpy()) == bits(want)).all()
    if keep == 1.0:
        assert (bits(want) == bits(x)).all()


def test_dropout_wrapper_backward_replay_and_inference(T):
    st = T.set_store(T.VariableStore(seed=(3 << 32) + 9))
    x = dev(np.random.default_rng(1).standard_normal((64, 512)).astype(np.float32)).requires_grad_(True)
    assert T.dropout(x, False, "dp1", keep_prob=0.4) is x and T.dropout(x, None, "dp1", keep_prob=0.4) is x
    assert st.dropout_calls == 0
    with T.variable_scope("head"):
        y = T.dropout(x, True, "dp1", keep_prob=0.4)
        sid = T.dropout_stream_id("head/dp1")
    assert st.dropout_calls == 1 and 0 <= sid < 1 << 32 and sid != T.dropout_stream_id("head/dp2")
    want = R.dropout(x.detach().cpu().numpy(), 0.4, st.seed, sid, 0)
    assert (bits(y.detach().cpu().numpy()) == bits(want)).all()
    g = np.random.default_rng(2).standard_normal((64, 512)).astype(np.float32)
    y.backward(dev(g))
    assert (bits(x.grad.cpu().numpy()) == bits(R.dropout(g, 0.4, st.seed, sid, 0))).all()   # the forward applied to the gradient
    with T.variable_scope("head"):
        y1 = T.dropout(x, True, "dp1", keep_prob=0.4)       # the next call: another mask
        st.dropout_calls = 0
        y0 = T.dropout(x, True, "dp1", keep_prob=0.4)       # the counter set back: the first mask again
    assert (bits(y0.detach().cpu().numpy()) == bits(want)).all() and not (y1 == y0).all()
    with pytest.raises(NotImplementedError):
        T.dropout(x, True, "dp1", keep_prob=0.4, noise_shape=[64, 1])
    with pytest.raises(TypeError):
        T.dropout(x, torch.tensor(True), "dp1")
