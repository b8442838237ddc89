"""The fused backward of the input-space non-local cell (csrc/nl_input_grad.hip; include/pasnl.h: pasnl_cls_nl_cell_input_grad)
through pointasnl_util.nl_cell_input's autograd function, through the C ABI and through PointNonLocalCell.

Reference: tests/nl_cell_input_grad_ref.py, the header's formulas in float64.  Measure: err(X) = max |X - X64| / max |X64| per
gradient.  Yardstick: the float32 projected op-by-op chain (X wkv + bkv, Z wq + bq, matmul -> / sqrt(cb) -> softmax -> matmul)
differentiated by torch on the CPU, against the same float64 -- computed here, never taken from the code under test.  Allowed:
err <= max(4 * err_chain, 1e-5), the rule of tests/test_gpu_nl_grad.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nl_cell_input_grad_ref as R
from guarded import ALT_BYTE, ALT_WS_BYTE, NAN_BYTE, WS_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu

OK, EWORKSPACE = 0, -3

# the forward's own edge shapes (b, p, n, c, cz, cb)
SHAPES = [(2, 70, 45, 3, 6, 32),       # ragged, fewer keys than a block
          (1, 1, 1, 3, 6, 32),
          (3, 130, 333, 3, 6, 32),     # three query tiles, uneven key ranges
          (1, 64, 3, 3, 6, 32),        # fewer keys than waves
          (2, 33, 77, 6, 9, 64),
          (1, 40, 200, 8, 16, 128),
          (1, 64, 600, 3, 6, 32),      # 8 waves
          (1, 70, 4500, 3, 6, 32),     # 16 waves, a ragged second chunk
          (512, 1, 1100, 3, 6, 32),    # one query per tile, 512 partials to fold
          (1, 10, 2100, 5, 7, 64)]     # the generic width
SPIKE = (1, 64, 300, 3, 6, 32)
ABI_SHAPES = [(2, 70, 45, 3, 6, 32), (1, 40, 200, 8, 16, 128)]


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()  # (the cached cases are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def U():
    from pointasnl_amd.utils import pointasnl_util

    return pointasnl_util


def spike_problem():
    h, g = R.problem(*SPIKE)
    h = dict(h)
    f = np.array(h["feature"])
    f[0, 250] *= np.float32(40.0)
    f.setflags(write=False)
    h["feature"] = f
    return h, g


@functools.lru_cache(maxsize=None)
def case(shape, spike=False):
    """inputs, float64 gradients and the float32 chain's error against them -- computed once per shape, never modified"""
    h, g = spike_problem() if spike else R.problem(*shape)
    want = R.backward(h, g)
    _, chain = R.chain_autograd(h, g, torch.float32)
    for a in want.values():
        a.setflags(write=False)
    return h, g, want, {k: R.err(chain[k], want[k]) for k in R.NAMES}


def run_public(U, h, g, need=R.NAMES):
    t = {k: dev(h[k]).requires_grad_(k in need) for k in R.NAMES}
    out = U.nl_cell_input(*(t[k] for k in R.NAMES))
    out.backward(dev(g))
    return {k: None if t[k].grad is None else t[k].grad.cpu().numpy() for k in R.NAMES}


def check_parity(shape, got, c):
    h, _, want, chain = c
    cb = shape[-1]
    errs = {k: R.err(got[k], want[k]) for k in R.NAMES}
    print(f"nl_cell_input_grad {shape}: " + "  ".join(f"{k} {errs[k]:.3g} (chain {chain[k]:.3g})" for k in R.NAMES))
    for k in R.NAMES:
        assert got[k].dtype == np.float32 and got[k].shape == h[k].shape, k
        assert np.isfinite(got[k]).all(), k
    for k in R.NAMES:
        assert errs[k] <= max(4 * chain[k], 1e-5), k
    assert (bits(got["bkv"][:cb]) == 0).all()  # dbk: exact zeros


# ---------------------------------------------------------------------------------------------------------------------------
# parity through the public interface
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_through_the_public_interface(U, shape):
    c = case(shape)
    got = run_public(U, c[0], c[1])
    assert all(got[k] is not None for k in R.NAMES)
    check_parity(shape, got, c)


def test_spike(U):
    c = case(SPIKE, spike=True)
    _, w, _, _ = R.forward(c[0])
    onehot = (1.0 - w[0].max(axis=-1)) < 2.0 ** -30
    assert onehot.any() and (w[0].argmax(axis=-1)[onehot] == 250).all()  # some queries see key 250 alone
    got = run_public(U, c[0], c[1])
    check_parity(SPIKE, got, c)


def test_zero_grad_out_gives_exact_zeros(U):
    h, g = R.problem(2, 70, 45, 3, 6, 32)
    got = run_public(U, h, np.zeros_like(g))
    for k in R.NAMES:
        assert (got[k] == 0).all(), k


# ---------------------------------------------------------------------------------------------------------------------------
# needs_input_grad / NULL outputs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ABI_SHAPES)
@pytest.mark.parametrize("need", [("wkv", "bkv", "wq", "bq"), ("feature",), ("new_point",)], ids=["weights", "feature", "new_point"])
def test_needs_input_grad(U, shape, need):
    h, g = case(shape)[:2]
    full = run_public(U, h, g)
    part = run_public(U, h, g, need=need)
    for k in R.NAMES:
        if k in need:
            np.testing.assert_array_equal(bits(part[k]), bits(full[k]), err_msg=k)
        else:
            assert part[k] is None, k


def ptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else 0 if t is None else t.data_ptr())


def call_abi(shape, ins, g, grads, ws, ws_bytes):
    from pointasnl_amd import _hip

    status = _hip.lib().pasnl_cls_nl_cell_input_grad(*shape, *(ptr(ins[k]) for k in R.NAMES), ptr(g), *(ptr(grads[k]) for k in R.NAMES),
                                                     ptr(ws), ctypes.c_size_t(ws_bytes), _hip.stream_ptr())
    torch.cuda.synchronize()
    return status


def workspace_bytes(shape):
    from pointasnl_amd import _hip

    return int(_hip.lib().pasnl_cls_nl_cell_input_grad_workspace_bytes(*shape))


@pytest.mark.parametrize("shape", ABI_SHAPES)
def test_abi_null_outputs_leave_the_others_unchanged(shape):
    h, g = case(shape)[:2]
    ins, gd = {k: dev(h[k]) for k in R.NAMES}, dev(g)
    nbytes = workspace_bytes(shape)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    runs = {}
    for skip in (None,) + R.NAMES:
        grads = {k: torch.full_like(ins[k], float("nan")) for k in R.NAMES}
        assert call_abi(shape, ins, gd, {k: None if k == skip else grads[k] for k in R.NAMES}, ws, nbytes) == OK
        runs[skip] = {k: grads[k].cpu().numpy() for k in R.NAMES}
    for k in R.NAMES:
        assert np.isfinite(runs[None][k]).all(), k  # every element written
    for skip in R.NAMES:
        for k in R.NAMES:
            if k == skip:
                assert np.isnan(runs[skip][k]).all(), (skip, k)  # the gradient not asked for: its buffer as it was
            else:
                np.testing.assert_array_equal(bits(runs[skip][k]), bits(runs[None][k]), err_msg=f"{k} without {skip}")


# ---------------------------------------------------------------------------------------------------------------------------
# guarded run: outputs and an exact-size workspace inside guarded buffers, two runs over different stale bytes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ABI_SHAPES + [(3, 130, 333, 3, 6, 32)])
def test_guarded_outputs_and_exact_workspace(shape):
    c = case(shape)
    h, g = c[:2]
    ins, gd = {k: dev(h[k]) for k in R.NAMES}, dev(g)
    nbytes = workspace_bytes(shape)
    assert nbytes > 0
    runs = []
    for fill, ws_fill in ((NAN_BYTE, WS_BYTE), (ALT_BYTE, ALT_WS_BYTE)):
        grads = {k: Guarded(4 * h[k].size, fill, output_guard(4 * h[k].shape[-1])) for k in R.NAMES}
        ws = Guarded(nbytes, ws_fill)
        ptrs = {k: grads[k].ptr for k in R.NAMES}
        # one byte short: refused before any launch, nothing touched
        assert call_abi(shape, ins, gd, ptrs, ws.ptr, nbytes - 1) == EWORKSPACE
        assert all(grads[k].untouched() for k in R.NAMES) and ws.untouched()
        assert call_abi(shape, ins, gd, ptrs, ws.ptr, nbytes) == OK
        assert all(grads[k].guards_intact() for k in R.NAMES) and ws.guards_intact()
        runs.append({k: grads[k].floats(h[k].shape) for k in R.NAMES})
        assert all(np.isfinite(runs[-1][k]).all() for k in R.NAMES)  # every element written
    for k in R.NAMES:  # a pure function of the inputs, whatever the outputs and the workspace held
        np.testing.assert_array_equal(bits(runs[0][k]), bits(runs[1][k]), err_msg=k)
    check_parity(shape, runs[0], c)


def test_no_query_zero_fills_what_is_given():
    """p == 0: success; every gradient given is all zeros and nothing beside it is written"""
    b, n, c, cz, cb = 2, 45, 3, 6, 32
    sizes = dict(feature=b * n * c, wkv=c * 2 * cb, bkv=2 * cb, wq=cz * cb, bq=cb)
    grads = {k: Guarded(4 * v, NAN_BYTE, output_guard(4 * cb)) for k, v in sizes.items()}
    ptrs = {k: grads[k].ptr if k in grads else None for k in R.NAMES}
    assert call_abi((b, 0, n, c, cz, cb), {k: None for k in R.NAMES}, None, ptrs, None, 0) == OK
    for k, v in sizes.items():
        assert grads[k].guards_intact() and (grads[k].array((v,), np.uint32) == 0).all(), k


# ---------------------------------------------------------------------------------------------------------------------------
# the forward is what it was
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 70, 45, 3, 6, 32), (1, 70, 4500, 3, 6, 32), (1, 40, 200, 8, 16, 128)])
def test_forward_unchanged(U, shape):
    from pointasnl_amd import _hip

    h = case(shape)[0]
    b, p, n, c, cz, cb = shape
    ins = {k: dev(h[k]) for k in R.NAMES}
    direct = torch.empty((b, p, cb), dtype=torch.float32, device="cuda")
    assert _hip.lib().pasnl_cls_nl_cell_input(*shape, *(ptr(ins[k]) for k in R.NAMES), ptr(direct), _hip.stream_ptr()) == OK
    torch.cuda.synchronize()
    want = direct.cpu().numpy()
    plain = U.nl_cell_input(*(ins[k] for k in R.NAMES))
    assert plain.grad_fn is None and not plain.requires_grad
    np.testing.assert_array_equal(bits(plain.cpu().numpy()), bits(want))
    tr = {k: dev(h[k]).requires_grad_() for k in R.NAMES}
    with torch.no_grad():
        quiet = U.nl_cell_input(*(tr[k] for k in R.NAMES))
    assert quiet.grad_fn is None and not quiet.requires_grad
    np.testing.assert_array_equal(bits(quiet.cpu().numpy()), bits(want))
    tracked = U.nl_cell_input(*(tr[k] for k in R.NAMES))  # and the differentiable path returns the same forward bits
    assert tracked.grad_fn is not None
    np.testing.assert_array_equal(bits(tracked.detach().cpu().numpy()), bits(want))


# ---------------------------------------------------------------------------------------------------------------------------
# through the model code: PointNonLocalCell on a 3-channel level, BN folding differentiated by torch
# ---------------------------------------------------------------------------------------------------------------------------
LEAVES = ("weights", "biases", "bn/gamma", "bn/beta")


def folded_chain(vars_, x, z, cb, dtype):
    """the cell before its back-projection from the store's own variables on the CPU, BN folded as VariableStore.layer folds it
    -> (out, leaves)"""
    from pointasnl_amd.utils import tf_util

    leaves, layers = {}, {}
    for conv in ("conv_kv", "conv_query"):
        v = {leaf: torch.from_numpy(vars_[f"nl/{conv}/{leaf}"]).to(dtype)
             for leaf in LEAVES + ("bn/moving_mean", "bn/moving_variance")}
        for leaf in LEAVES:
            leaves[f"nl/{conv}/{leaf}"] = v[leaf].requires_grad_()
        s = v["bn/gamma"] / torch.sqrt(v["bn/moving_variance"] + tf_util.BN_EPS)
        layers[conv] = (v["weights"] * s, (v["biases"] - v["bn/moving_mean"]) * s + v["bn/beta"])
    t = dict(feature=torch.from_numpy(x).to(dtype), new_point=torch.from_numpy(z).to(dtype), wkv=layers["conv_kv"][0],
             bkv=layers["conv_kv"][1], wq=layers["conv_query"][0], bq=layers["conv_query"][1])
    return R.chain_tensors(t, cb), leaves


def test_gradients_reach_the_variables_through_the_cell(U):
    from pointasnl_amd.utils import tf_util

    b, p, n, c, cb = 2, 70, 45, 3, 32
    rng = np.random.default_rng(11)
    x = rng.standard_normal((b, n, c)).astype(np.float32)
    z = rng.standard_normal((b, p, c)).astype(np.float32)
    g = rng.standard_normal((b, p, cb)).astype(np.float32)
    st = tf_util.set_store(tf_util.VariableStore(seed=5, randomize_bn=True))
    xd, zd = dev(x), dev(z).reshape(b, p, 1, c)
    with torch.no_grad():  # the first call creates the variables
        U.PointNonLocalCell(xd, zd, [cb], False, None, None, "nl", project=False)
    names = [f"nl/{conv}/{leaf}" for conv in ("conv_kv", "conv_query") for leaf in LEAVES]
    for name in names:
        st.vars[name].requires_grad_()
    st._folded.clear()
    out = U.PointNonLocalCell(xd, zd, [cb], False, None, None, "nl", project=False)
    assert out.shape == (b, p, cb) and out.grad_fn is not None
    out.backward(dev(g))
    vars_ = {k: v.detach().cpu().numpy() for k, v in st.vars.items()}
    want, chain = {}, {}
    for dtype, res in ((torch.float64, want), (torch.float32, chain)):
        o, leaves = folded_chain(vars_, x, z, cb, dtype)
        o.backward(torch.from_numpy(g).to(dtype))
        res.update({k: v.grad.numpy() for k, v in leaves.items()})
    for name in names:
        grad = st.vars[name].grad
        assert grad is not None, name
        e, ec = R.err(grad.cpu().numpy(), want[name]), R.err(chain[name], want[name])
        print(f"PointNonLocalCell {name}: err {e:.3g} (chain {ec:.3g})")
        assert e <= max(4 * ec, 1e-5), name
