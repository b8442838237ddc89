"""The fused backward of the non-local attention core (csrc/nl_grad.hip; include/pasnl.h: pasnl_cls_nl_attention_grad) through
pointasnl_util.nl_attention's autograd function and through the C ABI.

Reference: tests/nl_grad_ref.py, the header's six formulas in float64.  Measure: err(X) = max |X - X64| / max |X64| per gradient.
Yardstick: the float32 op-by-op chain (matmul -> / sqrt(cb) -> softmax -> matmul) differentiated by torch on the CPU, against
the same float64 -- computed here, never taken from the code under test.  Allowed: err <= max(4 * err_chain, 1e-5): the factor 4
covers the hardware exp2 (about 1 ulp) and a different association of the sums, 1e-5 is the project's tolerance for the attention
cores, relative to scale."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import nl_grad_ref as R
from guarded import ALT_BYTE, ALT_WS_BYTE, NAN_BYTE, WS_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu

OK, EWORKSPACE = 0, -3

# the smallest shapes at which each branch can go wrong (b, p, n, cb)
SHAPES = [(2, 45, 77, 32), (2, 33, 64, 64),   # ragged in both dimensions
          (1, 1, 1, 64),
          (2, 40, 80, 128),                   # the cb = 128 form (K and V tiles of the key-major kernel in LDS)
          (1, 70, 300, 32),                   # several blocks per wave
          (3, 64, 32, 32),                    # one key block
          (1, 512, 1024, 32),                 # cls layer 1 at b = 1: the split at its production value
          (1, 96, 4096, 32)]                  # the forward takes the keys-over-workgroups form: `out` comes from that path


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()  # (the cached cases are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def U():
    from pointasnl_amd.utils import pointasnl_util

    return pointasnl_util


@functools.lru_cache(maxsize=None)
def case(shape, spike=False):
    """inputs, float64 gradients and the float32 chain's error against them -- computed once per shape, never modified"""
    q, kv, g = spike_problem() if spike else R.problem(*shape)
    want_q, want_kv = R.backward(q, kv, g)
    _, cq, ckv = R.chain_autograd(q, kv, g, torch.float32)
    for a in (q, kv, g, want_q, want_kv):
        a.setflags(write=False)
    return q, kv, g, want_q, want_kv, R.err(cq, want_q), R.err(ckv, want_kv)


SPIKE = (1, 64, 300, 32)


def spike_problem():
    """the construction of test_gpu_cells.py::test_nl_attention_spike (same seed, same shape): a late key (250) that is 6 x query
    3 over keys of scale 0.1 -- q_3 . k_250 = 6 |q_3|^2 is in the hundreds, query 3's softmax is one-hot, and key 250 spreads
    the other queries' scores over tens of units"""
    b, p, n, cb = SPIKE
    rng = np.random.default_rng(5)
    q = rng.standard_normal((b, p, cb)).astype(np.float32)
    kv = rng.standard_normal((b, n, 2 * cb)).astype(np.float32) * np.float32(0.1)
    kv[0, 250, :cb] = q[0, 3] * np.float32(6.0)
    g = rng.standard_normal((b, p, cb)).astype(np.float32)
    return q, kv, g


def run_public(U, q, kv, g, need_q=True, need_kv=True):
    qd, kvd = dev(q).requires_grad_(need_q), dev(kv).requires_grad_(need_kv)
    out = U.nl_attention(qd, kvd)
    out.backward(dev(g))
    return (None if qd.grad is None else qd.grad.cpu().numpy()), (None if kvd.grad is None else kvd.grad.cpu().numpy())


def check_parity(shape, got_q, got_kv, c):
    _, _, _, want_q, want_kv, chain_q, chain_kv = c
    eq, ekv = R.err(got_q, want_q), R.err(got_kv, want_kv)
    print(f"nl_grad {shape}: err dq {eq:.3g} (chain {chain_q:.3g})  err dkv {ekv:.3g} (chain {chain_kv:.3g})")
    assert got_q.dtype == np.float32 and got_kv.dtype == np.float32
    assert np.isfinite(got_q).all() and np.isfinite(got_kv).all()
    assert eq <= max(4 * chain_q, 1e-5)
    assert ekv <= max(4 * chain_kv, 1e-5)


# ---------------------------------------------------------------------------------------------------------------------------
# parity through the public interface
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_through_the_public_interface(U, shape):
    c = case(shape)
    got_q, got_kv = run_public(U, *c[:3])
    assert got_q is not None and got_kv is not None  # (None without the autograd function)
    assert got_q.shape == c[0].shape and got_kv.shape == c[1].shape
    check_parity(shape, got_q, got_kv, c)
    if shape == SHAPES[-1]:  # ... and that shape's forward did split its keys over workgroups
        from pointasnl_amd import _hip

        assert U.NL_KEY_PARTS and int(_hip.lib().pasnl_nl_attention_workspace_bytes(*shape)) > 0


def test_spike(U):
    c = case(SPIKE, spike=True)
    q, kv = c[0].astype(np.float64), c[1].astype(np.float64)
    dots = q[0] @ kv[0, :, :32].T
    assert dots[3, 250] > 100 and dots[3].argmax() == 250                    # the raw score in the hundreds
    lead = (dots[3, 250] - np.delete(dots[3], 250).max()) * np.log2(np.e) / np.sqrt(32)
    assert lead > 30                                                         # every other probability of query 3 below 2^-30
    got_q, got_kv = run_public(U, *c[:3])
    check_parity(SPIKE, got_q, got_kv, c)


def test_zero_grad_out_gives_exact_zeros(U):
    q, kv, g = R.problem(2, 45, 77, 32)
    got_q, got_kv = run_public(U, q, kv, np.zeros_like(g))
    assert (got_q == 0).all() and (got_kv == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# needs_input_grad / NULL outputs
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 45, 77, 32), (2, 40, 80, 128)])
def test_needs_input_grad(U, shape):
    q, kv, g = case(shape)[:3]
    both_q, both_kv = run_public(U, q, kv, g)
    only_q, none_kv = run_public(U, q, kv, g, need_kv=False)
    none_q, only_kv = run_public(U, q, kv, g, need_q=False)
    assert none_kv is None and none_q is None
    np.testing.assert_array_equal(bits(only_q), bits(both_q))
    np.testing.assert_array_equal(bits(only_kv), bits(both_kv))


def ptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else 0 if t is None else t.data_ptr())


def call_abi(shape, q, kv, out, g, gq, gkv, ws, ws_bytes):
    from pointasnl_amd import _hip

    status = _hip.lib().pasnl_cls_nl_attention_grad(*shape, ptr(q), ptr(kv), ptr(out), ptr(g), ptr(gq), ptr(gkv), ptr(ws),
                                                    ctypes.c_size_t(ws_bytes), _hip.stream_ptr())
    torch.cuda.synchronize()
    return status


def workspace_bytes(shape):
    from pointasnl_amd import _hip

    return int(_hip.lib().pasnl_cls_nl_attention_grad_workspace_bytes(*shape))


def forward_direct(shape, qd, kvd):
    """a direct launch of the forward entry the mirror would choose -> out"""
    from pointasnl_amd import _hip

    b, p, n, cb = shape
    out = torch.empty_like(qd)
    nbytes = int(_hip.lib().pasnl_nl_attention_workspace_bytes(b, p, n, cb))
    if nbytes:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        status = _hip.lib().pasnl_nl_attention_ws(b, p, n, cb, ptr(qd), ptr(kvd), ptr(out), 0, ptr(ws), ctypes.c_size_t(nbytes),
                                                  _hip.stream_ptr())
    else:
        status = _hip.lib().pasnl_nl_attention(b, p, n, cb, ptr(qd), ptr(kvd), ptr(out), 0, _hip.stream_ptr())
    torch.cuda.synchronize()
    assert status == OK
    return out


@pytest.mark.parametrize("shape", [(2, 45, 77, 32), (2, 40, 80, 128)])
def test_abi_null_outputs_leave_the_other_unchanged(shape):
    b, p, n, cb = shape
    q, kv, g = case(shape)[:3]
    qd, kvd, gd = dev(q), dev(kv), dev(g)
    out = forward_direct(shape, qd, kvd)
    nbytes = workspace_bytes(shape)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    runs = {}
    for name, want_q, want_kv in (("both", True, True), ("q", True, False), ("kv", False, True)):
        gq = torch.full_like(qd, float("nan")) if want_q else None
        gkv = torch.full_like(kvd, float("nan")) if want_kv else None
        assert call_abi(shape, qd, kvd, out, gd, gq, gkv, ws, nbytes) == OK
        runs[name] = (None if gq is None else gq.cpu().numpy(), None if gkv is None else gkv.cpu().numpy())
    np.testing.assert_array_equal(bits(runs["q"][0]), bits(runs["both"][0]))
    np.testing.assert_array_equal(bits(runs["kv"][1]), bits(runs["both"][1]))
    assert np.isfinite(runs["both"][0]).all() and np.isfinite(runs["both"][1]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# guarded run: outputs and an exact-size workspace inside guarded buffers, two runs over different stale bytes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 45, 77, 32), (2, 40, 80, 128)])
def test_guarded_outputs_and_exact_workspace(shape):
    b, p, n, cb = shape
    c = case(shape)
    qd, kvd, gd = dev(c[0]), dev(c[1]), dev(c[2])
    out = forward_direct(shape, qd, kvd)
    nbytes = workspace_bytes(shape)
    assert 0 < nbytes <= 8 * b * p + 256
    runs = []
    for fill, ws_fill in ((NAN_BYTE, WS_BYTE), (ALT_BYTE, ALT_WS_BYTE)):
        gq = Guarded(4 * b * p * cb, fill, output_guard(4 * cb))
        gkv = Guarded(4 * b * n * 2 * cb, fill, output_guard(4 * 2 * cb))
        ws = Guarded(nbytes, ws_fill)
        # one byte short: refused before any launch, nothing touched
        assert call_abi(shape, qd, kvd, out, gd, gq.ptr, gkv.ptr, ws.ptr, nbytes - 1) == EWORKSPACE
        assert gq.untouched() and gkv.untouched() and ws.untouched()
        assert call_abi(shape, qd, kvd, out, gd, gq.ptr, gkv.ptr, ws.ptr, nbytes) == OK
        assert gq.guards_intact() and gkv.guards_intact() and ws.guards_intact()
        runs.append((gq.floats((b, p, cb)), gkv.floats((b, n, 2 * cb))))
        assert np.isfinite(runs[-1][0]).all() and np.isfinite(runs[-1][1]).all()  # every element written
    np.testing.assert_array_equal(bits(runs[0][0]), bits(runs[1][0]))
    np.testing.assert_array_equal(bits(runs[0][1]), bits(runs[1][1]))
    check_parity(shape, runs[0][0], runs[0][1], c)


def test_no_query_zero_fills_grad_kv():
    """p == 0: success; grad_kv, when given, is all zeros (no query contributes) and nothing beside it is written"""
    b, n, cb = 2, 45, 32
    gkv = Guarded(4 * b * n * 2 * cb, NAN_BYTE, output_guard(4 * 2 * cb))
    assert call_abi((b, 0, n, cb), None, None, None, None, None, gkv.ptr, None, 0) == OK
    assert gkv.guards_intact() and (bits(gkv.floats((b, n, 2 * cb))) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the forward is what it was
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 45, 77, 32), (1, 96, 4096, 32), (2, 40, 80, 128)])
def test_forward_unchanged(U, shape):
    q, kv, _ = case(shape)[:3]
    qd, kvd = dev(q), dev(kv)
    want = forward_direct(shape, qd, kvd).cpu().numpy()
    plain = U.nl_attention(qd, kvd)
    assert plain.grad_fn is None and not plain.requires_grad
    np.testing.assert_array_equal(bits(plain.cpu().numpy()), bits(want))
    qg, kvg = dev(q).requires_grad_(), dev(kv).requires_grad_()
    with torch.no_grad():
        quiet = U.nl_attention(qg, kvg)
    assert quiet.grad_fn is None and not quiet.requires_grad
    np.testing.assert_array_equal(bits(quiet.cpu().numpy()), bits(want))
    tracked = U.nl_attention(qg, kvg)  # and the differentiable path returns the same forward bits
    assert tracked.grad_fn is not None
    np.testing.assert_array_equal(bits(tracked.detach().cpu().numpy()), bits(want))
