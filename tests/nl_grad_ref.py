"""The backward of the non-local attention core in numpy float64: the six formulas of include/pasnl.h
(pasnl_cls_nl_attention_grad), written out.  Shared by tests/test_nl_grad_flow.py (CPU: equal to torch's float64 autograd of
the op-by-op chain) and tests/test_gpu_nl_grad.py (GPU: the reference of the fused kernels)."""
import numpy as np

SHAPES_FLOW = [(2, 45, 77, 32), (1, 1, 1, 64), (2, 40, 80, 128)]


def problem(b, p, n, cb, seed=None):
    """q (b,p,cb), kv (b,n,2cb), g (b,p,cb) as float32, standard normal"""
    rng = np.random.default_rng(b * 1000003 + p * 1009 + n * 31 + cb if seed is None else seed)
    q = rng.standard_normal((b, p, cb)).astype(np.float32)
    kv = rng.standard_normal((b, n, 2 * cb)).astype(np.float32)
    g = rng.standard_normal((b, p, cb)).astype(np.float32)
    return q, kv, g


def forward(q, kv):
    """-> (P (b,p,n), O (b,p,cb)) in float64"""
    q, kv = np.asarray(q, np.float64), np.asarray(kv, np.float64)
    cb = q.shape[-1]
    k, v = kv[..., :cb], kv[..., cb:]
    s = np.einsum("bic,bjc->bij", q, k) / np.sqrt(cb)
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    prob = e / e.sum(axis=-1, keepdims=True)
    return prob, np.einsum("bij,bjc->bic", prob, v)


def backward(q, kv, g):
    """-> (grad_q (b,p,cb), grad_kv (b,n,2cb)) in float64"""
    q, kv, g = np.asarray(q, np.float64), np.asarray(kv, np.float64), np.asarray(g, np.float64)
    cb = q.shape[-1]
    k, v = kv[..., :cb], kv[..., cb:]
    prob, o = forward(q, kv)
    delta = (g * o).sum(axis=-1)                              # delta_i = sum_c g_ic O_ic
    dp = np.einsum("bic,bjc->bij", g, v)                      # dP_ij = g_i . v_j
    ds = prob * (dp - delta[..., None])                       # dS_ij = P_ij (dP_ij - delta_i)
    dq = np.einsum("bij,bjc->bic", ds, k) / np.sqrt(cb)       # dQ_i = sum_j dS_ij k_j / sqrt(cb)
    dk = np.einsum("bij,bic->bjc", ds, q) / np.sqrt(cb)       # dK_j = sum_i dS_ij q_i / sqrt(cb)
    dv = np.einsum("bij,bic->bjc", prob, g)                   # dV_j = sum_i P_ij g_i
    return dq, np.concatenate([dk, dv], axis=-1)


def chain_autograd(q, kv, g, dtype):
    """torch on the CPU: matmul -> / sqrt(cb) -> softmax -> matmul, differentiated by autograd in `dtype`
    -> (out, grad_q, grad_kv) as numpy arrays of that dtype"""
    import torch

    qt = torch.from_numpy(np.asarray(q)).to(dtype).requires_grad_()
    kvt = torch.from_numpy(np.asarray(kv)).to(dtype).requires_grad_()
    cb = qt.shape[-1]
    att = torch.matmul(qt, kvt[..., :cb].transpose(1, 2))
    att = torch.softmax(att / (float(cb) ** 0.5), dim=-1)
    out = torch.matmul(att, kvt[..., cb:])
    out.backward(torch.from_numpy(np.asarray(g)).to(dtype))
    return out.detach().numpy(), qt.grad.numpy(), kvt.grad.numpy()


def err(x, x64):
    """max |X - X64| / max |X64|"""
    x64 = np.asarray(x64, np.float64)
    scale = np.abs(x64).max()
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / (scale if scale > 0 else 1.0))
