"""The backward of the input-space non-local cell in numpy float64: the formulas of include/pasnl.h
(pasnl_cls_nl_cell_input_grad), written out.  Shared by tests/test_nl_cell_input_grad_flow.py (CPU: equal to torch's float64
autograd of the projected op-by-op chain) and tests/test_gpu_nl_cell_input_grad.py (GPU: the reference of the fused kernels).

Notation: X = feature (b,n,c), Z = new_point (b,p,cz), wkv = [Wk | Wv] (c,2cb), bkv = [bk | bv], r = 1/sqrt(cb), G = grad_out."""
import numpy as np

import nl_cell_input_ref

NAMES = ("feature", "new_point", "wkv", "bkv", "wq", "bq")  # the order of the entry point's operands and gradients
SHAPES_FLOW = [(2, 70, 45, 3, 6, 32), (1, 1, 1, 3, 6, 32), (2, 33, 77, 6, 9, 64), (1, 40, 200, 8, 16, 128), (1, 64, 3, 3, 6, 32)]


def problem(b, p, n, c, cz, cb, seed=0):
    """(h, g): the inputs of nl_cell_input_ref.problem and a seeded standard-normal grad_out (b,p,cb), float32, read-only"""
    h = nl_cell_input_ref.problem(b, p, n, c, cz, cb, seed)
    g = np.random.default_rng([seed, b, p, n, c, cz, cb, 7]).standard_normal((b, p, cb)).astype(np.float32)
    g.setflags(write=False)
    return h, g


def forward(h):
    """-> (u (b,p,c) = Wk Q, w (b,p,n), ctr (b,p,c), out (b,p,cb)) in float64"""
    x, z, wkv, bkv, wq, bq = (np.asarray(h[k], np.float64) for k in NAMES)
    cb = wq.shape[1]
    q = z @ wq + bq
    u = q @ wkv[:, :cb].T
    s = np.einsum("bic,bjc->bij", u, x) / np.sqrt(cb)
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    w = e / e.sum(axis=-1, keepdims=True)
    ctr = np.einsum("bij,bjc->bic", w, x)
    return u, w, ctr, ctr @ wkv[:, cb:] + bkv[cb:]


def backward(h, g):
    """-> {name: gradient} in float64, the layouts of the six inputs"""
    x, z, wkv, bkv, wq, bq = (np.asarray(h[k], np.float64) for k in NAMES)
    g = np.asarray(g, np.float64)
    cb = wq.shape[1]
    r = 1.0 / np.sqrt(cb)
    wk, wv = wkv[:, :cb], wkv[:, cb:]
    u, w, ctr, _ = forward(h)
    hh = g @ wv.T                                             # h_i = Wv G_i
    t = np.einsum("bic,bjc->bij", hh, x)                      # t_ij = h_i . X_j
    delta = (hh * ctr).sum(axis=-1)                           # delta_i = h_i . ctr_i
    ds = w * (t - delta[..., None])                           # dS_ij = w_ij (t_ij - delta_i)
    du = r * np.einsum("bij,bjc->bic", ds, x)                 # du_i = r sum_j dS_ij X_j
    dx = np.einsum("bij,bic->bjc", w, hh) + r * np.einsum("bij,bic->bjc", ds, u)
    a = np.einsum("bia,bic->ac", z, du)                       # A = sum_i Z_i^T du_i (cz,c)
    s = du.sum(axis=(0, 1))                                   # s = sum_i du_i
    dwk = a.T @ wq + np.outer(s, bq)                          # dWk = A^T Wq + s (x) bq
    dwv = np.einsum("bic,bik->ck", ctr, g)
    dbv = g.sum(axis=(0, 1))
    return dict(feature=dx, new_point=(du @ wk) @ wq.T, wkv=np.concatenate([dwk, dwv], axis=1),
                bkv=np.concatenate([np.zeros(cb), dbv]), wq=a @ wk, bq=s @ wk)


def chain_tensors(t, cb):
    """torch: X wkv + bkv and Z wq + bq, then matmul, / sqrt(cb), softmax, matmul -> out (b,p,cb)"""
    import torch

    kv = torch.matmul(t["feature"], t["wkv"]) + t["bkv"]
    q = torch.matmul(t["new_point"], t["wq"]) + t["bq"]
    att = torch.matmul(q, kv[..., :cb].transpose(1, 2))
    att = torch.softmax(att / (float(cb) ** 0.5), dim=-1)
    return torch.matmul(att, kv[..., cb:])


def chain_autograd(h, g, dtype):
    """the projected op-by-op chain on the CPU, differentiated by torch in `dtype` -> (out, {name: gradient}) as numpy arrays"""
    import torch

    t = {k: torch.from_numpy(np.array(h[k])).to(dtype).requires_grad_() for k in NAMES}
    out = chain_tensors(t, h["wq"].shape[1])
    out.backward(torch.from_numpy(np.array(g)).to(dtype))
    return out.detach().numpy(), {k: t[k].grad.numpy() for k in NAMES}


def err(x, x64):
    """max |X - X64| / max |X64|; the scale is 1 where the reference is all zeros"""
    x64 = np.asarray(x64, np.float64)
    scale = np.abs(x64).max()
    return float(np.abs(np.asarray(x, np.float64) - x64).max() / (scale if scale > 0 else 1.0))
