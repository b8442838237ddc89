"""The backward of the AdaptiveSampling cell's three fused parts in numpy float64: the formulas of include/pasnl.h
(pasnl_cls_as_attention_grad, pasnl_cls_as_reweight_grad / _x_grad, pasnl_cls_as_gather_grad), written out, plus torch on the CPU
differentiating the op-by-op chain (bmm, softmax, bmm, softmax(dim=2), sums) in a dtype of choice -- each part and the whole
cell: gather, projections, attention, mlp2, re-weighting.  Shared by tests/test_as_grad_flow.py (CPU: the formulas equal torch's
float64 autograd) and tests/test_gpu_as_grad.py (GPU: the reference and the yardstick of the fused kernels)."""
import numpy as np

import nl_grad_ref as N

err = N.err  # max |X - X64| / max |X64|

SHAPES_FLOW = [(3, 12, 32), (1, 1, 33), (2, 16, 65)]  # (g, as, cb)
GATHER_FLOW = (2, 50, 3, 7, 20, 12)                   # (b, n, c, m, k, as)


# ---------------------------------------------------------------------------------------------------------------------------
# micro attention: nl_grad_ref's six formulas with p = n = as, one "cloud" per group
# ---------------------------------------------------------------------------------------------------------------------------
def attention_problem(g, as_, cb, seed=None):
    """q (g,as,cb), kv (g,as,2cb), grad_out (g,as,cb) as float32, standard normal"""
    return N.problem(g, as_, as_, cb, seed=g * 7919 + as_ * 104729 + cb if seed is None else seed)


def attention_forward(q, kv):
    return N.forward(q, kv)[1]


def attention_backward(q, kv, g):
    """-> (grad_q (g,as,cb), grad_kv (g,as,2cb) = [dK | dV]) in float64"""
    return N.backward(q, kv, g)


def attention_chain(q, kv, g, dtype):
    """-> (out, grad_q, grad_kv): torch's autograd of matmul -> / sqrt(cb) -> softmax -> matmul in `dtype`"""
    return N.chain_autograd(q, kv, g, dtype)


def pack_kvq(q, kv):
    """[K | V | Q] rows, the layout of pasnl_as_attention_qkv"""
    return np.ascontiguousarray(np.concatenate([kv, q], axis=-1))


# ---------------------------------------------------------------------------------------------------------------------------
# re-weighting tail
# ---------------------------------------------------------------------------------------------------------------------------
def reweight_problem(g, as_, nsample, ch, seed=None):
    """logits (g,as,1+ch), X (g,nsample,3), F (g,nsample,ch), gxyz (g,3), gfeat (g,ch) as float32"""
    rng = np.random.default_rng(g * 1000003 + as_ * 1009 + nsample * 31 + ch if seed is None else seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return dict(logits=f(g, as_, 1 + ch), X=f(g, nsample, 3), F=f(g, nsample, ch), gxyz=f(g, 3), gfeat=f(g, ch))


def _softmax_s(logits):
    z = np.asarray(logits, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def reweight_forward(logits, X, F):
    """-> (new_xyz (g,3), new_feature (g,ch)) in float64"""
    as_ = logits.shape[1]
    w = _softmax_s(logits)
    X, F = np.asarray(X, np.float64)[:, :as_], np.asarray(F, np.float64)[:, :as_]
    return (w[:, :, :1] * X).sum(axis=1), (w[:, :, 1:] * F).sum(axis=1)


def reweight_backward(logits, X, F, gxyz, gfeat):
    """-> (grad_logits (g,as,1+ch), dX (g,nsample,3), dF (g,nsample,ch)) in float64; rows as..nsample-1 are zeros"""
    as_ = logits.shape[1]
    w = _softmax_s(logits)
    X64, F64 = np.asarray(X, np.float64), np.asarray(F, np.float64)
    gxyz, gfeat = np.asarray(gxyz, np.float64), np.asarray(gfeat, np.float64)
    t = np.concatenate([(X64[:, :as_] * gxyz[:, None, :]).sum(axis=-1, keepdims=True), F64[:, :as_] * gfeat[:, None, :]], axis=-1)
    dlogits = w * (t - (w * t).sum(axis=1, keepdims=True))      # w[s,o] (t_s - sum_r w[r,o] t_r)
    dX, dF = np.zeros_like(X64), np.zeros_like(F64)
    dX[:, :as_] = w[:, :, :1] * gxyz[:, None, :]                # dX[s,d] = w[s,0] gxyz[d]
    dF[:, :as_] = w[:, :, 1:] * gfeat[:, None, :]               # dF[s,j] = w[s,1+j] gfeat[j]
    return dlogits, dX, dF


def reweight_x_backward(logits, x, gxyz, gfeat):
    """x (g,as,3+ch): coordinates and features both start at column 3 -> (grad_logits, grad_x (g,as,3+ch)) in float64"""
    dlogits, dX, dF = reweight_backward(logits, x[:, :, 3:6], x[:, :, 3:], gxyz, gfeat)
    gx = np.zeros(x.shape, np.float64)
    gx[:, :, 3:] = dF
    gx[:, :, 3:6] += dX
    return dlogits, gx


def reweight_chain(logits, X, F, gxyz, gfeat, dtype):
    """torch's autograd of softmax(dim=1) and the two weighted sums -> dict(new_xyz, new_feature, logits, X, F)"""
    import torch

    t = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_() for k, v in dict(logits=logits, X=X, F=F).items()}
    as_ = logits.shape[1]
    w = torch.softmax(t["logits"], dim=1)
    new_xyz = (w[:, :, :1] * t["X"][:, :as_]).sum(dim=1)
    new_feature = (w[:, :, 1:] * t["F"][:, :as_]).sum(dim=1)
    torch.autograd.backward([new_xyz, new_feature], [torch.from_numpy(np.asarray(gxyz)).to(dtype), torch.from_numpy(np.asarray(gfeat)).to(dtype)])
    out = dict(new_xyz=new_xyz.detach().numpy(), new_feature=new_feature.detach().numpy())
    out.update({k: v.grad.numpy() for k, v in t.items()})
    return out


def reweight_x_chain(logits, x, gxyz, gfeat, dtype):
    """the same on x rows -> dict(new_xyz, new_feature, logits, x)"""
    import torch

    lt = torch.from_numpy(np.asarray(logits)).to(dtype).requires_grad_()
    xt = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_()
    w = torch.softmax(lt, dim=1)
    new_xyz = (w[:, :, :1] * xt[:, :, 3:6]).sum(dim=1)
    new_feature = (w[:, :, 1:] * xt[:, :, 3:]).sum(dim=1)
    torch.autograd.backward([new_xyz, new_feature], [torch.from_numpy(np.asarray(gxyz)).to(dtype), torch.from_numpy(np.asarray(gfeat)).to(dtype)])
    return dict(new_xyz=new_xyz.detach().numpy(), new_feature=new_feature.detach().numpy(), logits=lt.grad.numpy(), x=xt.grad.numpy())


# ---------------------------------------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------------------------------------
def gather_problem(b, n, c, m, k, as_, seed=None):
    """xyz (b,n,3), feature (b,n,c), idx (b,m,k) int32, grad_x (b,m,as,6+c).  Where the shape allows: group 0 repeats its
    neighbour 0 at slot as-1, point 1 is drawn by every group (slot 1), and the last point by none."""
    rng = np.random.default_rng(b * 1000003 + n * 1009 + c * 31 + m * 7 + k if seed is None else seed)
    xyz = rng.standard_normal((b, n, 3)).astype(np.float32)
    feature = rng.standard_normal((b, n, c)).astype(np.float32)
    idx = rng.integers(0, max(n - 1, 1), size=(b, m, k)).astype(np.int32)  # never n - 1 (for n > 1)
    if n > 2 and as_ > 2 and m > 0:
        idx[:, :, 1] = 1
        idx[:, 0, as_ - 1] = idx[:, 0, 0]
    gx = rng.standard_normal((b, m, as_, 6 + c)).astype(np.float32)
    return xyz, feature, idx, gx


def gather_forward(xyz, feature, idx, as_):
    """x (b,m,as,6+c) = [xyz[i_s] - xyz[i_0] | xyz[i_s] | feature[i_s]]"""
    bi = np.arange(xyz.shape[0])[:, None, None]
    i = idx[:, :, :as_]
    p, f = xyz[bi, i], feature[bi, i]
    return np.concatenate([p - p[:, :, :1], p, f], axis=-1)


def gather_fold(gx):
    """r[j,s] = [gx[0:3] + gx[3:6] - (s == 0 ? sum_t gx[j,t,0:3] : 0) | gx[6:]] in float64"""
    gx = np.asarray(gx, np.float64)
    r = np.concatenate([gx[..., 0:3] + gx[..., 3:6], gx[..., 6:]], axis=-1)
    r[:, :, 0, 0:3] -= gx[..., 0:3].sum(axis=2)
    return r


def gather_backward(gx, idx, n):
    """-> (grad_xyz (b,n,3), grad_feature (b,n,c)) in float64: the folded rows scattered to their points"""
    b, m, as_, w = gx.shape
    r = gather_fold(gx)
    out = np.zeros((b, n, w - 3), np.float64)
    bi = np.broadcast_to(np.arange(b)[:, None, None], (b, m, as_))
    np.add.at(out, (bi, idx[:, :, :as_]), r)
    return out[..., :3], out[..., 3:]


def gather_tensors(xyz, feature, idx, as_):
    """the gather as differentiable torch ops"""
    import torch

    b, m, _ = idx.shape
    i = torch.as_tensor(np.asarray(idx[:, :, :as_], np.int64)).reshape(b, m * as_)
    take = lambda t: torch.gather(t, 1, i[:, :, None].expand(-1, -1, t.shape[-1])).reshape(b, m, as_, t.shape[-1])
    p, f = take(xyz), take(feature)
    return torch.cat([p - p[:, :, :1], p, f], dim=-1)


def gather_chain(xyz, feature, idx, gx, dtype):
    """-> (x, grad_xyz, grad_feature) by torch's autograd in `dtype`"""
    import torch

    xt = torch.from_numpy(np.asarray(xyz)).to(dtype).requires_grad_()
    ft = torch.from_numpy(np.asarray(feature)).to(dtype).requires_grad_()
    x = gather_tensors(xt, ft, idx, gx.shape[2])
    x.backward(torch.from_numpy(np.asarray(gx)).to(dtype))
    return x.detach().numpy(), xt.grad.numpy(), ft.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# the whole cell
# ---------------------------------------------------------------------------------------------------------------------------
CELL_LAYERS = ("conv_kv_ds", "conv_query_ds", "mlp2_0", "mlp2_1")


def cell_tensors(xyz, feature, idx, as_, layers):
    """AdaptiveSampling + SampleWeights op by op on torch tensors: layers[name] = (W, b), BN folded -> (new_xyz, new_feature)"""
    import torch

    x = gather_tensors(xyz, feature, idx, as_)                       # (b,m,as,6+c)
    b, m = x.shape[:2]
    cb = layers["conv_query_ds"][0].shape[1]
    kv = x @ layers["conv_kv_ds"][0] + layers["conv_kv_ds"][1]
    q = x @ layers["conv_query_ds"][0] + layers["conv_query_ds"][1]
    q, kv = q.reshape(b * m, as_, cb), kv.reshape(b * m, as_, 2 * cb)
    att = torch.softmax(torch.bmm(q, kv[..., :cb].transpose(1, 2)) / (float(cb) ** 0.5), dim=-1)
    att = torch.bmm(att, kv[..., cb:]).reshape(b, m, as_, cb)
    hid = torch.relu(att @ layers["mlp2_0"][0] + layers["mlp2_0"][1])
    logits = hid @ layers["mlp2_1"][0] + layers["mlp2_1"][1]
    w = torch.softmax(logits, dim=2)
    return (w[..., :1] * x[..., 3:6]).sum(dim=2), (w[..., 1:] * x[..., 3:]).sum(dim=2)
