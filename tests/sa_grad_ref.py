"""The backward of a set-abstraction layer's grouping and local cell in numpy float64: the formulas of include/pasnl.h
(pasnl_cls_sa_local_cell_grad, pasnl_cls_sa_group_grad), written out, plus torch on the CPU differentiating the op-by-op chain
(matmul, relu, transpose, matmul; gather, cat, amax) in a dtype of choice, and the problem generators.  Shared by
tests/test_sa_grad_flow.py (CPU: the formulas equal torch's float64 autograd) and tests/test_gpu_sa_grad.py (GPU: the reference
and the yardstick of the fused kernels).

ReLU kinks and maximum ties make a float64 reference ambiguous, so the generators guarantee, and `relu_margins` / `ties_ok`
let the tests assert:
  (a) every float64 pre-activation of conv0, conv1 and the weight net lies at least MARGIN x that layer's largest
      |pre-activation| away from zero (about 100 x float32's chain error); rows that break it are redrawn -- everything up to M
      is row-wise, so a redraw is local;
  (b) in every group and column the float32 maximum is attained by one element, or only by elements with the same source index
      (the hand-built tie case aside: two different points with bit-equal coordinates and features in one group)."""
import numpy as np

import nl_grad_ref as N

err = N.err  # max |X - X64| / max |X64|

MARGIN = 1e-4
SLOT_CAP = 1024  # include/pasnl.h: min(groups, 1024) partial slots

# (g, k, c, c1): rows are 6 + c wide
# one group; idle waves; a wave takes more than one group and the fold sees every slot; a ragged second chunk, three tiles (three
# launches); w = 70 at 64 channels (three launches) and at 32 (two)
CELL_SHAPES = [(1, 32, 3, 32), (5, 32, 3, 64), (4 * SLOT_CAP + 6, 32, 3, 64), (5, 96, 30, 64), (3, 64, 64, 64), (3, 64, 64, 32)]
CELL_WIDE = (2, 32, 3, 128)  # beyond the fused backward: the op-by-op chain
CELL_FLOW = [(2, 32, 3, 32), (1, 64, 5, 64)]
# (b, n, c, m, k)
GROUP_SHAPES = [(2, 50, 3, 7, 32), (1, 64, 64, 1, 32), (3, 300, 6, 77, 64)]
CELL_NAMES = ("x", "w0", "b0", "w1", "b1", "ww", "bw")


# ---------------------------------------------------------------------------------------------------------------------------
# local cell
# ---------------------------------------------------------------------------------------------------------------------------
def _pre_activations(x, p):
    """float64 (Z1, Z2, Zg), rows flattened"""
    x = x.reshape(-1, x.shape[-1]).astype(np.float64)
    z1 = x @ p["w0"].astype(np.float64) + p["b0"]
    z2 = np.maximum(z1, 0) @ p["w1"].astype(np.float64) + p["b1"]
    zg = x[:, :3] @ p["ww"].astype(np.float64) + p["bw"]
    return z1, z2, zg


def relu_margins(x, p):
    """min |Z| / max |Z| of the three layers' float64 pre-activations: condition (a) is min(...) >= MARGIN"""
    return tuple(float(np.abs(z).min() / np.abs(z).max()) for z in _pre_activations(x, p))


def cell_problem(g, k, c, c1, seed=None):
    """x (g,k,6+c), {w0 (6+c,c1), b0, w1 (c1,c1), b1, ww (3,32), bw}, grad_out (g,c1,32) as float32; condition (a) holds"""
    w = 6 + c
    rng = np.random.default_rng(1000 * c1 + 10 * c + k + g if seed is None else seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    p = {"w0": f(w, c1) / np.float32(np.sqrt(w)), "b0": 0.3 * f(c1), "w1": f(c1, c1) / np.float32(np.sqrt(c1)), "b1": 0.3 * f(c1),
         "ww": f(3, 32) / np.float32(np.sqrt(3)), "bw": 0.3 * f(32)}
    x = f(g, k, w)
    flat = x.reshape(-1, w)
    for _ in range(200):
        zs = _pre_activations(x, p)
        bad = np.zeros(flat.shape[0], dtype=bool)
        for z in zs:
            bad |= (np.abs(z) < 2 * MARGIN * np.abs(z).max()).any(axis=1)  # (2 x: the maxima move a little with the redraws)
        if not bad.any():
            break
        flat[bad] = f(int(bad.sum()), w)
    assert min(relu_margins(x, p)) >= MARGIN
    return x, p, f(g, c1, 32)


def cell_forward(x, p):
    """M (g,c2,32) = H2^T G in float64"""
    g, k, w = x.shape
    z1, z2, zg = _pre_activations(x, p)
    h2 = np.maximum(z2, 0).reshape(g, k, -1)
    return np.einsum("gkc,gkj->gcj", h2, np.maximum(zg, 0).reshape(g, k, 32))


def cell_backward(x, p, gout):
    """the header's formulas -> {x, w0, b0, w1, b1, ww, bw} gradients in float64"""
    g, k, w = x.shape
    x64 = x.reshape(-1, w).astype(np.float64)
    z1, z2, zg = _pre_activations(x, p)
    h1, h2, gg = np.maximum(z1, 0), np.maximum(z2, 0), np.maximum(zg, 0)
    dm = gout.astype(np.float64)                                            # (g, c2, 32)
    dh2 = np.einsum("gkj,gcj->gkc", gg.reshape(g, k, 32), dm).reshape(g * k, -1)  # G dM^T
    dg = np.einsum("gkc,gcj->gkj", h2.reshape(g, k, -1), dm).reshape(g * k, 32)   # H2 dM
    dz2 = dh2 * (z2 > 0)
    dzg = dg * (zg > 0)
    dh1 = dz2 @ p["w1"].astype(np.float64).T
    dz1 = dh1 * (z1 > 0)
    dx = dz1 @ p["w0"].astype(np.float64).T
    dx[:, :3] += dzg @ p["ww"].astype(np.float64).T
    return {"x": dx.reshape(g, k, w), "w0": x64.T @ dz1, "b0": dz1.sum(0), "w1": h1.T @ dz2, "b1": dz2.sum(0),
            "ww": x64[:, :3].T @ dzg, "bw": dzg.sum(0)}


def cell_tensors(x, p):
    """the op-by-op chain (pointasnl_util.py:264-274) on torch tensors"""
    import torch

    h2 = torch.relu(torch.relu(x @ p["w0"] + p["b0"]) @ p["w1"] + p["b1"])
    return h2.transpose(1, 2) @ torch.relu(x[..., 0:3] @ p["ww"] + p["bw"])


def cell_chain(x, p, gout, dtype):
    """torch autograd of the chain on the CPU in `dtype` -> (M, {gradients})"""
    import torch

    leaves = {"x": torch.from_numpy(x).to(dtype).requires_grad_()}
    leaves.update({k_: torch.from_numpy(v).to(dtype).requires_grad_() for k_, v in p.items()})
    out = cell_tensors(leaves["x"], leaves)
    out.backward(torch.from_numpy(gout).to(dtype))
    return out.detach().numpy(), {k_: v.grad.numpy() for k_, v in leaves.items()}


# ---------------------------------------------------------------------------------------------------------------------------
# grouping
# ---------------------------------------------------------------------------------------------------------------------------
def group_forward(xyz, feature, idx, new_xyz):
    """new_point (b,m,k,6+c), skip (b,m,6+c) in the inputs' dtype: gathers, one subtraction, a maximum"""
    b = np.arange(xyz.shape[0])[:, None, None]
    gx = xyz[b, idx]
    new_point = np.concatenate([gx - new_xyz[:, :, None, :], gx, feature[b, idx]], axis=-1)
    return new_point, new_point.max(axis=2)


def ties_ok(xyz, feature, idx, new_xyz):
    """condition (b) on the float32 forward: a column's maximum is attained by elements of one source index only"""
    new_point, skip = group_forward(xyz, feature, idx, new_xyz)
    at_max = new_point == skip[:, :, None, :]                                   # (b, m, k, W)
    src = np.broadcast_to(idx[..., None], at_max.shape)
    lo = np.where(at_max, src, np.iinfo(np.int32).max).min(axis=2)
    hi = np.where(at_max, src, -1).max(axis=2)
    return bool((lo == hi).all())


def group_problem(b, n, c, m, k, seed=None):
    """xyz (b,n,3), feature (b,n,c), idx (b,m,k), new_xyz (b,m,3), grad_new_point (b,m,k,6+c), grad_skip (b,m,6+c).
    Group 0 of every cloud draws its neighbour 0 twice (padded crops do); point n - 1 is drawn by no group; (b) holds."""
    for attempt in range(20):
        rng = np.random.default_rng((100 * n + 10 * c + m if seed is None else seed) + 7919 * attempt)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        xyz, feature, new_xyz = f(b, n, 3), f(b, n, c), f(b, m, 3)
        idx = rng.integers(0, max(n - 1, 1), size=(b, m, k)).astype(np.int32)
        idx[:, 0, k - 1] = idx[:, 0, 0]
        if ties_ok(xyz, feature, idx, new_xyz):
            return xyz, feature, idx, new_xyz, f(b, m, k, 6 + c), f(b, m, 6 + c)
    raise AssertionError("no tie-free problem")


def group_tie_problem():
    """one cloud, one group of 32 among 40 points: points 3 and 7 are DIFFERENT points with bit-equal coordinates and features,
    both in the group, and the maximum of every column -- the equal-shares rule gives each half of grad_skip"""
    b, n, c, m, k = 1, 40, 4, 1, 32
    rng = np.random.default_rng(77)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    xyz, feature, new_xyz = f(b, n, 3), f(b, n, c), f(b, m, 3)
    xyz[0, 3] = xyz[0, 7] = np.float32(9.0) + np.abs(xyz[0, 3])
    feature[0, 3] = feature[0, 7] = np.float32(9.0) + np.abs(feature[0, 3])
    idx = rng.permutation(n - 1)[:k].astype(np.int32)
    idx[5], idx[20] = 3, 7
    others = [i for i in range(n - 1) if i not in (3, 7)]
    for pos in range(k):
        if pos not in (5, 20) and idx[pos] in (3, 7):
            idx[pos] = others[pos]
    idx = idx.reshape(b, m, k)
    assert (idx == 3).sum() == 1 and (idx == 7).sum() == 1 and not ties_ok(xyz, feature, idx, new_xyz)
    return xyz, feature, idx, new_xyz, f(b, m, k, 6 + c), f(b, m, 6 + c)


def group_backward(xyz, feature, idx, new_xyz, gnp, gskip):
    """the header's formulas in float64 -> (grad_xyz, grad_feature, grad_new_xyz); the maximum's mask is taken on the forward's own
    float32 values"""
    b, n, c = feature.shape
    _, m, k = idx.shape
    new_point, skip = group_forward(xyz, feature, idx, new_xyz)  # float32
    mask = new_point == skip[:, :, None, :]
    count = mask.sum(axis=2, keepdims=True)
    e = np.zeros(mask.shape, dtype=np.float64)
    if gnp is not None:
        e += gnp.astype(np.float64)
    if gskip is not None:
        e += mask * (gskip.astype(np.float64)[:, :, None, :] / count)
    r_xyz = e[..., 0:3] + e[..., 3:6]
    grad_new_xyz = -e[..., 0:3].sum(axis=2)
    grad_xyz, grad_feature = np.zeros((b, n, 3)), np.zeros((b, n, c))
    bi = np.broadcast_to(np.arange(b)[:, None, None], idx.shape)
    np.add.at(grad_xyz, (bi, idx), r_xyz)
    np.add.at(grad_feature, (bi, idx), e[..., 6:])
    return grad_xyz, grad_feature, grad_new_xyz


def group_tensors(xyz, feature, idx, new_xyz):
    """gather, cat, amax on torch tensors -> new_point, skip"""
    import torch

    b = torch.arange(xyz.shape[0])[:, None, None]
    ix = torch.as_tensor(idx, dtype=torch.int64)
    gx = xyz[b, ix]
    new_point = torch.cat([gx - new_xyz[:, :, None, :], gx, feature[b, ix]], dim=-1)
    return new_point, new_point.amax(dim=2)


def group_chain(xyz, feature, idx, new_xyz, gnp, gskip, dtype):
    """torch autograd of the chain on the CPU in `dtype` -> (new_point, skip, (grad_xyz, grad_feature, grad_new_xyz))"""
    import torch

    leaves = [torch.from_numpy(a).to(dtype).requires_grad_() for a in (xyz, feature, new_xyz)]
    new_point, skip = group_tensors(leaves[0], leaves[1], idx, leaves[2])
    torch.autograd.backward([new_point, skip], [torch.from_numpy(gnp).to(dtype), torch.from_numpy(gskip).to(dtype)])
    return new_point.detach().numpy(), skip.detach().numpy(), tuple(t.grad.numpy() for t in leaves)
