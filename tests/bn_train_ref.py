"""Host restatement of csrc/bn_train.hip (include/pasnl.h: pasnl_cls_bn_train, pasnl_cls_bn_train_grad, pasnl_cls_dropout): the
header's formulas in float64 numpy -- forward, moving update, backward --, the dropout mask restated with
tests/philox_ref.philox4x32_10, the torch chain the GPU tests take their yardstick from, the problem generators and the case list.

The kernels' widths (csrc/bn_train.hip), which every case names what it is ragged against:
    VW           4    floats per 16-byte access (c % 4 == 0 and aligned pointers), else 1
    MAX_LX      64    lanes along the channel axis: a channel tile is 64 * VW columns at most (256 vector, 64 scalar)
    SMALL_ROWS 128    up to here a call is one launch, its channel tile SMALL_LX * VW = 8 * VW columns
    SLAB_ROWS  256    rows per partial-sum workgroup at least; MAX_BLOCKS 2048 of them at most
"""
import numpy as np
import torch

import philox_ref

EPS = 1e-3
VW, MAX_LX, SMALL_ROWS, SMALL_LX, SLAB_ROWS, MAX_BLOCKS = 4, 64, 128, 8, 256, 2048
MARGIN = 1e-3  # no pre-activation of a ReLU case lies closer to 0: the float32 mask is the float64 one
CUS = 256


def slabs(rows, c):
    return min(-(-rows // SLAB_ROWS), max(1, MAX_BLOCKS // -(-c // (MAX_LX * VW))))


def workspace_bytes(rows, c):
    """the header's formula"""
    return 0 if rows <= 0 or c <= 0 else 16 * c * slabs(rows, c)


def err(got, want):
    """max |X - X64| / max |X64| (tests/test_gpu_sa_grad.py's measure)"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ---- the header's formulas
def forward(x, gamma, beta, act, eps=EPS):
    """-> y, mean, var (biased), rstd, all float64"""
    x, gamma, beta = (np.asarray(a, np.float64) for a in (x, gamma, beta))
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    rstd = 1.0 / np.sqrt(var + eps)
    z = (x - mean) * rstd * gamma + beta
    return (np.maximum(z, 0.0) if act else z), mean, var, rstd


def batch_variance(var, rows, unbiased):
    return var * rows / max(rows - 1, 1) if unbiased else var


def moving(m, batch, decay):
    """assign_moving_average(zero_debias=False), decay as the float32 the entry receives"""
    m = np.asarray(m, np.float64)
    return m - (m - batch) * (1.0 - float(np.float32(decay)))


def backward(x, gamma, beta, act, grad_y, eps=EPS):
    """grad_x, grad_gamma, grad_beta (float64) of y = act(gamma xhat + beta): g = grad_y [y > 0] when act"""
    x, gamma, gy = (np.asarray(a, np.float64) for a in (x, gamma, grad_y))
    rows = x.shape[0]
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (x - mean) * rstd
    g = gy * ((xh * gamma + np.asarray(beta, np.float64)) > 0) if act else gy
    grad_beta = g.sum(axis=0)
    grad_gamma = (g * xh).sum(axis=0)
    grad_x = gamma * rstd * (g - grad_beta / rows - xh * grad_gamma / rows)
    return grad_x, grad_gamma, grad_beta


def chain(x, gamma, beta, act, grad_y, dtype, eps=EPS):
    """the formula on torch's CPU ops in `dtype` -- centred mean / var / normalise --, differentiated by torch
    -> dict(y, mean, rstd, var, grad_x, grad_gamma, grad_beta) of numpy arrays"""
    t = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in (x, gamma, beta)]
    mean = t[0].mean(dim=0)
    var = ((t[0] - mean) ** 2).mean(dim=0)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (t[0] - mean) * rstd * t[1] + t[2]
    y = torch.relu(z) if act else z
    y.backward(torch.tensor(np.asarray(grad_y), dtype=dtype))
    out = dict(y=y, mean=mean, rstd=rstd, var=var, grad_x=t[0].grad, grad_gamma=t[1].grad, grad_beta=t[2].grad)
    return {k: v.detach().numpy() for k, v in out.items()}


# ---- problems
def relu_margin(x, gamma, beta):
    """the smallest |pre-activation| in float64"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=0)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=0) + EPS)
    return float(np.abs((x - mean) * rstd * gamma + beta).min())


def problem(rows, c, act, offset=False, seed=0):
    """float32 x (rows,c), gamma, beta, moving_mean, moving_var (c), grad_y (rows,c).  offset: columns with mean 8 and standard
    deviation 0.25 (a float32 E[x^2] - mean^2 loses the variance there); else per-column means in [-1,1] and deviations in
    [0.5,2].  With act, elements whose pre-activation lies within 2 MARGIN of 0 are pushed away from it."""
    rng = np.random.default_rng([seed, rows, c, int(act), int(offset)])
    if offset:
        mu, sd = np.full(c, 8.0), np.full(c, 0.25)
    else:
        mu, sd = rng.uniform(-1, 1, c), rng.uniform(0.5, 2.0, c)
    x = (mu + sd * rng.standard_normal((rows, c))).astype(np.float32)
    gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    beta = (rng.uniform(0.05, 0.2, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)
    mm = rng.uniform(-0.5, 0.5, c).astype(np.float32)
    mv = rng.uniform(0.5, 1.5, c).astype(np.float32)
    gy = rng.standard_normal((rows, c)).astype(np.float32)
    if act:
        for _ in range(8):
            x64 = x.astype(np.float64)
            mean = x64.mean(axis=0)
            rstd = 1.0 / np.sqrt(((x64 - mean) ** 2).mean(axis=0) + EPS)
            z = (x64 - mean) * rstd * gamma + beta
            near = np.abs(z) < 2 * MARGIN
            if not near.any():
                break
            step = 6 * MARGIN / (np.abs(gamma.astype(np.float64)) * rstd)  # moves z by 6 MARGIN (less the shift of the mean)
            x = np.where(near, x64 + np.sign(z + (z == 0)) * np.sign(gamma) * step, x64).astype(np.float32)
    return x, gamma, beta, mm, mv, gy


# (rows, c, act, offset, ragged against) -- every dispatch branch: one launch / three launches x vector / scalar; one and several
# channel tiles; one and several slabs; more than one partial per CU at c = 4
CASES = [
    (1, 4, 1, False, "rows == 1 (variance 0, the unbiased guard); one launch, vector"),
    (1, 129, 0, False, "rows == 1; one launch, scalar, 17 tiles of SMALL_LX"),
    (2, 5, 1, False, "one launch, scalar, c < SMALL_LX"),
    (2, 64, 0, False, "one launch, vector, 2 tiles of SMALL_LX * VW"),
    (127, 33, 1, False, "one launch, scalar, rows ragged against the 32 rows of a step, c against SMALL_LX"),
    (127, 64, 1, False, "one launch, vector"),
    (128, 260, 0, False, "SMALL_ROWS itself; vector, 9 tiles, the last one ragged"),
    (129, 4, 1, False, "SMALL_ROWS + 1: three launches, one slab, lx = 1"),
    (513, 64, 0, False, "3 slabs, the last of 1 row; vector lx = 16"),
    (4099, 1, 0, False, "c = 1: scalar, lx = 1, 17 slabs"),
    (4099, 4, 1, False, "vector lx = 1"),
    (4099, 5, 0, False, "scalar, c ragged against lx = 8"),
    (4099, 129, 1, False, "scalar, 3 channel tiles of MAX_LX, the last of one column"),
    (4099, 260, 1, False, "vector, 2 channel tiles of MAX_LX * VW, the last of 4 columns"),
    (70001, 4, 1, False, "274 slabs: more than one partial per CU at c = 4, and more than a wave of slabs per column"),
    (4099, 33, 0, True, "offset columns, scalar"),
    (300, 64, 1, True, "offset columns, vector, with the ReLU mask"),
    (100, 32, 1, True, "offset columns, one launch"),
]


def case_id(case):
    rows, c, act, offset, _ = case
    return f"{rows}x{c}-act{act}" + ("-offset" if offset else "")


# ---- dropout
def dropout_keep(n, keep_prob, seed, stream_id, call):
    """bool (n,): element i is kept iff uniform(word i & 3 of the block at counter (i >> 2 lo, i >> 2 hi, call, stream_id)) <
    float32(keep_prob), key (seed lo, seed hi)"""
    blocks = (n + 3) // 4
    blk = np.arange(blocks, dtype=np.uint64)
    ctr = np.empty((blocks, 4), np.uint32)
    ctr[:, 0], ctr[:, 1] = (blk & np.uint64(0xFFFFFFFF)).astype(np.uint32), (blk >> np.uint64(32)).astype(np.uint32)
    ctr[:, 2], ctr[:, 3] = np.uint32(call & 0xFFFFFFFF), np.uint32(stream_id & 0xFFFFFFFF)
    words = philox_ref.philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    return (philox_ref.uniform(words).reshape(-1)[:n] < np.float32(keep_prob))


def dropout(x, keep_prob, seed, stream_id, call):
    x = np.asarray(x, np.float32)
    keep = dropout_keep(x.size, keep_prob, seed, stream_id, call).reshape(x.shape)
    return np.where(keep, x / np.float32(keep_prob), np.float32(0)).astype(np.float32)
