"""What tests/test_nl_cell_input_algebra.py and tests/test_gpu_nl_cell_input.py share: seeded problems for
pasnl_cls_nl_cell_input (csrc/nl_input.hip), the fp64 restatement of the cb-wide cell (oracle.cells) and a numpy mirror of the
kernel's own order of operations (fp32, key ranges per wave, blocks of keys, online rescale, merge in ascending wave order)."""
import numpy as np

from oracle import cells

KB = 16        # keys per softmax block (NLI_KB)
MIN_KEYS = 64  # NLI_MIN_ITEMS
LOG2E = np.float32(1.4426950408889634)

_PROBLEMS = {}


def problem(b, p, n, c, cz, cb, seed=0):
    """standard-normal inputs and biases, weights standard-normal / sqrt(fan-in) (float32) -- made once, shared, never changed.
    The weights keep the variance of their input, so keys, values and queries come out at the scale of the standard-normal q
    and kv that tests/test_gpu_cells.py feeds the cb-wide kernel under the same 1e-5: scores of a few units.  (Unscaled
    weights put |score| in the tens, where one fp32 rounding of a score is already a tenth of the bound for ANY kernel.)"""
    key = (b, p, n, c, cz, cb, seed)
    if key not in _PROBLEMS:
        rng = np.random.default_rng([seed, b, p, n, c, cz, cb])
        f = lambda *sh: rng.standard_normal(sh).astype(np.float32)
        h = dict(feature=f(b, n, c), new_point=f(b, p, cz), wkv=f(c, 2 * cb) / np.float32(np.sqrt(c)), bkv=f(2 * cb),
                 wq=f(cz, cb) / np.float32(np.sqrt(cz)), bq=f(cb))
        for v in h.values():
            v.setflags(write=False)
        _PROBLEMS[key] = h
    return _PROBLEMS[key]


def restated(h, cb):
    """the cell before its back-projection as oracle.cells states it, in fp64: softmax(Q K^T / sqrt(cb)) V -> (b,p,cb)"""
    g = {k: v.astype(np.float64) for k, v in h.items()}
    kv = cells._layer(g["feature"], {"w": g["wkv"], "b": g["bkv"]}, None)
    q = cells._layer(g["new_point"], {"w": g["wq"], "b": g["bq"]}, None)
    return cells.nl_attention_core(q, kv, cb)


def split_of(b, p, n, c):
    """waves per workgroup: csrc/nl_input_core.hpp's nli_split, capped as its nli_with_split caps the generic width"""
    tiles = b * ((p + 63) // 64)
    split = 4
    while split < 16 and tiles * split < 2048 and n // (split * 2) >= MIN_KEYS:
        split *= 2
    return min(split, 8) if c != 3 else split


def mirror(h, cb, split, kb=KB):
    """the kernel's arithmetic in numpy, float32 throughout -> (b,p,cb)"""
    f32 = np.float32
    x, z, wkv, bkv, wq, bq = (h[k] for k in ("feature", "new_point", "wkv", "bkv", "wq", "bq"))
    b, n, c = x.shape
    p, cz = z.shape[1], z.shape[2]
    # u = Wk (Z Wq + bq): the bottleneck's columns in groups of four dealt to the waves, partial sums added in wave order
    u = np.zeros((b, p, c), f32)
    for w in range(split):
        part = np.zeros((b, p, c), f32)
        for kg in range(4 * w, cb, 4 * split):
            for k in range(kg, kg + 4):
                qk = np.full((b, p), bq[k], f32)
                for i in range(cz):
                    qk = z[:, :, i] * wq[i, k] + qk
                for ch in range(c):
                    part[:, :, ch] = qk * wkv[ch, k] + part[:, :, ch]
        u = part if w == 0 else u + part
    u = u * f32(LOG2E / np.sqrt(f32(cb)))
    per = ((n + split - 1) // split + kb - 1) // kb * kb
    parts = []
    for w in range(split):
        k0 = min(w * per, n)
        k1 = min(k0 + per, n)
        m = np.full((b, p), -np.inf, f32)
        l = np.zeros((b, p), f32)
        acc = np.zeros((b, p, c), f32)
        for j0 in range(k0, k1, kb):
            xb = x[:, j0:min(j0 + kb, k1)]                      # (b, kb', c)
            s = u[:, :, None, 0] * xb[:, None, :, 0]
            for ch in range(1, c):
                s = u[:, :, None, ch] * xb[:, None, :, ch] + s
            mnew = np.maximum(m, s.max(axis=2))
            with np.errstate(invalid="ignore"):
                alpha = np.where(np.isneginf(m), f32(0), np.exp2(m - mnew)).astype(f32)
            l = l * alpha
            acc = acc * alpha[:, :, None]
            pj = np.exp2(s - mnew[:, :, None]).astype(f32)
            for j in range(pj.shape[2]):
                l = l + pj[:, :, j]
                acc = pj[:, :, j, None] * xb[:, None, j, :] + acc
            m = mnew
        parts.append((m, l, acc))
    m, l, acc = parts[0]
    for mw, lw, aw in parts[1:]:
        mnew = np.maximum(m, mw)
        with np.errstate(invalid="ignore"):
            a0 = np.where(np.isneginf(m), f32(0), np.exp2(m - mnew)).astype(f32)
            a1 = np.where(np.isneginf(mw), f32(0), np.exp2(mw - mnew)).astype(f32)
        l = l * a0 + lw * a1
        acc = acc * a0[:, :, None] + aw * a1[:, :, None]
        m = mnew
    ctr = acc * (f32(1) / l)[:, :, None]
    out = np.broadcast_to(bkv[cb:], (b, p, cb)).astype(f32)
    for ch in range(c):
        out = ctr[:, :, ch, None] * wkv[ch, cb:] + out
    assert out.dtype == np.float32
    return out


def worst_ratio(got, want, tol=1e-5):
    """max over the elements of |got - want| / (tol + tol |want|): <= 1 is numpy.testing.assert_allclose(rtol=atol=tol)"""
    return float((np.abs(got - want) / (tol + tol * np.abs(want))).max())
