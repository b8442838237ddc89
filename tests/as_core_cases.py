"""Cases, inputs and the guarded C-ABI calls shared by tests/test_gpu_as_core_parent_bits.py and tests/golden/make_as_core.py
(which recorded tests/golden/as_core.npz on the commit BEFORE the AdaptiveSampling cell's forward moved out of csrc/cells.hip
into csrc/as_cell.hip and its forward and backward were folded onto csrc/as_core.hpp: the fixture holds every later build to the
bits that commit computed).

Every entry here sums in a fixed order without atomics, so the comparison is equality.  Inputs are seeded by the shape alone
(as_grad_ref's generators where they exist).  Every output and the exact-size workspace sit in `Guarded` views pre-filled with
bytes the caller chooses.  A case is (entry, shape); a runner returns {output name: array}, for the gradient entries only the
outputs of `need` (the others are passed as NULL)."""
import ctypes
import functools
import hashlib

import numpy as np
import torch

import as_grad_ref as R
from guarded import Guarded, output_guard

RW_G, RW_NSAMPLE = 70, 32  # the re-weighting gradients' groups and neighbours (tests/test_gpu_as_grad.py)

CASES = [(entry, shape) for entry, shapes in (
    # (g, as, cb)
    ("as_attention", [(5, 12, 32), (7, 16, 40), (3, 1, 33), (6, 4, 65)]),  # ragged 16-block with a full tile; one key, ragged 4-step
    ("as_attention_qkv", [(5, 12, 32), (7, 16, 40), (3, 1, 33), (6, 4, 65)]),
    # (g, as, cb, w): KS = 2, 3, 4 at CBLK = 2, then at CBLK = 4; more than 2048 workgroups (the persistent stride runs)
    ("as_attention_proj", [(9, 12, 32, 6), (9, 12, 32, 9), (65, 4, 32, 15), (7, 16, 64, 1), (11, 12, 64, 9), (9, 8, 64, 13),
                           (8200, 12, 32, 9)]),
    # (g, as, cb, ch), w = 3 + ch
    ("as_cell_narrow", [(3, 1, 32, 4), (9, 12, 32, 6), (5, 16, 64, 12), (7, 8, 64, 6), (8200, 12, 32, 6)]),
    # (g, as, cb, ch, ld): CBLK = 1; full last block; ragged last block; ld > 3 cb; CBLK = 9; above the 768-workgroup cap
    ("as_cell_wide_ld", [(5, 12, 16, 29, 48), (6, 8, 32, 61, 96), (6, 12, 33, 67, 99), (4, 12, 33, 67, 128), (3, 4, 141, 280, 423),
                         (3, 16, 65, 131, 195), (3080, 12, 33, 67, 99)]),
    # (g, as, nsample, ch)
    ("as_reweight", [(5, 12, 32, 7), (3, 1, 4, 4), (2, 16, 16, 20)]),
    # (g, as, ch)
    ("as_reweight_x", [(5, 12, 6), (2, 16, 131)]),
    # (b, n, c, m, k, as): element form; row form; more than 64 columns
    ("as_gather", [(2, 40, 3, 9, 8, 4), (1, 50, 32, 7, 16, 12), (1, 30, 70, 5, 16, 16)]),
    # the ABI shapes of tests/test_gpu_as_grad.py
    ("as_attention_grad", [(5, 12, 33), (3, 1, 32), (4, 16, 65)]),
    ("as_attention_qkv_grad", [(5, 12, 33), (3, 1, 32), (4, 16, 65)]),
    ("as_reweight_grad", [(12, 6), (16, 131), (1, 4)]),    # (as, ch) at RW_G groups of RW_NSAMPLE
    ("as_reweight_x_grad", [(12, 6), (16, 131), (1, 4)]),
    ("as_gather_grad", [(2, 50, 3, 7, 20, 12), (2, 50, 64, 7, 20, 12), (2, 1, 3, 5, 20, 12)]),
) for shape in shapes]

# the gradient entries' outputs, and the calls that ask for a part of them (the other `NULL` paths)
SUBSETS = {"as_attention_grad": {"q": ("q",), "kv": ("kv",)},
           "as_attention_qkv_grad": {},
           "as_reweight_grad": {"logits": ("logits",), "xyz": ("xyz",), "feature": ("feature",)},
           "as_reweight_x_grad": {"logits": ("logits",), "x": ("x",)},
           "as_gather_grad": {"xyz": ("xyz",), "feature": ("feature",)}}


def case_id(case):
    return case[0] + "-" + "-".join(str(v) for v in case[1])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _ptr(v):
    return ctypes.c_void_p(0 if v is None else v if isinstance(v, int) else v.data_ptr())


class _Outputs:
    """guarded outputs by name: `shapes` = {name: shape}, float32, the guard one row of the last axis"""

    def __init__(self, shapes, fill):
        self.shapes = shapes
        self.views = {k: Guarded(4 * int(np.prod(s)), fill, output_guard(4 * s[-1])) for k, s in shapes.items()}

    def ptr(self, name):
        return _ptr(self.views[name].ptr if name in self.views else None)

    def collect(self, *workspaces):
        torch.cuda.synchronize()
        assert all(v.guards_intact() for v in self.views.values()) and all(w.guards_intact() for w in workspaces)
        return {k: v.floats(self.shapes[k]) for k, v in self.views.items()}


def _call(symbol, *args):
    from pointasnl_amd import _hip

    assert getattr(_hip.lib(), symbol)(*args, _hip.stream_ptr()) == 0, symbol


@functools.lru_cache(maxsize=None)
def cell_problem(g, as_, cb, w, ch=0, ld=0):
    """x (g,as,w), the BN-folded projection wkvq (w,3cb) / bkvq (3cb), mlp2's wa (cb,32), ba (32), wb (32,1+ch), bb (1+ch) and the
    projected rows kvq (g as, ld) of the wide cell, as float32 with unit-variance products"""
    rng = np.random.default_rng([g, as_, cb, w, ch, ld])
    f = lambda scale, *s: (rng.standard_normal(s) * scale).astype(np.float32)
    h = dict(x=f(1.0, g, as_, w), wkvq=f(w ** -0.5, w, 3 * cb), bkvq=f(0.1, 3 * cb), wa=f(cb ** -0.5, cb, 32), ba=f(0.1, 32),
             wb=f(32 ** -0.5, 32, 1 + ch), bb=f(0.1, 1 + ch), kvq=f(1.0, g * as_, max(ld, 1)))
    for a in h.values():
        a.setflags(write=False)
    return h


def reweight_x_rows(h, as_):
    """the x form's rows [centred | X | F[:, :, 3:]] from a re-weighting problem (ch channels = the coordinates and ch - 3 more)"""
    return np.ascontiguousarray(np.concatenate([h["X"][:, :as_] - h["X"][:, :1], h["X"][:, :as_], h["F"][:, :as_, 3:]], axis=-1))


# ---- the forward entries -------------------------------------------------------------------------------------------------
def run_as_attention(shape, fill, ws_fill=None, need=None, packed=False):
    g, as_, cb = shape
    q, kv, _ = R.attention_problem(g, as_, cb)
    o = _Outputs({"out": (g, as_, cb)}, fill)
    if packed:
        kvq = _dev(R.pack_kvq(q, kv))
        _call("pasnl_as_attention_qkv", g, as_, cb, _ptr(kvq), o.ptr("out"))
    else:
        qd, kvd = _dev(q), _dev(kv)
        _call("pasnl_as_attention", g, as_, cb, _ptr(qd), _ptr(kvd), o.ptr("out"))
    return o.collect()


def run_as_attention_qkv(shape, fill, ws_fill=None, need=None):
    return run_as_attention(shape, fill, packed=True)


def run_as_attention_proj(shape, fill, ws_fill=None, need=None):
    g, as_, cb, w = shape
    d = {k: _dev(v) for k, v in cell_problem(g, as_, cb, w).items()}
    o = _Outputs({"out": (g, as_, cb)}, fill)
    _call("pasnl_as_attention_proj", g, as_, cb, w, _ptr(d["x"]), _ptr(d["wkvq"]), _ptr(d["bkvq"]), o.ptr("out"))
    return o.collect()


def run_as_cell_narrow(shape, fill, ws_fill=None, need=None):
    g, as_, cb, ch = shape
    d = {k: _dev(v) for k, v in cell_problem(g, as_, cb, 3 + ch, ch).items()}
    o = _Outputs({"new_feature": (g, ch), "new_xyz": (g, 3)}, fill)
    _call("pasnl_as_cell_narrow", g, as_, cb, 3 + ch, ch, *(_ptr(d[k]) for k in ("x", "wkvq", "bkvq", "wa", "ba", "wb", "bb")),
          o.ptr("new_xyz"), o.ptr("new_feature"))
    return o.collect()


def run_as_cell_wide_ld(shape, fill, ws_fill=None, need=None):
    g, as_, cb, ch, ld = shape
    d = {k: _dev(v) for k, v in cell_problem(g, as_, cb, 3 + ch, ch, ld).items()}
    o = _Outputs({"new_feature": (g, ch), "new_xyz": (g, 3)}, fill)
    _call("pasnl_as_cell_wide_ld", g, as_, cb, 3 + ch, ch, _ptr(d["kvq"]), ld, *(_ptr(d[k]) for k in ("x", "wa", "ba", "wb", "bb")),
          o.ptr("new_xyz"), o.ptr("new_feature"))
    return o.collect()


def run_as_reweight(shape, fill, ws_fill=None, need=None):
    g, as_, nsample, ch = shape
    d = {k: _dev(v) for k, v in R.reweight_problem(g, as_, nsample, ch).items()}
    o = _Outputs({"new_feature": (g, ch), "new_xyz": (g, 3)}, fill)
    _call("pasnl_as_reweight", g, as_, nsample, ch, _ptr(d["logits"]), _ptr(d["X"]), _ptr(d["F"]), o.ptr("new_xyz"), o.ptr("new_feature"))
    return o.collect()


def run_as_reweight_x(shape, fill, ws_fill=None, need=None):
    g, as_, ch = shape
    h = R.reweight_problem(g, as_, as_, ch)
    logits, x = _dev(h["logits"]), _dev(reweight_x_rows(h, as_))
    o = _Outputs({"new_feature": (g, ch), "new_xyz": (g, 3)}, fill)
    _call("pasnl_as_reweight_x", g, as_, ch, _ptr(logits), _ptr(x), o.ptr("new_xyz"), o.ptr("new_feature"))
    return o.collect()


def run_as_gather(shape, fill, ws_fill=None, need=None):
    b, n, c, m, k, as_ = shape
    xyz, feature, idx = (_dev(a) for a in R.gather_problem(*shape)[:3])
    o = _Outputs({"x": (b, m, as_, 6 + c)}, fill)
    _call("pasnl_as_gather", b, n, c, m, k, as_, _ptr(xyz), _ptr(feature), _ptr(idx), o.ptr("x"))
    return o.collect()


# ---- the gradient entries ------------------------------------------------------------------------------------------------
def run_as_attention_grad(shape, fill, ws_fill=None, need=("q", "kv")):
    g, as_, cb = shape
    q, kv, go = (_dev(a) for a in R.attention_problem(g, as_, cb))
    o = _Outputs({k: s for k, s in (("kv", (g, as_, 2 * cb)), ("q", (g, as_, cb))) if k in need}, fill)
    _call("pasnl_cls_as_attention_grad", g, as_, cb, _ptr(q), _ptr(kv), _ptr(go), o.ptr("q"), o.ptr("kv"))
    return o.collect()


def run_as_attention_qkv_grad(shape, fill, ws_fill=None, need=("kvq",)):
    g, as_, cb = shape
    q, kv, go = R.attention_problem(g, as_, cb)
    kvq, god = _dev(R.pack_kvq(q, kv)), _dev(go)
    o = _Outputs({"kvq": (g, as_, 3 * cb)}, fill)
    _call("pasnl_cls_as_attention_qkv_grad", g, as_, cb, _ptr(kvq), _ptr(god), o.ptr("kvq"))
    return o.collect()


def run_as_reweight_grad(shape, fill, ws_fill=None, need=("logits", "xyz", "feature")):
    as_, ch = shape
    d = {k: _dev(v) for k, v in R.reweight_problem(RW_G, as_, RW_NSAMPLE, ch).items()}
    shapes = (("feature", (RW_G, RW_NSAMPLE, ch)), ("logits", (RW_G, as_, 1 + ch)), ("xyz", (RW_G, RW_NSAMPLE, 3)))
    o = _Outputs({k: s for k, s in shapes if k in need}, fill)
    _call("pasnl_cls_as_reweight_grad", RW_G, as_, RW_NSAMPLE, ch, *(_ptr(d[k]) for k in ("logits", "X", "F", "gxyz", "gfeat")),
          o.ptr("logits"), o.ptr("xyz"), o.ptr("feature"))
    return o.collect()


def run_as_reweight_x_grad(shape, fill, ws_fill=None, need=("logits", "x")):
    as_, ch = shape
    h = R.reweight_problem(RW_G, as_, RW_NSAMPLE, ch)
    d = {k: _dev(v) for k, v in h.items()}
    x = _dev(reweight_x_rows(h, as_))
    o = _Outputs({k: s for k, s in (("logits", (RW_G, as_, 1 + ch)), ("x", (RW_G, as_, 3 + ch))) if k in need}, fill)
    _call("pasnl_cls_as_reweight_x_grad", RW_G, as_, ch, _ptr(d["logits"]), _ptr(x), _ptr(d["gxyz"]), _ptr(d["gfeat"]),
          o.ptr("logits"), o.ptr("x"))
    return o.collect()


def run_as_gather_grad(shape, fill, ws_fill, need=("xyz", "feature")):
    from pointasnl_amd import _hip

    b, n, c, m, k, as_ = shape
    _, _, idx, gx = R.gather_problem(*shape)
    idxd, gxd = _dev(idx), _dev(gx)
    nbytes = int(_hip.lib().pasnl_cls_as_gather_grad_workspace_bytes(b, n, c, m, as_))
    ws = Guarded(nbytes, ws_fill)
    o = _Outputs({k_: s for k_, s in (("feature", (b, n, c)), ("xyz", (b, n, 3))) if k_ in need}, fill)
    _call("pasnl_cls_as_gather_grad", b, n, c, m, k, as_, _ptr(gxd), _ptr(idxd), o.ptr("xyz"), o.ptr("feature"), _ptr(ws.ptr),
          ctypes.c_size_t(nbytes))
    return o.collect(ws)


def run(case, fill, ws_fill, need=None):
    """one guarded call of the case's entry -> {output name: float32 array}; `need`: the gradients asked for (default: all)"""
    fn = globals()["run_" + case[0]]
    return fn(case[1], fill, ws_fill) if need is None else fn(case[1], fill, ws_fill, need)


def end_rows(a):
    """the first and the last row of a tensor's last axis as raw words -> (2,w) uint32"""
    flat = np.ascontiguousarray(a).reshape(-1, a.shape[-1])
    return flat[[0, -1]].view(np.uint32)


def record(outs):
    """what the fixture holds of one case: the digests of its outputs in the order of their names, and the end rows of the first"""
    names = sorted(outs)
    return {"sha256": np.array([digest(outs[k]) for k in names], dtype="S64"), "rows": end_rows(outs[names[0]])}
