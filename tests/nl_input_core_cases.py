"""Shapes, inputs and the guarded C-ABI calls shared by tests/test_gpu_nl_input_parent_bits.py and
tests/golden/make_nl_input_core.py (which recorded tests/golden/nl_input_core.npz on the commit BEFORE the forward and the backward
of the input-space non-local cell were folded onto csrc/nl_input_core.hpp: the fixture holds every later build to the bits that
commit computed).

Both entry points (pasnl_cls_nl_cell_input, pasnl_cls_nl_cell_input_grad) sum in a fixed order without atomics, so the comparison
is equality.  Inputs are nl_cell_input_grad_ref.problem's, seeded by the shape alone.  Every output and the exact-size workspace
sit in `Guarded` views pre-filled with bytes the caller chooses."""
import ctypes
import hashlib

import numpy as np
import torch

import nl_cell_input_grad_ref as R
from guarded import Guarded, output_guard

# (b, p, n, c, cz, cb): the shapes of tests/test_gpu_nl_cell_input.py and tests/test_gpu_nl_cell_input_grad.py
SHAPES = [(2, 70, 45, 3, 6, 32),       # ragged, fewer keys than a block
          (1, 1, 1, 3, 6, 32),
          (3, 130, 333, 3, 6, 32),     # three query tiles, uneven key ranges
          (1, 64, 3, 3, 6, 32),        # fewer keys than waves
          (2, 33, 77, 6, 9, 64),
          (1, 40, 200, 8, 16, 128),
          (1, 64, 600, 3, 6, 32),      # 8 waves
          (1, 70, 4500, 3, 6, 32),     # 16 waves, a ragged second chunk
          (512, 1, 1100, 3, 6, 32),    # one query per tile, 512 partial moments
          (1, 10, 2100, 5, 7, 64)]     # the generic width
ABI_SHAPES = [(2, 70, 45, 3, 6, 32), (1, 40, 200, 8, 16, 128)]
# the calls that take the other `flags` paths of the backward: the gradients asked for, the rest NULL
SUBSETS = {"weights": ("wkv", "bkv", "wq", "bq"), "feature": ("feature",), "new_point": ("new_point",)}


def shape_id(shape):
    return "-".join(str(v) for v in shape)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()  # (the cached problems are read-only)


def _ptr(v):
    return ctypes.c_void_p(0 if v is None else v if isinstance(v, int) else v.data_ptr())


def run_forward(shape, h, fill):
    """pasnl_cls_nl_cell_input into a guarded view pre-filled with `fill` -> (b,p,cb) float32"""
    from pointasnl_amd import _hip

    b, p, _, _, _, cb = shape
    ins = [_dev(h[k]) for k in R.NAMES]
    out = Guarded(4 * b * p * cb, fill, output_guard(4 * cb))
    assert _hip.lib().pasnl_cls_nl_cell_input(*shape, *(_ptr(t) for t in ins), _ptr(out.ptr), _hip.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.floats((b, p, cb))


def run_grad(shape, h, g, need, fill, ws_fill):
    """one call of pasnl_cls_nl_cell_input_grad with the gradients of `need` requested (the others NULL), outputs and the
    exact-size workspace in guarded views pre-filled with `fill` / `ws_fill` -> {name: float32 array}"""
    from pointasnl_amd import _hip

    lib = _hip.lib()
    ins, gd = [_dev(h[k]) for k in R.NAMES], _dev(g)
    nbytes = int(lib.pasnl_cls_nl_cell_input_grad_workspace_bytes(*shape))
    ws = Guarded(nbytes, ws_fill)
    grads = {k: Guarded(4 * h[k].size, fill, output_guard(4 * h[k].shape[-1])) for k in need}
    status = lib.pasnl_cls_nl_cell_input_grad(*shape, *(_ptr(t) for t in ins), _ptr(gd),
                                              *(_ptr(grads[k].ptr if k in grads else None) for k in R.NAMES), _ptr(ws.ptr),
                                              ctypes.c_size_t(nbytes), _hip.stream_ptr())
    torch.cuda.synchronize()
    assert status == 0
    assert ws.guards_intact() and all(v.guards_intact() for v in grads.values())
    return {k: v.floats(h[k].shape) for k, v in grads.items()}


def end_rows(a):
    """the first and the last query row of a (b,p,w) tensor as raw words -> (2,w) uint32"""
    flat = np.ascontiguousarray(a).reshape(-1, a.shape[-1])
    return flat[[0, -1]].view(np.uint32)


def record(out, full, subsets):
    """what the fixture holds of one shape: the digest of the forward's output and of each of the six gradients of the full
    call, the end rows of `out` and grad_new_point, and the digests of what each subset call computed"""
    rec = {"out_sha256": np.array(digest(out)), "out_rows": end_rows(out), "grad_new_point_rows": end_rows(full["new_point"])}
    for k in R.NAMES:
        rec[f"grad_{k}_sha256"] = np.array(digest(full[k]))
    for name, got in subsets.items():
        for k, a in got.items():
            rec[f"{name}/grad_{k}_sha256"] = np.array(digest(a))
    return rec
