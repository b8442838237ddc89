"""Cases, inputs and the guarded C-ABI call shared by tests/test_gpu_sa_cell_diet.py and tests/golden/make_sa_cell_diet.py (which
recorded tests/golden/sa_cell_diet.npz on the commit BEFORE the cells' load order, wait counts and the placement of their skip-maxima
folds changed: the fixture holds every later build to the bits that commit computed).

A case is (form, b, n, c, m, k, c1, c2, index-table kind).  Inputs come from numpy generators seeded by the case alone, weights
included: nothing here depends on the variable store.  `run` calls pasnl_sa_cell / _centre0 or pasnl_sa_project + pasnl_sa_cell_pre
/ _pre_centre0 with every output in a `Guarded` view, so that a store past a group's (c2 x 32) block or past skip_max is a changed
guard byte."""
import ctypes
import hashlib

import numpy as np
import torch

from guarded import Guarded, output_guard

# (form, b, n, c, m, k, c1, c2, idx kind)
CASES = [
    ("pre", 2, 96, 128, 5, 64, 128, 128, "random"),   # the 128-channel cell: two tiles per group, five chunks of skip columns
    ("pre", 2, 96, 128, 5, 64, 128, 128, "one"),      # every neighbour of a group is one point
    ("pre", 2, 96, 128, 5, 64, 128, 128, "last0"),    # neighbour 0 is the last row of its cloud (the last row of the tables)
    ("pre", 17, 64, 64, 3, 32, 64, 64, "random"),     # 51 groups on 13 workgroups of 4 waves: a ragged last wave
    ("pre", 16, 64, 64, 4, 32, 64, 64, "random"),     # 16 workgroups, 16 clouds: the XCD map (whole clouds per XCD)
    ("pre", 2, 40, 24, 3, 32, 32, 32, "random"),      # a one-chunk row (8 + 24 columns) on the 32-channel cell: one weight batch
    ("pre", 1, 50, 36, 2, 64, 64, 64, "random"),      # two chunks, two blocks: the second block folds the last chunk again
    # more groups than the resident waves (256 workgroups of 4 waves, one per CU): a wave takes a second, third and -- some -- a
    # fourth group, so the index and row requests that cross a group boundary run; the last round is ragged (m <= n: the
    # centre0 entries take their centres from the cloud)
    ("pre", 3, 768, 32, 750, 32, 128, 128, "random"), # 2250 groups, the linear map
    ("pre", 17, 160, 32, 130, 32, 128, 128, "random"), # 2210 groups, the XCD map: 390 groups on 128 waves of XCD 0, 260 elsewhere
    ("xyz3", 3, 1536, 3, 1500, 32, 64, 64, "random"), # 4500 groups on 256 workgroups of 8 waves: two or three groups per wave
    ("xyz3", 2, 40, 3, 7, 32, 64, 64, "random"),      # 14 groups on 2 workgroups of 8 waves: fewer groups than the stride
    ("xyz3", 16, 64, 3, 33, 32, 64, 64, "random"),    # 528 groups on 66 workgroups
    ("xyz3", 16, 64, 3, 4, 32, 64, 64, "random"),     # 8 workgroups, 16 clouds: the XCD map
    ("xyz3", 2, 40, 3, 7, 32, 64, 64, "last0"),
]
# groups of `out` kept in the fixture next to the digest of the whole tensor
KEEP_GROUPS = 2


def case_id(case):
    return "-".join(str(v) for v in case)


def inputs(case):
    form, b, n, c, m, k, c1, c2, kind = case
    rng = np.random.Generator(np.random.PCG64([b, n, c, m, k, c1, len(kind)]))
    v = rng.standard_normal((b, n, 3))
    xyz = (v / np.linalg.norm(v, axis=-1, keepdims=True) * rng.random((b, n, 1)) ** (1 / 3)).astype(np.float32)
    feat = rng.standard_normal((b, n, c)).astype(np.float32)
    idx = rng.integers(0, n, (b, m, k)).astype(np.int32)
    if kind == "one":
        idx[:] = idx[:, :, 5:6]
    elif kind == "last0":
        idx[:, :, 0] = n - 1
    w = 6 + c
    d = {"xyz": xyz, "feat": feat, "idx": idx,
         "w0": (rng.standard_normal((w, c1)) / np.sqrt(w)).astype(np.float32), "b0": (0.1 * rng.standard_normal(c1)).astype(np.float32),
         "w1": (rng.standard_normal((c1, c2)) / np.sqrt(c1)).astype(np.float32), "b1": (0.1 * rng.standard_normal(c2)).astype(np.float32),
         "ww": rng.standard_normal((3, 32)).astype(np.float32), "bw": (0.1 * rng.standard_normal(32)).astype(np.float32)}
    d["centres"] = xyz[np.arange(b)[:, None], idx[:, :, 0]]
    return d


def oracle(case, d):
    """fp64: (b,m,c2,32) cell output, and the float32-exact (b,m,6+c) skip maxima and (b,m,3+c) neighbour-0 rows"""
    from oracle import cells

    b = case[1]
    bi = np.arange(b)[:, None, None]
    gx = d["xyz"][bi, d["idx"]]
    x = np.concatenate([gx - d["centres"][:, :, None, :], gx, d["feat"][bi, d["idx"]]], axis=-1)  # float32, exact
    x64 = x.astype(np.float64)
    h = cells._layer(cells._layer(x64, {"w": d["w0"], "b": d["b0"]}, "relu"), {"w": d["w1"], "b": d["b1"]}, "relu")
    wn = cells._layer(x64[..., :3], {"w": d["ww"], "b": d["bw"]}, "relu")
    nf = np.concatenate([d["centres"], d["feat"][np.arange(b)[:, None], d["idx"][:, :, 0]]], axis=-1)
    return np.swapaxes(h, 2, 3) @ wn, x.max(axis=2), nf


class Run:
    """one launch's outputs (numpy) and whether every guard byte survived"""


def run(case, d, centre0, fill):
    from pointasnl_amd import _hip

    form, b, n, c, m, k, c1, c2, _ = case
    t = {name: torch.from_numpy(np.ascontiguousarray(a)).cuda() for name, a in d.items()}
    p = {name: _hip.ptr(a) for name, a in t.items()}
    g = b * m
    out = Guarded(g * c2 * 32 * 4, fill, output_guard(c2 * 32 * 4))
    skip = Guarded(g * (6 + c) * 4, fill, output_guard((6 + c) * 4))
    cen = Guarded(g * 3 * 4, fill, output_guard(12))
    nf = Guarded(g * (3 + c) * 4, fill, output_guard((3 + c) * 4))
    vp = ctypes.c_void_p
    if form == "pre":
        proj = torch.empty((b, n, c1), dtype=torch.float32, device="cuda")
        _hip.launch("pasnl_sa_project", "sa_project", b, n, c, c1, p["xyz"], p["feat"], p["w0"], p["b0"], _hip.ptr(proj))
        if centre0:
            _hip.launch("pasnl_sa_cell_pre_centre0", "sa_cell_pre", b, n, c, m, k, c1, c2, p["xyz"], p["feat"], _hip.ptr(proj), p["idx"],
                        p["w0"], p["w1"], p["b1"], p["ww"], p["bw"], vp(out.ptr), vp(skip.ptr), vp(cen.ptr), vp(nf.ptr))
        else:
            _hip.launch("pasnl_sa_cell_pre", "sa_cell_pre", b, n, c, m, k, c1, c2, p["xyz"], p["feat"], _hip.ptr(proj), p["idx"],
                        p["centres"], p["w0"], p["w1"], p["b1"], p["ww"], p["bw"], vp(out.ptr), vp(skip.ptr))
    elif centre0:
        _hip.launch("pasnl_sa_cell_centre0", "sa_cell", b, n, c, m, k, c1, c2, p["xyz"], p["feat"], p["idx"], p["w0"], p["b0"], p["w1"],
                    p["b1"], p["ww"], p["bw"], vp(out.ptr), vp(skip.ptr), vp(cen.ptr), vp(nf.ptr))
    else:
        _hip.launch("pasnl_sa_cell", "sa_cell", b, n, c, m, k, c1, c2, p["xyz"], p["feat"], p["idx"], p["centres"], p["w0"], p["b0"],
                    p["w1"], p["b1"], p["ww"], p["bw"], vp(out.ptr), vp(skip.ptr))
    torch.cuda.synchronize()
    r = Run()
    r.out = out.floats((b, m, c2, 32))
    r.skip = skip.floats((b, m, 6 + c))
    r.guards = out.guards_intact() and skip.guards_intact() and cen.guards_intact() and nf.guards_intact()
    if centre0:
        r.cen, r.nf = cen.floats((b, m, 3)), nf.floats((b, m, 3 + c))
    else:
        r.cen = r.nf = None
        r.guards = r.guards and cen.untouched() and nf.untouched()
    return r


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def kept_groups(case):
    g = case[1] * case[4]
    return np.unique(np.linspace(0, g - 1, min(g, KEEP_GROUPS)).astype(np.int64))


def record(case, r, centre0):
    """what the fixture holds of one run: digests of the whole tensors and, of the centre-table form only (the two forms are
    asserted bit-equal), KEEP_GROUPS groups of `out`"""
    form, b, n, c, m, k, c1, c2, _ = case
    rec = {"out_sha256": np.array(digest(r.out)), "skip_sha256": np.array(digest(r.skip))}
    if not centre0:
        rec["out_groups"] = r.out.reshape(b * m, c2, 32)[kept_groups(case)]
    return rec
