"""GPU: the crop's radix selection (csrc/crop.hip) and the LDS sort behind it (csrc/test_loop.hpp: op_sort) where lidar-like
scans never take them -- a selection decided in each of the later passes among many bins, pass-0 boundary bins on the seams of
cr_find_bin, the tie cut at chosen places inside a thread's items, across waves and across blocks, done and live crops in one
launch, radii that underflow and overflow, scan_stride > n, non-finite keys (a NaN with the sign bit set among them), the
descriptor entries with three scans in one launch, and the sort at every small count, around the powers of two and at its
capacity.  tests/crop_select_cases.py builds the inputs and tests/test_crop_select_cases.py shows on the CPU that each is where it
claims to be and that a wrong selection would change it.

Everything is compared bit for bit with the oracle: indices, counts and the uint64 view of d2; outputs are pre-filled and live
inside guarded buffers, workspaces are exactly the size the header states."""
import ctypes

import numpy as np
import pytest
import torch

import crop_select_cases as E
from guarded import ALT_WS_BYTE, NAN_BYTE, WS_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu

IDX_SENTINEL = np.int32(-1)                        # four NAN_BYTEs
D2_SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)        # eight of them


@pytest.fixture(scope="module")
def G():
    from pointasnl_amd.SemanticKITTI import semantic_kitti_dataset_grid as G

    return G


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return ctypes.c_void_p(t if isinstance(t, int) else 0 if t is None else t.data_ptr())


def launch(symbol, *args):
    from pointasnl_amd import _hip

    _hip.launch(symbol, "test_gpu_crop_select", *args)


def crop_workspace_bytes(b, n):
    from pointasnl_amd import _hip

    return int(_hip.lib().pasnl_knn_crop_workspace_bytes(int(b), ctypes.c_long(int(n))))


class CropOut:
    """out_idx (b,kcap), out_d2 (b,kcap) and out_count (b) of a crop entry, pre-filled, and a workspace of exactly
    pasnl_knn_crop_workspace_bytes(b, n) bytes: all inside guarded buffers"""

    def __init__(self, b, n, kcap, ws_fill=WS_BYTE):
        self.b, self.kcap = b, kcap
        self.idx = Guarded(4 * b * kcap, NAN_BYTE, output_guard(4 * kcap))
        self.d2 = Guarded(8 * b * kcap, NAN_BYTE, output_guard(8 * kcap))
        self.cnt = Guarded(4 * b, NAN_BYTE)
        self.ws_bytes = crop_workspace_bytes(b, n)
        self.ws = Guarded(self.ws_bytes, ws_fill)

    def args(self):
        return ptr(self.idx.ptr), ptr(self.d2.ptr), ptr(self.cnt.ptr), ptr(self.ws.ptr), ctypes.c_size_t(self.ws_bytes)

    def read(self):
        torch.cuda.synchronize()
        assert self.idx.guards_intact() and self.d2.guards_intact() and self.cnt.guards_intact() and self.ws.guards_intact()
        return (self.idx.array((self.b, self.kcap), np.int32), self.d2.array((self.b, self.kcap), np.uint64),
                self.cnt.array((self.b,), np.int32))


def check_row(idx, d2, cnt, want, what):
    """one crop against (ascending indices, key bits): the count, the entries in front of it, the sentinel behind it"""
    sel, bits = want
    assert cnt == len(sel), (what, int(cnt), len(sel))
    m = min(len(sel), len(idx))
    np.testing.assert_array_equal(idx[:m], sel[:m], err_msg=str(what))
    np.testing.assert_array_equal(d2[:m], bits[:m], err_msg=str(what))
    assert (idx[m:] == IDX_SENTINEL).all() and (d2[m:] == D2_SENTINEL).all(), what


def run_direct(case):
    """one call of pasnl_knn_crop, n, scan_stride and the radius passed as the case states them"""
    out = CropOut(case["b"], case["n"], case["kcap"])
    pts, cen = dev(case["points"]), dev(case["centres"])
    kd = dev(np.array(case["ks"], np.int32)) if case["ks"] is not None else None
    launch("pasnl_knn_crop", case["b"], ctypes.c_long(case["n"]), ctypes.c_long(case["stride"]), ptr(pts), ptr(cen), ptr(kd),
           case["kcap"], ctypes.c_double(case["radius"]), *out.args())
    return out.read()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the direct form
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.DIRECT))
def test_direct_form(G, name):
    """Every direct-form case through the C ABI into pre-filled outputs: indices, d2 bits and count are the oracle's, nothing is
    written behind the count.  Where the mirror's wrapper can state the call (no stride of its own), select_batch gives the same."""
    case = E.DIRECT[name]()
    idx, d2, cnt = run_direct(case)
    for c in range(case["b"]):
        check_row(idx[c], d2[c], cnt[c], E.want(case, c), (name, c, case["claims"][c].get("variant")))
    if case["stride"] == 0:
        kd = dev(np.array(case["ks"], np.int32)) if case["ks"] is not None else None
        sidx, sd2, scnt = G.select_batch(dev(case["points"]), dev(case["centres"]), k=kd, kcap=case["kcap"], radius=case["radius"],
                                         want_d2=True)
        sidx, sd2, scnt = sidx.cpu().numpy(), sd2.cpu().numpy().view(np.uint64), scnt.cpu().numpy()
        np.testing.assert_array_equal(scnt, cnt)
        for c in range(case["b"]):
            np.testing.assert_array_equal(sidx[c, :cnt[c]], idx[c, :cnt[c]])
            np.testing.assert_array_equal(sd2[c, :cnt[c]], d2[c, :cnt[c]])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the descriptor entries: three scans in one launch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,layout", [("pasnl_knn_crop_indirect", "scan_desc"), ("pasnl_knn_crop_scene", "scene_desc")])
def test_desc_multi(entry, layout):
    """b = 3 descriptors (k = 0 on 700 points, k >= n on 2048, a live k decided in pass 3 on 5000) in ONE launch: guards intact,
    rows behind each count untouched, the oracle's results, the bits of pasnl_knn_crop on the same scan, centre and k -- and
    the same again over a workspace that held other bytes."""
    case = E.desc_multi()
    pts, desc = dev(case["points"]), dev(case[layout].view(np.uint8))
    runs = []
    for fill in (WS_BYTE, ALT_WS_BYTE):
        out = CropOut(3, case["nmax"], case["kcap"], fill)
        launch(entry, 3, ctypes.c_long(case["nmax"]), ptr(pts), ptr(desc), case["kcap"], *out.args())
        idx, d2, cnt = out.read()
        for c in range(3):
            check_row(idx[c], d2[c], cnt[c], E.want_desc(case, c), (entry, c, fill))
        runs.append((idx, d2, cnt))
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    idx, d2, cnt = runs[0]
    assert cnt.tolist() == [0, 2048, case["ks"][2]]
    for c in range(3):
        lo = int(case["offsets"][c])
        one = E.direct("one", case["points"][lo:lo + case["ns"][c]], case["centres"][c], [case["ks"][c]], kcap=case["kcap"])
        oidx, od2, ocnt = run_direct(one)
        np.testing.assert_array_equal(ocnt[0], cnt[c])
        np.testing.assert_array_equal(oidx[0], idx[c])
        np.testing.assert_array_equal(od2[0], d2[c])


def test_fused_pick_is_pick_then_crop():
    """pasnl_scene_pick_crop on the scene that holds the ring (the pick's point plus the noise is the origin, so the crop is
    decided in pass 3): the descriptor, indices, d2 and count of pasnl_scene_pick followed by pasnl_knn_crop_scene."""
    case = E.desc_multi()
    rng = np.random.default_rng(8100)
    total, pick, lo = len(case["points"]), 1234, int(case["offsets"][2])
    pot = 1.0 + rng.random(total)
    pot[lo + pick] = 0.5
    min_pot = np.array([pot[case["offsets"][i]:case["offsets"][i + 1]].min() for i in range(3)])
    assert int(np.argmin(min_pot)) == 2 and int(np.argmin(pot[lo:])) == pick
    noise = -case["points"][lo + pick].astype(np.float64)
    pts, off, potd, mind = dev(case["points"]), dev(case["offsets"]), dev(pot), dev(min_pot)
    kd, nd = dev(np.array([case["ks"][2]], np.int32)), dev(noise)
    nmax, kcap = case["nmax"], case["kcap"]
    got = []
    for fused in (False, True):
        desc, cloud = Guarded(E.SCENE_DESC.itemsize, NAN_BYTE), Guarded(4, NAN_BYTE)
        out = CropOut(1, nmax, kcap)
        head = (3, ptr(off), ptr(potd), ptr(mind), ptr(pts), ptr(kd), ptr(nd), ptr(desc.ptr), ptr(cloud.ptr))
        if fused:
            launch("pasnl_scene_pick_crop", *head, ctypes.c_long(nmax), kcap, *out.args())
        else:
            launch("pasnl_scene_pick", *head)
            launch("pasnl_knn_crop_scene", 1, ctypes.c_long(nmax), ptr(pts), ptr(desc.ptr), kcap, *out.args())
        idx, d2, cnt = out.read()
        assert desc.guards_intact() and cloud.guards_intact()
        check_row(idx[0], d2[0], cnt[0], E.want_desc(case, 2), ("fused" if fused else "pick, crop"))
        got.append((desc.array((1,), E.SCENE_DESC), cloud.array((1,), np.int32), idx, d2, cnt))
    d = got[0][0][0]
    assert (d["offset"], d["cloud"], d["pick"], d["n"], d["k"]) == (lo, 2, pick, 5000, case["ks"][2]) and got[0][1][0] == 2
    assert np.array([d["cx"], d["cy"], d["cz"]]).view(np.uint64).tolist() == [0, 0, 0]
    assert got[0][0].tobytes() == got[1][0].tobytes()
    for a, b in zip(got[0][1:], got[1][1:]):
        np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. op_sort
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", range(len(E.sort_groups())))
def test_sort_sweep(g):
    """Launch g of the sweep through pasnl_crop_order_permute and pasnl_scene_order_gather (nfeat = 0, abs_coords off and on):
    out_select[c][j] = idx[c][order[perm[c][j]]] with order the full sort by (d2 bits, position); out_points / out_input the rows
    the header states.  Up to 64 crops of different counts share a launch and a kcap; the capacity, 14336, has its own."""
    case = E.sort_group(g)
    b, kcap, ms = case["b"], case["kcap"], case["ms"]
    assert b <= 64 and kcap == max(ms) <= E.OP_CAP and (g < len(E.sort_groups()) - 1 or ms == [E.OP_CAP] * 3)
    points = E.sort_points()
    rows = points[case["offsets"][:, None] + case["select"]]                           # (b, kcap, 3)
    ctr = case["centres"][:, None, :]
    xyz = (rows.astype(np.float64) - ctr).astype(np.float32)                            # (points[inds] - pick_point).astype(float32)
    absolute = (xyz.astype(np.float64) + ctr).astype(np.float32)
    ns = [E.SORT_SCAN_N] * b
    pts, idx, d2, perm = dev(points), dev(case["idx"]), dev(case["d2"]), dev(case["perm"])
    scan_desc = dev(E.descriptors(E.SCAN_DESC, case["offsets"], ns, ms, np.zeros((b, 3), np.float32)).view(np.uint8))
    scene_desc = dev(E.descriptors(E.SCENE_DESC, case["offsets"], ns, ms, case["centres"]).view(np.uint8))

    def outputs(width):
        return Guarded(4 * b * kcap, NAN_BYTE, output_guard(4 * kcap)), Guarded(4 * b * kcap * width, NAN_BYTE, output_guard(4 * kcap * width))

    sel, out = outputs(3)
    launch("pasnl_crop_order_permute", b, ptr(scan_desc), ptr(pts), ptr(idx), ptr(d2), kcap, ptr(perm), kcap, ptr(sel.ptr), ptr(out.ptr))
    torch.cuda.synchronize()
    assert sel.guards_intact() and out.guards_intact()
    np.testing.assert_array_equal(sel.array((b, kcap), np.int32), case["select"])
    np.testing.assert_array_equal(out.array((b, kcap, 3), np.uint32), rows.view(np.uint32))
    for abs_coords in (0, 1):
        width = 6 if abs_coords else 3
        sel, out = outputs(width)
        launch("pasnl_scene_order_gather", b, ptr(scene_desc), ptr(pts), ptr(None), 0, ptr(idx), ptr(d2), kcap, ptr(perm), kcap,
               abs_coords, ptr(sel.ptr), ptr(out.ptr))
        torch.cuda.synchronize()
        assert sel.guards_intact() and out.guards_intact()
        np.testing.assert_array_equal(sel.array((b, kcap), np.int32), case["select"])
        expect = np.concatenate([xyz, absolute], 2) if abs_coords else xyz
        np.testing.assert_array_equal(out.array((b, kcap, width), np.uint32), np.ascontiguousarray(expect).view(np.uint32))
