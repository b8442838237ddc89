"""GPU: the entries of csrc/radius_crop.hip -- pasnl_scan_radius_members, pasnl_scene_radius_members,
pasnl_scan_radius_gather, pasnl_scene_radius_gather -- against numpy (tests/radius_flow_ref.sphere, the membership and order
that tests/test_radius_flow.py pins to sklearn), on guarded buffers (tests/guarded.py), twice over different stale bytes, with
workspaces of exactly pasnl_scan_radius_workspace_bytes."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import guarded as G
import radius_flow_ref as R
from scene_flow_ref import scene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCAN_DESC = np.dtype([("offset", "<i8"), ("cloud", "<i4"), ("pick", "<i4"), ("n", "<i4"), ("k", "<i4"), ("c", "<f4", 3), ("pad", "<i4")])
SCENE_DESC = np.dtype([("offset", "<i8"), ("cloud", "<i4"), ("pick", "<i4"), ("n", "<i4"), ("k", "<i4"), ("c", "<f8", 3)])
FILLS = ((G.NAN_BYTE, G.WS_BYTE), (G.ALT_BYTE, G.ALT_WS_BYTE))
KINDS = {"scan": (SCAN_DESC, "pasnl_scan_radius_members"), "scene": (SCENE_DESC, "pasnl_scene_radius_members")}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def descriptors(kind, sizes, centres):
    """one descriptor per scan of the flat buffer, with the given centres -> (host records, device bytes)"""
    d = np.zeros(len(sizes), KINDS[kind][0])
    d["offset"] = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    d["cloud"], d["n"], d["c"] = np.arange(len(sizes)), sizes, centres
    return d, dev(d.view(np.uint8))


def run_members(kind, points, desc_dev, b, nmax, radius, order, fills):
    """-> members (b,nmax) i32 and count (b,) i32 as numpy, after checking that nothing outside them was written"""
    from pointasnl_amd import _hip

    out_fill, ws_fill = fills
    nbytes = int(_hip.lib().pasnl_scan_radius_workspace_bytes(b, ctypes.c_long(nmax)))
    assert nbytes == b * ((nmax + 63) // 64) * 4
    mem = G.Guarded(b * nmax * 4, out_fill, G.output_guard(nmax * 4))
    cnt = G.Guarded(b * 4, out_fill)
    ws = G.Guarded(nbytes, ws_fill)
    _hip.launch(KINDS[kind][1], "test", b, ctypes.c_long(nmax), _hip.ptr(points), _hip.ptr(desc_dev), ctypes.c_double(radius),
                _hip.ptr(order), ctypes.c_void_p(mem.ptr), ctypes.c_long(nmax), ctypes.c_void_p(cnt.ptr), ctypes.c_void_p(ws.ptr),
                ctypes.c_size_t(nbytes))
    torch.cuda.synchronize()
    assert mem.guards_intact() and cnt.guards_intact() and ws.guards_intact()
    return mem.array((b, nmax), np.int32), cnt.array((b,), np.int32)


def check_members(kind, scans, centres, radius, orders, fills):
    sizes = [len(s) for s in scans]
    nmax, b = max(sizes), len(scans)
    desc, desc_dev = descriptors(kind, sizes, centres)
    flat_order = None if orders is None else dev(np.concatenate(orders).astype(np.int32))
    members, count = run_members(kind, dev(np.concatenate(scans)), desc_dev, b, nmax, radius, flat_order, fills)
    stale = np.frombuffer(bytes([fills[0]]) * 4, np.int32)[0]
    for c in range(b):
        want = R.sphere(scans[c].astype(np.float64), desc["c"][c].astype(np.float64), radius, None if orders is None else orders[c])
        assert count[c] == len(want)
        np.testing.assert_array_equal(members[c, :len(want)], want)
        assert (members[c, len(want):] == stale).all()  # entries behind the count are not written
    return count


def cloud(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * np.array([3.0, 3.0, 0.5])).astype(np.float32)


@pytest.mark.parametrize("kind", ["scan", "scene"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 4097])
def test_members_equal_numpy(kind, n):
    """b = 3 crops over scans of different n in one launch; radii that give an empty sphere, the centre alone, a middle
    count and the whole scan; order NULL and a random permutation"""
    sizes = [n, max(1, (n * 3) // 5), 130]
    scans = [cloud(10 * n + i, m) for i, m in enumerate(sizes)]
    rng = np.random.default_rng(n)
    perms = [rng.permutation(m) for m in sizes]
    at_point = np.stack([s[len(s) // 2] for s in scans]).astype(np.float64)
    mid = float(np.median(np.linalg.norm(scans[0].astype(np.float64) - at_point[0], axis=1))) if n > 1 else 0.5
    far = at_point + 1e3
    seen = set()
    for fills in FILLS:
        for orders in (None, perms):
            assert (check_members(kind, scans, far, 1.0, orders, fills) == 0).all()
            assert (check_members(kind, scans, at_point, 1e-7, orders, fills) == 1).all()
            assert check_members(kind, scans, at_point, 1e6, orders, fills).tolist() == sizes
            seen.add(int(check_members(kind, scans, at_point, mid, orders, fills)[0]))
    if n > 2:
        assert all(1 < c < n for c in seen)
    if kind == "scene":  # a float64 centre that is no float32 value
        check_members(kind, scans, at_point + np.pi * 1e-3, mid, perms, FILLS[0])


@pytest.mark.parametrize("kind", ["scan", "scene"])
def test_members_in_a_real_tree_order(kind):
    """the committed idx_array of sklearn's trees over the 700/450/900-point scenes of the flow tests"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_radius_flow as M

    orders = M.load_orders(np.load(os.path.join(HERE, "golden", "radius_flow.npz")))["scene"]
    scans = [scene(900 + i, m)[0] for i, m in enumerate(M.SIZES)]
    centres = np.stack([s[7] for s in scans]).astype(np.float64)
    for fills in FILLS:
        count = check_members(kind, scans, centres, 0.8, orders, fills)
        assert (count > 1).all() and (count < np.asarray(M.SIZES)).all()


@pytest.mark.parametrize("kind", ["scan", "scene"])
def test_sphere_boundary_and_nan(kind):
    """a point exactly on the sphere is kept (centre 0, point (3,4,0), r = 5: 25 <= 25), with r = nextafter(5, 0) it is
    dropped; a point with a NaN coordinate is no member at any radius"""
    pts = np.array([[3, 4, 0], [0, 0, 1], [np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [0, 6, 0]], np.float32)
    zero = np.zeros((1, 3))
    for fills in FILLS:
        desc, desc_dev = descriptors(kind, [6], zero)
        m, c = run_members(kind, dev(pts), desc_dev, 1, 6, 5.0, None, fills)
        assert c[0] == 2 and m[0, :2].tolist() == [0, 1]
        m, c = run_members(kind, dev(pts), desc_dev, 1, 6, float(np.nextafter(5.0, 0.0)), None, fills)
        assert c[0] == 1 and m[0, 0] == 1
        m, c = run_members(kind, dev(pts), desc_dev, 1, 6, 1e30, None, fills)
        assert c[0] == 3 and m[0, :3].tolist() == [0, 1, 5]
        m, c = run_members(kind, dev(pts), desc_dev, 1, 6, 1e30, dev(np.array([5, 4, 3, 2, 1, 0], np.int32)), fills)
        assert c[0] == 3 and m[0, :3].tolist() == [5, 1, 0]


def gather_case(seed, sizes, num_point):
    """members, counts and perms of b crops: crop 0 a full sphere with repeats in perm, crop 1 fewer members than num_point
    (the duplicated rows), crop 2 perm entries outside [0, count)"""
    rng = np.random.default_rng(seed)
    b, nmax = len(sizes), max(sizes)
    members = np.stack([np.concatenate([rng.permutation(m), np.full(nmax - m, -77)]) for m in sizes]).astype(np.int32)
    count = np.array([sizes[0], min(sizes[1], num_point // 3), sizes[2] // 2], np.int32)
    members[1, count[1]:] = -77  # nothing behind the count may be read
    members[2, count[2]:] = -77
    perm = np.stack([rng.integers(0, c, num_point) for c in count]).astype(np.int32)
    perm[1, :count[1]] = rng.permutation(count[1])
    bad = np.array([1, 5, 17, num_point - 1])
    perm[2, bad] = [-1, count[2], nmax + 3, np.iinfo(np.int32).max]
    return members, count, perm, bad


@pytest.mark.parametrize("num_point", [64, 300])
def test_scan_gather_equals_numpy(num_point):
    from pointasnl_amd import _hip

    sizes = [257, 40, 130]
    scans = [cloud(70 + i, m) for i, m in enumerate(sizes)]
    members, count, perm, bad = gather_case(num_point, sizes, num_point)
    desc, desc_dev = descriptors("scan", sizes, np.zeros((3, 3)))
    points, members_d, count_d, perm_d = dev(np.concatenate(scans)), dev(members), dev(count), dev(perm)
    for out_fill, _ in FILLS:
        sel = G.Guarded(3 * num_point * 4, out_fill, G.output_guard(num_point * 4))
        out = G.Guarded(3 * num_point * 12, out_fill, G.output_guard(num_point * 12))
        _hip.launch("pasnl_scan_radius_gather", "test", 3, _hip.ptr(desc_dev), _hip.ptr(points), _hip.ptr(members_d),
                    ctypes.c_long(max(sizes)), _hip.ptr(count_d), _hip.ptr(perm_d), num_point, ctypes.c_void_p(sel.ptr),
                    ctypes.c_void_p(out.ptr))
        torch.cuda.synchronize()
        assert sel.guards_intact() and out.guards_intact()
        got_sel, got = sel.array((3, num_point), np.int32), out.array((3, num_point, 3), np.int32)
        stale = np.frombuffer(bytes([out_fill]) * 4, np.int32)[0]
        for c in range(3):
            keep = np.ones(num_point, bool)
            if c == 2:
                keep[bad] = False
            want = members[c][perm[c][keep]]
            np.testing.assert_array_equal(got_sel[c][keep], want)
            np.testing.assert_array_equal(got[c][keep], scans[c][want].view(np.int32))
            assert (got_sel[c][~keep] == stale).all() and (got[c][~keep] == stale).all()  # the row stays as it was


@pytest.mark.parametrize("nfeat,abs_coords", [(0, 0), (3, 0), (3, 1)])
def test_scene_gather_equals_numpy(nfeat, abs_coords):
    from pointasnl_amd import _hip

    num_point, sizes = 64, [257, 40, 130]
    width = 3 + nfeat + 3 * abs_coords
    scans = [cloud(80 + i, m) for i, m in enumerate(sizes)]
    colors = [np.random.default_rng(90 + i).random((m, 3)).astype(np.float32) for i, m in enumerate(sizes)]
    members, count, perm, bad = gather_case(nfeat + abs_coords, sizes, num_point)
    centres = np.stack([s[3].astype(np.float64) + np.array([0.1, -0.2, np.pi * 1e-2]) for s in scans])
    desc, desc_dev = descriptors("scene", sizes, centres)
    points, members_d, count_d, perm_d = dev(np.concatenate(scans)), dev(members), dev(count), dev(perm)
    cols = dev(np.concatenate(colors)) if nfeat else None
    for out_fill, _ in FILLS:
        sel = G.Guarded(3 * num_point * 4, out_fill, G.output_guard(num_point * 4))
        out = G.Guarded(3 * num_point * width * 4, out_fill, G.output_guard(num_point * width * 4))
        _hip.launch("pasnl_scene_radius_gather", "test", 3, _hip.ptr(desc_dev), _hip.ptr(points), _hip.ptr(cols), nfeat,
                    _hip.ptr(members_d), ctypes.c_long(max(sizes)), _hip.ptr(count_d), _hip.ptr(perm_d), num_point, abs_coords,
                    ctypes.c_void_p(sel.ptr), ctypes.c_void_p(out.ptr))
        torch.cuda.synchronize()
        assert sel.guards_intact() and out.guards_intact()
        got_sel, got = sel.array((3, num_point), np.int32), out.array((3, num_point, width), np.int32)
        stale = np.frombuffer(bytes([out_fill]) * 4, np.int32)[0]
        for c in range(3):
            keep = np.ones(num_point, bool)
            if c == 2:
                keep[bad] = False
            want = members[c][perm[c][keep]]
            np.testing.assert_array_equal(got_sel[c][keep], want)
            xyz = (scans[c].astype(np.float64)[want] - centres[c]).astype(np.float32)  # D:519
            rows = [xyz] + ([colors[c][want]] if nfeat else []) + ([(xyz + centres[c]).astype(np.float32)] if abs_coords else [])
            np.testing.assert_array_equal(got[c][keep], np.hstack(rows).view(np.int32))
            assert (got_sel[c][~keep] == stale).all() and (got[c][~keep] == stale).all()
