"""GPU: SemanticKITTI's two training-time validation loops on the device (csrc/kitti_block_test.hip,
pointasnl_amd.SemanticKITTI.block_tester and the drop-in dataset classes) against the numpy restatement
tests/kitti_block_flow_ref.py run live on the same machine (it is pinned to the reference classes in
tests/test_kitti_block_tester_flow.py) and the reference's own run tests/golden/kitti_block_flow.npz.  Every comparison is
exact -- bit patterns or integers -- but two: the rotated coordinates, held to one float32 ulp of the float64 product (numpy's
dgemm fixes no summation order), and the loss, held to 1e-5 * max(1, |ref|) as BlockTester's is."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import kitti_block_flow_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
C, P, B = 20, 64, 3
NAMES = ["class%02d" % k for k in range(C)]
L, D = ctypes.c_long, ctypes.c_double


@pytest.fixture(scope="module")
def T():
    from pointasnl_amd.SemanticKITTI import block_tester as T

    return T


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "kitti_block_flow.npz"))


@pytest.fixture(scope="module")
def scans(gold):
    return [(gold["scan%d/points" % k], gold["scan%d/remissions" % k], gold["scan%d/labels" % k]) for k in range(5)]


@pytest.fixture(scope="module")
def content(gold):
    return dict(zip(gold["content_keys"].tolist(), gold["content_values"].tolist()))


@pytest.fixture(scope="module")
def lut(content):
    return R.label_weights_lut(content)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def state_of(rng):
    st = rng.get_state()
    return np.concatenate([st[1].astype(np.int64), [st[2]]])


def ulps_apart(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def same_item(got, want):
    """device (data, seg, smpw) against the restatement's or the fixture's: bits and dtypes"""
    data, seg, smpw = (host(a) for a in got)
    assert data.dtype == np.float32 and seg.dtype == np.int32 and smpw.dtype == np.float32
    assert want[0].dtype == np.float32 and want[2].dtype == np.float32 and data.shape == want[0].shape
    np.testing.assert_array_equal(bits(data), bits(want[0]))
    np.testing.assert_array_equal(seg, want[1])
    np.testing.assert_array_equal(bits(smpw), bits(want[2]))


def around(values):
    """float32 neighbours of float64 bounds: the nearest float32 and one ulp to either side of it"""
    out = []
    for v in values:
        f = np.float32(v)
        out += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return np.array(out, np.float32)


def device_lists(x, bounds, centre, half, nx, ny, block, padding, hist, counts):
    """pasnl_kblock_fill called directly -> member indices and masks, the columns' lists back to back"""
    from pointasnl_amd import _hip

    woff = np.where(counts > 0, np.cumsum(counts) - counts, -1).astype(np.int32)
    cap = int(counts.sum())
    idx = torch.full((cap + 8,), -7, dtype=torch.int32, device="cuda")
    mask = torch.full((cap + 8,), 9, dtype=torch.uint8, device="cuda")
    w = dev(woff)
    _hip.launch("pasnl_kblock_fill", "fill", L(x.shape[0]), ptr(x), ptr(bounds), L(centre), D(half), nx, ny, D(block), D(padding), ptr(hist),
                ptr(w), L(cap), ptr(idx), ptr(mask))
    idx, mask = host(idx), host(mask)
    assert (idx[cap:] == -7).all() and (mask[cap:] == 9).all()  # nothing at or past cap
    return idx[:cap], mask[:cap]


def device_crop(xyz, labels, bounds6, centre, block_size, padding):
    """one try through the entry points, bounds handed in -> m, labelled, member indices, mask"""
    from pointasnl_amd import _hip

    n = xyz.shape[0]
    x, lab, b = dev(xyz), dev(labels.astype(np.int32)), dev(np.asarray(bounds6, np.float32))
    hist = torch.empty((int(_hip.lib().pasnl_window_hist_bytes(L(n), 2, 1)) // 4,), dtype=torch.int32, device="cuda")
    stats = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    _hip.launch("pasnl_kblock_crop_stats", "stats", L(n), ptr(x), ptr(lab), ptr(b), L(centre), D(block_size / 2), ptr(hist), ptr(stats))
    m, labelled = (int(v) for v in host(stats))
    idx, mask = device_lists(x, b, centre, block_size / 2, 1, 1, 1.0, padding, hist, np.array([m]))
    return m, labelled, idx, mask.astype(bool)


def device_grid(xyz, bounds6, nx, ny, block_size, padding):
    """the whole-scan columns through the entry points, bounds handed in -> counts, member indices, masks"""
    from pointasnl_amd import _hip

    n = xyz.shape[0]
    x, b = dev(xyz), dev(np.asarray(bounds6, np.float32))
    nbytes = int(_hip.lib().pasnl_kwindow_hist_bytes(L(n), nx, ny))
    assert nbytes == nx * ny * ((n + 63) // 64) * 4
    hist = torch.full((nbytes // 4,), 12345, dtype=torch.int32, device="cuda")  # the call clears it
    cnt = torch.full((nx * ny,), -1, dtype=torch.int32, device="cuda")
    _hip.launch("pasnl_kblock_grid_count", "count", L(n), ptr(x), ptr(b), nx, ny, D(block_size), ptr(hist), ptr(cnt))
    counts = host(cnt).astype(np.int64)
    idx, mask = device_lists(x, b, -1, 0.0, nx, ny, block_size, padding, hist, counts)
    return counts, idx, mask.astype(bool)


def ref_grid(xyz, coordmin, coordmax, nx, ny, block_size, padding):
    members, masks = [], []
    for i in range(nx):
        for j in range(ny):
            lo, hi = R.column_box(coordmin, coordmax, i, j, block_size)
            k = np.flatnonzero(R.inside(xyz, lo, hi, R.OUTER))
            members.append(k)
            masks.append(R.inside(xyz[k], lo, hi, padding))
    return members, masks


@pytest.mark.parametrize("block_size", [10, 2.5])
@pytest.mark.parametrize("n", [40, 64, 65, 257, 3000])
def test_crop_stats_and_fill_at_every_chunking(T, scans, n, block_size):
    """D:82-95 with less than a chunk, exactly one, one point more, several with a ragged last one, and several workgroups;
    the centre on the scan's min corner, on its max corner and inside; an int and a float block_size.  Counts, the member
    list in ascending index and the padding mask are the restatement's, through the entry points and through the class."""
    xyz, lab = scans[1][0][:n].copy(), scans[1][2][:n].copy()
    lo, hi = R.bounds(xyz)
    xyz[0], xyz[1] = lo, hi
    t = T.KittiBlockTester([xyz], [lab], num_classes=C, block_points=P, block_size=block_size)
    np.testing.assert_array_equal(bits(t.bounds_host[0]), bits(np.concatenate([lo, hi])))
    for centre in (0, 1, n // 2):
        want = R.crop_stats(xyz, lab, xyz[centre], block_size, 0.01, lo[2], hi[2])
        assert 0 < want["m"] and (n < 257 or want["m"] < n) and centre in want["members"]
        m, labelled, idx, mask = device_crop(xyz, lab, np.concatenate([lo, hi]), centre, block_size, 0.01)
        assert (m, labelled) == (want["m"], want["labelled"])
        np.testing.assert_array_equal(idx, want["members"])
        np.testing.assert_array_equal(mask, want["mask"])
        assert t.crop_stats(0, centre)[:2] == (want["m"], want["labelled"])


@pytest.mark.parametrize("block_size,padding", [(10, 0.01), (2.5, 0.05)])
def test_crop_membership_one_ulp_either_side_of_every_bound(block_size, padding):
    """D:87, D:95: float32 coordinates at, one ulp below and one ulp above curmin - 0.2, curmax + 0.2, curmin - padding and
    curmax + padding on every axis (the z bounds handed in, so that points lie on both sides of them)"""
    rng = np.random.default_rng(5)
    centre = np.array([0.3, -1.1, 0.9], np.float32)
    zmin, zmax = np.float32(0.25), np.float32(2.125)
    lo, hi = R.crop_box(centre, block_size, zmin, zmax)
    s = block_size + 1.0
    pts = [centre[None, :], (rng.random((150, 3)) * [s, s, 2.6] + [0.3 - s / 2, -1.1 - s / 2, -0.1]).astype(np.float32)]
    for a in range(3):
        edge = around([lo[a] - 0.2, hi[a] + 0.2, lo[a] - padding, hi[a] + padding])
        block = np.tile(centre, (len(edge), 1))
        block[:, a] = edge
        pts.append(block)
    xyz = np.concatenate(pts).astype(np.float32)
    labels = rng.integers(0, C, xyz.shape[0])
    want = R.crop_stats(xyz, labels, centre, block_size, padding, zmin, zmax)
    assert 0 < want["mask"].sum() < want["m"] < xyz.shape[0]
    m, labelled, idx, mask = device_crop(xyz, labels, [0, 0, zmin, 0, 0, zmax], 0, block_size, padding)
    assert (m, labelled) == (want["m"], want["labelled"])
    np.testing.assert_array_equal(idx, want["members"])
    np.testing.assert_array_equal(mask, want["mask"])
    # a float32 comparison would sort some of these to the other side
    f32 = np.all((xyz >= (lo - 0.2).astype(np.float32)) & (xyz <= (hi + 0.2).astype(np.float32)), axis=1)
    assert not np.array_equal(np.flatnonzero(f32), want["members"])


def test_rejection_loop_first_try_later_try_never_and_exactly_seventy_percent(T, scans, lut):
    """D:81-99 with seeds chosen on the CPU: an item valid on try 1, one on a later try, one on none (scan 3 is 60 %
    unlabelled everywhere, so the tenth crop is used); and a crop with exactly 7 labelled of 10 members, which 7 / 10 >= 0.7
    accepts.  The tries, the item and the RNG state agree in each."""
    rng0 = np.random.default_rng(3)
    cluster = (rng0.random((10, 3)) + [5.0, 5.0, 0.0]).astype(np.float32)
    far = (rng0.random((30, 3)) + [60.0, 5.0, 0.0]).astype(np.float32)
    seventy = (np.concatenate([cluster, far]), None, np.concatenate([np.arange(10) < 7, np.zeros(30)]).astype(np.int32) * 3)
    cases = {"first": scans[1], "later": scans[1], "never": scans[3], "seventy": seventy}
    picked = {}
    for seed in range(60):
        for kind, (p, _, l) in cases.items():
            tries = R.chopped_item(p, None, l, lut, P, np.random.RandomState(seed))[3]["tries"]
            n, last = len(tries), tries[-1]
            ok = {"first": n == 1, "later": 1 < n < 10 and last["valid"], "never": n == 10 and not last["valid"],
                  "seventy": n == 1 and (last["m"], last["labelled"]) == (10, 7)}[kind]
            if ok and kind not in picked:
                picked[kind] = (seed, n)
    assert set(picked) == set(cases)
    for kind, (seed, n) in picked.items():
        p, _, l = cases[kind]
        ref_rng, rng, probe = (np.random.RandomState(seed) for _ in range(3))
        want = R.chopped_item(p, None, l, lut, P, ref_rng)
        centre, m, _, tries = T.KittiBlockTester([p], [l], num_classes=C, block_points=P, rng=probe).draw_crop(0)
        assert tries == n and centre == want[3]["tries"][-1]["centre"] and m == want[3]["tries"][-1]["m"]
        t = T.KittiBlockTester([p], [l], num_classes=C, block_points=P, batch_size=B, label_weights_lut=lut, rng=rng)
        same_item(t.item(0), want[:3])
        np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))


@pytest.mark.parametrize("case", ["empty_column", "four_columns", "83_columns", "block_2.5"])
def test_grid_counts_lists_and_masks(T, scans, case):
    """D:182-193: a scan with an empty column; a point within 0.2 of a corner, a member of four columns; more than 64 columns
    on one axis (the 41 m scan at block_size 0.5); block_size 2.5.  Counts equal list lengths, the lists are in ascending
    index and, with the padding masks, the restatement's; through the entry points and through the class."""
    k, block_size = {"empty_column": (4, 10), "four_columns": (1, 10), "83_columns": (2, 0.5), "block_2.5": (1, 2.5)}[case]
    xyz = scans[k][0].copy()
    lo, hi = R.bounds(xyz)
    if case == "four_columns":
        xyz[5] = (lo.astype(np.float64) + [10.1, 9.9, 1.0]).astype(np.float32)
    if case == "83_columns":  # a centimetre past 41 m
        xyz[np.argmax(xyz[:, 0]), 0] = hi[0] + np.float32(0.01)
        hi = R.bounds(xyz)[1]
    nx, ny = R.grid(lo, hi, block_size)
    members, masks = ref_grid(xyz, lo, hi, nx, ny, block_size, 0.01)
    lens = np.array([len(m) for m in members])
    if case == "empty_column":
        assert (nx, ny) == (3, 2) and (lens == 0).sum() == 1
    if case == "four_columns":
        assert sum(5 in m for m in members) == 4
    if case == "83_columns":
        assert nx == 83 and ny == 18 and (lens == 0).sum() > 0
    if case == "block_2.5":
        assert (nx, ny) == (16, 11)
    assert lens.sum() > xyz.shape[0]  # the 0.2 margin: some points are in several columns
    counts, idx, mask = device_grid(xyz, np.concatenate([lo, hi]), nx, ny, block_size, 0.01)
    np.testing.assert_array_equal(counts, lens)
    np.testing.assert_array_equal(idx, np.concatenate(members))
    np.testing.assert_array_equal(mask, np.concatenate(masks))
    for a, b in zip(np.cumsum(lens) - lens, np.cumsum(lens)):
        assert (np.diff(idx[a:b]) > 0).all()
    t = T.KittiBlockTester([xyz], [scans[k][2]], num_classes=C, block_points=P, block_size=block_size)
    shape, got, _ = t.column_counts(0)
    assert shape == (nx, ny)
    np.testing.assert_array_equal(got, lens)


@pytest.mark.parametrize("block_size,padding", [(10, 0.01), (2.5, 0.05)])
def test_grid_membership_one_ulp_either_side_of_every_bound(block_size, padding):
    """D:184-187, D:193 over 3 x 2 columns: coordinates round coordmin + i * block - 0.2, coordmin + (i + 1) * block + 0.2
    and the padding margins on every axis; the upper bound is coordmin + (i + 1) * block, which is not curmin + block at this
    x origin (the two differ in the last bits of the float64 bound)."""
    rng = np.random.default_rng(6)
    s = float(block_size)
    coordmin = np.array([1.4124656e-10, -0.7, 0.3], np.float32)
    coordmax = (coordmin.astype(np.float64) + [2.8 * s, 1.9 * s, 2.6]).astype(np.float32)
    pts = [(rng.random((300, 3)) * [3.2 * s, 2.3 * s, 3.2] + [-0.2 * s, -0.7 - 0.2 * s, 0.0]).astype(np.float32)]
    differs = False
    for i in range(3):
        for j in range(2):
            lo, hi = R.column_box(coordmin, coordmax, i, j, block_size)
            differs |= bool(np.any(hi[:2] != lo[:2] + block_size))
            for a in range(3):
                edge = around([lo[a] - 0.2, hi[a] + 0.2, lo[a] - padding, hi[a] + padding])
                block = np.tile(((lo + hi) / 2).astype(np.float32), (len(edge), 1))
                block[:, a] = edge
                pts.append(block)
    assert differs
    xyz = np.concatenate(pts).astype(np.float32)
    assert xyz.shape[0] % 64 != 0 and R.grid(coordmin, coordmax, block_size) == (3, 2)
    members, masks = ref_grid(xyz, coordmin, coordmax, 3, 2, block_size, padding)
    counts, idx, mask = device_grid(xyz, np.concatenate([coordmin, coordmax]), 3, 2, block_size, padding)
    np.testing.assert_array_equal(counts, [len(k) for k in members])
    np.testing.assert_array_equal(idx, np.concatenate(members))
    np.testing.assert_array_equal(mask, np.concatenate(masks))
    assert 0 < np.concatenate(masks).sum() < len(idx)


@pytest.mark.parametrize("rem", [False, True])
@pytest.mark.parametrize("quirks", [True, False])
def test_gather_both_quirk_settings_with_and_without_remission(T, scans, lut, quirks, rem):
    """D:100-107, D:195-203 through `item` and `scan_blocks` on the 40-point scan (64 draws of at most 40 members: draws
    repeat), the 3000-point scan and the scan with an empty column: rows, labels and float32 weight bits are the
    restatement's under either setting, and so is the RNG state"""
    ks = (0, 1, 4)
    ref_rng, rng = np.random.RandomState(13), np.random.RandomState(13)
    t = T.KittiBlockTester([scans[k][0] for k in ks], [scans[k][2] for k in ks], remissions=[scans[k][1] for k in ks] if rem else None,
                           num_classes=C, block_points=P, batch_size=B, label_weights_lut=lut, reference_quirks=quirks, rng=rng)
    for i, k in enumerate(ks):
        p, r, l = scans[k]
        want = R.chopped_item(p, r if rem else None, l, lut, P, ref_rng, reference_quirks=quirks)
        if k == 0:
            assert len(np.unique(want[3]["choice"])) < P
        same_item(t.item(i), want[:3])
        want = R.whole_item(p, r if rem else None, l, lut, P, ref_rng, reference_quirks=quirks)
        got = t.scan_blocks(i)
        assert got[0].shape == (len(want[3]["columns"]), P, 4 if rem else 3)
        assert k == 0 or 0 < (want[2] == 0).sum() < want[2].size  # rows inside the 0.2 margin but outside the padding weigh 0
        same_item(got, want[:3])
        np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))


@pytest.mark.parametrize("kind,rem", [("chopped", False), ("chopped", True), ("whole", False), ("whole", True)])
def test_items_equal_the_reference_run(T, gold, scans, lut, kind, rem):
    """`item` / `scan_blocks` over the fixture's scans, every scan twice: the reference's arrays bit for bit and its RNG state
    after every call"""
    tag = "%s/%s" % (kind, "rem" if rem else "xyz")
    rng = np.random.RandomState(int(gold["seed"][0]))
    t = T.KittiBlockTester([p for p, _, _ in scans], [l for _, _, l in scans], remissions=[r for _, r, _ in scans] if rem else None,
                           num_classes=C, block_points=int(gold["sample_points"][0]), batch_size=B, block_size=int(gold["block_size"][0]),
                           padding=float(gold["padding"][0]), label_weights_lut=lut, rng=rng)
    for visit in range(2 * len(scans)):
        got = t.item(visit % 5) if kind == "chopped" else t.scan_blocks(visit % 5)
        same_item(got, [gold["%s/%d/%s" % (tag, visit, name)] for name in ("data", "seg", "smpw")])
        np.testing.assert_array_equal(state_of(rng), gold["%s/%d/rng" % (tag, visit)].astype(np.int64))


@pytest.mark.parametrize("width", [3, 4])
@pytest.mark.parametrize("in_place", [True, False])
def test_rotate_in_place_and_out_of_place(T, scans, width, in_place):
    """P:71-89 as T:290 applies it: x and y within one float32 ulp of numpy's float64 product, columns 2.. copied exactly"""
    p, r, l = scans[2]
    t = T.KittiBlockTester([p], [l], remissions=[r] if width == 4 else None, num_classes=C, block_points=P, batch_size=B,
                           rng=np.random.RandomState(2))
    data, _, _ = t.scan_blocks(0)
    raw = host(data).copy()
    assert raw.shape == (5, P, width)
    angles = list(np.random.RandomState(7).uniform(size=B) * 2 * np.pi)
    out = None if in_place else torch.full_like(data, 7.0)
    got = host(t.rotate(data, B, angles, out=out))
    want = raw[:B].astype(np.float64)
    want[:, :, :3] = R.rotate_z(want[:, :, :3], angles)
    want = want.astype(np.float32)
    worst = ulps_apart(got[:B, :, :2], want[:, :, :2]).max()
    print("rotation: %.3f ulp at most" % worst)
    assert worst <= 1.0 and np.abs(got[:B, :, :2] - raw[:B, :, :2]).max() > 1.0
    np.testing.assert_array_equal(bits(got[:B, :, 2:]), bits(raw[:B, :, 2:]))
    if in_place:
        np.testing.assert_array_equal(bits(got[B:]), bits(raw[B:]))  # the rows past `rows` are not touched
    else:
        assert (got[B:] == 7.0).all()
        np.testing.assert_array_equal(bits(host(data)), bits(raw))


def device_forward(w, b, fed, logits):
    wt, bt = dev(w), dev(b)

    def forward(x):
        out = torch.sin(x[:, :, :3] @ wt + bt) * 4.0
        out[1, 0, :] = 1.5            # np.argmax: the first maximum
        out[2, 3, 1:3] = 7.0
        fed.append(host(x).copy())
        logits.append(host(out).copy())
        return out

    return forward


def replay(fed, logits, rotated):
    """the restatement's forward: checks that it is asked for the batch the device was given, answers with the device's logits"""
    k = [0]

    def forward(x):
        got = fed[k[0]]
        if rotated:
            assert ulps_apart(got[:, :, :2], x[:, :, :2]).max() <= 1.0
            np.testing.assert_array_equal(bits(got[:, :, 2:]), bits(x[:, :, 2:]))
        else:
            np.testing.assert_array_equal(bits(got), bits(x))
        k[0] += 1
        return logits[k[0] - 1]

    return forward, k


def same_results(t, out, whole, extra):
    tot = t.totals()
    assert (tot["total_correct"], tot["total_seen"]) == (out["total_correct"], out["total_seen"]) and out["total_seen"] > 0
    for name in ("seen", "correct", "deno", "hist"):
        assert tot[name].dtype == np.int64
        np.testing.assert_array_equal(tot[name], out[name])
    np.testing.assert_array_equal(bits(t.class_iou()), bits(out["class_iou"]))
    assert t.miou() == out["miou"]
    print("mean loss: device %.9f, restatement %.9f" % (t.mean_loss(extra), out["mean_loss"]))
    assert abs(t.mean_loss(extra) - out["mean_loss"]) <= 1e-5 * max(1.0, abs(out["mean_loss"]))
    got, want = t.report(NAMES, extra), R.report(out, NAMES, whole)
    assert got[1:] == want[1:] and len(got) == 5  # both loops print the per-class table
    head, value = got[0].rsplit(" ", 1)
    assert head == want[0].rsplit(" ", 1)[0] and abs(float(value) - float(want[0].rsplit(" ", 1)[1])) <= 2e-5 * max(1.0, abs(out["mean_loss"]))


@pytest.mark.parametrize("rem", [False, True])
def test_run_whole_through_every_branch_of_the_carry_over(T, scans, lut, rem):
    """T:331-418 over scans of 1, 1, 5, 12, 1, 1 columns with B = 3: fewer than B twice (continue), then 7 > B (3 fed, 4
    carried), 12 + 4 > B, then 1 + 13 ...; and a second order that meets a batch of exactly B.  The batches fed (unrotated),
    the counters, mIoU, the mean loss (divided by S, not by the forwards), the report lines, the rows left over and the RNG
    state are the restatement's."""
    seen = set()
    for order in ([0, 0, 2, 1, 0, 0], [0, 0, 0, 2, 0]):
        ref_rng, rng = np.random.RandomState(21), np.random.RandomState(21)
        w, b = R.stand_in_weights(3, C)
        fed, logits = [], []
        t = T.KittiBlockTester([scans[k][0] for k in order], [scans[k][2] for k in order],
                               remissions=[scans[k][1] for k in order] if rem else None, num_classes=C, block_points=P, batch_size=B,
                               label_weights_lut=lut, rng=rng)
        miou = t.run_whole(device_forward(w, b, fed, logits))
        forward, asked = replay(fed, logits, False)

        def getitem(i):
            p, r, l = scans[order[i]]
            return R.whole_item(p, r if rem else None, l, lut, P, ref_rng)[:3]

        out = R.eval_whole(getitem, len(order), B, forward, C, extra=0.125)
        seen |= {"<" if s < B else ("=" if s == B else ">") for s in out["rows"]}
        assert asked[0] == len(fed) == t.forwards == len(out["fed"]) > 0 and out["num_batches"] == len(order) == t.num_batches
        assert t.left == out["left"] and miou == out["miou"]
        same_results(t, out, True, 0.125)
        np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))
    assert out["rows"] == [1, 2, 3, 5, 3] and out["left"] == 0 and t.forwards == 3
    assert seen == {"<", "=", ">"}


@pytest.mark.parametrize("rem", [False, True])
def test_run_chopped_drops_the_remainder_and_rotates(T, scans, lut, rem):
    """T:267-328 over seven scans with B = 3: two batches, the seventh scan is never drawn; B items, then B angles; the
    rotated coordinates within one float32 ulp of numpy's float64 product, z, remission, labels and weights exact."""
    order = [0, 1, 2, 3, 4, 1, 0]
    ref_rng, rng = np.random.RandomState(31), np.random.RandomState(31)
    w, b = R.stand_in_weights(4, C)
    fed, logits = [], []
    t = T.KittiBlockTester([scans[k][0] for k in order], [scans[k][2] for k in order], remissions=[scans[k][1] for k in order] if rem else None,
                           num_classes=C, block_points=P, batch_size=B, label_weights_lut=lut, rng=rng)
    assert t.S % B != 0
    miou = t.run_chopped(device_forward(w, b, fed, logits))
    forward, asked = replay(fed, logits, True)

    def getitem(i):
        p, r, l = scans[order[i]]
        return R.chopped_item(p, r if rem else None, l, lut, P, ref_rng)[:3]

    out = R.eval_chopped(getitem, len(order), B, P, 4 if rem else 3, forward, C, ref_rng, extra=0.5)
    assert asked[0] == len(fed) == 2 == out["num_batches"] == t.num_batches == t.forwards and miou == out["miou"] and t.left == 0
    np.testing.assert_array_equal(host(t.batch_label), out["labels"][-1])
    np.testing.assert_array_equal(bits(host(t.batch_smpw)), bits(out["smpw"][-1]))
    same_results(t, out, False, 0.5)
    np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))


@pytest.mark.parametrize("kind", ["chopped", "whole"])
def test_drop_in_dataset_classes(gold, scans, content, kind):
    """`SemanticKittiDataset` / `SemanticKittiDataset_whole` over the scans in memory: `__len__`, `__getitem__` (the
    reference's dtypes) against the fixture, the weight table from the frequencies, and the :47-52 subset"""
    from pointasnl_amd.SemanticKITTI import semantic_kitti_dataset as D

    cls = D.SemanticKittiDataset if kind == "chopped" else D.SemanticKittiDataset_whole
    for rem in (False, True):
        tag = "%s/%s" % (kind, "rem" if rem else "xyz")
        rng = np.random.RandomState(int(gold["seed"][0]))
        ds = cls([p for p, _, _ in scans], [l for _, _, l in scans], remissions=[r for _, r, _ in scans], sample_points=int(gold["sample_points"][0]),
                 block_size=int(gold["block_size"][0]), split="valid", with_remission=rem, label_frequencies=content, rng=rng)
        assert len(ds) == int(gold[tag + "/len"][0]) == 5
        np.testing.assert_array_equal(bits(ds.label_weights_lut), bits(gold[tag + "/lut"]))
        for visit in range(5):
            item = ds[visit]
            assert len(item) == 3
            for got, name in zip(item, ("data", "seg", "smpw")):
                want = gold["%s/%d/%s" % (tag, visit, name)]
                assert got.dtype == want.dtype and got.shape == want.shape
                np.testing.assert_array_equal(bits(got), bits(want))
            np.testing.assert_array_equal(state_of(rng), gold["%s/%d/rng" % (tag, visit)].astype(np.int64))
    names = ["%d" % k for k in range(5)]
    sub = cls([p for p, _, _ in scans], [l for _, _, l in scans], sample_points=P, random_sample=True, random_rate=0.5, points_name=names)
    random.Random(100).shuffle(names)
    assert len(sub) == 2 and sub.points_name == names[:2] and [str(k) for k in sub.order] == names[:2]
    np.testing.assert_array_equal(bits(sub.scans[0]), bits(scans[int(names[0])][0]))


def test_value_errors_where_the_reference_crashes(T, scans):
    p, r, l = scans[0]
    flat = p.copy()
    flat[:, 0] = flat[0, 0]  # zero extent in x: the reference finds no column and concatenates nothing
    t = T.KittiBlockTester([flat], [l], num_classes=C, block_points=P)
    with pytest.raises(ValueError):
        t.scan_blocks(0)
    with pytest.raises(ValueError):
        R.whole_item(flat, None, l, np.ones(C, np.float32), P, np.random.RandomState(0))
    same_item(T.KittiBlockTester([flat], [l], num_classes=C, block_points=P, rng=np.random.RandomState(1)).item(0),
              R.chopped_item(flat, None, l, np.ones(C, np.float32), P, np.random.RandomState(1))[:3])  # the chopped loop does not mind
    bad = p.copy()
    bad[3, 1] = np.inf
    with pytest.raises(ValueError):
        T.KittiBlockTester([bad], [l], num_classes=C, block_points=P)
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        T.KittiBlockTester([bad], [l], num_classes=C, block_points=P)
    few, lab = p[:15], (np.arange(15) + 5).astype(np.int32)  # n = 15 <= max(label) = 19
    with pytest.raises(ValueError):
        T.KittiBlockTester([few], [lab], num_classes=C, block_points=P)
    t = T.KittiBlockTester([few], [lab], num_classes=C, block_points=P, reference_quirks=False, rng=np.random.RandomState(2))
    same_item(t.item(0), R.chopped_item(few, None, lab, np.ones(C, np.float32), P, np.random.RandomState(2), reference_quirks=False)[:3])
    with pytest.raises(ValueError):
        T.KittiBlockTester([p], [l + C], num_classes=C, block_points=P)
    with pytest.raises(ValueError):
        T.KittiBlockTester([p], [l], num_classes=C, block_points=P, label_weights_lut=np.ones(C + 1))
