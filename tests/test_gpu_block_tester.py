"""GPU: ScanNet's two training-time validation loops on the device (csrc/block_test.hip,
pointasnl_amd.ScanNet.block_tester and the drop-in dataset classes) against the numpy restatement tests/block_flow_ref.py
run live on the same machine (it is pinned to the reference classes in tests/test_block_tester_flow.py) and the reference's
own run tests/golden/block_flow.npz.  Every comparison is exact -- bit patterns or integers -- but two: the rotated
coordinates, held to one float32 ulp of the float64 product, and the loss, held to 1e-5 * max(1, |ref|)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import block_flow_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
C, P, B = 5, 64, 3
NAMES = ["unannotated", "wall", "floor", "chair", "table"]
WEIGHTS = np.array([1.0, 0.5, 2.0, 1.25, 3.0])


@pytest.fixture(scope="module")
def T():
    from pointasnl_amd.ScanNet import block_tester as T

    return T


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "block_flow.npz"))


@pytest.fixture(scope="module")
def scenes(gold):
    return [(gold["scene%d/points" % k], gold["scene%d/labels" % k]) for k in range(4)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def host(t):
    return t.cpu().numpy()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def state_of(rng):
    st = rng.get_state()
    return np.concatenate([st[1].astype(np.int64), [st[2]]])


def ulps_apart(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def same_item(got, want):
    """device (data, seg, smpw f32) against the restatement's or the fixture's (data, seg, smpw f64)"""
    data, seg, smpw = (host(a) for a in got)
    np.testing.assert_array_equal(bits(data), bits(want[0]))
    np.testing.assert_array_equal(seg, want[1])
    assert seg.dtype == np.int32 and smpw.dtype == np.float32
    np.testing.assert_array_equal(bits(smpw), bits(np.asarray(want[2]).astype(np.float32)))


def around(values):
    """float32 neighbours of float64 bounds: the nearest float32 and one ulp to either side of it"""
    out = []
    for v in values:
        f = np.float32(v)
        out += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    return np.array(out, np.float32)


def device_lists(T, xyz, bounds, centre, nx, ny, hist, counts):
    """pasnl_block_fill called directly -> member indices and masks, the columns' lists back to back"""
    from pointasnl_amd import _hip

    woff = np.where(counts > 0, np.cumsum(counts) - counts, -1).astype(np.int32)
    cap = int(counts.sum())
    idx = torch.full((cap + 8,), -7, dtype=torch.int32, device="cuda")
    mask = torch.full((cap + 8,), 9, dtype=torch.uint8, device="cuda")
    w = torch.from_numpy(woff).cuda()
    _hip.launch("pasnl_block_fill", "fill", ctypes.c_long(xyz.shape[0]), ptr(xyz), ptr(bounds), ctypes.c_long(centre), nx, ny, ptr(hist),
                ptr(w), ctypes.c_long(cap), ptr(idx), ptr(mask))
    idx, mask = host(idx), host(mask)
    assert (idx[cap:] == -7).all() and (mask[cap:] == 9).all()  # nothing at or past cap
    return idx[:cap], mask[:cap]


def test_crop_membership_one_ulp_either_side_of_every_bound(T):
    """D:46, D:52: float32 coordinates at, one ulp below and one ulp above curmin - 0.2, curmax + 0.2, curmin - 0.01 and
    curmax + 0.01 on every axis (the z bounds handed in, so that points lie on both sides of them): the counts, the member
    list in ascending index and the 0.01 mask are the restatement's."""
    rng = np.random.default_rng(5)
    centre = np.array([0.3, -1.1, 0.9], np.float32)
    zmin, zmax = np.float32(0.25), np.float32(2.125)
    lo, hi = R.crop_box(centre, zmin, zmax)
    pts = [centre[None, :], (rng.random((150, 3)) * [2.4, 2.4, 2.6] + [-0.9, -2.3, -0.1]).astype(np.float32)]
    for a in range(3):
        edge = around([lo[a] - 0.2, hi[a] + 0.2, lo[a] - 0.01, hi[a] + 0.01])
        block = np.tile(centre, (len(edge), 1))
        block[:, a] = edge
        pts.append(block)
    xyz = np.concatenate(pts).astype(np.float32)
    labels = rng.integers(0, C, xyz.shape[0])
    t = T.BlockTester([xyz], [labels], num_classes=C, block_points=P, batch_size=B)
    bounds = torch.tensor([0, 0, zmin, 0, 0, zmax], dtype=torch.float32, device="cuda")
    want = R.crop_stats(xyz, labels, centre, zmin, zmax)
    m, labelled, nuniq, hist = t.crop_stats(0, 0, bounds=bounds)
    assert (m, labelled, nuniq) == (want["m"], want["labelled"], want["nuniq"])
    assert 0 < want["mask"].sum() < m < xyz.shape[0]
    idx, mask = device_lists(T, t.xyz[0], bounds, 0, 1, 1, hist, np.array([m]))
    np.testing.assert_array_equal(idx, want["members"])
    np.testing.assert_array_equal(mask.astype(bool), want["mask"])
    # a float32 comparison would sort some of these to the other side
    f32 = np.all((xyz >= (lo - 0.2).astype(np.float32)) & (xyz <= (hi + 0.2).astype(np.float32)), axis=1)
    assert not np.array_equal(np.flatnonzero(f32), want["members"])


def test_grid_membership_one_ulp_either_side_of_every_bound(T):
    """D:107-109, D:115 over 3 x 2 columns: coordinates round coordmin + i * 1.5 - 0.2, coordmin + (i + 1) * 1.5 + 0.2 and
    the 0.001 margins on every axis; the upper bound is coordmin + (i + 1) * 1.5, which is not curmin + 1.5 at this x
    origin (the two differ in the last bits of the float64 bound)."""
    from pointasnl_amd import _hip

    rng = np.random.default_rng(6)
    coordmin, coordmax = np.array([6.3957345e-10, -0.7, 0.3], np.float32), np.array([4.3, 2.2, 2.9], np.float32)
    pts = [(rng.random((300, 3)) * [4.8, 3.5, 3.2] + [-0.2, -1.0, 0.0]).astype(np.float32)]
    mid = np.array([1.0, 0.0, 1.0], np.float32)
    differs = False
    for i in range(3):
        for j in range(2):
            lo, hi = R.column_box(coordmin, coordmax, i, j)
            differs |= bool(np.any(hi[:2] != lo[:2] + 1.5))
            for a in range(3):
                edge = around([lo[a] - 0.2, hi[a] + 0.2, lo[a] - 0.001, hi[a] + 0.001])
                block = np.tile(((lo + hi) / 2).astype(np.float32), (len(edge), 1))
                block[:, a] = edge
                pts.append(block)
    assert differs
    xyz = np.concatenate(pts + [mid[None, :]]).astype(np.float32)
    n = xyz.shape[0]
    assert n % 64 != 0
    x = torch.from_numpy(xyz).cuda()
    bounds = torch.from_numpy(np.concatenate([coordmin, coordmax])).cuda()
    hist = torch.empty((int(_hip.lib().pasnl_window_hist_bytes(ctypes.c_long(n), 3, 2)) // 4,), dtype=torch.int32, device="cuda")
    cnt = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    _hip.launch("pasnl_block_grid_count", "count", ctypes.c_long(n), ptr(x), ptr(bounds), 3, 2, ptr(hist), ptr(cnt))
    counts = host(cnt).astype(np.int64)
    members, masks = [], []
    for i in range(3):
        for j in range(2):
            lo, hi = R.column_box(coordmin, coordmax, i, j)
            k = np.flatnonzero(R.inside(xyz, lo, hi, R.OUTER))
            members.append(k)
            masks.append(R.inside(xyz[k], lo, hi, R.WHOLE_INNER))
    np.testing.assert_array_equal(counts, [len(k) for k in members])
    idx, mask = device_lists(T, x, bounds, -1, 3, 2, hist, counts)
    np.testing.assert_array_equal(idx, np.concatenate(members))
    np.testing.assert_array_equal(mask.astype(bool), np.concatenate(masks))


@pytest.mark.parametrize("kind,rgb,split", [("chopped", True, "val"), ("chopped", False, "val"), ("chopped", True, "train"),
                                            ("whole", True, "val"), ("whole", False, "val"), ("whole", True, "train")])
def test_items_equal_the_reference_run(T, gold, scenes, kind, rgb, split):
    """`item` / `scene_blocks` over the fixture's scenes -- 40 points (less than a chunk), 1000 (no multiple of 64), a 3 x 2
    grid with an empty column, tries that pass and tries that never do -- with and without rgb, with ones and with the
    'train' label weights: the reference's arrays bit for bit and its RNG state after every call."""
    tag = "%s/%s/%s" % (kind, "rgb" if rgb else "xyz", split)
    Pg = int(gold["block_points"][0])
    rng = np.random.RandomState(int(gold["seed"][0]))
    t = T.BlockTester([p if rgb else p[:, 0:3] for p, _ in scenes], [l for _, l in scenes], num_classes=21, block_points=Pg, batch_size=B,
                      labelweights=gold[tag + "/labelweights"], rng=rng)
    for visit in range(2 * len(scenes)):
        got = t.item(visit % 4) if kind == "chopped" else t.scene_blocks(visit % 4)
        same_item(got, [gold["%s/%d/%s" % (tag, visit, name)] for name in ("data", "seg", "smpw")])
        np.testing.assert_array_equal(state_of(rng), gold["%s/%d/rng" % (tag, visit)])


def test_rejection_loop_first_try_middle_try_and_never(T, scenes):
    """D:40-57 with seeds chosen on the CPU: an item valid on try 1, one on a middle try, one on none (scene 3 is more than
    30 % unlabelled everywhere, so the tenth crop is used).  The tries, the item and the RNG state agree in each."""
    picked = {}
    for seed in range(40):
        for k in (1, 3):
            info = R.chopped_item(*scenes[k], WEIGHTS, P, np.random.RandomState(seed))[3]
            n = len(info["tries"])
            kind = "first" if n == 1 else ("never" if not info["tries"][-1]["valid"] else ("middle" if 1 < n < 10 else None))
            if kind and kind not in picked:
                picked[kind] = (k, seed, n)
    assert set(picked) == {"first", "middle", "never"} and picked["never"][2] == 10
    for kind, (k, seed, n) in picked.items():
        ref_rng, rng = np.random.RandomState(seed), np.random.RandomState(seed)
        want = R.chopped_item(*scenes[k], WEIGHTS, P, ref_rng)
        t = T.BlockTester([scenes[k][0]], [scenes[k][1]], num_classes=C, block_points=P, batch_size=B, labelweights=WEIGHTS, rng=rng)
        probe = np.random.RandomState(seed)
        centre, m, _, tries = T.BlockTester([scenes[k][0]], [scenes[k][1]], num_classes=C, block_points=P, rng=probe).draw_crop(0)
        assert tries == n and centre == want[3]["tries"][-1]["centre"] and m == want[3]["tries"][-1]["m"]
        same_item(t.item(0), want[:3])
        np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))


def test_voxel_key_collisions_and_negative_cells(T):
    """D:53-54: the count is of distinct KEYS.  Cells (0, 1, 0) and (0, 0, 62) share key 62 and count once; and with a z
    bound above some members (handed in: a scene's own coordmin_z lies below every point, so vz >= 0 there) and a z extent
    small against the 0.01 margin, vz and the key go far below zero and are still told apart."""
    rng = np.random.default_rng(8)
    centre = np.array([0.75, 0.75, 1.0], np.float32)
    twins = np.array([[0.0, 0.024, 0.0], [0.0, 0.0, 3.0]], np.float32)
    xyz = np.concatenate([centre[None, :], twins, (rng.random((500, 3)) * [1.5, 1.5, 3.0]).astype(np.float32)])
    labels = rng.integers(0, C, xyz.shape[0])
    want = R.crop_stats(xyz, labels, centre, np.float32(0.0), np.float32(3.0))
    lo, hi = R.crop_box(centre, np.float32(0.0), np.float32(3.0))
    cells = np.ceil((xyz[want["members"]][want["mask"]] - lo) / (hi - lo) * R.GRID)
    assert len(np.unique(cells, axis=0)) > want["nuniq"]  # distinct triples collide
    t = T.BlockTester([xyz], [labels], num_classes=C, block_points=P)
    assert t.crop_stats(0, 0)[:3] == (want["m"], want["labelled"], want["nuniq"])

    flat = xyz.copy()
    flat[:, 2] = (np.float32(1.0) + flat[:, 2] * np.float32(0.004 / 3.0)).astype(np.float32)  # a z extent of 4 mm
    t = T.BlockTester([flat], [labels], num_classes=C, block_points=P)
    zmin, zmax = flat[:, 2].min(), flat[:, 2].max()
    want = R.crop_stats(flat, labels, flat[0], zmin, zmax)
    assert t.crop_stats(0, 0)[:3] == (want["m"], want["labelled"], want["nuniq"]) and want["keys"].min() >= 0
    raised = np.float32(zmin + np.float32(0.003))
    want = R.crop_stats(flat, labels, flat[0], raised, zmax)
    assert want["keys"].min() < -40 and want["nuniq"] > 100
    bounds = torch.tensor([0, 0, raised, 0, 0, zmax], dtype=torch.float32, device="cuda")
    assert t.crop_stats(0, 0, bounds=bounds)[:3] == (want["m"], want["labelled"], want["nuniq"])


def test_key_span_limits(T):
    """a span past the bitmap's capacity raises PasnlUnsupported (from the host's bound and from the library); zero z extent
    raises ValueError"""
    from pointasnl_amd import _hip

    rng = np.random.default_rng(9)
    xyz = (rng.random((100, 3)) * [1.0, 1.0, 1e-6] + [0, 0, 1.0]).astype(np.float32)
    xyz[:, 2] = np.where(np.arange(100) % 2 == 0, np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0)))
    labels = rng.integers(0, C, 100)
    t = T.BlockTester([xyz], [labels], num_classes=C, block_points=P)
    with pytest.raises(_hip.PasnlUnsupported):
        t.item(0)
    cap = t.key_capacity
    hist = torch.zeros((4,), dtype=torch.int32, device="cuda")
    args = (ctypes.c_long(100), ptr(t.xyz[0]), ptr(t.labels[0]), ptr(t.bounds), ctypes.c_long(0), ctypes.c_longlong(0))
    with pytest.raises(_hip.PasnlUnsupported):
        _hip.launch("pasnl_block_crop_stats", "span", *args, ctypes.c_long(cap + 1), ptr(hist), ptr(t.bitmap), ptr(t.stats))
    xyz[:, 2] = np.float32(1.0)
    t = T.BlockTester([xyz], [labels], num_classes=C, block_points=P)
    with pytest.raises(ValueError):
        t.item(0)


def test_whole_scene_grid_with_an_empty_column(T, scenes):
    """D:98-122 on the 3 x 2 scene: the column list (one empty column, skipped without a draw), the draws and the rows"""
    p, l = scenes[2]
    ref_rng, rng = np.random.RandomState(11), np.random.RandomState(11)
    t = T.BlockTester([p], [l], num_classes=C, block_points=P, labelweights=WEIGHTS, rng=rng)
    shape, counts, _ = t.column_counts(0)
    rshape, rcounts, found = R.columns(p[:, 0:3])
    assert shape == rshape == (3, 2) and (counts == 0).sum() == 1
    np.testing.assert_array_equal(counts, rcounts)
    want = R.whole_item(p, l, WEIGHTS, P, ref_rng)
    got = t.scene_blocks(0)
    assert got[0].shape[0] == len(found) == 5
    same_item(got, want[:3])
    np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))


def test_normalize_equals_numpy_bit_for_bit(T, scenes):
    """P:8-24 in float64, rounded once to float32: the centroid's chain of adds, the norm's (x*x + y*y) + z*z, the division"""
    p, l = scenes[1]
    t = T.BlockTester([p], [l], num_classes=C, block_points=128, batch_size=B, rng=np.random.RandomState(2))
    data, _, _ = t.scene_blocks(0)
    raw = host(data)
    got = host(t.normalize(data, B))
    want = raw[:B].astype(np.float64)
    want[:, :, :3] = R.normalize_data(want[:, :, :3])
    np.testing.assert_array_equal(bits(got), bits(want.astype(np.float32)))


def device_forward(w, b, fed, logits):
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()

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
            assert ulps_apart(got[:, :, :3], x[:, :, :3]).max() <= 1.0
            np.testing.assert_array_equal(bits(got[:, :, 3:]), bits(x[:, :, 3:]))
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
    assert got[1:] == want[1:] and len(got) == (5 if whole else 4)
    head, value = got[0].rsplit(" ", 1)
    assert head == want[0].rsplit(" ", 1)[0] and abs(float(value) - float(want[0].rsplit(" ", 1)[1])) <= 2e-5 * max(1.0, abs(out["mean_loss"]))


def test_score_argmax_rule_and_the_loss_without_a_weighted_entry(T, scenes):
    """T:311-321 on logits with ties and NaN: np.argmax over ALL classes takes the first maximum and the first NaN, and the
    integer counters are the restatement's; a NaN row under a non-zero weight makes the loss NaN there as here; a batch
    whose weights are all zero has loss 0 (count(w != 0) == 0), not 0 / 0."""
    rng = np.random.default_rng(12)
    t = T.BlockTester([scenes[0][0]], [scenes[0][1]], num_classes=C, block_points=P, batch_size=B)
    logits = rng.standard_normal((B, P, C)).astype(np.float32)
    logits[0, 0:8, :] = np.nan
    logits[0, 8:16, 2] = np.nan
    logits[0, 16:24, 3:] = np.nan
    logits[1, :, 1] = logits[1, :, 3] = 9.0
    logits[2, 0:32, :] = 0.25
    label = rng.integers(0, C, (B, P)).astype(np.int32)
    smpw = (WEIGHTS[label] * (rng.random((B, P)) < 0.8)).astype(np.float32)
    dev = [torch.from_numpy(a).cuda() for a in (logits, label, smpw)]
    t.score(*dev)
    t._finish(1, False)
    out = R.new_totals(C)
    R.score(out, logits, label, smpw, C)
    tot = t.totals()
    assert (tot["total_correct"], tot["total_seen"]) == (out["total_correct"], out["total_seen"]) and out["total_correct"] > 0
    for name in ("seen", "correct", "deno", "hist"):
        np.testing.assert_array_equal(tot[name], out[name])
    assert np.isnan(out["losses"][0]) and np.isnan(t.mean_loss())
    t.reset()
    smpw[0, 0:24] = 0.0  # the NaN rows carry no weight: the loss is finite again
    t.score(dev[0], dev[1], torch.from_numpy(smpw).cuda())
    t._finish(1, False)
    want = R.classify_loss(logits, label, smpw)
    print("loss: device %.9f, restatement %.9f" % (t.mean_loss(), want))
    assert np.isfinite(want) and abs(t.mean_loss() - want) <= 1e-5 * max(1.0, abs(want))
    t.reset()
    t.score(dev[0], dev[1], torch.zeros((B, P), dtype=torch.float32, device="cuda"))
    t._finish(1, False)
    assert t.mean_loss() == 0.0 and R.classify_loss(logits, label, np.zeros((B, P), np.float32)) == 0.0
    assert t.totals()["total_seen"] == 0 and t.totals()["hist"].sum() == B * P


@pytest.mark.parametrize("rgb", [True, False])
def test_run_whole_through_every_branch_of_the_carry_over(T, scenes, rgb):
    """T:333-420 over six scenes of 2, 1, 5, 4, 1, 1 blocks with B = 3: fewer than B (continue), exactly B, more than B, B
    rows still carried after the forward (4 + 2 -> 3 fed, 3 carried), rows left unscored at the end.  The batches fed, the
    counters, mIoU, the mean loss (divided by S, not by the forwards) and the report lines are the restatement's."""
    p0, l0 = scenes[0]
    two = (np.concatenate([p0, p0 + np.array([1.6, 0, 0, 0, 0, 0], np.float32)]).astype(np.float32), np.concatenate([l0, l0]))
    order = [two, scenes[0], scenes[2], scenes[1], scenes[0], scenes[0]]
    order = [(p if rgb else p[:, 0:3], l) for p, l in order]
    ref_rng, rng = np.random.RandomState(21), np.random.RandomState(21)
    w, b = R.stand_in_weights(3, C)
    fed, logits = [], []
    t = T.BlockTester([p for p, _ in order], [l for _, l in order], num_classes=C, block_points=P, batch_size=B, labelweights=WEIGHTS, rng=rng)
    miou = t.run_whole(device_forward(w, b, fed, logits))
    forward, asked = replay(fed, logits, False)
    blocks = []

    def getitem(i):
        item = R.whole_item(*order[i], WEIGHTS, P, ref_rng, with_rgb=rgb)
        blocks.append(item[0].shape[0])
        return item[:3]

    out = R.eval_whole(getitem, len(order), B, forward, C, extra=0.125)
    assert blocks == [2, 1, 5, 4, 1, 1] and asked[0] == len(fed) == 4 and out["num_batches"] == 6
    assert t.left == out["left"] == 2 and t.forwards == 4 and miou == out["miou"]
    same_results(t, out, True, 0.125)
    np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))


def test_run_chopped_drops_the_remainder_and_rotates(T, scenes):
    """T:279-329 over seven scenes with B = 3: two batches, the seventh scene is never drawn; B items, then B angles; the
    rotated coordinates within one float32 ulp of numpy's float64 product, rgb, labels and weights exact."""
    order = [scenes[k] for k in (0, 1, 2, 3, 1, 2, 0)]
    ref_rng, rng = np.random.RandomState(31), np.random.RandomState(31)
    w, b = R.stand_in_weights(4, C)
    fed, logits = [], []
    t = T.BlockTester([p for p, _ in order], [l for _, l in order], num_classes=C, block_points=P, batch_size=B, labelweights=WEIGHTS, rng=rng)
    miou = t.run_chopped(device_forward(w, b, fed, logits))
    forward, asked = replay(fed, logits, True)
    out = R.eval_chopped(lambda i: R.chopped_item(*order[i], WEIGHTS, P, ref_rng)[:3], len(order), B, P, 6, forward, C, ref_rng, extra=0.5)
    assert asked[0] == len(fed) == 2 == out["num_batches"] == t.num_batches and miou == out["miou"]
    assert np.abs(fed[0][:, :, :2] - out["fed"][0][:, :, :2]).max() < 1e-5 and np.abs(fed[0][:, :, :3]).max() <= 1.0 + 1e-6
    np.testing.assert_array_equal(host(t.batch_label), out["labels"][-1])
    np.testing.assert_array_equal(bits(host(t.batch_smpw)), bits(out["smpw"][-1]))
    same_results(t, out, False, 0.5)
    np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))


@pytest.mark.parametrize("kind", ["chopped", "whole"])
def test_drop_in_dataset_classes(gold, scenes, kind):
    """`ScannetDataset` / `ScannetDatasetWholeScene` from the four lists in memory: `__len__`, `__getitem__` (the reference's
    dtypes, float64 weights included) against the fixture, and the split='train' label weights against the reference's"""
    from pointasnl_amd.ScanNet import scannet_dataset as D

    cls = D.ScannetDataset if kind == "chopped" else D.ScannetDatasetWholeScene
    Pg = int(gold["block_points"][0])
    for split, rgb in (("val", False), ("train", True)):
        tag = "%s/%s/%s" % (kind, "rgb" if rgb else "xyz", split)
        rng = np.random.RandomState(int(gold["seed"][0]))
        ds = cls(None, block_points=Pg, split=split, with_rgb=rgb, scene_points_list=[p.copy() for p, _ in scenes],
                 semantic_labels_list=[l.copy() for _, l in scenes], scene_points_id=[np.arange(len(l)) for _, l in scenes],
                 scene_points_num=[len(l) for _, l in scenes], rng=rng)
        assert len(ds) == int(gold[tag + "/len"][0]) == 4
        np.testing.assert_array_equal(bits(ds.labelweights), bits(gold[tag + "/labelweights"]))
        for visit in range(4):
            item = ds[visit]
            for got, name in zip(item, ("data", "seg", "smpw")):
                want = gold["%s/%d/%s" % (tag, visit, name)]
                assert got.dtype == want.dtype and got.shape == want.shape
                np.testing.assert_array_equal(bits(got), bits(want))
            np.testing.assert_array_equal(state_of(rng), gold["%s/%d/rng" % (tag, visit)])


def spread(seed, n, extent):
    """n points uniform over `extent` metres from (-1.0, 0.3, 0.1), and labels -> (n,3) f32, (n,) i64"""
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * extent + [-1.0, 0.3, 0.1]).astype(np.float32), rng.integers(0, C, n)


def same_columns(T, t, xyz, hist, counts):
    """the grid's counts and, through pasnl_block_fill, its lists and masks against the restatement's"""
    shape, rcounts, found = R.columns(xyz)
    np.testing.assert_array_equal(counts, rcounts)
    idx, mask = device_lists(T, t.xyz[0], t.bounds[0], -1, shape[0], shape[1], hist, counts)
    np.testing.assert_array_equal(idx, np.concatenate([m for _, m, _ in found]))
    np.testing.assert_array_equal(mask.astype(bool), np.concatenate([m for _, _, m in found]))
    return shape, found


@pytest.mark.parametrize("n", [2, 63, 64, 65, 257])
def test_crop_and_grid_at_every_chunking(T, n):
    """D:42-55 and D:98-115 with a two-lane wave (the smallest scene that has a grid), a wave one short of full, a full
    one, one point past the wave boundary, and five chunks (two workgroups of four): the try's statistics, the chopped
    column's list and 0.01 mask, and the grid's counts, lists and 0.001 masks are the restatement's.  One point has zero
    extent and raises as it always did."""
    xyz, labels = spread(80 + n, n, (4.0, 2.6, 2.2))
    one = T.BlockTester([xyz[:1]], [labels[:1]], num_classes=C, block_points=P, batch_size=B)
    with pytest.raises(ValueError, match="zero z extent"):
        one.crop_stats(0, 0)
    with pytest.raises(ValueError, match="zero extent"):
        one.column_counts(0)
    t = T.BlockTester([xyz], [labels], num_classes=C, block_points=P, batch_size=B)
    coordmin, coordmax = R.bounds(xyz)
    for centre in sorted({0, n // 2, n - 1}):
        want = R.crop_stats(xyz, labels, xyz[centre], coordmin[2], coordmax[2])
        m, labelled, nuniq, hist = t.crop_stats(0, centre)
        assert (m, labelled, nuniq) == (want["m"], want["labelled"], want["nuniq"]) and centre in want["members"]
        idx, mask = device_lists(T, t.xyz[0], t.bounds[0], centre, 1, 1, hist, np.array([m]))
        np.testing.assert_array_equal(idx, want["members"])
        np.testing.assert_array_equal(mask.astype(bool), want["mask"])
    shape, counts, hist = t.column_counts(0)
    assert same_columns(T, t, xyz, hist, counts)[0] == shape and (n < 63 or shape == (3, 2))


def test_more_than_64_columns_per_axis(T):
    """300 points over 100 m x 2 m: 66 or more columns of 1.5 m in x, which the 64-bit masks of the earlier kernels
    refused; most columns are empty for any one wave.  Counts, lists, masks and the rows are the restatement's; and the
    count kernel stores only non-zero counts, so the entry point must clear a stale histogram itself."""
    from pointasnl_amd import _hip

    n = 300
    xyz, labels = spread(91, n, (100.0, 2.0, 2.2))
    ref_rng, rng = np.random.RandomState(91), np.random.RandomState(91)
    t = T.BlockTester([xyz], [labels], num_classes=C, block_points=P, batch_size=B, labelweights=WEIGHTS, rng=rng)
    shape, counts, hist = t.column_counts(0)  # (raises PasnlUnsupported if the limit came back)
    assert shape[0] > 64
    _, found = same_columns(T, t, xyz, hist, counts)
    assert any((np.bincount(m // 64, minlength=5) == 0).any() for _, m, _ in found)  # cells no wave ever stores
    same_item(t.scene_blocks(0), R.whole_item(xyz, labels, WEIGHTS, P, ref_rng, with_rgb=False)[:3])
    np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))
    stale = torch.full_like(hist, 0x7f7f7f7f)
    cnt = torch.full((shape[0] * shape[1],), -1, dtype=torch.int32, device="cuda")
    _hip.launch("pasnl_block_grid_count", "count", ctypes.c_long(n), ptr(t.xyz[0]), ptr(t.bounds[0]), shape[0], shape[1], ptr(stale), ptr(cnt))
    np.testing.assert_array_equal(host(cnt), counts)
    same_columns(T, t, xyz, stale, counts)
