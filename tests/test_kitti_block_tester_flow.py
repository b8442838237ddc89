"""CPU: tests/kitti_block_flow_ref.py, the numpy restatement of SemanticKITTI's two training-time validation loops, against
the reference's own classes `SemanticKittiDataset` and `SemanticKittiDataset_whole` (imported from the reference tree, built
with __new__ over a stub scan object; skipped when the tree is absent) and against their recorded run
tests/golden/kitti_block_flow.npz (tests/golden/make_kitti_block_flow.py) -- arrays bit for bit, the RNG state included --
the two reference behaviours against the plain form, the restated epochs against a recount and a model of the carry-over
written apart from them, and the rotation against provider.rotate_point_cloud_z."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest

import kitti_block_flow_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PASNL_REFERENCE", "/root/reference")
RUNS = [("chopped", False), ("chopped", True), ("whole", False), ("whole", True)]
sys.path.insert(0, os.path.join(HERE, "golden"))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "kitti_block_flow.npz"))


def scans_of(gold):
    k, out = 0, []
    while "scan%d/points" % k in gold.files:
        out.append((gold["scan%d/points" % k], gold["scan%d/remissions" % k], gold["scan%d/labels" % k]))
        k += 1
    return out


def lut_of(gold):
    return R.label_weights_lut(dict(zip(gold["content_keys"].tolist(), gold["content_values"].tolist())))


def state_of(rng):
    st = rng.get_state()
    return np.concatenate([st[1].astype(np.int64), [st[2]]])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def same(got, want, dtypes=(np.float32, np.int32, np.float32)):
    for a, b, dt in zip(got, want, dtypes):
        assert a.dtype == b.dtype == dt and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(bits(a), bits(b))


def test_fixture_scans_are_the_recorded_inputs(gold):
    scans = scans_of(gold)
    assert len(scans) == 5 and os.path.getsize(os.path.join(HERE, "golden", "kitti_block_flow.npz")) < os.path.getsize(
        os.path.join(HERE, "golden", "block_flow.npz"))
    for got, want in zip(R.fixture_scans(), scans):
        same(got, want, (np.float32, np.float32, np.int32))


@pytest.mark.parametrize("kind,rem", RUNS)
@pytest.mark.parametrize("block_size,padding", [(10, 0.01), (2.5, 0.05)])
def test_restatement_equals_the_reference_classes(gold, kind, rem, block_size, padding):
    """live against the reference tree: every scan twice, data, labels and weights bit for bit, and the global RNG state"""
    if not os.path.exists(os.path.join(REF, "SemanticKITTI", "semantic_kitti_dataset.py")):
        pytest.skip("reference tree absent")
    import make_kitti_block_flow as M

    scans = scans_of(gold)
    mod = M.reference_module(REF)
    ds = M.reference_dataset(mod, kind, scans, rem, sample_points=48, block_size=block_size, padding=padding)
    rng = np.random.RandomState(77)
    np.random.seed(77)
    item = R.chopped_item if kind == "chopped" else R.whole_item
    for visit in range(2 * len(scans)):
        p, r, l = scans[visit % len(scans)]
        same(item(p, r if rem else None, l, ds.label_weights_lut, 48, rng, block_size, padding)[:3], ds[visit % len(scans)])
        np.testing.assert_array_equal(state_of(rng), state_of(np.random))


@pytest.mark.parametrize("kind,rem", RUNS)
def test_restatement_equals_the_recorded_run(gold, kind, rem):
    scans = scans_of(gold)
    tag = "%s/%s" % (kind, "rem" if rem else "xyz")
    P = int(gold["sample_points"][0])
    lut = lut_of(gold)
    np.testing.assert_array_equal(bits(lut), bits(gold[tag + "/lut"]))
    assert lut.dtype == np.float32 and int(gold[tag + "/len"][0]) == len(scans)
    rng = np.random.RandomState(int(gold["seed"][0]))
    item = R.chopped_item if kind == "chopped" else R.whole_item
    tries = []
    for visit in range(2 * len(scans)):
        p, r, l = scans[visit % len(scans)]
        got = item(p, r if rem else None, l, lut, P, rng, int(gold["block_size"][0]), float(gold["padding"][0]))
        same(got[:3], [gold["%s/%d/%s" % (tag, visit, name)] for name in ("data", "seg", "smpw")])
        np.testing.assert_array_equal(state_of(rng), gold["%s/%d/rng" % (tag, visit)].astype(np.int64))
        tries.append(len(got[3]["tries"]) if kind == "chopped" else got[0].shape[0])
    if kind == "chopped":
        assert tries[:4] == [1, 2, 1, 10] == gold[tag + "/tries"][:4].tolist()  # first try, a later try, never
    else:
        assert tries[:5] == [1, 12, 5, 9, 5]
        assert (R.columns(scans[4][0])[1] == 0).sum() == 1  # an empty column, skipped without a draw


@pytest.mark.parametrize("kind", ["chopped", "whole"])
def test_the_two_reference_behaviours_and_the_plain_form(gold, kind):
    """quirks: smpw[e] = lut[label[seg[e]]] * mask and the remission of scan point number choice[e]; plain: lut[seg[e]] * mask
    and the member's own remission.  Same draws, same coordinates and labels; they differ in the weights and the remission."""
    p, r, l = scans_of(gold)[1]
    lut = lut_of(gold)
    item = R.chopped_item if kind == "chopped" else R.whole_item
    q = item(p, r, l, lut, 64, np.random.RandomState(3), reference_quirks=True)
    plain = item(p, r, l, lut, 64, np.random.RandomState(3), reference_quirks=False)
    info = q[3]
    if kind == "chopped":
        members, mask, choice = [info["members"]], [info["mask"]], [info["choice"]]
    else:
        found = R.columns(p)[2]
        members, mask, choice = [f[1] for f in found], [f[2] for f in found], info["choices"]
    data, seg, smpw = (a.reshape((-1,) + a.shape[-1:]) if a is q[0] else a.reshape(-1) for a in q[:3])
    pdata, pseg, psmpw = (a.reshape((-1,) + a.shape[-1:]) if a is plain[0] else a.reshape(-1) for a in plain[:3])
    idx = np.concatenate([m[c] for m, c in zip(members, choice)])
    msk = np.concatenate([m[c] for m, c in zip(mask, choice)])
    raw = np.concatenate(choice)
    np.testing.assert_array_equal(seg, l[idx])
    np.testing.assert_array_equal(pseg, seg)
    np.testing.assert_array_equal(bits(data[:, :3]), bits(p[idx]))
    np.testing.assert_array_equal(bits(pdata[:, :3]), bits(p[idx]))
    np.testing.assert_array_equal(bits(smpw), bits(lut[l[seg]] * msk.astype(np.float32)))
    np.testing.assert_array_equal(bits(psmpw), bits(lut[seg] * msk.astype(np.float32)))
    np.testing.assert_array_equal(bits(data[:, 3]), bits(r[raw]))
    np.testing.assert_array_equal(bits(pdata[:, 3]), bits(r[idx]))
    assert not np.array_equal(smpw, psmpw) and not np.array_equal(data[:, 3], pdata[:, 3])
    assert 0 < msk.sum() < len(msk) or kind == "chopped"
    with pytest.raises(IndexError):  # n <= max(label): the per-point weights are indexed past their end
        item(p[:15], r[:15], np.arange(15, dtype=np.int32) + 5, lut, 64, np.random.RandomState(3))


def expected_whole_batches(row_counts, B):
    """The carry-over of the whole-scan epoch over row identities only -> (fed, sizes, left): each fed batch as B (scan, row)
    pairs, the number of rows in hand after every scan, and the rows never scored.  Rows wait in `held`; a new scan's rows go
    behind them while a batch is being filled up and in front of them otherwise; at most one batch leaves per scan."""
    held, filling, fed, sizes = [], False, [], []
    for s, count in enumerate(row_counts):
        new = [(s, r) for r in range(count)]
        held = held + new if filling else new + held
        sizes.append(len(held))
        filling = len(held) < B
        if not filling:
            fed.append(held[:B])
            held = held[B:]
    return fed, sizes, len(held)


@pytest.mark.parametrize("whole", [False, True])
def test_epoch_restatements_against_an_independent_recount(gold, whole):
    """the restated epochs (T:267-328 / T:331-418) checked by properties and a recount written apart from them: which rows are
    fed in which order (all three branches of the carry-over, the rows left over, the dropped remainder), what is done to
    them (nothing / the rotation about z), the counters entry by entry, the divisor of the mean loss (S against S // B) and
    the lines of the table"""
    scans = scans_of(gold)
    C, P, B = 20, 32, 5
    lut = lut_of(gold)
    w, b = R.stand_in_weights(3, C)
    order = [0, 2, 1, 0, 3, 4, 0, 0, 2, 0, 0]  # rows 1, 5, 12, 1, 9, 5, 1, 1, 5, 1, 1
    logits = []

    def forward(fed):
        logits.append(R.stand_in_forward_np(fed, w, b))
        return logits[-1]

    rng = np.random.RandomState(4)
    if whole:
        items = [R.whole_item(scans[k][0], None, scans[k][2], lut, P, rng)[:3] for k in order]
        out = R.eval_whole(lambda i: items[i], len(order), B, forward, C, extra=0.25)
        fed, sizes, left = expected_whole_batches([it[0].shape[0] for it in items], B)
        assert any(s < B for s in sizes) and any(s == B for s in sizes) and any(s > B for s in sizes)
        assert out["rows"] == sizes and out["left"] == left > 0 and len(out["fed"]) == len(fed) < len(order)
        for k, batch in enumerate(fed):  # fed as they are: no rotation, no normalisation
            np.testing.assert_array_equal(bits(out["fed"][k]), bits(np.stack([items[s][0][r] for s, r in batch])))
            np.testing.assert_array_equal(out["labels"][k], np.stack([items[s][1][r] for s, r in batch]))
            np.testing.assert_array_equal(bits(out["smpw"][k]), bits(np.stack([items[s][2][r] for s, r in batch])))
        divisor = len(order)  # S, not the number of forwards
    else:
        items = [R.chopped_item(scans[k][0], None, scans[k][2], lut, P, rng)[:3] for k in order]
        angle_rng, mirror = np.random.RandomState(9), np.random.RandomState(9)
        out = R.eval_chopped(lambda i: items[i], len(order), B, P, 3, forward, C, angle_rng, extra=0.25)
        divisor = len(order) // B
        assert len(out["fed"]) == divisor == 2 and len(order) % B == 1  # the eleventh scan is never fed
        for k in range(divisor):
            rows = np.stack([items[k * B + i][0] for i in range(B)])
            angles = np.array([mirror.uniform() * 2 * np.pi for _ in range(B)])  # B angles behind the batch's B items
            got = out["fed"][k]
            np.testing.assert_array_equal(bits(got[:, :, 2]), bits(rows[:, :, 2]))
            x = rows[:, :, 0].astype(np.float64) * np.cos(angles)[:, None] - rows[:, :, 1].astype(np.float64) * np.sin(angles)[:, None]
            y = rows[:, :, 0].astype(np.float64) * np.sin(angles)[:, None] + rows[:, :, 1].astype(np.float64) * np.cos(angles)[:, None]
            np.testing.assert_allclose(got[:, :, 0], x, rtol=0, atol=4e-6)  # coordinates below 32 m: a float32 ulp is 2e-6
            np.testing.assert_allclose(got[:, :, 1], y, rtol=0, atol=4e-6)
            np.testing.assert_array_equal(out["labels"][k], np.stack([items[k * B + i][1] for i in range(B)]))
            np.testing.assert_array_equal(bits(out["smpw"][k]), bits(np.stack([items[k * B + i][2] for i in range(B)])))
        np.testing.assert_array_equal(state_of(angle_rng), state_of(mirror))
    assert out["num_batches"] == divisor
    tc, ts, seen, correct, deno, hist = R.recount(out["labels"], out["smpw"], logits, C)
    assert (tc, ts) == (out["total_correct"], out["total_seen"]) and ts > 0
    for got, ref in ((seen, out["seen"]), (correct, out["correct"]), (deno, out["deno"]), (hist, out["hist"])):
        np.testing.assert_array_equal(got, ref)
    iou = correct[1:] / (deno[1:].astype(np.float64) + 1e-6)
    np.testing.assert_array_equal(bits(out["class_iou"]), bits(iou))
    assert out["miou"] == iou.mean() and out["accuracy"] == tc / ts
    assert out["class_acc"] == (correct[1:] / (seen[1:].astype(np.float64) + 1e-6)).mean()
    assert out["mean_loss"] == pytest.approx((sum(out["losses"]) + 0.25 * len(out["losses"])) / divisor, rel=1e-12)
    names = ["c%d" % k for k in range(C)]
    lines = R.report(out, names, whole)
    head = "Eval whole scene" if whole else "Eval"
    assert lines[:4] == ["%s mean loss: %f" % (head, out["mean_loss"]), "Eval point avg class IoU: %f" % iou.mean(),
                         "%s point accuracy: %f" % (head, tc / ts), "%s point avg class acc: %f" % (head, out["class_acc"])]
    table = lines[4].split("\n")  # both loops print the per-class table
    assert len(lines) == 5 and table[0] == "------- IoU --------" and len(table) == C + 1 and table[C] == ""
    share = hist[1:].astype(np.float32) / hist[1:].astype(np.float32).sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        for l in range(1, C):
            assert table[l] == "class %-14s weight: %.3f, IoU: %.3f " % (names[l], share[l - 1], np.float64(correct[l]) / deno[l])


def test_rotation_is_the_providers_under_the_same_seed():
    if not os.path.exists(os.path.join(REF, "utils", "provider.py")):
        pytest.skip("reference tree absent")
    spec = importlib.util.spec_from_file_location("_ref_provider", os.path.join(REF, "utils", "provider.py"))
    provider = importlib.util.module_from_spec(spec)
    absent = importlib.util.find_spec("h5py") is None
    if absent:
        sys.modules["h5py"] = types.ModuleType("h5py")  # imported at the top of provider.py for its file readers only
    try:
        spec.loader.exec_module(provider)
    finally:
        if absent:
            del sys.modules["h5py"]
    batch = (np.random.default_rng(0).standard_normal((4, 50, 3)) * 30.0).astype(np.float32).astype(np.float64)
    np.random.seed(11)
    want = provider.rotate_point_cloud_z(batch)
    rng = np.random.RandomState(11)
    got = R.rotate_z(batch, [rng.uniform() * 2 * np.pi for _ in range(4)])
    assert want.dtype == got.dtype == np.float32
    np.testing.assert_array_equal(bits(got), bits(want))
    assert np.random.randint(1 << 30) == rng.randint(1 << 30)


def test_label_weights_helper_is_D54_58(gold):
    from pointasnl_amd.SemanticKITTI.block_tester import label_weights_from_content

    content = dict(zip(gold["content_keys"].tolist(), gold["content_values"].tolist()))
    lut = label_weights_from_content(content)
    assert lut.dtype == np.float32 and lut.shape == (20,)
    np.testing.assert_array_equal(bits(lut), bits(gold["chopped/xyz/lut"]))
