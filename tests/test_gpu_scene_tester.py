"""GPU: the ScanNet grid test and validation loops on the device (csrc/scene_test.hip, the scene entries of csrc/crop.hip,
pointasnl_amd.ScanNet.scene_tester) against the numpy restatement tests/scene_flow_ref.py (pinned to the reference's
generator and metrics in tests/test_scene_tester_flow.py) and the golden run tests/golden/scene_flow.npz."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import scene_flow_ref as R
from scan_flow_ref import proj_brute, stand_in_forward_np
from scene_flow_ref import SceneFlowRef, nearest_first, scene, softmax_f32

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def T():
    from pointasnl_amd.ScanNet import scene_tester as T

    return T


def _hip():
    from pointasnl_amd import _hip

    return _hip


def P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def make_desc(off, cloud, pick, n, k, centre):
    d = np.zeros(48, np.uint8)
    d[0:8] = np.array([off], np.int64).view(np.uint8)
    d[8:24] = np.array([cloud, pick, n, k], np.int32).view(np.uint8)
    d[24:48] = np.asarray(centre, np.float64).view(np.uint8)
    return d


def desc_of(d):
    """decode one pasnl_scene_crop_t (48,) uint8 -> offset, (cloud, pick, n, k), centre f64"""
    a = d.cpu().numpy().reshape(-1)
    return int(a[0:8].copy().view(np.int64)[0]), a[8:24].copy().view(np.int32), a[24:48].copy().view(np.float64)


def scenes_of(seeds_sizes, snapped=False):
    pc = [scene(s, n, snapped) for s, n in seeds_sizes]
    return [p for p, _ in pc], [c for _, c in pc]


def test_pick_is_numpy_argmin_and_float64_centre():
    rng = np.random.default_rng(0)
    cases = []
    a = [rng.random(3000), rng.random(5000), rng.random(1)]
    cases.append((a, [float(np.min(x)) for x in a]))
    b = [np.full(4000, 0.25), np.full(2500, 0.25)]  # ties everywhere: first scene, first index
    b[1][1700] = b[1][2400] = 0.1
    cases.append((b, [0.1, 0.1]))
    c = [rng.random(2000), rng.random(3000)]
    c[1][77] = c[1][1500] = np.nan
    cases.append((c, [0.5, float(np.min(c[1]))]))  # min propagates NaN: the NaN scene is picked, then its first NaN
    cases.append(([np.array([0.3]), np.array([0.2]), np.array([0.2])], [0.3, 0.2, 0.2]))  # one-point scenes
    e = [rng.random(1500), -np.zeros(1000), np.zeros(900)]  # -0 == +0
    cases.append((e, [0.5, -0.0, 0.0]))
    for pots, mins in cases:
        pts = [(rng.random((len(p), 3)) * 7).astype(np.float32) for p in pots]
        noise = rng.normal(scale=0.35, size=(1, 3))
        offs = np.concatenate([[0], np.cumsum([len(p) for p in pots])]).astype(np.int64)
        desc = torch.zeros((48,), dtype=torch.uint8, device="cuda")
        cloud = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        k = torch.tensor([5], dtype=torch.int32, device="cuda")
        args = [dev(offs), dev(np.concatenate(pots)), dev(np.asarray(mins, np.float64)), dev(np.concatenate(pts)), k, dev(noise)]
        _hip().launch("pasnl_scene_pick", "pick", len(pots), *[P(t) for t in args], P(desc), P(cloud))
        off, ints, centre = desc_of(desc)
        wc = int(np.argmin(mins))
        wp = int(np.argmin(pots[wc]))
        assert (int(cloud.item()), ints[0], ints[1], ints[2], ints[3], off) == (wc, wc, wp, len(pots[wc]), 5, offs[wc])
        want = pts[wc].astype(np.float64)[wp].reshape(1, -1) + noise  # D:485-489
        np.testing.assert_array_equal(bits(centre), bits(want[0]))


@pytest.mark.parametrize("seed,snapped", [(0, False), (1, True), (2, True)])
def test_scene_crop_is_the_restatement_and_the_indirect_crop(T, seed, snapped):
    pts, cols = scenes_of([(300 + seed, 9000), (310 + seed, 23000), (320 + seed, 4100)], snapped)
    tester = T.SceneTester(pts, colors=cols, num_classes=4, num_point=2000, num_buffer=400, batch_size=2,
                           label_values=np.arange(4), rng=np.random.RandomState(seed))
    rng = np.random.default_rng(seed)
    idx = torch.full((tester.kcap,), -1, dtype=torch.int32, device="cuda")
    d2 = torch.zeros((tester.kcap,), dtype=torch.float64, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")

    def crop(desc_bytes, symbol):
        idx.fill_(-1)
        dd = dev(desc_bytes)  # (kept alive across the launch)
        _hip().launch(symbol, "crop", 1, ctypes.c_long(tester.nmax), P(tester.points), P(dd), tester.kcap, P(idx), P(d2), P(cnt),
                      P(tester.ws), ctypes.c_size_t(tester.ws_bytes))
        return int(cnt.item()), idx.cpu().numpy().copy(), d2.cpu().numpy().copy()
    for ci, pick, k in [(1, 5, 2399), (0, 8999, 2000), (2, 17, 2100), (1, 22999, 2200)]:
        s = pts[ci]
        off = int(tester.offsets_host[ci])
        centre = s[pick].astype(np.float64) + rng.normal(scale=0.35, size=3)
        if snapped:
            centre = np.round(centre / 0.02) * 0.02  # on the half lattice: many equal distances
        n, gi, gd = crop(make_desc(off, ci, pick, len(s), k, centre), "pasnl_knn_crop_scene")
        order, key = nearest_first(s.astype(np.float64), centre, k)
        assert n == k
        np.testing.assert_array_equal(gi[:k], np.sort(order))  # the selected set, ascending; boundary ties to the lowest index
        np.testing.assert_array_equal(bits(gd[:k]), bits(key[np.sort(order)]))
        # a float32-representable centre: bit for bit pasnl_knn_crop_indirect
        n1, i1, d1 = crop(make_desc(off, ci, pick, len(s), k, s[pick].astype(np.float64)), "pasnl_knn_crop_scene")
        d40 = np.zeros(40, np.uint8)
        d40[0:8] = np.array([off], np.int64).view(np.uint8)
        d40[8:24] = np.array([ci, pick, len(s), k], np.int32).view(np.uint8)
        d40[24:36] = s[pick].view(np.uint8)
        n2, i2, d2_ = crop(d40, "pasnl_knn_crop_indirect")
        assert n1 == n2 == k
        np.testing.assert_array_equal(i1[:k], i2[:k])
        np.testing.assert_array_equal(bits(d1[:k]), bits(d2_[:k]))


def _assert_state(tester, ref):
    for i in range(len(ref.scenes)):
        np.testing.assert_array_equal(bits(tester.potentials_of(i).cpu().numpy()), bits(ref.potentials[i]))
    np.testing.assert_array_equal(bits(tester.min_potentials()), bits(np.asarray(ref.min_potentials, np.float64)))


@pytest.mark.parametrize("with_rgb,abs_coords", [(True, True), (True, False), (False, False)])
def test_next_batch_is_the_restatement(T, with_rgb, abs_coords):
    """point_inds, cloud_inds, every column of the model input and the potentials, bit for bit, crop after crop, on plain
    and lattice-snapped scenes"""
    for snapped in (False, True):
        pts, cols = scenes_of([(40 + snapped, 6000), (41, 5000), (42, 7000)], snapped)
        kw = dict(num_classes=4, num_point=1024, num_buffer=256, batch_size=2, label_values=np.arange(4))
        tester = T.SceneTester(pts, colors=cols if with_rgb else None, with_rgb=with_rgb, abs_coords=abs_coords,
                               rng=np.random.RandomState(9), **kw)
        ref = SceneFlowRef(pts, colors=cols, rng=np.random.RandomState(9), **kw)
        for _ in range(6):
            x, inds, clouds = tester.next_batch()
            rx, ri, rc, _ = ref.batch(abs_coords=abs_coords, with_rgb=with_rgb)
            assert x.shape == (2, 1024, 3 + 3 * with_rgb + 3 * abs_coords)
            np.testing.assert_array_equal(clouds.cpu().numpy(), rc)
            np.testing.assert_array_equal(inds.cpu().numpy(), ri)
            np.testing.assert_array_equal(bits(x.cpu().numpy()), bits(rx))
            _assert_state(tester, ref)


def test_next_batch_over_the_golden_epochs(T):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_scene_flow as M

    gold = np.load(os.path.join(HERE, "golden", "scene_flow.npz"))
    pts, cols = M.scenes()
    for split in ("test", "validation"):
        tester = T.SceneTester(pts, colors=cols, num_classes=M.NUM_CLASSES, num_point=M.NUM_POINT, num_buffer=M.NUM_BUFFER,
                               batch_size=M.BATCH, split=split, validation_size=M.VALIDATION_SIZE, label_values=M.LABEL_VALUES,
                               ignored_labels=M.IGNORED, rng=np.random.RandomState(M.SEED))
        got_c, got_i = [], []
        for e in range(M.EPOCHS):
            for _ in range(M.VALIDATION_SIZE):
                _, inds, clouds = tester.next_batch()
                got_c.append(clouds.cpu().numpy())
                got_i.append(inds.cpu().numpy())
            np.testing.assert_array_equal(bits(tester.potentials.cpu().numpy()), bits(gold[split + "_potentials"][e]))
            np.testing.assert_array_equal(bits(tester.min_potentials()), bits(gold[split + "_min_potentials"][e]))
        np.testing.assert_array_equal(np.concatenate(got_c), gold[split + "_cloud"])
        np.testing.assert_array_equal(np.concatenate(got_i), gold[split + "_selected"])


def test_update_last_write_wins_and_nan():
    """pasnl_scene_potential_update with repeated indices (numpy fancy-index +=: the last occurrence) and a crop whose points
    all coincide with its centre (0/0 -> NaN, and np.min propagates it)"""
    rng = np.random.default_rng(5)
    n, npt = 3000, 700
    pts = (rng.random((n, 3)) * 10).astype(np.float32)
    pts[2000:2100] = pts[2000]
    for case in range(2):
        pots = rng.random(n) * 1e-3
        if case == 0:
            centre = pts[11].astype(np.float64) + rng.normal(scale=0.35, size=3)
            sel = rng.integers(0, n, npt).astype(np.int32)  # many repeats
        else:
            centre = pts[2000].astype(np.float64)
            sel = rng.integers(2000, 2100, npt).astype(np.int32)
        desc, dp, dx, ds = dev(make_desc(0, 0, 11, n, npt, centre)), dev(pots), dev(pts), dev(sel)
        mins = torch.zeros((1,), dtype=torch.float64, device="cuda")
        win = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        _hip().launch("pasnl_scene_potential_update", "upd", npt, P(desc), P(dx), P(ds), P(dp), P(mins), P(win))
        dists = np.sum(np.square((pts.astype(np.float64)[sel] - centre.reshape(1, 3)).astype(np.float32)), axis=1)
        with np.errstate(invalid="ignore"):
            delta = np.square(1 - dists / np.max(dists))
        want = pots.copy()
        want[sel] += delta
        got = dp.cpu().numpy()
        # bit for bit, except the sign of a NaN (x86's 0/0 is -NaN, gfx950's +NaN; no rule of the flow reads it)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        np.testing.assert_array_equal(bits(got[ok]), bits(want[ok]))
        m = mins.cpu().numpy()
        assert (np.isnan(m[0]) and np.isnan(np.min(want))) or bits(m)[0] == bits(np.array([np.min(want)]))[0]
        assert (win.cpu().numpy() == -1).all()
        assert np.isnan(mins.item()) == (case == 1)


@pytest.mark.parametrize("split", ["test", "validation"])
def test_vote_is_bit_exact_and_softmax_error_is_bounded(T, split):
    rng = np.random.default_rng(8)
    C, npt, B = 21, 3000, 3
    pts, cols = scenes_of([(70, 4000), (71, 4000), (72, 4000)])
    kw = dict(num_classes=C, num_point=npt, num_buffer=400, batch_size=B, split=split, label_values=np.arange(C))
    tester = T.SceneTester(pts, colors=cols, rng=np.random.RandomState(0), **kw)
    ref = SceneFlowRef(pts, colors=cols, rng=np.random.RandomState(0), **kw)
    init = [(rng.random((4000, C - 1)) * 0.8).astype(np.float32) for _ in range(2)]
    for i in range(2):
        ref.test_probs[i] = init[i].copy()
        tester.test_probs(i).copy_(dev(init[i]))
    clouds = np.array([0, 1, 0], np.int32)   # crops 0 and 2 of one batch on one scene
    for rep in range(3):
        inds = rng.integers(0, 4000, (B, npt)).astype(np.int32)
        inds[0, 100:160] = 9                 # a repeated index inside a crop
        inds[2, :500] = inds[0, :500]
        logits = (rng.standard_normal((B, npt, C)) * 3).astype(np.float32)
        probs = softmax_f32(logits[:, :, 1:])
        tester.vote(dev(probs), dev(inds), dev(clouds), is_logits=False)
        ref.vote(probs, inds, clouds)
        for i in range(3):
            assert tester.test_probs(i).dtype == torch.float32
            np.testing.assert_array_equal(bits(tester.test_probs(i).cpu().numpy()), bits(ref.test_probs[i]))
    # logits in: the device's float32 softmax and numpy's, both against a float64 softmax of the same logits
    zero = T.SceneTester(pts, colors=cols, rng=np.random.RandomState(0), test_smooth=0.0, **kw)  # table = 0 * old + 1 * probs
    ident = np.tile(np.arange(npt, dtype=np.int32), (B, 1))
    zero.vote(dev(logits), dev(ident), dev(np.array([0, 1, 2], np.int32)))
    got = np.stack([zero.test_probs(i)[:npt].cpu().numpy() for i in range(3)]).astype(np.float64)
    x = logits[:, :, 1:].astype(np.float64)
    w = np.exp(x - x.max(-1, keepdims=True))
    w /= w.sum(-1, keepdims=True)
    err_dev = np.abs(got - w).max()
    err_np = np.abs(softmax_f32(logits[:, :, 1:]).astype(np.float64) - w).max()
    print(f"softmax worst error vs float64: device {err_dev:.3e}, numpy float32 {err_np:.3e}")
    assert err_dev <= 2 * err_np


@pytest.mark.parametrize("ignored", [(0,), (4,)])
def test_reprojection_outputs_are_exact(T, ignored):
    lv = np.array([0, 1, 2, 4, 7, 9])
    nc = len(lv) - len(ignored)
    pts, cols = scenes_of([(80, 3000), (81, 3000)])
    kw = dict(num_classes=nc + 1, num_point=1000, num_buffer=100, batch_size=2, label_values=lv, ignored_labels=ignored)
    tester = T.SceneTester(pts, colors=cols, rng=np.random.RandomState(0), **kw)
    ref = SceneFlowRef(pts, colors=cols, rng=np.random.RandomState(0), **kw)
    rng = np.random.default_rng(1)
    tab = (rng.random((3000, nc)) * 0.5).astype(np.float32)
    tab[:50, 1] = tab[:50, 3] = np.float32(0.75)   # ties: the first maximum
    tab[50:60] = 0                                  # all-equal rows: column 0 of the expanded row
    tab[60:70, 2] = np.nan                          # numpy's argmax takes the first NaN
    tester.test_probs(1).copy_(dev(tab))
    ref.test_probs[1] = tab
    raw = scene(82, 5000)[0]
    proj = proj_brute(pts[1], raw)
    for kwargs, rproj in ((dict(raw_points=raw), proj), (dict(proj_inds=proj), proj), (dict(), None)):
        preds, pots, probs = tester.reproject(1, **kwargs)
        wp, wo, wb = ref.reproject(1, rproj)
        assert preds.dtype == np.int32 and pots.dtype == np.float64 and probs.dtype == np.float32
        np.testing.assert_array_equal(preds, wp)
        np.testing.assert_array_equal(bits(pots), bits(wo))
        np.testing.assert_array_equal(bits(probs), bits(wb))


def test_confusion_matrix_is_exact(T):
    rng = np.random.default_rng(2)
    lv = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39], np.int32)  # ScanNet's 21 values
    total = np.zeros((21, 21), np.int64)
    acc = torch.zeros((21, 21), dtype=torch.int64, device="cuda")
    for n in (0, 1, 100000, 3000000):
        p = rng.random(21) ** 4
        p /= p.sum()                                    # skewed classes
        pool = np.append(lv, [13, -1, 40])              # values outside label_values
        pp = np.append(p * 0.97, [0.01, 0.01, 0.01])
        t = rng.choice(pool, n, p=pp).astype(np.int32)
        q = np.where(rng.random(n) < 0.7, t, rng.choice(pool, n, p=pp)).astype(np.int32)
        got = T.confusion_matrix(t, q, lv)
        ti, qi = np.searchsorted(lv, t), np.searchsorted(lv, q)
        ok = (ti < 21) & (qi < 21)
        ok[ok] &= (lv[ti[ok]] == t[ok]) & (lv[qi[ok]] == q[ok])
        want = np.bincount(ti[ok] * 21 + qi[ok], minlength=441).reshape(21, 21).astype(np.int64)
        if n <= 100000:
            np.testing.assert_array_equal(want, R.confusion(t, q, lv))
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, want)
        total += want
        dt, dq, dl = dev(t), dev(q), dev(lv)  # (kept alive across the launch)
        _hip().launch("pasnl_confusion_matrix", "cm", ctypes.c_long(n), P(dt) if n else ctypes.c_void_p(0),
                      P(dq) if n else ctypes.c_void_p(0), P(dl), 21, P(acc))
    np.testing.assert_array_equal(acc.cpu().numpy(), total)  # accumulation over scenes is the sum


def _stand_in(C, w, b):
    wt, bt = dev(w), dev(b)
    return (lambda x: torch.sin(x[:, :, :3] @ wt + bt) * 4.0), (lambda x: stand_in_forward_np(x[:, :, :3], w, b))


@pytest.mark.parametrize("split", ["test", "validation"])
def test_run_end_to_end_against_restatement_and_golden(T, split):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_scene_flow as M

    gold = np.load(os.path.join(HERE, "golden", "scene_flow.npz"))
    fwd_t, fwd_np = _stand_in(M.NUM_CLASSES, *M.forward_weights())
    pts, cols = M.scenes()
    tester = T.SceneTester(pts, colors=cols, num_classes=M.NUM_CLASSES, num_point=M.NUM_POINT, num_buffer=M.NUM_BUFFER,
                           batch_size=M.BATCH, split=split, validation_size=M.VALIDATION_SIZE, label_values=M.LABEL_VALUES,
                           ignored_labels=M.IGNORED, rng=np.random.RandomState(M.SEED))
    ref = M.make_ref(split)
    fired_t, fired_r = [], []
    got_inds, got_clouds = [], []
    orig = tester.next_batch

    def spy():
        out = orig()
        got_inds.append(out[1].cpu().numpy().copy())
        got_clouds.append(out[2].cpu().numpy().copy())
        return out
    tester.next_batch = spy
    e1 = tester.run(fwd_t, num_votes=M.NUM_VOTES, max_epochs=M.EPOCHS, on_checkpoint=lambda t, m: fired_t.append(float(m)))
    e2 = ref.run(fwd_np, num_votes=M.NUM_VOTES, max_epochs=M.EPOCHS, on_checkpoint=lambda t, m: fired_r.append(float(m)))
    assert e1 == e2 == int(gold[split + "_epochs"][0]) == M.EPOCHS
    assert tester.checkpoints == ref.checkpoints and fired_t == fired_r == [m for _, m in ref.checkpoints]
    np.testing.assert_array_equal(np.asarray(tester.checkpoints, np.float64).reshape(-1, 2), gold[split + "_checkpoints"])
    assert len(fired_t) >= 1
    np.testing.assert_array_equal(np.concatenate(got_clouds), gold[split + "_cloud"])
    np.testing.assert_array_equal(np.concatenate(got_inds), gold[split + "_selected"])
    np.testing.assert_array_equal(bits(tester.potentials.cpu().numpy()), bits(gold[split + "_potentials"][-1]))
    np.testing.assert_array_equal(bits(tester.min_potentials()), bits(gold[split + "_min_potentials"][-1]))
    # The votes: the stand-in's logits differ between torch on the device and numpy by a few float32 ulps of a value <= 4
    # (the 3-term dot, sin, the softmax's exp) -- under 1e-5 on a probability -- and a table entry is a convex combination of
    # such probabilities, so it inherits the bound.
    table = np.concatenate([tester.test_probs(i).cpu().numpy() for i in range(3)])
    assert np.abs(table - gold[split + "_test_probs"]).max() <= 2e-5
    assert np.abs(table - np.concatenate(ref.test_probs)).max() <= 2e-5
    # labels, confusion, IoU: with the restatement's tables on the device the scoring is exact
    for i in range(3):
        tester.test_probs(i).copy_(dev(ref.test_probs[i]))
    labels = M.labels()
    C = tester.confusion(labels)
    np.testing.assert_array_equal(C, gold[split + "_confusion"])
    np.testing.assert_array_equal(C, ref.confusion(labels))
    raw = [scene(970 + i, 700)[0] for i in range(3)]
    proj = [proj_brute(pts[i], raw[i]) for i in range(3)]
    mesh_labels = [np.random.default_rng(i).choice(M.LABEL_VALUES, 700).astype(np.int32) for i in range(3)]
    Cm = tester.confusion(mesh_labels, proj_inds=proj)
    np.testing.assert_array_equal(Cm, ref.confusion(mesh_labels, proj))
    from pointasnl_amd.ScanNet.scene_tester import iou_from_confusions

    ious = iou_from_confusions(tester.drop_ignored(Cm))
    np.testing.assert_array_equal(ious, R.iou_from_confusions(R.drop_ignored(Cm, M.LABEL_VALUES, M.IGNORED)))
    assert ious.shape == (M.NUM_CLASSES - 1,)


def test_next_batch_captured_and_replayed_equals_eager(T):
    pts, cols = scenes_of([(60, 5000), (61, 6000), (62, 4500)])
    kw = dict(num_classes=4, num_point=1024, num_buffer=256, batch_size=2, label_values=np.arange(4))
    eager = T.SceneTester(pts, colors=cols, rng=np.random.RandomState(4), **kw)
    cap = T.SceneTester(pts, colors=cols, rng=np.random.RandomState(4), **kw)
    want = [[t.cpu().numpy() for t in eager.next_batch()] for _ in range(3)]
    out = (torch.empty((2, 1024, 6), device="cuda"), torch.empty((2, 1024), dtype=torch.int32, device="cuda"),
           torch.empty((2,), dtype=torch.int32, device="cuda"))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            cap.enqueue(out)
    torch.cuda.current_stream().wait_stream(s)
    for w in want:
        cap.stage(cap.draw_batch())
        g.replay()
        for a, b in zip(out, w):
            np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(b))
    np.testing.assert_array_equal(bits(cap.potentials.cpu().numpy()), bits(eager.potentials.cpu().numpy()))


def test_construction_rejects(T):
    big, col = scene(1, 20000)
    with pytest.raises(NotImplementedError):
        T.SceneTester([big] * 2, colors=[col] * 2, in_radius=1.2)
    small, scol = scene(2, 9000)  # 9000 < 8192 + 1024 + 255
    with pytest.raises(ValueError):
        T.SceneTester([big, small], colors=[col, scol])
    with pytest.raises(_hip().PasnlUnsupported):
        T.SceneTester([big] * 2, colors=[col] * 2, num_point=14000, num_buffer=400)  # kcap = 14499 > 14336
    with pytest.raises(ValueError):
        T.SceneTester([big] * 2, colors=[col, col[:-1]])
    with pytest.raises(ValueError):
        T.SceneTester([big] * 2, colors=[col])
    with pytest.raises(ValueError):
        T.SceneTester([big] * 2, colors=[col] * 2, label_values=np.arange(20))  # 20 columns + 1 ignored != 20 values


def test_real_model_one_validation_epoch(T):
    from pointasnl_amd.models import pointasnl_sem_seg
    from pointasnl_amd.ScanNet.scene_tester import iou_from_confusions
    from pointasnl_amd.utils import tf_util

    pts, cols = scenes_of([(120, 30000), (121, 28000)])
    lv = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39], np.int32)
    tester = T.SceneTester(pts, colors=cols, num_classes=21, num_point=8192, num_buffer=1024, batch_size=2, split="validation",
                           validation_size=2, label_values=lv, rng=np.random.RandomState(2))
    tf_util.set_store(tf_util.VariableStore(seed=5))
    seen = []

    def forward(x):
        with torch.no_grad():
            out = pointasnl_sem_seg.get_model(x, False, 21, feature_channel=3)
        lg = out[0] if isinstance(out, (tuple, list)) else out
        assert x.shape == (2, 8192, 6) and lg.shape == (2, 8192, 21) and bool(torch.isfinite(lg).all())
        seen.append(1)
        return lg.float().contiguous()
    assert tester.run(forward, num_votes=100, max_epochs=1) == 1
    assert len(seen) == 2
    for i in range(2):
        tab = tester.test_probs(i)
        assert tab.shape == (tester.sizes[i], 20) and bool(torch.isfinite(tab).all()) and float(tab.max()) > 0
    targets = [np.random.default_rng(i).choice(lv, n).astype(np.int32) for i, n in enumerate(tester.sizes)]
    C = tester.confusion(targets)
    assert C.shape == (21, 21) and C.sum() == sum(tester.sizes)
    ious = iou_from_confusions(tester.drop_ignored(C))
    assert ious.shape == (20,) and np.isfinite(ious).all()
