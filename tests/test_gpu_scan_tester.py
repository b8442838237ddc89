"""GPU: the SemanticKITTI test loop on the device (csrc/scan_test.hip, pasnl_knn_crop_indirect in csrc/crop.hip,
pointasnl_amd.SemanticKITTI.scan_tester) against the numpy restatement tests/scan_flow_ref.py (pinned to the reference's
generator in tests/test_scan_tester_flow.py) and the golden run tests/golden/scan_flow.npz."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from scan_flow_ref import ScanFlowRef, nearest_first, proj_brute, scan, softmax_f32, stand_in_forward_np

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def T():
    from pointasnl_amd.SemanticKITTI import scan_tester as T

    return T


def _hip():
    from pointasnl_amd import _hip

    return _hip


def P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def desc_of(d):
    """decode pasnl_scan_crop_t rows (B,40) uint8"""
    a = d.cpu().numpy()
    off = a[:, 0:8].copy().view(np.int64)[:, 0]
    ints = a[:, 8:24].copy().view(np.int32)
    return off, ints[:, 0], ints[:, 1], ints[:, 2], ints[:, 3], a[:, 24:28].copy().view(np.float32)[:, 0]


def run_pick(poss, mins, pts):
    offs = np.concatenate([[0], np.cumsum([len(p) for p in poss])]).astype(np.int64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    desc = torch.zeros((1, 40), dtype=torch.uint8, device="cuda")
    cloud = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    k = torch.tensor([5], dtype=torch.int32, device="cuda")
    o, p, m, x = dev(offs), dev(np.concatenate(poss).astype(np.float64)), dev(np.asarray(mins, np.float64)), dev(np.concatenate(pts))
    _hip().launch("pasnl_scan_pick", "pick", len(poss), P(o), P(p), P(m), P(x), P(k), P(desc), P(cloud))
    off, c, pick, n, kk, cx = desc_of(desc)
    assert int(cloud.item()) == c[0] and kk[0] == 5 and off[0] == offs[c[0]] and n[0] == len(poss[c[0]])
    assert cx[0] == np.concatenate(pts)[off[0] + pick[0], 0]
    return int(c[0]), int(pick[0])


def test_pick_is_numpy_argmin_ties_nan_single_point():
    rng = np.random.default_rng(0)
    cases = []
    a = [rng.random(3000), rng.random(5000), rng.random(1)]
    cases.append((a, [float(np.min(x)) for x in a]))
    b = [np.full(4000, 0.25), np.full(2500, 0.25)]  # ties everywhere: first scan, first index
    b[1][1700] = 0.1
    b[1][2400] = 0.1
    cases.append((b, [0.1, 0.1, ]))
    c = [rng.random(2000), rng.random(3000)]
    c[1][77] = np.nan
    c[1][1500] = np.nan
    cases.append((c, [0.5, float(np.min(c[1]))]))  # min propagates NaN: the NaN scan is picked, then its first NaN
    d = [np.array([0.3]), np.array([0.2]), np.array([0.2])]
    cases.append((d, [0.3, 0.2, 0.2]))
    e = [rng.random(1500), -np.zeros(1000), np.zeros(900)]  # -0 == +0
    cases.append((e, [0.5, -0.0, 0.0]))
    for poss, mins in cases:
        pts = [rng.random((len(p), 3)).astype(np.float32) for p in poss]
        want_c = int(np.argmin(mins))
        assert run_pick(poss, mins, pts) == (want_c, int(np.argmin(poss[want_c])))


@pytest.mark.parametrize("seed,snapped", [(0, False), (1, True), (2, True)])
def test_indirect_crop_is_bit_identical_to_knn_crop(T, seed, snapped):
    from pointasnl_amd.SemanticKITTI import semantic_kitti_dataset_grid as G

    scans = [scan(300 + seed, 9000, snapped), scan(310 + seed, 23000, snapped), scan(320 + seed, 4100, snapped)]
    tester = T.ScanTester(scans, num_classes=4, num_point=2000, num_buffer=400, batch_size=2, rng=np.random.RandomState(seed))
    for ci, pick, k in [(1, 5, 2399), (0, 8999, 2000), (2, 17, 2100), (1, 22999, 2200)]:
        s = scans[ci]
        off = int(tester.offsets_host[ci])
        d = np.zeros(40, np.uint8)
        d[0:8] = np.array([off], np.int64).view(np.uint8)
        d[8:24] = np.array([ci, pick, len(s), k], np.int32).view(np.uint8)
        d[24:36] = s[pick].view(np.uint8)
        desc = torch.from_numpy(d).cuda()
        idx = torch.full((tester.kcap,), -1, dtype=torch.int32, device="cuda")
        d2 = torch.zeros((tester.kcap,), dtype=torch.float64, device="cuda")
        cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
        _hip().launch("pasnl_knn_crop_indirect", "ind", 1, ctypes.c_long(tester.nmax), P(tester.points), P(desc), tester.kcap, P(idx),
                      P(d2), P(cnt), P(tester.ws), ctypes.c_size_t(tester.ws_bytes))
        wi, wd, wc = G.select_batch(torch.from_numpy(s).cuda(), torch.from_numpy(s[pick:pick + 1].copy()).cuda(), k=k, want_d2=True)
        assert int(cnt.item()) == int(wc.item()) == k
        np.testing.assert_array_equal(idx[:k].cpu().numpy(), wi[0].cpu().numpy())
        np.testing.assert_array_equal(d2[:k].cpu().numpy().view(np.int64), wd[0].cpu().numpy().view(np.int64))


def test_next_batch_order_permute_and_update_are_the_restatement(T):
    """order/permute (lexsort on (d2, idx) then the permutation; sklearn's order on tie-free scans) and the possibility update,
    bit for bit, crop after crop, on plain and snapped scans"""
    for snapped in (False, True):
        scans = [scan(40 + snapped, 6000, snapped), scan(41, 5000, snapped), scan(42, 7000, snapped)]
        kw = dict(num_classes=4, num_point=1024, num_buffer=256, batch_size=2)
        tester = T.ScanTester(scans, rng=np.random.RandomState(9), **kw)
        ref = ScanFlowRef(scans, rng=np.random.RandomState(9), **kw)
        for _ in range(6):
            pts, inds, clouds = tester.next_batch()
            rp, ri, rc, _ = ref.batch()
            np.testing.assert_array_equal(clouds.cpu().numpy(), rc[:, 0])
            np.testing.assert_array_equal(inds.cpu().numpy(), ri)
            np.testing.assert_array_equal(pts.cpu().numpy(), rp)
            for i in range(3):
                np.testing.assert_array_equal(tester.possibility_of(i).cpu().numpy().view(np.int64), ref.possibility[i].view(np.int64))
            np.testing.assert_array_equal(tester.min_possibility().view(np.int64), np.asarray(ref.min_possibility).view(np.int64))
    # on a tie-free scan the (d2, index) order is sklearn's nearest-first order
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    s = scan(40, 6000)
    p64 = s.astype(np.float64)
    nf, _ = nearest_first(p64, p64[123], 1200)
    np.testing.assert_array_equal(KDTree(s).query(s[123:124], k=1200)[1][0], nf)


def test_update_last_write_wins_and_nan():
    """pasnl_scan_possibility_update with repeated indices (numpy fancy-index +=: the last occurrence) and a crop whose points
    all coincide with its centre (0/0 -> NaN, and np.min propagates it)"""
    rng = np.random.default_rng(5)
    n, npt = 3000, 700
    pts = rng.random((n, 3)).astype(np.float32) * 10
    pts[2000:2100] = pts[2000]
    for case in range(2):
        poss = rng.random(n) * 1e-3
        if case == 0:
            pick = 11
            sel = rng.integers(0, n, npt).astype(np.int32)  # many repeats
        else:
            pick = 2000
            sel = rng.integers(2000, 2100, npt).astype(np.int32)
        d = np.zeros(40, np.uint8)
        d[0:8] = np.array([0], np.int64).view(np.uint8)
        d[8:24] = np.array([0, pick, n, npt], np.int32).view(np.uint8)
        d[24:36] = pts[pick].view(np.uint8)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        desc, P_, pp, ss = dev(d), dev(poss), dev(pts), dev(sel)
        mins = torch.zeros((1,), dtype=torch.float64, device="cuda")
        win = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        scratch = torch.zeros((1,), dtype=torch.float32, device="cuda")
        _hip().launch("pasnl_scan_possibility_update", "upd", npt, P(desc), P(pp), P(ss), P(P_), P(mins), P(win), P(scratch))
        pc = pts.astype(np.float64)
        dists = np.sum(np.square((pc[sel] - pc[pick]).astype(np.float32)), axis=1)
        with np.errstate(invalid="ignore"):
            delta = np.square(1 - dists / np.max(dists))
        want = poss.copy()
        want[sel] += delta
        # bit for bit, except the sign of a NaN (x86's 0/0 is -NaN, gfx950's +NaN; no rule of the flow reads it)
        got = P_.cpu().numpy()
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        np.testing.assert_array_equal(got[ok].view(np.int64), want[ok].view(np.int64))
        m = mins.cpu().numpy()
        assert (np.isnan(m[0]) and np.isnan(np.min(want))) or m.view(np.int64)[0] == np.array([np.min(want)]).view(np.int64)[0]
        assert (win.cpu().numpy() == -1).all()
        if case == 1:
            assert np.isnan(mins.item())


def test_vote_is_bit_exact_and_softmax(T):
    rng = np.random.default_rng(8)
    C, npt, B = 20, 3000, 3
    scans = [scan(70, 4000), scan(71, 4000), scan(72, 4000)]
    tester = T.ScanTester(scans, num_classes=C, num_point=npt, num_buffer=400, batch_size=B, rng=np.random.RandomState(0))
    ref = ScanFlowRef(scans, num_classes=C, num_point=npt, num_buffer=400, batch_size=B, rng=np.random.RandomState(0))
    init = [(rng.random((4000, C)) * 0.8).astype(np.float16) for _ in range(2)]
    init[0][:8] = np.float16(0.5) + np.arange(8)[:, None].astype(np.float16) * np.float16(2 ** -11)  # odd last bits
    for i in range(2):
        ref.test_probs[i] = init[i].copy()
        tester.test_probs(i).copy_(torch.from_numpy(init[i]).cuda())
    for rep in range(3):
        inds = rng.integers(0, 4000, (B, npt)).astype(np.int32)
        inds[0, 100:160] = 9                       # repeats inside a crop
        inds[2, :500] = inds[0, :500]              # crops 0 and 2 of one batch on one scan
        clouds = np.array([0, 1, 0], np.int32)
        logits = (rng.standard_normal((B, npt, C)) * 3).astype(np.float32)
        probs = softmax_f32(logits)
        probs[0, :8] = np.float32(2 ** -12)
        tester.vote(torch.from_numpy(probs).cuda(), torch.from_numpy(inds).cuda(), torch.from_numpy(clouds).cuda(), is_logits=False)
        ref.vote(probs, inds, clouds)
        for i in range(2):
            np.testing.assert_array_equal(tester.test_probs(i).cpu().numpy().view(np.uint16), ref.test_probs[i].view(np.uint16))
    # logits form: the float32 softmax here vs numpy's -> at most one float16 ulp per vote
    tester.vote(torch.from_numpy(logits).cuda(), torch.from_numpy(inds).cuda(), torch.from_numpy(clouds).cuda())
    ref.vote(softmax_f32(logits), inds, clouds)
    for i in range(2):
        a = tester.test_probs(i).cpu().numpy().view(np.uint16).astype(np.int64)
        b = ref.test_probs[i].view(np.uint16).astype(np.int64)
        assert np.abs(a - b).max() <= 1
    # the softmax of one row against float64
    x = logits[1, 5].astype(np.float64)
    w = np.exp(x - x.max())
    w /= w.sum()
    t2 = T.ScanTester(scans, num_classes=C, num_point=npt, num_buffer=400, batch_size=B, rng=np.random.RandomState(0), test_smooth=0.0)
    t2.vote(torch.from_numpy(logits).cuda(), torch.from_numpy(np.tile(np.arange(npt, dtype=np.int32), (B, 1))).cuda(),
            torch.from_numpy(np.array([0, 1, 0], np.int32)).cuda())
    got = t2.test_probs(1)[5].float().cpu().numpy()  # fp16(p): the softmax to float16 precision
    assert np.abs(got - w).max() <= 2 ** -11 * max(w.max(), 1e-3) + 1e-7


@pytest.mark.parametrize("seed,snapped,n_sub,n_raw", [(0, True, 3000, 6000), (1, True, 500, 2000), (2, False, 4000, 5000)])
def test_reprojection_is_exact(T, seed, snapped, n_sub, n_raw):
    sub = scan(500 + seed, n_sub, snapped)
    raw = scan(600 + seed, n_raw, snapped)
    raw[:200] = sub[:200]                                  # raw points ON sub points
    raw[200:210] = np.array([1000, -1000, 50], np.float32)  # far outside the grid
    got = T.project(torch.from_numpy(sub).cuda(), torch.from_numpy(raw).cuda()).cpu().numpy()
    np.testing.assert_array_equal(got, proj_brute(sub, raw))
    if not snapped:
        KDTree = pytest.importorskip("sklearn.neighbors").KDTree
        np.testing.assert_array_equal(got, KDTree(sub).query(raw, return_distance=False)[:, 0])


def test_reproject_argmax_first_max_and_lut(T):
    C = 20
    scans = [scan(80, 3000), scan(81, 3000)]
    tester = T.ScanTester(scans, num_classes=C, num_point=1000, num_buffer=100, batch_size=2, rng=np.random.RandomState(0))
    rng = np.random.default_rng(1)
    tab = (rng.random((3000, C)) * 0.5).astype(np.float16)
    tab[:50, 3] = tab[:50, 11] = np.float16(0.75)          # fp16 ties: the first maximum
    tab[50:60] = 0                                         # all-equal rows
    tester.test_probs(1).copy_(torch.from_numpy(tab).cuda())
    ref = ScanFlowRef(scans, num_classes=C, num_point=1000, num_buffer=100, batch_size=2, rng=np.random.RandomState(0))
    ref.test_probs[1] = tab
    lut = (np.arange(C + 80) * 7 + 1).astype(np.int32)
    raw = scan(82, 5000)
    proj = proj_brute(scans[1], raw)
    np.testing.assert_array_equal(tester.reproject(1, raw_points=raw, remap_lut=lut), ref.reproject(1, proj, lut))
    np.testing.assert_array_equal(tester.reproject(1, proj_inds=proj, remap_lut=lut), ref.reproject(1, proj, lut))
    got = tester.reproject(1)
    assert got.dtype == np.uint32 and (got[:50] == 3).all() and (got[50:60] == 0).all()


def _stand_in(C, seed=3):
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((3, C)) * 0.3).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    return (lambda x: torch.sin(x @ wt + bt) * 4.0), (lambda x: stand_in_forward_np(x, w, b))


def test_run_end_to_end_against_restatement_and_golden(T):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_scan_flow as M

    gold = np.load(os.path.join(HERE, "golden", "scan_flow.npz"))
    C = 6
    fwd_t, fwd_np = _stand_in(C)
    kw = dict(num_classes=C, num_point=M.NUM_POINT, num_buffer=M.NUM_BUFFER, batch_size=M.BATCH)
    tester = T.ScanTester(M.scans(), rng=np.random.RandomState(M.SEED), **kw)
    ref = ScanFlowRef(M.scans(), rng=np.random.RandomState(M.SEED), **kw)
    log = []
    got_inds, got_clouds = [], []
    orig = tester.next_batch

    def spy():
        out = orig()
        got_inds.append(out[1].cpu().numpy().copy())
        got_clouds.append(out[2].cpu().numpy().copy())
        return out
    tester.next_batch = spy
    e1 = tester.run(fwd_t, num_votes=1e9, max_epochs=M.EPOCHS)
    e2 = ref.run(fwd_np, num_votes=1e9, max_epochs=M.EPOCHS, log=log)
    assert e1 == e2 == M.EPOCHS
    np.testing.assert_array_equal(np.concatenate(got_clouds), [c for c, _, _ in log])
    np.testing.assert_array_equal(np.concatenate(got_inds), np.stack([s for _, _, s in log]))
    np.testing.assert_array_equal(np.concatenate(got_clouds), gold["cloud"])
    np.testing.assert_array_equal(np.concatenate(got_inds), gold["selected"])
    np.testing.assert_array_equal(np.concatenate([tester.possibility_of(i).cpu().numpy() for i in range(3)]).view(np.int64),
                                  gold["possibility"][-1].view(np.int64))
    np.testing.assert_array_equal(tester.min_possibility().view(np.int64), gold["min_possibility"][-1].view(np.int64))
    for i in range(3):
        a = tester.test_probs(i).cpu().numpy()
        b = ref.test_probs[i]
        assert np.abs(a.view(np.uint16).astype(np.int64) - b.view(np.uint16).astype(np.int64)).max() <= 1
        la, lb = tester.reproject(i), ref.reproject(i)
        srt = np.sort(b.astype(np.float32), 1)
        close = (srt[:, -1] - srt[:, -2]) <= np.spacing(srt[:, -1].astype(np.float16)).astype(np.float32)
        assert (la[~close] == lb[~close]).all()


def test_run_stops_on_min_possibility(T):
    C = 3
    fwd_t, _ = _stand_in(C)
    scans = [scan(90, 1300), scan(91, 1400)]
    tester = T.ScanTester(scans, num_classes=C, num_point=1024, num_buffer=64, batch_size=2, rng=np.random.RandomState(1))
    ep = tester.run(fwd_t, num_votes=0.5, max_epochs=50)
    assert ep < 50 and tester.min_possibility().min() > 0.5


def test_next_batch_captured_and_replayed_equals_eager(T):
    scans = [scan(60, 5000), scan(61, 6000), scan(62, 4500)]
    kw = dict(num_classes=4, num_point=1024, num_buffer=256, batch_size=2)
    eager = T.ScanTester(scans, rng=np.random.RandomState(4), **kw)
    cap = T.ScanTester(scans, rng=np.random.RandomState(4), **kw)
    want = [[t.cpu().numpy() for t in eager.next_batch()] for _ in range(3)]
    out = (torch.empty((2, 1024, 3), device="cuda"), torch.empty((2, 1024), dtype=torch.int32, device="cuda"),
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
            np.testing.assert_array_equal(a.cpu().numpy(), b)
    np.testing.assert_array_equal(cap.possibility.cpu().numpy().view(np.int64), eager.possibility.cpu().numpy().view(np.int64))


def test_construction_rejects(T):
    with pytest.raises(NotImplementedError):
        T.ScanTester([scan(1, 20000)] * 2, batch_size=2, in_radius=2.0)
    with pytest.raises(ValueError):
        T.ScanTester([scan(1, 20000)] * 2, batch_size=4)
    with pytest.raises(ValueError):
        T.ScanTester([scan(1, 20000), scan(2, 11000)], batch_size=2)  # 11000 < 10240 + 1024 + 255


def test_real_model_one_epoch(T):
    from pointasnl_amd.models import pointasnl_sem_seg_res
    from pointasnl_amd.utils import tf_util

    scans = [scan(120, 30000), scan(121, 28000)]
    kw = dict(num_classes=20, num_point=10240, num_buffer=1024, batch_size=2)
    tester = T.ScanTester(scans, rng=np.random.RandomState(2), **kw)
    ref = ScanFlowRef(scans, rng=np.random.RandomState(2), **kw)
    tf_util.set_store(tf_util.VariableStore(seed=5))
    seen = []

    def forward(x):
        with torch.no_grad():
            out = pointasnl_sem_seg_res.get_model(x, False, 20, feature_channel=0)
        lg = out[0] if isinstance(out, (tuple, list)) else out
        assert lg.shape == (2, 10240, 20) and bool(torch.isfinite(lg).all())
        seen.append(1)
        return lg.float().contiguous()
    orig = tester.next_batch
    got = []

    def spy():
        o = orig()
        got.append((o[2].cpu().numpy().copy(), o[1].cpu().numpy().copy()))
        return o
    tester.next_batch = spy
    tester.run(forward, num_votes=1e9, max_epochs=1)
    assert len(seen) == tester.crops_per_epoch // 2
    for c, inds in got:
        _, ri, rc, _ = ref.batch()
        np.testing.assert_array_equal(c, rc[:, 0])
        np.testing.assert_array_equal(inds, ri)
