"""GPU: the ModelNet40 evaluation loop on the device (csrc/modelnet_test.hip, pointasnl_amd.modelnet_tester and the
reference-named dataset class) against the numpy restatement tests/modelnet_flow_ref.py run live on the same machine (it is
pinned to the reference's class in tests/test_modelnet_tester_flow.py).  Every comparison is exact -- bit patterns or
integers -- except the loss, which takes the tolerance of tests/test_gpu_cells.py::test_get_loss_cls."""
import ctypes

import numpy as np
import pytest
import torch

import modelnet_flow_ref as R
from conftest import clouds

pytestmark = pytest.mark.gpu
L = ctypes.c_long


@pytest.fixture(scope="module")
def T():
    from pointasnl_amd import modelnet_tester as T

    return T


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def assert_same(got, want):
    """bit for bit; where numpy has a NaN the device has one too (a NaN's sign and payload are the machine's)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(bits(got)[~nan], bits(want)[~nan])


def host(t):
    return t.cpu().numpy()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


class Starts:
    """an RNG whose randint answers the given start indices, in order"""

    def __init__(self, starts):
        self.starts = list(starts)

    def randint(self, lo, hi):
        s = self.starts.pop(0)
        assert lo <= s < hi
        return s


def lattice6(seed, n):
    return np.ascontiguousarray(np.hstack([clouds(seed, 1, n, kind="lattice")[0], np.ones((n, 3), np.float32)]))


def fps_on_device(shapes, starts, npoint, ids=None):
    """pasnl_modelnet_fps over `shapes` in one call -> (indices (S,npoint) i32, rows (S,npoint,6) f32), numpy"""
    from pointasnl_amd import _hip

    S = len(shapes)
    sizes = np.array([s.shape[0] for s in shapes], np.int64)
    row0 = np.concatenate([[0], np.cumsum(sizes)])[:-1].astype(np.int64)
    raw, row0_t, nraw_t, start_t = dev(np.concatenate(shapes)), dev(row0), dev(sizes.astype(np.int32)), dev(np.asarray(starts, np.int32))
    out_idx = torch.full((S, npoint), -1, dtype=torch.int32, device="cuda")
    out_rows = torch.full((S, npoint, 6), -7.0, dtype=torch.float32, device="cuda")
    ids_t = None if ids is None else dev(np.asarray(ids, np.int32))
    call = sizes if ids is None else sizes[np.asarray(ids)]
    _hip.launch("pasnl_modelnet_fps", "test", len(starts), npoint, 6, L(S), ptr(ids_t), ptr(row0_t), ptr(nraw_t), ptr(start_t),
                int(call.min()), int(call.max()), L(int(sizes.sum())), ptr(raw), ptr(out_idx), ptr(out_rows), 6)
    return host(out_idx), host(out_rows)


def check_fps(shapes, starts, npoint, ids=None):
    got_idx, got_rows = fps_on_device(shapes, starts, npoint, ids)
    order = range(len(shapes)) if ids is None else ids
    for j, i in enumerate(order):
        want = R.fps_indices(shapes[i], npoint, Starts([starts[j]]))
        np.testing.assert_array_equal(got_idx[i], want)
        np.testing.assert_array_equal(bits(got_rows[i]), bits(shapes[i][want]))
    return got_idx


def tied_rounds(xyz, picks):
    """the rounds of a sampling in which more than one point holds the maximum running distance, so that the tie rule and
    not the distance chose the next pick"""
    running, n = np.full((xyz.shape[0],), 1e10), 0
    for p in picks[:-1]:
        running = np.minimum(running, np.sum((xyz - xyz[p]) ** 2, -1))
        n += np.count_nonzero(running == running.max()) > 1
    return n


def test_fps_full_record_is_numpys_sampling():
    """the real raw size: 10 000 rows in the LDS record, 1024 picks; beside it a shape of ten rows over a multiple of the
    workgroup"""
    shapes = [R.shape(11, 10000), R.shape(12, 1034)]
    idx = check_fps(shapes, [4711, 1033], 1024)
    assert len(np.unique(idx[0])) == 1024 and idx[0][0] == 4711 and idx[0].max() >= 9000


def test_fps_small_shapes_ties_and_duplicates_in_one_call():
    """several shapes of different n_raw in one call, through an id list: 300 / 64, n_raw == npoint, n_raw = npoint + 1, a
    lattice cloud (many equal maxima: the first index decides), duplicated points (distance 0 ties once the distinct points
    are used up), start index 0 and n_raw - 1"""
    shapes = [R.shape(21, 300), R.shape(22, 64), R.shape(23, 65), lattice6(24, 300), R.shape(25, 300, "dup"), R.shape(26, 64, "dup"),
              lattice6(27, 65), R.shape(28, 1500)]
    ids = [3, 0, 7, 1, 2, 4, 6, 5]
    starts = [0, 299, 1499, 63, 0, 17, 64, 5]
    idx = check_fps(shapes, starts, 64, ids)
    lat = shapes[3][:, 0:3]
    assert len(np.unique(lat, axis=0)) < 300                       # the lattice repeats points,
    assert tied_rounds(lat, idx[3]) > 1 and tied_rounds(shapes[6][:, 0:3], idx[6]) > 1  # and the first index decides picks
    assert len(np.unique(idx[5])) < 64                             # duplicates: an index comes back once all distances are 0
    assert sorted(idx[1]) == list(range(64))                       # n_raw == npoint, distinct points: a permutation
    check_fps(shapes[:3], [299, 0, 64], 64)                        # and without an id list


def test_fps_limits(T):
    from pointasnl_amd import _hip

    cap = T.fps_cap()
    assert cap >= 10240
    raw = torch.zeros((cap + 1, 6), dtype=torch.float32, device="cuda")
    out = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    row0, start = torch.zeros((1,), dtype=torch.int64, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")

    def call(npoint, n):
        nraw = torch.tensor([n], dtype=torch.int32, device="cuda")
        _hip.launch("pasnl_modelnet_fps", "test", 1, npoint, 6, L(1), ptr(None), ptr(row0), ptr(nraw), ptr(start), n, n, L(cap + 1), ptr(raw),
                    ptr(out), ptr(None), 6)
        torch.cuda.synchronize()

    with pytest.raises(_hip.PasnlUnsupported):
        call(64, cap + 1)  # past the LDS record
    with pytest.raises(ValueError):
        call(64, 63)       # npoint > n_raw
    assert (host(out) == -1).all()  # neither launched anything
    call(64, cap)          # the cap itself runs: every point equal, so every pick is the first index
    assert not host(out).any()
    with pytest.raises(_hip.PasnlUnsupported):
        T.ModelNetTester([np.zeros((cap + 1, 6), np.float32)], [0], num_point=64, uniform=True)
    with pytest.raises(ValueError):
        T.ModelNetTester([R.shape(1, 63)], [0], num_point=64)
    with pytest.raises(ValueError):
        T.ModelNetTester([], [], num_point=64)
    t = T.ModelNetTester([R.shape(1, 64)], [0], num_point=64, batch_size=2)
    with pytest.raises(ValueError):
        t.run(lambda x: x, num_noisy_point=65)


@pytest.mark.parametrize("npoint", [1, 7, 64, 1024, 1500])
@pytest.mark.parametrize("normals", [True, False])
def test_normalize_is_numpys_pc_normalize(T, npoint, normals):
    """D:9-14 through the constructor (uniform=False prepares every shape there): the sequential float32 centroid, the
    float32 norm and both divisions; one point normalises to 0 / 0"""
    shapes = [R.shape(30 + i, npoint + 3 * i) for i in range(3)]
    t = T.ModelNetTester(shapes, [0, 1, 2], num_point=npoint, batch_size=2, normal_channel=normals)
    got = host(t.prepared)
    for i, s in enumerate(shapes):
        want = s[:npoint].copy()
        with np.errstate(invalid="ignore", divide="ignore"):
            want[:, 0:3] = R.pc_normalize(want[:, 0:3])
        assert_same(got[i], want if normals else want[:, 0:3])
    raw = T.ModelNetTester(shapes, [0, 1, 2], num_point=npoint, batch_size=2, normal_channel=normals, normalize=False)
    np.testing.assert_array_equal(bits(host(raw.prepared)), bits(np.stack([s[:npoint, :6 if normals else 3] for s in shapes])))


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("ch", [6, 3])
def test_noise_is_numpys_normalize_data(T, k, ch):
    """T:129-132 / P:8-24 on a short batch (bsize 3 of 4): the float64 blocks rounded to float32 over rows 0..K-1 of the real
    shapes; normals, later rows and the stale row untouched; K = 1 is 0 / 0"""
    shapes = [R.shape(40 + i, 130) for i in range(7)]
    rng = np.random.RandomState(3)
    t = T.ModelNetTester(shapes, np.arange(7) % 5, num_point=128, batch_size=4, normal_channel=ch == 6, rng=rng)
    t.next_batch()
    _, _, bsize = t.next_batch()
    assert bsize == 3
    before = host(t.batch).copy()
    t.add_noise(k)
    want = before.copy()
    want[:3, :k, :3] = R.normalize_data(np.random.RandomState(3).random((3, k, 3))).astype(np.float32)
    assert_same(host(t.batch), want)
    assert np.isnan(want).any() == (k == 1)


def stand_in(w, b, log=None):
    def forward(x):
        data = host(x)
        if log is not None:
            log.append(data.copy())
        return dev(R.stand_in_forward_np(data, w, b))

    return forward


def hooked(t):
    """records the vote sums and labels of every batch just before the tally clears them"""
    rec, tally = dict(sums=[], labels=[]), t.finish_batch

    def finish():
        rec["sums"].append(host(t.vote_sums()).copy())
        rec["labels"].append(host(t.label).copy())
        tally()

    t.finish_batch = finish
    return rec


def compare_epoch(t, rec, fed, want, votes):
    S = t.S
    assert len(fed) == len(want["fed"]) * votes
    for j, w in enumerate(want["fed"]):
        for v in range(votes):
            assert_same(fed[j * votes + v], w)
        np.testing.assert_array_equal(rec["labels"][j], want["labels"][j])
        assert_same(rec["sums"][j], want["sums"][j])
    np.testing.assert_array_equal(host(t.predictions()), np.concatenate(want["preds"]))
    got = t.totals()
    for key in ("total_correct", "total_seen", "total_object"):
        assert got[key] == want[key]
    np.testing.assert_array_equal(got["seen_class"], want["seen_class"])
    np.testing.assert_array_equal(got["correct_class"], want["correct_class"])
    assert got["total_seen"] == S and got["total_object"] == t.num_batches * t.B
    np.testing.assert_array_equal(bits(t.class_accuracy()), bits(want["class_accuracy"]))
    assert t.accuracy() == want["accuracy"]
    for reg, ref_loss in ((0.0, want["mean_loss"]), (0.25, want["mean_loss"] + 0.25 * t.num_batches / want["total_object"])):
        assert abs(t.mean_loss(reg) - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))  # the tolerance of test_get_loss_cls
    assert not host(t.vote_sums()).any()


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("k", [0, 10])
@pytest.mark.parametrize("votes", [1, 3])
@pytest.mark.parametrize("S,B", [(37, 8), (5, 8)])
def test_whole_epochs_equal_the_restatement(T, S, B, votes, k, uniform):
    """T:105-174 twice over: 37 shapes in batches of 8 leave a last batch of 5 with three stale rows; 5 shapes in a batch of 8
    leave the zero rows and zero labels the buffers start with.  Classes 4 and 5 stay empty."""
    C, N = 6, 64
    shapes = [R.shape(500 + i, 300 - i, ("blob", "lattice", "dup")[i % 3]) for i in range(S)]
    labels = np.random.default_rng(S).integers(0, 4, S)
    w, b = R.stand_in_weights(2, 6, C)
    rng_t, rng_r = np.random.RandomState(100 + S), np.random.RandomState(100 + S)
    t = T.ModelNetTester(shapes, labels, num_classes=C, num_point=N, batch_size=B, normal_channel=True, uniform=uniform, rng=rng_t)
    ds = R.ModelNetFlowRef(shapes, labels, batch_size=B, npoints=N, normal_channel=True, uniform=uniform, rng=rng_r)
    rec = hooked(t)
    for epoch, (nv, noisy) in enumerate([(votes, k), (1, 0)]):  # the second epoch samples nothing and feeds the same shapes
        fed = []
        rec["sums"].clear(), rec["labels"].clear()
        want = R.eval_one_epoch(ds, lambda x: R.stand_in_forward_np(x, w, b), C, nv, noisy, rng_r)
        acc = t.run(stand_in(w, b, fed), nv, noisy)
        assert acc == want["accuracy"]
        compare_epoch(t, rec, fed, want, nv)
        assert rng_t.randint(1 << 30) == rng_r.randint(1 << 30)  # both streams at the same place
        last = want["fed"][-1]
        if S == 37:
            assert want["bsizes"][-1] == 5 and want["total_object"] == 40 and want["total_seen"] == 37
            np.testing.assert_array_equal(bits(fed[-1][5:]), bits(want["fed"][-2][5:]))  # the stale rows: the batch before
            np.testing.assert_array_equal(rec["labels"][-1][5:], want["labels"][-2][5:])
        else:
            assert want["bsizes"] == [5] and want["total_object"] == 8
            assert not last[5:].any() and not fed[-1][5:].any() and not rec["labels"][-1][5:].any()
    assert ds.fps_draws == (S if uniform else 0) and bool(t.ready.all())
    assert np.isnan(t.class_accuracy()[4:]).all() and not np.isnan(t.class_accuracy()[:4]).any()
    names = ["class_%d" % c for c in range(C)]
    assert t.report(names)[1:] == R.report(want, names)[1:]
    assert t.report(names)[0].startswith("Eval mean loss: ")


def test_model_epoch_equals_feeding_the_restatements_batches(T):
    """pointasnl_cls.get_model as the forward: the tester's predictions and counts are those of the same model fed the
    restatement's batches"""
    from pointasnl_amd.models import pointasnl_cls
    from pointasnl_amd.utils import tf_util

    tf_util.set_store(tf_util.VariableStore(seed=77))
    S, B, N = 6, 4, 1024
    shapes = [R.shape(700 + i, 1100) for i in range(S)]
    labels = np.array([3, 17, 0, 39, 17, 8])

    def model(x):
        with torch.no_grad():
            return pointasnl_cls.get_model(x, is_training=False, use_normal=True)[0]

    rng_t, rng_r = np.random.RandomState(5), np.random.RandomState(5)
    t = T.ModelNetTester(shapes, labels, num_point=N, batch_size=B, normal_channel=True, uniform=True, rng=rng_t)
    ds = R.ModelNetFlowRef(shapes, labels, batch_size=B, npoints=N, normal_channel=True, uniform=True, rng=rng_r)
    want = R.eval_one_epoch(ds, lambda fed: host(model(dev(fed))), 40, 2, 0, rng_r)
    acc = t.run(model, num_votes=2)
    np.testing.assert_array_equal(host(t.predictions()), np.concatenate(want["preds"]))
    got = t.totals()
    assert (got["total_correct"], got["total_seen"], got["total_object"]) == (want["total_correct"], 6, 8)
    np.testing.assert_array_equal(got["seen_class"], want["seen_class"])
    np.testing.assert_array_equal(got["correct_class"], want["correct_class"])
    assert acc == want["accuracy"]
    assert abs(t.mean_loss() - want["mean_loss"]) < 1e-5 * max(1.0, abs(want["mean_loss"]))
    assert rng_t.randint(1 << 30) == rng_r.randint(1 << 30)


def test_robustness_table_equals_the_restatement(T):
    S, B, C, N = 10, 4, 5, 64
    shapes = [R.shape(800 + i, 200) for i in range(S)]
    labels = np.arange(S) % C
    w, b = R.stand_in_weights(3, 6, C)
    rng_t, rng_r = np.random.RandomState(9), np.random.RandomState(9)
    t = T.ModelNetTester(shapes, labels, num_classes=C, num_point=N, batch_size=B, uniform=True, rng=rng_t)
    ds = R.ModelNetFlowRef(shapes, labels, batch_size=B, npoints=N, normal_channel=True, uniform=True, rng=rng_r)
    want = R.robustness(ds, lambda x: R.stand_in_forward_np(x, w, b), C, 2, (1, 10), rng_r)
    got = t.robustness(stand_in(w, b), 2, (1, 10))
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert got[2].splitlines()[0] == "Noise    Accuracy" and got[2].splitlines()[2].startswith(" 001       ")
    assert rng_t.randint(1 << 30) == rng_r.randint(1 << 30)


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("uniform", [False, True])
def test_dataset_class_sequences(shuffle, uniform):
    """has_next_batch / next_batch / reset under a seeded np.random: two epochs and one cut short by a reset"""
    import pointasnl_amd

    pointasnl_amd.install_paths()
    import modelnet_dataset

    S, B, N = 10, 4, 64
    shapes = [R.shape(900 + i, 150) for i in range(S)]
    labels = np.arange(S) % 3
    np.random.seed(5)
    ds = modelnet_dataset.ModelNetDataset(shapes, labels, batch_size=B, npoints=N, split="test", normal_channel=False, shuffle=shuffle,
                                          uniform=uniform)
    ref = R.ModelNetFlowRef(shapes, labels, batch_size=B, npoints=N, normal_channel=False, shuffle=shuffle, uniform=uniform,
                            rng=np.random.RandomState(5))
    assert len(ds) == S and ds.num_channel() == 3 and ds.shuffle == shuffle
    for stop in (1, 99, 99):  # the first epoch is cut short after one batch: later batches mix sampled and new shapes
        seen = 0
        while ds.has_next_batch() and seen < stop:
            assert ref.has_next_batch()
            data, label = ds.next_batch()
            wd, wl = ref.next_batch()
            assert data.is_cuda and data.dtype == torch.float32 and label.dtype == torch.int32
            np.testing.assert_array_equal(bits(host(data)), bits(wd.astype(np.float32)))
            np.testing.assert_array_equal(host(label), wl)
            seen += 1
        assert ds.has_next_batch() == ref.has_next_batch()
        assert ds.batch_idx == ref.batch_idx
        ds.reset(), ref.reset()
        np.testing.assert_array_equal(ds.idxs, ref.idxs)
    ps, cls = ds[7]
    wps, wcls = ref.get_item(7)
    np.testing.assert_array_equal(bits(host(ps)), bits(wps))
    assert cls.dtype == np.int32 and cls.tolist() == wcls.tolist()
    assert np.random.randint(1 << 30) == ref.rng.randint(1 << 30)
