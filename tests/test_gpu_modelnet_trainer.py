"""GPU: the ModelNet40 training input loop on the device (pasnl_modelnet_augment in csrc/modelnet_test.hip and
pointasnl_amd.modelnet_trainer) against the numpy restatement tests/modelnet_train_flow_ref.py run live on the same machine
(it is pinned to the reference's functions and to their golden run in tests/test_modelnet_trainer_flow.py).  Every
comparison is exact -- bit patterns or integers -- except the loss, which takes the tolerance of
tests/test_gpu_modelnet_tester.py."""
import ctypes

import numpy as np
import pytest
import torch

import guarded
import modelnet_flow_ref as R
import modelnet_train_flow_ref as A

pytestmark = pytest.mark.gpu
L = ctypes.c_long


@pytest.fixture(scope="module")
def T():
    from pointasnl_amd import modelnet_trainer as T

    return T


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def host(t):
    return t.cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def prepared_set(seed, S, npoint, ch):
    """S prepared shapes (S, npoint, ch) float32: the first npoint rows, pc_normalize on xyz"""
    out = np.zeros((S, npoint, ch), np.float32)
    for i in range(S):
        s = R.shape(seed + i, npoint + 5, ("blob", "lattice", "dup")[i % 3])[:npoint]
        if npoint > 1:  # one point normalises to 0 / 0
            s[:, 0:3] = R.pc_normalize(s[:, 0:3])
        out[i] = s[:, :ch]
    return out


def crafted_draws(rng, npoint, rotation, perm_kind):
    """three clouds: every point dropped through the tie u = ratio = 0; none dropped; u == ratio at single points"""
    d = A.draw(rng, 3, npoint, rotation)
    d["u"][0], d["ratio"][0] = 0.0, 0.0
    d["u"][1], d["ratio"][1] = np.maximum(d["u"][1], 1e-3), 0.0
    d["ratio"][2] = 0.4
    ties = sorted({0, npoint // 2, npoint - 1})
    d["u"][2][ties] = 0.4
    if perm_kind == "reversed":
        d["perm"] = np.arange(npoint)[::-1].astype(np.int32)
    elif npoint > 1 and d["perm"][0] == 0:
        d["perm"][[0, 1]] = d["perm"][[1, 0]]
    return d, ties


@pytest.mark.parametrize("rotation", [False, True])
@pytest.mark.parametrize("ch", [6, 3])
@pytest.mark.parametrize("npoint", [1, 67, 300])
def test_augment_entry_equals_the_restatement(npoint, ch, rotation):
    """the entry alone through the C ABI: b = 5, bsize = 3, start = 2 in a shuffled order of 7 shapes.  67 points are ragged
    against a wave and a 256-thread block, 300 take two blocks per cloud and straddle clouds inside a block.  Rows 3..4 of
    the batch and the labels keep their sentinel; the bytes around the guarded batch are intact."""
    from pointasnl_amd import _hip

    S, b, bsize, start = 7, 5, 3, 2
    prepared = prepared_set(60 + npoint, S, npoint, ch)
    shape_labels = (np.arange(S) * 3 % 11).astype(np.int32)
    rng = np.random.RandomState(1000 + npoint + ch)
    order = rng.permutation(S).astype(np.int32)
    assert not np.array_equal(order, np.arange(S))
    prepared_t, labels_t, order_t = dev(prepared), dev(shape_labels), dev(order)
    for perm_kind in ("shuffled", "reversed"):
        d, ties = crafted_draws(rng, npoint, rotation, perm_kind)
        assert npoint == 1 or d["perm"][0] != 0
        ids = order[start:start + bsize]
        want = A.augment(prepared[ids].astype(np.float64), d).astype(np.float32)
        src2 = A.source_rows(d, 2)  # the third cloud: the tied points are dropped, and it still shows other rows where it can
        assert (src2[ties] == d["perm"][0]).all() and (npoint == 1 or len(np.unique(src2)) > 1)
        assert (A.source_rows(d, 0) == d["perm"][0]).all() and np.array_equal(A.source_rows(d, 1), d["perm"])
        batch = guarded.Guarded(b * npoint * ch * 4, guarded.NAN_BYTE, guarded.output_guard(npoint * ch * 4))
        labels = torch.full((b,), -9, dtype=torch.int32, device="cuda")
        mats = dev(d["mats"].reshape(bsize, 2, 9)) if rotation else None
        scale, shift, perm, ratio, u = dev(d["scale"]), dev(d["shift"]), dev(d["perm"]), dev(d["ratio"]), dev(d["u"])
        assert perm.dtype == torch.int32 and u.dtype == torch.float64
        _hip.launch("pasnl_modelnet_augment", "test", b, bsize, npoint, ch, ptr(order_t), L(S), L(start), L(S), ptr(prepared_t),
                    ptr(labels_t), ptr(mats), ptr(scale), ptr(shift), ptr(perm), ptr(ratio), ptr(u), ctypes.c_void_p(batch.ptr), ptr(labels))
        torch.cuda.synchronize()
        got = batch.floats((b, npoint, ch))
        np.testing.assert_array_equal(bits(got[:bsize]), bits(want))
        assert (bits(got[bsize:]) == -1).all()  # the sentinel bytes
        assert batch.guards_intact()
        np.testing.assert_array_equal(host(labels), list(shape_labels[ids]) + [-9, -9])
        if rotation:  # not a copy
            assert not np.array_equal(want[1][:, 3:], prepared[ids[1]][d["perm"]][:, 3:]) or ch == 3
        else:         # normals are copied
            np.testing.assert_array_equal(bits(want[1][:, 3:]), bits(prepared[ids[1]][d["perm"]][:, 3:]))
    # bsize = 0 launches nothing
    _hip.launch("pasnl_modelnet_augment", "test", b, 0, npoint, ch, ptr(order_t), L(S), L(start), L(S), ptr(prepared_t), ptr(labels_t),
                ptr(None), ptr(scale), ptr(shift), ptr(perm), ptr(ratio), ptr(u), ctypes.c_void_p(batch.ptr), ptr(labels))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bits(batch.floats((b, npoint, ch))[:bsize]), bits(want))


def twin(T, shapes, labels, seed, **kw):
    """a trainer and the restated dataset under two RNGs at the same place"""
    rng_t, rng_r = np.random.RandomState(seed), np.random.RandomState(seed)
    t = T.ModelNetTrainer(shapes, labels, rng=rng_t, **kw)
    ds = R.ModelNetFlowRef(shapes, labels, batch_size=t.B, npoints=t.P, normal_channel=t.ch == 6, shuffle=True, uniform=t.tester.uniform,
                           rng=rng_r)
    np.testing.assert_array_equal(t.idxs, ds.idxs)
    return t, ds, rng_t, rng_r


def test_one_batch_at_the_real_shape(T):
    """B = 16, N = 1024, ch = 6, rotation on, through ModelNetTrainer.augment_batch"""
    S, B, N = 16, 16, 1024
    shapes = [R.shape(300 + i, 1100) for i in range(S)]
    labels = np.arange(S) * 7 % 40
    t, ds, rng_t, rng_r = twin(T, shapes, labels, 21, num_point=N, batch_size=B, normal_channel=True, rotation=True)
    batch, label, bsize = t.augment_batch()
    data, want_label = ds.next_batch()
    d = A.draw(rng_r, B, N, True)
    want = A.augment(data, d)
    assert bsize == B and want.dtype == np.float32
    np.testing.assert_array_equal(bits(host(batch)), bits(want))
    np.testing.assert_array_equal(host(label), want_label)
    dropped = np.mean([np.mean(d["u"][k] <= d["ratio"][k]) for k in range(B)])
    assert 0.1 < dropped < 0.8  # the dropout did something
    assert rng_t.randint(1 << 30) == rng_r.randint(1 << 30)
    assert not t.has_next_batch()
    with pytest.raises(IndexError):
        t.augment_batch()


def device_step(w, b, log):
    def step(x, y):
        assert x.is_cuda and x.dtype == torch.float32 and y.is_cuda and y.dtype == torch.int32
        data = host(x)
        log.append((data.copy(), host(y).copy()))
        return dev(R.stand_in_forward_np(data, w, b))

    return step


@pytest.mark.parametrize("uniform,rotation,normals", [(False, True, True), (True, True, False), (False, False, False), (True, False, True)])
def test_two_epochs_equal_the_restatement(T, uniform, rotation, normals):
    """T:208-264 twice over: 10 shapes in batches of 4 leave a last batch of 2 whose stale rows are the augmented batch before
    it; the second epoch visits another order, samples nothing and starts from a zeroed batch"""
    S, B, N, C = 10, 4, 64, 5
    ch = 6 if normals else 3
    shapes = [R.shape(500 + i, 300 - i, ("blob", "lattice", "dup")[i % 3]) for i in range(S)]
    labels = np.random.default_rng(S).integers(0, 4, S)
    w, b = R.stand_in_weights(2, ch, C)
    t, ds, rng_t, rng_r = twin(T, shapes, labels, 100 + S, num_classes=C, num_point=N, batch_size=B, normal_channel=normals,
                               rotation=rotation, uniform=uniform)
    at_start, augment = [], t.augment_batch

    def recording():
        if t.tester.batch_idx == 0:
            at_start.append((host(t.tester.batch).copy(), host(t.tester.label).copy()))
        return augment()

    t.augment_batch = recording
    orders = []
    for epoch in range(2):
        orders.append(ds.idxs.copy())
        fed = []
        want = A.train_one_epoch(ds, lambda x, y: R.stand_in_forward_np(x, w, b), C, rotation=rotation, rng=rng_r)
        acc = t.run(device_step(w, b, fed))
        assert want["bsizes"] == [4, 4, 2] and len(fed) == 3
        for j in range(3):
            np.testing.assert_array_equal(bits(fed[j][0]), bits(want["fed"][j]))
            np.testing.assert_array_equal(fed[j][1], want["labels"][j])
        np.testing.assert_array_equal(bits(fed[2][0][2:]), bits(fed[1][0][2:]))  # the stale rows: the batch before, augmented
        np.testing.assert_array_equal(host(t.predictions()), np.concatenate(want["preds"]))
        got = t.totals()
        assert (got["total_correct"], got["total_seen"], got["total_object"]) == (want["total_correct"], S, 3 * B)
        np.testing.assert_array_equal(got["seen_class"], np.bincount(labels, minlength=C))
        assert acc == t.accuracy() == want["accuracy"]
        for reg, ref_loss in ((0.0, want["mean_loss"]), (0.25, want["mean_loss"] + 0.25 * 3 / 2)):  # int(10 / 4) = 2 divides
            print("epoch %d mean_loss(%g): device %.12g restatement %.12g" % (epoch, reg, t.mean_loss(reg), ref_loss))
            assert abs(t.mean_loss(reg) - ref_loss) < 1e-5 * max(1.0, abs(ref_loss))  # the tolerance of test_gpu_modelnet_tester
        assert t.report(0.001, 0.25)[0] == "Current Learning Rate 0.001000"
        assert t.report(0.001)[2] == A.report(want, 0.001)[2]
        assert t.report(0.001)[1].startswith("Training loss: ")
        assert rng_t.randint(1 << 30) == rng_r.randint(1 << 30)  # both streams at the same place
        np.testing.assert_array_equal(t.idxs, ds.idxs)             # the next epoch's order is drawn
    assert not np.array_equal(orders[0], orders[1])
    assert len(at_start) == 2 and all(not d.any() and not l.any() for d, l in at_start)  # each epoch starts from zeros
    assert ds.fps_draws == (S if uniform else 0) and bool(t.tester.ready.all())


def test_fewer_shapes_than_a_batch(T):
    """S = 3 < B = 4: the rows past the real ones are the zeros the epoch starts with, in both epochs; the reference would
    divide the loss by int(3 / 4) = 0, so mean_loss raises"""
    S, B, N, C = 3, 4, 67, 5
    shapes = [R.shape(900 + i, 100) for i in range(S)]
    labels = np.array([1, 0, 3])
    w, b = R.stand_in_weights(4, 6, C)
    t, ds, rng_t, rng_r = twin(T, shapes, labels, 8, num_classes=C, num_point=N, batch_size=B, rotation=True)
    for epoch in range(2):
        fed = []
        want = A.train_one_epoch(ds, lambda x, y: R.stand_in_forward_np(x, w, b), C, rotation=True, rng=rng_r)
        assert t.run(device_step(w, b, fed)) == want["accuracy"]
        np.testing.assert_array_equal(bits(fed[0][0]), bits(want["fed"][0]))
        assert not fed[0][0][3:].any() and fed[0][1][3] == 0 and fed[0][0][:3].any(axis=(1, 2)).all()
        with pytest.raises(ValueError):
            t.mean_loss()
    assert rng_t.randint(1 << 30) == rng_r.randint(1 << 30)


@pytest.mark.parametrize("rotation", [False, True])
def test_augment_batch_alone_moves_the_rng_as_one_batch_of_run(T, rotation):
    S, B, N, C = 4, 4, 64, 5
    shapes = [R.shape(950 + i, 120 + i) for i in range(S)]
    labels = np.arange(S)
    w, b = R.stand_in_weights(5, 3, C)
    kw = dict(num_classes=C, num_point=N, batch_size=B, normal_channel=False, rotation=rotation, uniform=True)
    rng_a, rng_b, replay = np.random.RandomState(31), np.random.RandomState(31), np.random.RandomState(31)
    alone, looped = T.ModelNetTrainer(shapes, labels, rng=rng_a, **kw), T.ModelNetTrainer(shapes, labels, rng=rng_b, **kw)
    batch, label, bsize = alone.augment_batch()
    idxs = np.arange(S)
    replay.shuffle(idxs)
    for i in idxs:
        replay.randint(0, shapes[i].shape[0])
    A.draw(replay, B, N, rotation)
    assert rng_a.get_state()[2] == replay.get_state()[2] and (rng_a.get_state()[1] == replay.get_state()[1]).all()
    fed = []
    looped.run(device_step(w, b, fed))  # one batch, then the shuffle of the epoch's end
    np.testing.assert_array_equal(bits(host(batch)), bits(fed[0][0]))
    np.testing.assert_array_equal(host(label), fed[0][1])
    alone.reset()
    assert bsize == B and rng_a.randint(1 << 30) == rng_b.randint(1 << 30)
