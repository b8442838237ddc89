"""CPU: the numpy restatement of the ModelNet40 training input flow (tests/modelnet_train_flow_ref.py, the yardstick of
ModelNetTrainer) pinned to the reference's own augmentation functions (utils/provider.py, imported from the reference tree)
under the same seed and, always, to the committed golden run of those functions; the position of the RNG stream after two
epochs against a direct replay of the draws; the arithmetic facts the kernel relies on; and the feature's surface."""
import ctypes
import os
import sys

import numpy as np
import pytest

import modelnet_flow_ref as R
import modelnet_train_flow_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_modelnet_train_flow as M  # noqa: E402

REF = os.environ.get("PASNL_REFERENCE", "/root/reference")
REF_FILE = os.path.join(REF, "utils", "provider.py")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def restated_chain(normals, rotation, seed):
    rng = np.random.RandomState(seed)
    batch = M.batch(normals)
    out = A.augment(batch, A.draw(rng, M.BATCH, M.NPOINTS, rotation))
    return out, rng.randint(1 << 30)


def bound(normals):
    """per cloud 3 x spacing(float32(1.25 * rmax + 0.1)), rmax the cloud's largest row norm: a one-ulp difference of a rotated
    coordinate (numpy's dgemm fixes no summation order), scaled by at most 1.25, plus the two roundings that follow"""
    batch = M.batch(normals)
    rows = batch.reshape(M.BATCH, -1, 3)  # xyz rows and normal rows alike
    rmax = np.sqrt((rows ** 2).sum(-1)).max(axis=1)
    return (3 * np.spacing((1.25 * rmax + 0.1).astype(np.float32)))[:, None, None]


def compare(got, want, normals, rotation, differing):
    """rotation off: float64 bits; rotation on: float32 within the bound, the elements that differ at all counted"""
    assert got.shape == want.shape and got.dtype == want.dtype == (np.float32 if rotation else np.float64)
    if not rotation:
        np.testing.assert_array_equal(bits(got), bits(want))
        return
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= bound(normals)).all(), "largest error %g against the bound %g" % (err.max(), bound(normals).min())
    differing[0] += int(np.count_nonzero(bits(got) != bits(want)))
    differing[1] += got.size


def test_restatement_equals_reference_functions():
    """the chain under the same seed, {normals, no normals} x {rotation, no rotation}, B = 5, N = 67, 20 seeds"""
    if not os.path.exists(REF_FILE):
        pytest.skip("reference tree absent")
    provider = M.reference_module()
    differing = [0, 0]
    for normals, rotation in M.COMBOS:
        for seed in range(20):
            want, want_after = M.reference_chain(provider, normals, rotation, seed)
            got, got_after = restated_chain(normals, rotation, seed)
            compare(got, want, normals, rotation, differing)
            assert got_after == want_after  # the RNG streams are still in step
    assert differing[1] == 20 * M.BATCH * M.NPOINTS * 9 == 60300
    assert differing[0] < 0.01 * differing[1], "%d of %d float32 elements differ from the reference" % tuple(differing)


def test_golden_modelnet_train_flow_is_the_restatement():
    path = os.path.join(HERE, "golden", "modelnet_train_flow.npz")
    gold = np.load(path)
    assert os.path.getsize(path) < 200 * 1024
    assert gold["seeds"].tolist() == list(M.GOLDEN_SEEDS) and gold["params"].tolist() == [M.SHAPE_SEED, M.BATCH, M.NPOINTS, M.N_RAW]
    differing = [0, 0]
    for normals, rotation in M.COMBOS:
        for seed in M.GOLDEN_SEEDS:
            got, after = restated_chain(normals, rotation, seed)
            compare(got, gold["%s/%d/out" % (M.tag(normals, rotation), seed)], normals, rotation, differing)
            assert after == int(gold["%s/%d/after" % (M.tag(normals, rotation), seed)][0])
    assert differing[0] < 0.01 * differing[1], "%d of %d float32 elements differ from the golden run" % tuple(differing)
    assert not np.array_equal(gold["normal_rot/0/out"][:, :, :3], gold["xyz_rot/0/out"])  # P:59 rounds between the two products


def step_of(w, b, log=None):
    def step(data, label):
        if log is not None:
            log.append((data.copy(), label.copy()))
        return R.stand_in_forward_np(data, w, b)

    return step


@pytest.mark.parametrize("uniform", [False, True])
def test_rng_stream_after_two_epochs_is_the_replayed_draws(uniform):
    """S = 10, B = 4, rotation on: the constructor's shuffle, then per batch [one randint per shape on its first visit, with
    uniform] bsize x uniform(), bsize x randn(3), uniform(0.8, 1.25, bsize), uniform(-0.1, 0.1, (bsize, 3)),
    shuffle(arange(N)), per cloud random() and random(N); a shuffle at each epoch's end"""
    S, B, N, C = 10, 4, 64, 5
    shapes, labels = [R.shape(4100 + i, 300) for i in range(S)], np.arange(S) % 4
    rng = np.random.RandomState(77)
    ds = R.ModelNetFlowRef(shapes, labels, batch_size=B, npoints=N, normal_channel=True, shuffle=True, uniform=uniform, rng=rng)
    w, b = R.stand_in_weights(1, 6, C)
    log = []
    first = A.train_one_epoch(ds, step_of(w, b, log), C, rotation=True, rng=rng)
    second = A.train_one_epoch(ds, step_of(w, b), C, rotation=True, rng=rng)
    assert ds.fps_draws == (S if uniform else 0)
    replay = np.random.RandomState(77)
    idxs = np.arange(S)
    replay.shuffle(idxs)  # the constructor's
    for epoch in range(2):
        for lo in range(0, S, B):
            bsize = min(B, S - lo)
            if uniform and epoch == 0:
                for i in idxs[lo:lo + bsize]:
                    replay.randint(0, shapes[i].shape[0])
            for _ in range(bsize):
                replay.uniform()
            for _ in range(bsize):
                replay.randn(3)
            replay.uniform(0.8, 1.25, bsize)
            replay.uniform(-0.1, 0.1, (bsize, 3))
            replay.shuffle(np.arange(N))
            for _ in range(bsize):
                replay.random()
                replay.random((N))
        idxs = np.arange(S)
        replay.shuffle(idxs)  # the epoch's end
    assert rng.randint(1 << 30) == replay.randint(1 << 30)
    np.testing.assert_array_equal(ds.idxs, idxs)
    assert first["bsizes"] == second["bsizes"] == [4, 4, 2] and first["total_seen"] == 10 and first["batches"] == 3
    # the short batch's stale rows are the batch before it, augmented; the second epoch starts from zeros again
    np.testing.assert_array_equal(bits(first["fed"][2][2:]), bits(first["fed"][1][2:]))
    np.testing.assert_array_equal(first["labels"][2][2:], first["labels"][1][2:])
    assert not np.array_equal(first["fed"][2][:2], first["fed"][1][:2])
    assert first["mean_loss"] == first["loss_sum"] / 2  # int(10 / 4): the floored count divides three batches' sum
    assert [l.tolist() for _, l in log] == [l.tolist() for l in first["labels"]]
    assert A.report(first, 0.001)[0] == "Current Learning Rate 0.001000" and A.report(first, 0.001)[2].endswith("\n")


def test_arithmetic_the_kernel_relies_on():
    """in-place float32 *= np.float64 multiplies in float64 and rounds once (numpy >= 2); += a float64 row adds in float64
    and rounds once; <= drops on an exact tie; after the shuffle, the dropped rows show row perm[0] of the unshuffled cloud"""
    assert int(np.__version__.split(".")[0]) >= 2, "the restatement and the kernel mirror numpy >= 2's in-place float32 *= float64"
    rng = np.random.RandomState(3)
    x = rng.standard_normal((5, 200, 3)).astype(np.float32)
    scales, shifts = rng.uniform(0.8, 1.25, 5), rng.uniform(-0.1, 0.1, (5, 3))
    assert isinstance(scales[0], np.float64)
    y = x.copy()
    for k in range(5):
        y[k, :, :] *= scales[k]
    want = (x.astype(np.float64) * scales[:, None, None]).astype(np.float32)
    np.testing.assert_array_equal(bits(y), bits(want))
    in_float32 = x * scales.astype(np.float32)[:, None, None]
    assert y.dtype == np.float32 and np.count_nonzero(bits(in_float32) != bits(want)) > 0  # a float32 product is another number
    z = y.copy()
    for k in range(5):
        z[k, :, :] += shifts[k, :]
    np.testing.assert_array_equal(bits(z), bits((y.astype(np.float64) + shifts[:, None, :]).astype(np.float32)))
    # the tie, and perm[0]
    batch = np.arange(2 * 6 * 3, dtype=np.float64).reshape(2, 6, 3)
    perm = np.array([4, 2, 0, 5, 1, 3], np.int32)
    u = np.array([[0.9, 0.25, 0.9, 0.1, 0.9, 0.9], [0.0] * 6])
    d = dict(mats=None, scale=np.ones(2), shift=np.zeros((2, 3)), perm=perm, ratio=np.array([0.25, 0.0]), u=u)
    out = A.augment(batch, d)
    np.testing.assert_array_equal(A.source_rows(d, 0), [4, 4, 0, 4, 1, 3])
    np.testing.assert_array_equal(A.source_rows(d, 1), [4] * 6)  # u = ratio = 0: every point dropped
    for k in range(2):
        np.testing.assert_array_equal(out[k], batch[k][A.source_rows(d, k)])
    # the same through the reference's own two statements
    data = batch[:, perm, :]
    for k in range(2):
        drop_idx = np.where(u[k] <= d["ratio"][k])[0]
        data[k, drop_idx, :] = data[k, 0, :]
    np.testing.assert_array_equal(out, data)
    # a product with the y rotation's zeros and ones: x1 passes through unchanged
    m = A.rotation_about_y(0.3)
    v = A.dot3(x[0], m)
    np.testing.assert_array_equal(bits(v[:, 1]), bits(x[0][:, 1].astype(np.float64)))
    assert np.abs(v - x[0].astype(np.float64) @ m).max() < 1e-15 * 8


def test_modelnet_augment_is_declared_exported_and_importable():
    """the feature's surface: the C-ABI entry, its host-side validation, and the Python module"""
    from pointasnl_amd import _hip

    lib = _hip.lib()
    assert "pasnl_modelnet_augment" in _hip.SYMBOLS and hasattr(lib, "pasnl_modelnet_augment")
    null, L = ctypes.c_void_p(0), ctypes.c_long
    nulls = [null] * 11  # prepared .. labels, the stream

    def call(b, bsize, npoint, ch, n_order=37, start=32):
        return lib.pasnl_modelnet_augment(b, bsize, npoint, ch, null, L(n_order), L(start), L(37), *nulls)

    assert call(8, 5, 64, 4) == -1     # ch not 3 or 6
    assert call(8, 9, 64, 6, 64, 0) == -1    # bsize > b
    assert call(8, 6, 64, 6) == -1     # past the order
    assert call(8, 5, 0, 6) == -1      # npoint < 1
    assert call(8, 5, 64, 6) == -2     # null pointers
    assert call(8, 5, 1, 3) == -2
    assert call(8, 0, 64, 6) == 0      # no cloud: a no-op
    from pointasnl_amd import modelnet_trainer

    assert modelnet_trainer.ModelNetTrainer.__name__ == "ModelNetTrainer"
    for name in ("run", "augment_batch", "reset", "has_next_batch", "accuracy", "mean_loss", "report", "totals", "predictions"):
        assert hasattr(modelnet_trainer.ModelNetTrainer, name)
    assert modelnet_trainer.ModelNetTrainer.MAX_DROPOUT_RATIO == A.MAX_DROPOUT_RATIO == 0.875
    # the two matrices the host builds are the restatement's
    g = np.random.RandomState(1).randn(3) * 5  # past the clip
    np.testing.assert_array_equal(bits(modelnet_trainer.perturbation(g)), bits(A.perturbation(g)))
    np.testing.assert_array_equal(bits(modelnet_trainer.rotation_about_y(0.77)), bits(A.rotation_about_y(0.77)))
