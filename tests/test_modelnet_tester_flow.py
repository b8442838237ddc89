"""CPU: the numpy restatement of the ModelNet40 evaluation flow (tests/modelnet_flow_ref.py, the yardstick of
ModelNetTester) pinned to the reference's own class `ModelNetDataset` (modelnet_dataset.py, imported from the reference
tree and run over a synthetic dataset root written to a temporary directory) and, always, to the committed golden run of
that class; the arithmetic facts the kernels rely on; and the position of the RNG stream after an epoch with noise and
votes against a direct replay of the draws."""
import ctypes
import os
import sys

import numpy as np
import pytest

import modelnet_flow_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_modelnet_flow as M  # noqa: E402

REF = os.environ.get("PASNL_REFERENCE", "/root/reference")
REF_FILE = os.path.join(REF, "modelnet_dataset.py")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def restated_epoch(uniform, normal_channel=True, shuffle=False, batch=M.BATCH):
    rng = np.random.RandomState(M.SEED)
    ds = R.ModelNetFlowRef(M.shapes(), M.labels(), batch_size=batch, npoints=M.NPOINTS, normal_channel=normal_channel, uniform=uniform,
                           shuffle=shuffle, rng=rng)
    out = []
    while ds.has_next_batch():
        out.append(ds.next_batch())
    return out, rng.randint(1 << 30)


@pytest.mark.parametrize("uniform,normal_channel,shuffle,batch", [(False, True, None, 4), (True, True, None, 4), (True, False, True, 3),
                                                                  (False, False, True, 16)])
def test_restatement_equals_reference_class(tmp_path, uniform, normal_channel, shuffle, batch):
    if not os.path.exists(REF_FILE):
        pytest.skip("reference tree absent")
    mod = M.reference_module()
    M.write_root(str(tmp_path))
    want, want_after = M.reference_epoch(mod, str(tmp_path), uniform, normal_channel, shuffle, batch)
    got, got_after = restated_epoch(uniform, normal_channel, bool(shuffle), batch)
    assert len(got) == len(want) == (M.SHAPES + batch - 1) // batch
    for (gd, gl), (wd, wl) in zip(got, want):
        assert gd.dtype == wd.dtype == np.float64 and gl.dtype == wl.dtype == np.int32 and gd.shape == wd.shape
        np.testing.assert_array_equal(bits(gd), bits(wd))
        np.testing.assert_array_equal(gl, wl)
    assert got_after == want_after  # the RNG streams are still in step


def test_restated_functions_equal_the_reference_functions():
    if not os.path.exists(REF_FILE):
        pytest.skip("reference tree absent")
    mod = M.reference_module()
    for seed, n, npoint, kind in [(1, 300, 64, "blob"), (2, 65, 64, "lattice"), (3, 64, 64, "dup"), (4, 500, 7, "lattice")]:
        raw = R.shape(seed, n, kind)
        np.random.seed(seed)
        want = mod.farthest_point_sample(raw, npoint)
        got = raw[R.fps_indices(raw, npoint, np.random.RandomState(seed))]
        np.testing.assert_array_equal(bits(got), bits(want))
        np.testing.assert_array_equal(bits(R.pc_normalize(raw[:, 0:3])), bits(mod.pc_normalize(raw[:, 0:3])))


def test_golden_modelnet_flow_is_the_restatement():
    path = os.path.join(HERE, "golden", "modelnet_flow.npz")
    gold = np.load(path)
    assert os.path.getsize(path) < 200 * 1024
    assert int(gold["seed"][0]) == M.SEED and gold["params"].tolist() == [M.SHAPE_SEED, M.SHAPES, M.N_RAW, M.NPOINTS, M.BATCH]
    for uniform, tag in ((False, "first"), (True, "uniform")):
        got, after = restated_epoch(uniform)
        data = np.concatenate([d for d, _ in got])
        np.testing.assert_array_equal(bits(data.astype(np.float32)), bits(gold[tag + "/data"]))
        np.testing.assert_array_equal(data.astype(np.float32).astype(np.float64), data)
        np.testing.assert_array_equal(np.concatenate([l for _, l in got]), gold[tag + "/label"])
        assert [d.shape[0] for d, _ in got] == gold[tag + "/bsizes"].tolist() == [4, 4, 2]
        assert after == int(gold[tag + "/after"][0])
    assert not np.array_equal(gold["first/data"], gold["uniform/data"])


def test_arithmetic_the_kernels_rely_on():
    """float32 FPS distance and norm are (x*x + y*y) + z*z; the means are one sum per column in row order, float32 over a
    strided (N,3) view of (N,6) rows and float64 over a (K,3) block; argmax takes the first of equal maxima; 1e10 is a float32"""
    raw = R.shape(9, 1500)
    xyz = raw[:, 0:3]
    d = xyz - xyz[17, :]
    np.testing.assert_array_equal(bits(np.sum(d ** 2, -1)), bits((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    mean = np.mean(xyz, axis=0)
    assert mean.dtype == np.float32
    np.testing.assert_array_equal(bits(mean), bits(np.cumsum(xyz, axis=0, dtype=np.float32)[-1] / np.float32(1500)))
    for k in (1, 2, 10, 100, 1024):
        u = np.random.RandomState(k).random((k, 3))
        np.testing.assert_array_equal(bits(np.mean(u, axis=0)), bits(np.cumsum(u, axis=0)[-1] / np.float64(k)))
    assert np.argmax(np.array([1.0, 3.0, 3.0, 2.0, 3.0])) == 1
    assert float(np.float32(1e10)) == 1e10
    one = R.normalize_data(np.random.RandomState(0).random((2, 1, 3)))
    assert np.isnan(one).all()  # a single noisy point: 0 / 0


def forward_of(w, b):
    return lambda data: R.stand_in_forward_np(data, w, b)


@pytest.mark.parametrize("uniform", [False, True])
def test_rng_stream_after_epochs_is_the_replayed_draws(uniform):
    """two epochs (the first noisy, three votes; the second clean, one vote) leave the RNG where a direct replay of the
    draws leaves it: per batch [one randint per shape, first epoch with uniform only] [random((bsize,K,3))] and a shuffle of
    arange(N) per vote"""
    B, K, C = 4, 10, 5
    shapes, labels = M.shapes(), M.labels()
    rng = np.random.RandomState(77)
    ds = R.ModelNetFlowRef(shapes, labels, batch_size=B, npoints=M.NPOINTS, normal_channel=True, uniform=uniform, rng=rng)
    w, b = R.stand_in_weights(1, 6, C)
    first = R.eval_one_epoch(ds, forward_of(w, b), C, num_votes=3, num_noisy_point=K, rng=rng)
    second = R.eval_one_epoch(ds, forward_of(w, b), C, num_votes=1, rng=rng)
    assert ds.fps_draws == (M.SHAPES if uniform else 0)
    replay = np.random.RandomState(77)
    for votes, k, sample in ((3, K, uniform), (1, 0, False)):
        for lo in range(0, M.SHAPES, B):
            bsize = min(B, M.SHAPES - lo)
            if sample:
                for i in range(lo, lo + bsize):
                    replay.randint(0, shapes[i].shape[0])
            if k:
                replay.random((bsize, k, 3))
            for _ in range(votes):
                replay.shuffle(np.arange(M.NPOINTS))
    assert rng.randint(1 << 30) == replay.randint(1 << 30)
    assert first["total_object"] == 12 and first["total_seen"] == 10 and first["bsizes"] == [4, 4, 2]
    # the short batch's stale rows are the batch before it, noise included; the second epoch starts from zeros again
    np.testing.assert_array_equal(bits(first["fed"][2][2:]), bits(first["fed"][1][2:]))
    np.testing.assert_array_equal(first["labels"][2][2:], first["labels"][1][2:])
    assert not np.array_equal(second["fed"][0][:, :K, :3], first["fed"][0][:, :K, :3])
    np.testing.assert_array_equal(bits(second["fed"][0][:, K:]), bits(first["fed"][0][:, K:]))
    np.testing.assert_array_equal(first["seen_class"], np.bincount(labels, minlength=C))
    assert np.isnan(first["class_accuracy"][4]) and first["seen_class"][4] == 0  # a class the labels leave empty


def test_modelnet_entries_are_declared_exported_and_importable():
    """the feature's surface: the C-ABI entries, their host-side validation, and the two Python modules"""
    import pointasnl_amd
    from pointasnl_amd import _hip

    names = ["pasnl_modelnet_fps_cap", "pasnl_modelnet_fps", "pasnl_modelnet_normalize", "pasnl_modelnet_batch", "pasnl_modelnet_noise",
             "pasnl_cls_vote", "pasnl_cls_tally"]
    lib = _hip.lib()
    for name in names:
        assert name in _hip.SYMBOLS and hasattr(lib, name)
    cap = lib.pasnl_modelnet_fps_cap()
    assert cap >= 10240
    null, L = ctypes.c_void_p(0), ctypes.c_long
    fps = lambda s, npoint, n_min, n_max: lib.pasnl_modelnet_fps(s, npoint, 6, L(4), null, null, null, null, n_min, n_max, L(10 ** 6), null,  # noqa: E731
                                                                  null, null, 6, null)
    assert fps(2, 64, 300, cap + 1) == -5   # past the LDS record
    assert fps(2, 64, 63, 300) == -1        # npoint > n_raw
    assert fps(2, 64, 64, 300) == -2        # null pointers
    assert fps(0, 64, 64, 300) == 0         # no shape: a no-op
    assert lib.pasnl_modelnet_normalize(0, 64, 6, L(4), null, null, null) == 0
    assert lib.pasnl_modelnet_normalize(2, 0, 6, L(4), null, null, null) == -1
    assert lib.pasnl_modelnet_normalize(2, 64, 6, L(4), null, null, null) == -2
    assert lib.pasnl_modelnet_batch(8, 5, 64, 4, null, L(37), L(32), L(37), null, null, null, null, null) == -1   # ch not 3 or 6
    assert lib.pasnl_modelnet_batch(8, 6, 64, 6, null, L(37), L(32), L(37), null, null, null, null, null) == -1   # past the order
    assert lib.pasnl_modelnet_batch(8, 5, 64, 6, null, L(37), L(32), L(37), null, null, null, null, null) == -2
    assert lib.pasnl_modelnet_batch(0, 0, 64, 6, null, L(37), L(0), L(37), null, null, null, null, null) == 0
    assert lib.pasnl_modelnet_noise(4, 65, null, 64, 6, null, null) == -1   # K > npoint
    assert lib.pasnl_modelnet_noise(4, 0, null, 64, 6, null, null) == -1
    assert lib.pasnl_modelnet_noise(4, 10, null, 64, 6, null, null) == -2
    assert lib.pasnl_cls_vote(0, 40, null, null, null, null, null) == 0
    assert lib.pasnl_cls_vote(16, 40, null, null, null, null, null) == -2
    assert lib.pasnl_cls_tally(16, 17, 40, 1, null, null, null, null, null, null, null, null) == -1
    assert lib.pasnl_cls_tally(16, 5, 40, 1, null, null, null, null, null, null, null, null) == -2
    pointasnl_amd.install_paths()
    import modelnet_dataset  # the reference's idiom

    from pointasnl_amd import modelnet_tester

    assert modelnet_dataset is pointasnl_amd.modelnet_dataset
    assert modelnet_dataset.ModelNetDataset.__name__ == "ModelNetDataset"
    for name in ("__len__", "__getitem__", "num_channel", "reset", "has_next_batch", "next_batch"):
        assert hasattr(modelnet_dataset.ModelNetDataset, name)
    assert modelnet_tester.NOISE_POINT == (1, 10, 50, 100)
    with pytest.raises(NotImplementedError):
        modelnet_dataset.ModelNetDataset([np.zeros((64, 6), np.float32)] * 3, [0, 0, 0], cache_size=2)
