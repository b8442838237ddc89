"""GPU: the SemanticKITTI grid training input loop on the device (pointasnl_amd.SemanticKITTI.scan_trainer:
pasnl_scan_pick_given, pasnl_knn_crop_indirect and pasnl_crop_order_permute at b = B, pasnl_scan_train_labels,
pasnl_scan_augment, pasnl_block_train_score) against the numpy restatement tests/grid_train_flow_ref.py run live under the
same seed (tests/test_grid_train_flow.py pins it to the reference's own generator), and the two new entries against
`crop_pc` over a `DeviceScan`."""
import ctypes

import numpy as np
import pytest
import torch

import grid_train_flow_ref as R
import philox_ref as P
from grid_train_checks import bits, formula_holds, host, same_batch, same_epoch, stand_in_step
from scan_flow_ref import scan

pytestmark = pytest.mark.gpu

SIZES, NPOINT, BUFFER, B = (700, 450, 900, 520, 610, 480), 64, 24, 2
C = 5
WEIGHTS = np.array([0.0, 1.3, 0.7, 2.1, 1.0])
AUG_SEED = 0xFEEDFACE87654321


@pytest.fixture(scope="module")
def data():
    lrng = np.random.default_rng(2)
    return [scan(900 + i, n) for i, n in enumerate(SIZES)], [lrng.integers(0, C, n).astype(np.int32) for n in SIZES]


def make(data, rng_seed, **kw):
    from pointasnl_amd.SemanticKITTI.scan_trainer import ScanTrainer

    scans, labels = data
    t = ScanTrainer(scans, labels, num_classes=C, num_point=NPOINT, num_buffer=BUFFER, batch_size=B, label_weights=WEIGHTS,
                    rng=np.random.RandomState(rng_seed), **kw)
    ref = R.ScanTrainFlowRef(scans, labels, label_weights=WEIGHTS, num_classes=C, num_point=NPOINT, num_buffer=BUFFER, batch_size=B,
                             rng=np.random.RandomState(rng_seed))
    return t, ref


def test_sixty_crops_equal_the_restatement(data):
    """30 batches of 2 items = 10 epochs of the 6 scans in list order, unaugmented: everything by bits, the RNG in step"""
    t, ref = make(data, 11, augment=False)
    assert t.steps_per_epoch == 3
    for n in range(30):
        got = t.next_batch()
        want = ref.batch()
        x = same_batch(got, want)
        assert x.shape == (B, NPOINT, 3) and want[4].tolist() == [(2 * n) % 6, (2 * n) % 6 + 1]
    assert t.rng.randint(1 << 30) == ref.rng.randint(1 << 30)
    assert t.item == 0


@pytest.mark.parametrize("symmetries", [(True, False, False), (False, False, False)])
def test_augmented_batches_are_the_formula(data, symmetries):
    """the training split's generator and, with the symmetries off, the validation split's (K:198-202)"""
    t, ref = make(data, 11, augment=True, seed=AUG_SEED, symmetries=symmetries)
    cfg = dict(P.DEFAULT, symmetries=symmetries)
    flips = set()
    for n in range(30):
        got = t.next_batch()
        want = ref.batch()
        x = same_batch(got, want, augmented=True)
        formula_holds(x, want[0], AUG_SEED, n * B, cfg)
        flips |= {float(np.sign(P.crop_params(AUG_SEED, n * B + c, cfg)["scales"][0])) for c in range(B)}
    assert flips == ({-1.0, 1.0} if symmetries[0] else {1.0})
    assert t.item == 60


def test_one_epoch_of_run_with_a_remainder(data):
    """S = 7, B = 2: three batches, the seventh scan is never drawn; a second epoch starts at the head of the list again"""
    scans, labels = data
    extra = (scans + [scan(977, 455)], labels + [np.zeros(455, np.int32)])
    t, ref = make(extra, 13, augment=True, seed=AUG_SEED)
    w, b = R.stand_in_weights(7, C)
    log = []
    acc = t.run(stand_in_step(w, b, log))
    assert len(log) == 3 == t.steps_per_epoch
    same_epoch(t, acc, log, C)
    for n in range(3):
        want = ref.batch()
        assert want[4].tolist() == [2 * n, 2 * n + 1]
        np.testing.assert_array_equal(log[n][1], want[1])
        np.testing.assert_array_equal(bits(log[n][2]), bits(want[2]))
        formula_holds(log[n][0], want[0], AUG_SEED, n * B)
    acc2 = t.run(stand_in_step(w, b, log))
    same_epoch(t, acc2, log[3:], C)
    want = ref.batch()
    assert want[4].tolist() == [0, 1]
    np.testing.assert_array_equal(log[3][1], want[1])
    formula_holds(log[3][0], want[0], AUG_SEED, 3 * B)


def test_error_paths(data):
    from pointasnl_amd.SemanticKITTI.scan_trainer import ScanTrainer

    scans, labels = data
    kw = dict(num_classes=C, num_point=NPOINT, num_buffer=BUFFER, batch_size=B, label_weights=WEIGHTS)
    with pytest.raises(IndexError):  # label 4 has no weight
        ScanTrainer(scans, labels, **dict(kw, label_weights=WEIGHTS[:4]))
    with pytest.raises(IndexError):
        ScanTrainer(scans, [l - 1 for l in labels], **kw)
    with pytest.raises(ValueError, match="k must be less than or equal to the number of training points"):
        ScanTrainer(scans, labels, **dict(kw, num_point=440))  # 440 + 24 + 6 - 1 = 469 > 450
    with pytest.raises(NotImplementedError):
        ScanTrainer(scans, labels, in_radius=1.0, **kw)
    with pytest.raises(ValueError):
        ScanTrainer(scans, labels[:3], **kw)
    t = ScanTrainer(scans[:1], labels[:1], **kw)  # S < B: the epoch is empty
    with pytest.raises(ValueError):
        t.next_batch()
    with pytest.raises(ValueError):  # no batch: the reference divides by zero in its log lines
        t.run(lambda x, y, w: None)
    t = ScanTrainer(scans, labels, **kw)
    with pytest.raises(ValueError, match="outside the scan"):
        t.stage((np.array([0, 1], np.int32), np.array([5, 450], np.int32), np.array([90, 90], np.int32),
                 np.zeros((B, NPOINT), np.int32)))


def test_pick_given_and_train_labels_equal_crop_pc(data):
    """pasnl_scan_pick_given -> crop -> order -> pasnl_scan_train_labels at B = 3 with a repeated scan in the batch and
    weights = NULL, against crop_pc over a DeviceScan item by item under the same draws"""
    from pointasnl_amd import _hip
    from pointasnl_amd.SemanticKITTI.scan_trainer import ScanTrainer
    from pointasnl_amd.SemanticKITTI.semantic_kitti_dataset_grid import DeviceScan, crop_pc

    scans, labels = data
    t = ScanTrainer(scans, labels, num_classes=C, num_point=NPOINT, num_buffer=BUFFER, batch_size=3, label_weights=WEIGHTS,
                    augment=False, rng=np.random.RandomState(5))
    clouds = np.array([4, 1, 4], np.int32)  # scan 4 twice
    rng, ref_rng = np.random.RandomState(21), np.random.RandomState(21)
    picks, ks, perms = np.empty(3, np.int32), np.empty(3, np.int32), np.empty((3, NPOINT), np.int32)
    want = []
    for c, cloud in enumerate(clouds):
        picks[c] = rng.choice(SIZES[cloud], 1)[0]
        k = NPOINT + BUFFER + rng.randint(0, BUFFER // 4)
        idx = np.arange(k)
        rng.shuffle(idx)
        ks[c], perms[c] = k, idx[:NPOINT]
        pick_idx = ref_rng.choice(SIZES[cloud], 1)
        want.append(crop_pc(scans[cloud], labels[cloud], DeviceScan(scans[cloud]), pick_idx, NPOINT, BUFFER, rng=ref_rng))
    t.stage((clouds, picks, ks, perms))
    pts, lab, wts, inds, cl = (host(a) for a in t.enqueue())
    desc = host(t.desc).view(np.int32).reshape(3, 10)
    for c, cloud in enumerate(clouds):
        sel_pts, sel_lab, sel_idx = want[c]
        np.testing.assert_array_equal(inds[c], sel_idx.astype(np.int32))
        np.testing.assert_array_equal(bits(pts[c]), bits(sel_pts))
        np.testing.assert_array_equal(lab[c], sel_lab)
        np.testing.assert_array_equal(bits(wts[c]), bits(WEIGHTS.astype(np.float32)[sel_lab]))
        assert desc[c, 2:6].tolist() == [cloud, picks[c], SIZES[cloud], ks[c]]
        assert int(desc[c, :2].view(np.int64)[0]) == int(t.offsets_host[cloud])
        np.testing.assert_array_equal(bits(desc[c, 6:9].view(np.float32)), bits(scans[cloud][picks[c]]))
    assert cl.tolist() == clouds.tolist()
    # weights == NULL: all-zero weights, the labels unchanged (the validation split, D:528-529)
    lab2 = torch.full((3, NPOINT), -7, dtype=torch.int32, device="cuda")
    wts2 = torch.full((3, NPOINT), np.nan, dtype=torch.float32, device="cuda")
    _hip.launch("pasnl_scan_train_labels", "test", 3, NPOINT, _hip.ptr(torch.from_numpy(inds).cuda()), _hip.ptr(t.cloud_stage),
                _hip.ptr(t.offsets), _hip.ptr(t.labels), ctypes.c_void_p(0), 0, _hip.ptr(lab2), _hip.ptr(wts2))
    np.testing.assert_array_equal(host(lab2), lab)
    assert (host(wts2) == 0).all()
    # a label outside the weight table is written as it is, with weight 0
    _hip.launch("pasnl_scan_train_labels", "test", 3, NPOINT, _hip.ptr(torch.from_numpy(inds).cuda()), _hip.ptr(t.cloud_stage),
                _hip.ptr(t.offsets), _hip.ptr(t.labels), _hip.ptr(t.label_weights), 2, _hip.ptr(lab2), _hip.ptr(wts2))
    np.testing.assert_array_equal(host(lab2), lab)
    np.testing.assert_array_equal(bits(host(wts2)), bits(np.where(lab < 2, WEIGHTS.astype(np.float32)[np.minimum(lab, 1)], np.float32(0))))
