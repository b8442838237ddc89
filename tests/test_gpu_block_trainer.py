"""GPU: ScanNet's training input loop on the device (pasnl_block_train_batch and pasnl_block_train_score of
csrc/block_test.hip, pointasnl_amd.ScanNet.block_trainer and `ScannetDataset.trainer`) against the numpy restatement
tests/block_train_flow_ref.py run live on the same machine (it is pinned to the reference's own run in
tests/test_block_trainer_flow.py).  Every comparison is exact -- bit patterns or integers; a NaN for a NaN where the
reference divides 0 by 0 -- but the loss, held to 1e-5 * max(1, |ref|) as tests/test_gpu_block_tester.py holds
pasnl_block_score's, whose code it shares."""
import ctypes
import os

import numpy as np
import pytest
import torch

import block_train_flow_ref as R
from block_train_checks import LOSS_TOL, bits, host, recording_step, replaying_step, same_bits_or_nan, same_epoch, state_of
from guarded import NAN_BYTE, WS_BYTE, Guarded, output_guard

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
C, P, B = 5, 70, 2
WEIGHTS = np.array([1.0, 0.5, 2.0, 1.25, 3.0])
LINE = "Training accuracy: %f"


@pytest.fixture(scope="module")
def scenes():
    """5 fixture scenes: the four of tests/golden/block_flow.npz and the dense room again"""
    gold = np.load(os.path.join(HERE, "golden", "block_flow.npz"))
    four = [(gold["scene%d/points" % k], gold["scene%d/labels" % k]) for k in range(4)]
    return four + [four[1]]


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def rot_of(angles):
    return torch.from_numpy(np.stack([np.cos(angles), np.sin(angles)], axis=1).astype(np.float64)).cuda()


def blocks(seed, rows, n, width):
    rng = np.random.default_rng(seed)
    return (rng.random((rows, n, width)) * 3.0 - [1.2, 0.4, 0.1] * (width // 3)).astype(np.float32)


# ---- pasnl_block_train_batch
@pytest.mark.parametrize("width", [3, 6])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_train_batch_equals_the_restatement(n, rows, width):
    """T:253-254 at the wave edges and across one BN_TILE boundary, with and without copied columns, angle 0 among the
    angles: rotate, round to float32, normalize, bit for bit; the guard bytes round the output stay as they were; the
    validation entry on the same input gives other bits (n == 1 is 0 / 0 in both).  In place (src == batch) gives the same."""
    from pointasnl_amd import _hip

    raw = blocks(100 + n, rows, n, width)
    angles = [0.0, 1.2345, 5.9][:rows] if rows > 1 else [2.5]
    with np.errstate(invalid="ignore", divide="ignore"):
        want = R.train_batch(raw, angles)
    src, rot = torch.from_numpy(raw).cuda(), rot_of(angles)
    out = Guarded(raw.nbytes, NAN_BYTE, output_guard(n * width * 4))
    _hip.launch("pasnl_block_train_batch", "train batch", rows, n, width, ptr(src), ptr(rot), ctypes.c_void_p(out.ptr))
    torch.cuda.synchronize()
    assert out.guards_intact()
    got = out.floats(raw.shape)
    same_bits_or_nan(got, want)
    assert np.isnan(want[:, :, :3]).all() if n == 1 else np.isfinite(want).all()
    np.testing.assert_array_equal(bits(got[:, :, 3:]), bits(raw[:, :, 3:]))
    ev = torch.zeros_like(src)
    _hip.launch("pasnl_block_normalize", "eval order", rows, n, width, ptr(src), ptr(rot), ptr(ev))
    if n > 1:
        assert (bits(host(ev)) != bits(got)).any()  # the other order is another result
    _hip.launch("pasnl_block_train_batch", "train batch in place", rows, n, width, ptr(src), ptr(rot), ptr(src))
    same_bits_or_nan(host(src), want)


def test_train_batch_of_identical_points_is_the_reference_nan():
    """a block whose rows are all one point (dyadic coordinates, angle 0: the chain and the rotation are exact) has m == 0 and
    gets 0 / 0 = NaN in its coordinates as in numpy; its copied columns and the blocks beside it are untouched by that"""
    from pointasnl_amd import _hip

    raw = blocks(7, 3, 64, 6)
    raw[1, :, :3] = np.array([0.75, -1.5, 2.0], np.float32)
    angles = [0.7, 0.0, 3.3]
    with np.errstate(invalid="ignore", divide="ignore"):
        want = R.train_batch(raw, angles)
    assert np.isnan(want[1, :, :3]).all() and np.isfinite(want[0]).all() and np.isfinite(want[2]).all()
    src, rot = torch.from_numpy(raw).cuda(), rot_of(angles)
    out = torch.zeros_like(src)
    _hip.launch("pasnl_block_train_batch", "train batch", 3, 64, 6, ptr(src), ptr(rot), ptr(out))
    same_bits_or_nan(host(out), want)


def test_train_batch_validation_codes():
    """as pasnl_block_normalize's, and rot is required"""
    from pointasnl_amd import _hip

    lib = _hip.lib()
    t = torch.zeros((64,), dtype=torch.float64, device="cuda")
    some, null = ptr(t), ctypes.c_void_p(0)
    for args, code in (((-1, 8, 3, some, some, some), -1), ((1, 0, 3, some, some, some), -1), ((1, 8, 2, some, some, some), -1),
                       ((0, 8, 3, null, null, null), 0), ((1, 8, 3, null, some, some), -2), ((1, 8, 3, some, null, some), -2),
                       ((1, 8, 3, some, some, null), -2)):
        assert lib.pasnl_block_train_batch(*args, null) == code
    with pytest.raises(ValueError):
        _hip.launch("pasnl_block_train_batch", "width", 1, 8, 2, some, some, some)
    assert (host(t) == 0).all()


# ---- pasnl_block_train_score
def score_inputs(seed, rows, n, c):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((rows, n, c)).astype(np.float32)
    label = rng.integers(0, c, (rows, n)).astype(np.int32)
    logits[0, 0, :] = 0.25                     # a row of tied logits: the first maximum
    label[0, 0] = 0
    if rows * n > 1:
        flat = logits.reshape(-1, c)
        flat[-1, c - 1] = np.nan               # a row with a NaN logit: the first NaN is the prediction
        label.reshape(-1)[-1] = c - 1
    smpw = (rng.random((rows, n)) * 2.0 + 0.1).astype(np.float32)
    flat = smpw.reshape(-1)
    flat[rng.random(rows * n) < 0.3] = 0.0
    flat[rng.random(rows * n) < 0.2] = -0.75
    flat[-1] = 0.0                             # the NaN row carries no weight: the loss stays finite
    return logits, label, smpw


@pytest.mark.parametrize("c", [2, 21, 256])
@pytest.mark.parametrize("rows,n", [(1, 1), (1, 255), (1, 256), (1, 257), (3, 70)])
def test_train_score_tallies_and_loss(rows, n, c):
    """T:264-272 for one entry, a workgroup less one, a full one, one more, and 3 x 70; 2, 21 and the most classes: the three
    int64 tallies exactly -- over every entry, whatever smpw (0, negative, NaN) and label 0 included -- and the loss under
    the shared tolerance; two calls accumulate; a NaN weight makes the loss NaN there as here.  Counters, loss and the
    exact-size workspace sit in guarded memory."""
    from pointasnl_amd import _hip

    counters, loss = Guarded(24, 0), Guarded(16, 0)
    ws = Guarded(int(_hip.lib().pasnl_block_score_workspace_bytes()), WS_BYTE)
    ref = R.new_totals()

    def call(logits, label, smpw):
        dev = [torch.from_numpy(a).cuda() for a in (logits, label, smpw)]
        _hip.launch("pasnl_block_train_score", "train score", rows, n, c, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]),
                    ctypes.c_void_p(counters.ptr), ctypes.c_void_p(loss.ptr), ctypes.c_void_p(ws.ptr))
        torch.cuda.synchronize()
        with np.errstate(invalid="ignore"):
            R.train_score(ref, logits, label, smpw, c)
        assert counters.guards_intact() and loss.guards_intact() and ws.guards_intact()
        got = counters.array((3,), np.int64)
        assert list(got) == [ref["total_correct"], ref["total_seen"], ref["total_iou_deno"]]
        assert got[2] == 2 * got[1] - got[0]
        return loss.array((2,), np.float64).copy()

    first = score_inputs(1000 * c + n, rows, n, c)
    got = call(*first)
    tol = LOSS_TOL * max(1.0, abs(ref["losses"][0]))
    print("loss: device %.9f, restatement %.9f" % (got[1], ref["losses"][0]))
    assert np.isfinite(ref["losses"][0]) and abs(got[1] - ref["losses"][0]) <= tol and got[0] == got[1]
    assert (ref["total_correct"], ref["total_seen"], ref["total_iou_deno"]) == R.recount([first[1]], [first[0]])
    second = score_inputs(1000 * c + n + 1, rows, n, c)
    got = call(*second)
    tol2 = LOSS_TOL * max(1.0, abs(ref["losses"][1]))
    assert abs(got[1] - ref["losses"][1]) <= tol2 and abs(got[0] - (ref["losses"][0] + ref["losses"][1])) <= tol + tol2
    assert ref["total_seen"] == 2 * rows * n
    third = score_inputs(1000 * c + n + 2, rows, n, c)
    third[2].reshape(-1)[0] = np.nan
    got = call(*third)
    assert np.isnan(ref["losses"][2]) and np.isnan(got[1]) and np.isnan(got[0]) and ref["total_seen"] == 3 * rows * n


def test_train_score_refuses_more_classes_than_it_holds():
    from pointasnl_amd import _hip

    t = torch.zeros((257 * 4,), dtype=torch.float32, device="cuda")
    with pytest.raises(_hip.PasnlUnsupported):
        _hip.launch("pasnl_block_train_score", "classes", 1, 4, 257, ptr(t), ptr(t), ptr(t), ptr(t), ptr(t), ptr(t))
    assert (host(t) == 0).all()


# ---- the loop
@pytest.mark.parametrize("rgb", [True, False])
def test_two_epochs_equal_the_restatement(scenes, rgb):
    """T:233-276 over 5 scenes with B = 2, P = 70, two epochs in a row under one RandomState: the shuffled order, every batch
    handed to `step` with its labels and smpw (the fifth shuffled index draws nothing), the totals, the report lines and the
    RNG state after each epoch"""
    from pointasnl_amd.ScanNet.block_trainer import BlockTrainer

    width = 6 if rgb else 3
    ref_rng, rng = np.random.RandomState(51), np.random.RandomState(51)
    w, b = R.stand_in_weights(5, C)
    log = []
    t = BlockTrainer([p if rgb else p[:, 0:3] for p, _ in scenes], [l for _, l in scenes], num_classes=C, block_points=P, batch_size=B,
                     labelweights=WEIGHTS, rng=rng)
    step = recording_step(w, b, log)
    for epoch in range(2):
        acc = t.run(step)
        assert len(log) == 2 * (epoch + 1) and t.forwards == 2
        ref_step, asked = replaying_step(log, 2 * epoch)
        out = R.train_epoch(lambda i: R.chopped_item(*scenes[i], WEIGHTS, P, ref_rng, with_rgb=rgb)[:3], len(scenes), B, P, width,
                            R.train_batch, ref_step, C, ref_rng, extra=0.25)
        assert asked[0] == 2 * (epoch + 1) and log[-1][0].shape == (B, P, width)
        same_epoch(t, acc, out, LINE, 0.25)
        np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))
    assert not np.array_equal(bits(log[0][0]), bits(log[2][0]))  # the second epoch is another epoch


def test_dataset_trainer_and_train_batch_alone(scenes):
    """`ScannetDataset(split='train').trainer.run` over the same tester as `.tester` (21 classes, the split's own weights)
    equals the restatement; `train_batch(raw, angles)` alone is the restatement's transform; fewer scenes than a batch have
    no batch, and the results say so"""
    from pointasnl_amd.ScanNet.block_tester import BlockTester
    from pointasnl_amd.ScanNet.block_trainer import BlockTrainer
    from pointasnl_amd.ScanNet.scannet_dataset import ScannetDataset

    ref_rng, rng = np.random.RandomState(52), np.random.RandomState(52)
    ds = ScannetDataset(None, block_points=P, split="train", with_rgb=True, scene_points_list=[p.copy() for p, _ in scenes],
                        semantic_labels_list=[l.copy() for _, l in scenes], scene_points_id=[np.arange(len(l)) for _, l in scenes],
                        scene_points_num=[len(l) for _, l in scenes], rng=rng, batch_size=B)
    assert ds.trainer is ds.trainer and ds.trainer.tester is ds.tester and isinstance(ds.trainer, BlockTrainer)
    w, b = R.stand_in_weights(6, 21)
    log = []
    acc = ds.trainer.run(recording_step(w, b, log))
    ref_step, asked = replaying_step(log)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = R.train_epoch(lambda i: R.chopped_item(*scenes[i], ds.labelweights, P, ref_rng)[:3], len(scenes), B, P, 6, R.train_batch,
                            ref_step, 21, ref_rng)
    assert asked[0] == 2
    same_epoch(ds.trainer, acc, out, LINE, 0.0)
    np.testing.assert_array_equal(state_of(rng), state_of(ref_rng))

    raw = blocks(9, B, P, 6)
    angles = [0.0, 4.4]
    got = host(ds.trainer.train_batch(torch.from_numpy(raw).cuda(), angles))
    np.testing.assert_array_equal(bits(got), bits(R.train_batch(raw, angles)))

    few = BlockTrainer(tester=BlockTester([scenes[0][0]], [scenes[0][1]], num_classes=C, block_points=P, batch_size=B,
                                           rng=np.random.RandomState(1)))
    with pytest.raises(ValueError):
        few.run(lambda *a: None)
    with pytest.raises(ValueError):
        few.mean_loss()
    assert few.num_batches == 0 and few.totals() == dict(total_correct=0, total_seen=0, total_iou_deno=0)
