"""What tests/test_gpu_block_trainer.py and tests/test_gpu_kitti_block_trainer.py share: a step that records what the device
loop fed it, the restatement's step that answers with the device's logits, and the comparison of one epoch."""
import numpy as np
import torch

import block_train_flow_ref as R

LOSS_TOL = 1e-5  # * max(1, |ref|): the tolerance tests/test_gpu_block_tester.py holds pasnl_block_score's loss to (the code is shared)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def host(t):
    return t.cpu().numpy()


def state_of(rng):
    st = rng.get_state()
    return np.concatenate([st[1].astype(np.int64), [st[2]]])


def same_bits_or_nan(got, want):
    """bit for bit, but any NaN for a NaN (0 / 0 has no one bit pattern)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[keep], bits(want)[keep])


def recording_step(w, b, log):
    """the device loop's step: a fixed map of every point to C logits, with a tie and a run of equal rows; log gets
    (fed, labels, smpw, logits) of every call as host arrays"""
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()

    def step(x, labels, smpw):
        assert x.is_cuda and labels.dtype == torch.int32 and smpw.dtype == torch.float32
        out = torch.sin(x[:, :, :3] @ wt + bt) * 4.0
        out[1, 0, :] = 1.5            # np.argmax: the first maximum
        out[0, 3, 1:3] = 7.0
        log.append(tuple(host(a).copy() for a in (x, labels, smpw, out)))
        return out

    return step


def replaying_step(log, first=0):
    """the restatement's step: holds what it is given to what the device's step was given, bit for bit, and answers with the
    device's logits"""
    k = [first]

    def step(fed, labels, smpw):
        got = log[k[0]]
        np.testing.assert_array_equal(bits(got[0]), bits(fed))
        np.testing.assert_array_equal(got[1], labels)
        np.testing.assert_array_equal(bits(got[2]), bits(smpw))
        k[0] += 1
        return got[3]

    return step, k


def same_epoch(trainer, acc, out, line, extra):
    """the totals, the ratios and the three lines of the device's last epoch against the restatement's `out`"""
    tot = trainer.totals()
    want = {k: out[k] for k in ("total_correct", "total_seen", "total_iou_deno")}
    assert tot == want and 0 < want["total_correct"] < want["total_seen"]
    assert want["total_seen"] == out["num_batches"] * trainer.B * trainer.P and trainer.num_batches == out["num_batches"]
    np.testing.assert_array_equal(trainer.order, out["order"])
    assert acc == trainer.accuracy() == want["total_correct"] / float(want["total_seen"])
    assert trainer.iou() == want["total_correct"] / float(want["total_iou_deno"])
    ref_loss = out["loss_sum"] / out["num_batches"]
    print("mean loss: device %.9f, restatement %.9f" % (trainer.mean_loss(extra), ref_loss))
    assert abs(trainer.mean_loss(extra) - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss))
    got, ref = trainer.report(extra), R.report(out, line)
    assert got[1:] == ref[1:] and len(got) == 3
    head, value = got[0].rsplit(" ", 1)
    assert head == "Training loss:" and abs(float(value) - float(ref[0].rsplit(" ", 1)[1])) <= 2 * LOSS_TOL * max(1.0, abs(ref_loss))
