"""What tests/test_gpu_scene_trainer.py and tests/test_gpu_scan_trainer.py share: the comparison of device batches with the
restatement's, of augmented inputs with the kernel's formula, and of one epoch's tallies with numpy's."""
import numpy as np
import torch

import grid_train_flow_ref as R
import philox_ref as P
from block_train_checks import LOSS_TOL, bits, host  # LOSS_TOL: 1e-5 * max(1, |ref|), the block trainers' (the score's code is shared)


def same_batch(got, want, augmented=False):
    """(inputs, labels, weights, point_inds, cloud_inds) of the device against the restatement's, bit for bit (the inputs
    only where they are unaugmented)"""
    x, y, w, inds, clouds = (host(t) for t in got)
    assert y.dtype == np.int32 and w.dtype == np.float32 and inds.dtype == np.int32 and clouds.dtype == np.int32
    np.testing.assert_array_equal(inds, want[3])
    np.testing.assert_array_equal(clouds, want[4])
    np.testing.assert_array_equal(y, want[1])
    np.testing.assert_array_equal(bits(w), bits(want[2]))
    if not augmented:
        assert x.dtype == np.float32 and x.shape == want[0].shape
        np.testing.assert_array_equal(bits(x), bits(want[0]))
    return x


def formula_holds(augmented, plain, seed, item0, cfg=P.DEFAULT):
    """the trainer's augmented batch against the formula: the public kernel call on the unaugmented batch under the same
    (seed, item0) emits cos, sin, scales, keep and the normals; numpy applies them (philox_ref.apply) -- bit for bit; theta,
    the scales and keep are philox_ref's"""
    from pointasnl_amd import grid_augment

    out, params, normals = grid_augment.augment_input(torch.from_numpy(plain).cuda(), grid_augment.config_of(
        None, augment_rotation=cfg["rotation"], augment_symmetries=cfg["symmetries"]), seed, item0, return_params=True)
    params, normals = host(params), host(normals)
    np.testing.assert_array_equal(bits(host(out)), bits(augmented))
    for c in range(plain.shape[0]):
        q = P.crop_params(seed, item0 + c, cfg)
        assert bits(params[c, 0]) == bits(q["theta"]) and params[c, 6] == q["keep"]
        np.testing.assert_array_equal(bits(params[c, 3:6]), bits(q["scales"]))
        want = P.apply(plain[c], params[c, 1], params[c, 2], params[c, 3:6], params[c, 6], normals[c], cfg)
        np.testing.assert_array_equal(bits(augmented[c]), bits(want))
    assert (bits(augmented[:, :, :3]) != bits(plain[:, :, :3])).any()


def stand_in_step(w, b, log):
    """the device loop's step: a fixed map of xyz to C logits with a tie and a run of equal rows; log gets (inputs, labels,
    weights, logits) of every call as host arrays"""
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()

    def step(x, labels, weights):
        assert x.is_cuda and labels.dtype == torch.int32 and weights.dtype == torch.float32
        out = torch.sin(x[:, :, :3] @ wt + bt) * 4.0
        out[1, 0, :] = 1.5            # np.argmax: the first maximum
        out[0, 3, 1:3] = 7.0
        log.append(tuple(host(a).copy() for a in (x, labels, weights, out)))
        return out

    return step


def same_epoch(trainer, acc, log, num_classes):
    """the three integer tallies of the device's epoch against numpy's over what the step saw and answered, exactly; the
    loss within LOSS_TOL; the three lines"""
    out = R.new_totals()
    for x, y, w, logits in log:
        R.train_score(out, logits, y, w, num_classes)
    out["num_batches"] = len(log)
    want = {k: out[k] for k in ("total_correct", "total_seen", "total_iou_deno")}
    assert trainer.totals() == want and 0 < want["total_correct"] < want["total_seen"]
    assert want["total_seen"] == len(log) * trainer.B * trainer.P and trainer.num_batches == len(log) == trainer.forwards
    assert (want["total_correct"], want["total_seen"], want["total_iou_deno"]) == R.recount([l[1] for l in log], [l[3] for l in log])
    assert acc == trainer.accuracy() == want["total_correct"] / float(want["total_seen"])
    assert trainer.iou() == want["total_correct"] / float(want["total_iou_deno"])
    ref_loss = out["loss_sum"] / out["num_batches"]
    print("mean loss: device %.9f, numpy %.9f" % (trainer.mean_loss(), ref_loss))
    assert abs(trainer.mean_loss() - ref_loss) <= LOSS_TOL * max(1.0, abs(ref_loss))
    got, ref = trainer.report(), R.report(out)
    assert got[1:] == ref[1:] and len(got) == 3 and got[0].startswith("Training Loss: ")
    assert abs(float(got[0].rsplit(" ", 1)[1]) - float(ref[0].rsplit(" ", 1)[1])) <= 2 * LOSS_TOL * max(1.0, abs(ref_loss))
    assert abs(trainer.mean_loss(0.25) - trainer.mean_loss() - 0.25) < 1e-12
