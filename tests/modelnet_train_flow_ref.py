"""numpy restatement of the ModelNet40 training input flow, the yardstick of pointasnl_amd.modelnet_trainer: the augmentation
chain of the reference's utils/provider.py (P) as train.py (T) :226-237 applies it -- rotation about y, rotation
perturbation, scale, shift, point shuffle, point dropout -- with the draws given, and `train_one_epoch` (T:208-264) over
tests/modelnet_flow_ref.ModelNetFlowRef(shuffle=True).  Every matrix product is written as the explicit float64 sum
(x0*M[0][c] + x1*M[1][c]) + x2*M[2][c] the kernel computes (numpy's dgemm fixes no order); everything else is numpy's own
expression in the reference's dtypes.  tests/test_modelnet_trainer_flow.py pins it to the reference's functions.

The numpy mirrored is numpy >= 2: an in-place float32 `*=` by an np.float64 scalar multiplies in float64 and rounds once."""
import numpy as np

import modelnet_flow_ref as R

MAX_DROPOUT_RATIO = 0.875  # P:246


def rotation_about_y(u):
    """P:61-66, 99-104"""
    rotation_angle = u * 2 * np.pi
    cosval = np.cos(rotation_angle)
    sinval = np.sin(rotation_angle)
    return np.array([[cosval, 0, sinval],
                     [0, 1, 0],
                     [-sinval, 0, cosval]])


def perturbation(g, angle_sigma=0.06, angle_clip=0.18):
    """P:120-130, 190-200"""
    angles = np.clip(angle_sigma * g, -angle_clip, angle_clip)
    Rx = np.array([[1, 0, 0],
                   [0, np.cos(angles[0]), -np.sin(angles[0])],
                   [0, np.sin(angles[0]), np.cos(angles[0])]])
    Ry = np.array([[np.cos(angles[1]), 0, np.sin(angles[1])],
                   [0, 1, 0],
                   [-np.sin(angles[1]), 0, np.cos(angles[1])]])
    Rz = np.array([[np.cos(angles[2]), -np.sin(angles[2]), 0],
                   [np.sin(angles[2]), np.cos(angles[2]), 0],
                   [0, 0, 1]])
    return np.dot(Rz, np.dot(Ry, Rx))


def draw(rng, bsize, npoint, rotation):
    """the draws of one batch in the reference's order -> dict(mats (bsize,2,3,3) f64 or None, scale (bsize), shift (bsize,3),
    perm (npoint) i32, ratio (bsize), u (bsize,npoint))"""
    mats = None
    if rotation:
        mats = np.zeros((bsize, 2, 3, 3))
        for k in range(bsize):
            mats[k, 0] = rotation_about_y(rng.uniform())
        for k in range(bsize):
            mats[k, 1] = perturbation(rng.randn(3))
    scale = rng.uniform(0.8, 1.25, bsize)
    shift = rng.uniform(-0.1, 0.1, (bsize, 3))
    perm = np.arange(npoint)
    rng.shuffle(perm)
    ratio, u = np.zeros((bsize,)), np.zeros((bsize, npoint))
    for k in range(bsize):
        ratio[k] = rng.random() * MAX_DROPOUT_RATIO
        u[k] = rng.random((npoint))
    return dict(mats=mats, scale=scale, shift=shift, perm=perm.astype(np.int32), ratio=ratio, u=u)


def dot3(x, m):
    """(N,3) float64 @ (3,3) float64 as explicit sums"""
    x = x.astype(np.float64)
    return np.stack([(x[:, 0] * m[0, c] + x[:, 1] * m[1, c]) + x[:, 2] * m[2, c] for c in range(3)], axis=1)


def augment(batch, d):
    """T:226-237 on the float64 batch (bsize, N, 3|6) `next_batch` returned, with the draws `d` -> what T:240 copies into
    cur_batch_data: float32 with rotation, float64 without"""
    bsize, npoint, ch = batch.shape
    data = batch.copy()
    if d["mats"] is not None:
        rotated = np.zeros(data.shape, dtype=np.float32)
        for k in range(bsize):
            a, r = d["mats"][k, 0], d["mats"][k, 1]
            for h in range(0, ch, 3):
                v = dot3(data[k, :, h:h + 3], a)
                if ch == 3:
                    v = v.astype(np.float32)  # P:59: rotate_point_cloud allocates float32; P:107 writes into float64
                rotated[k, :, h:h + 3] = dot3(v, r)
        data = rotated
    for k in range(bsize):
        if data.dtype == np.float32:
            data[k, :, 0:3] = (data[k, :, 0:3].astype(np.float64) * d["scale"][k]).astype(np.float32)
        else:
            data[k, :, 0:3] = data[k, :, 0:3] * d["scale"][k]
    for k in range(bsize):
        if data.dtype == np.float32:
            data[k, :, 0:3] = (data[k, :, 0:3].astype(np.float64) + d["shift"][k, :]).astype(np.float32)
        else:
            data[k, :, 0:3] = data[k, :, 0:3] + d["shift"][k, :]
    data = data[:, d["perm"], :]
    for k in range(bsize):
        drop_idx = np.where(d["u"][k] <= d["ratio"][k])[0]
        if len(drop_idx) > 0:
            data[k, drop_idx, :] = data[k, 0, :]
    return data


def source_rows(d, k):
    """the row of the unshuffled cloud k that output row j shows: perm[0] where the point is dropped, perm[j] otherwise"""
    return np.where(d["u"][k] <= d["ratio"][k], d["perm"][0], d["perm"])


def train_one_epoch(ds, step, num_classes, rotation=False, rng=np.random, reg_loss=0.0):
    """T:208-264 over the dataset `ds` (shuffle=True).  step: ((B, N, ch) float32, (B,) int32) -> (B, num_classes) float32
    logits.  -> dict: accuracy, the counters, mean_loss, and per batch what was fed, the labels and the predictions."""
    B, N = ds.batch_size, ds.npoints
    cur_data = np.zeros((B, N, ds.num_channel()))
    cur_label = np.zeros((B), dtype=np.int32)
    out = dict(total_correct=0, total_seen=0, batches=0, fed=[], labels=[], preds=[], bsizes=[], draws=[])
    loss_sum = 0
    num_batch = int(len(ds) / B)
    while ds.has_next_batch():
        data, label = ds.next_batch()
        bsize = data.shape[0]
        d = draw(rng, bsize, N, rotation)
        cur_data[0:bsize, ...] = augment(data, d)
        cur_label[0:bsize] = label
        fed = cur_data.astype(np.float32)  # the feed into a float32 placeholder
        logits = np.asarray(step(fed, cur_label.copy()), np.float32)
        loss_sum += R.cross_entropy(logits, cur_label) + reg_loss
        pred = np.argmax(logits, 1)
        out["total_correct"] += int(np.sum(pred[0:bsize] == label[0:bsize]))
        out["total_seen"] += bsize
        out["batches"] += 1
        out["fed"].append(fed)
        out["labels"].append(cur_label.copy())
        out["preds"].append(pred[:bsize].astype(np.int32))
        out["bsizes"].append(bsize)
        out["draws"].append(d)
    out["loss_sum"] = loss_sum
    out["mean_loss"] = loss_sum / num_batch if num_batch else None
    out["accuracy"] = out["total_correct"] / float(out["total_seen"])
    ds.reset()
    return out


def report(out, learning_rate):
    """the lines T:261-263 log"""
    return ["Current Learning Rate %.6f" % learning_rate, "Training loss: %f" % out["mean_loss"],
            "Training accuracy: %f\n" % out["accuracy"]]
