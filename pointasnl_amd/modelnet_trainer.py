"""The ModelNet40 training input loop on the device -- reference train.py (T) :208-264 (`train_one_epoch`) with the
augmentation chain of utils/provider.py (P) :39-253 and the shuffled `ModelNetDataset` of modelnet_dataset.py (D) :77,
114-136.  It is the loop that trains `pointasnl_cls`.

`ModelNetTrainer` is built over a `ModelNetTester` (composition: the prepared set, the visiting order, the persistent batch,
the vote with one vote, the tally and the single read-back per epoch are the tester's).  One batch runs on the current
stream with no host synchronisation (csrc/modelnet_test.hip):

  [uniform, first visit of a shape: pasnl_modelnet_fps -> pasnl_modelnet_normalize]
  one staged copy of the batch's draws
  pasnl_modelnet_augment      -> the persistent (B, num_point, 3|6) batch and (B,) labels: next_batch and the whole chain
  step(batch, labels)         -> (B, C) logits (the caller's forward, backward and update)
  pasnl_cls_vote, pasnl_cls_tally -> predictions, int64 counters, the loss sum

Only RNG draws travel up; the counters come down once, at the end of the epoch.  The draws are the reference's, in its
order, from the caller's numpy RNG.  Construction: `shuffle(idxs)` (D:77 -> `reset`).  Per batch of `bsize` clouds: with
`uniform` one `randint(0, n_i)` per shape visited for the first time; with `rotation` bsize x `uniform()` (P:61, 99) then
bsize x `randn(3)` (P:120, 190); `uniform(0.8, 1.25, bsize)` (P:241); `uniform(-0.1, 0.1, (bsize, 3))` (P:227);
`shuffle(arange(num_point))` (P:47-48); per cloud `random()` then `random(num_point)` (P:249-250).  At the epoch's end
`reset()` draws the next epoch's shuffle (T:264).  The two rotation matrices of a cloud are built here, with numpy, from
the reference's expressions: the device never evaluates a sine.

The rows past the last real one of an epoch's final batch are not written: they still hold the batch before it, already
augmented (zeros when there is none), go through `step` and count in the loss, not in the accuracy -- T:214, 240.

Deviations: `shapes` are arrays, not files.  There is no summary writer (T:249).  The loss is the tester's -- the batch's
mean cross-entropy computed on the device over all B rows (a float32 log-sum-exp per row, float64 sums), not TensorFlow's
`loss_val`; the caller's regularisation term enters `mean_loss` as a number; it is compared under a tolerance, never by
bits.  The numpy mirrored is numpy >= 2 (checked under 2.2.6): with rotation the batch is float32 when it is scaled and
shifted, and an in-place float32 `*=` by an `np.float64` scalar multiplies in float64 and rounds once; numpy < 2 would
multiply in float32.  Products of a row with a rotation matrix are (x0*M[0][c] + x1*M[1][c]) + x2*M[2][c]; numpy's dgemm
fixes no summation order, so a rotated coordinate may differ from the reference's by one float32 ulp (measured: none of
60 300 does).
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.modelnet_tester import ModelNetTester

_p = _hip.ptr


def rotation_about_y(u):
    """P:61-66, 99-104 from the `uniform()` draw u"""
    rotation_angle = u * 2 * np.pi
    cosval = np.cos(rotation_angle)
    sinval = np.sin(rotation_angle)
    return np.array([[cosval, 0, sinval],
                     [0, 1, 0],
                     [-sinval, 0, cosval]])


def perturbation(g, angle_sigma=0.06, angle_clip=0.18):
    """P:120-130, 190-200 from the `randn(3)` draw g"""
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


class ModelNetTrainer:
    """`ModelNetTrainer(shapes, labels, num_classes=40, num_point=1024, batch_size=16, normal_channel=True, rotation=False,
    uniform=False, normalize=True, rng=np.random)`.

    shapes, labels, uniform, normalize, rng: as `ModelNetTester` takes them.  rotation: train.py's --rotation (the rotation
    about y and the perturbation in front of scale, shift, shuffle and dropout)."""

    MAX_DROPOUT_RATIO = 0.875  # P:246

    def __init__(self, shapes, labels, num_classes=40, num_point=1024, batch_size=16, normal_channel=True, rotation=False,
                 uniform=False, normalize=True, rng=np.random):
        self.tester = ModelNetTester(shapes, labels, num_classes=num_classes, num_point=num_point, batch_size=batch_size,
                                     normal_channel=normal_channel, uniform=uniform, normalize=normalize, rng=rng)
        t = self.tester
        self.S, self.C, self.P, self.B, self.ch, self.rng, self.rotation = t.S, t.C, t.P, t.B, t.ch, rng, bool(rotation)
        # the draws of one batch, in float64 words: mats | scale | shift | ratio | u | perm (int32, two to a word)
        B, N = self.B, self.P
        self.at = dict(mats=0, scale=18 * B, shift=19 * B, ratio=22 * B, u=23 * B, perm=23 * B + B * N)
        self.words = self.at["perm"] + (N + 1) // 2
        self.stage = torch.zeros((self.words,), dtype=torch.float64, device=t.device)
        self.reset()

    # ---- the dataset's side
    def reset(self):
        """D:114-119 with shuffle: the next epoch's visiting order"""
        self.idxs = np.arange(0, self.S)
        self.rng.shuffle(self.idxs)
        self.tester.set_order(self.idxs)

    def has_next_batch(self):
        return self.tester.has_next_batch()

    def draw(self, bsize):
        """the draws of one batch of bsize clouds in the reference's order -> one float64 host array laid out as the stage"""
        B, N, at, rng = self.B, self.P, self.at, self.rng
        host = np.zeros((self.words,), np.float64)
        if self.rotation:
            mats = host[:18 * bsize].reshape(bsize, 2, 9)
            for k in range(bsize):
                mats[k, 0] = rotation_about_y(rng.uniform()).reshape(9)
            for k in range(bsize):
                mats[k, 1] = perturbation(rng.randn(3)).reshape(9)
        host[at["scale"]:at["scale"] + bsize] = rng.uniform(0.8, 1.25, bsize)
        host[at["shift"]:at["shift"] + 3 * bsize] = rng.uniform(-0.1, 0.1, (bsize, 3)).reshape(-1)
        idx = np.arange(N)
        rng.shuffle(idx)
        host[at["perm"]:].view(np.int32)[:N] = idx
        for k in range(bsize):
            host[at["ratio"] + k] = rng.random() * self.MAX_DROPOUT_RATIO
            host[at["u"] + k * N:at["u"] + (k + 1) * N] = rng.random((N))
        return host

    def augment_batch(self):
        """T:224-241 into the persistent buffers -> (batch (B,num_point,3|6) f32, labels (B,) i32, bsize): the next batch of
        the epoch's order through rotation, perturbation, scale, shift, shuffle and dropout; rows bsize.. of both still hold
        what the batch before left there.  It moves the RNG exactly as one batch of `run` does."""
        t = self.tester
        if not t.has_next_batch():
            raise IndexError("no batch left in this epoch: reset()")
        start = t.batch_idx * self.B
        bsize = min(self.B, self.S - start)
        if t.uniform:
            t.prepare(t.idxs[start:start + bsize])
        self.stage.copy_(torch.from_numpy(self.draw(bsize)).pin_memory(), non_blocking=True)
        at = {k: _p(self.stage, 8 * v) for k, v in self.at.items()}
        _hip.launch("pasnl_modelnet_augment", "ModelNetTrainer augment", self.B, bsize, self.P, self.ch, _p(t.order), ctypes.c_long(self.S),
                    ctypes.c_long(start), ctypes.c_long(self.S), _p(t.prepared), _p(t.shape_labels),
                    at["mats"] if self.rotation else ctypes.c_void_p(0), at["scale"], at["shift"], at["perm"], at["ratio"], at["u"],
                    _p(t.batch), _p(t.label))
        t.batch_idx += 1
        t.bsize, t.batch_start = bsize, start
        return t.batch, t.label, bsize

    # ---- the loop's side
    def run(self, step):
        """T:208-264, one epoch.  step: ((B,num_point,3|6) f32, (B,) i32) device tensors -> (B,C) f32 logits, called once
        per batch (the caller's forward, backward and update).  -> total_correct / float(total_seen)."""
        t = self.tester
        t.begin_epoch(1)
        while t.has_next_batch():
            self.augment_batch()
            t.vote(step(t.batch, t.label))
            t.finish_batch()
        self.reset()  # T:264
        return t.accuracy()

    # ---- results: the tester's one readback per epoch
    def accuracy(self):
        """T:263"""
        return self.tester.accuracy()

    def totals(self):
        """-> dict(total_correct, total_seen, total_object, seen_class, correct_class); total_object counts B per batch"""
        return self.tester.totals()

    def mean_loss(self, reg_loss=0.0):
        """T:262: loss_sum / num_batch with num_batch = int(S / B), the floored count (T:220) although ceil(S / B) batches
        added to the sum; reg_loss is what the model's regularisation adds to every batch's loss"""
        num_batch = int(self.S / self.B)
        if num_batch < 1:
            raise ValueError(f"{self.S} shapes < batch_size = {self.B}: the reference divides by int(S / B) = 0")
        r = self.tester._read()
        return (r["loss_sum"] + float(reg_loss) * self.tester.batches_done) / num_batch

    def predictions(self):
        """np.argmax(pred_val, 1) of every shape, (S,) i32 device tensor in the epoch's visiting order"""
        return self.tester.preds

    def report(self, learning_rate, reg_loss=0.0):
        """the lines T:261-263 log"""
        return ["Current Learning Rate %.6f" % learning_rate, "Training loss: %f" % self.mean_loss(reg_loss),
                "Training accuracy: %f\n" % self.accuracy()]
