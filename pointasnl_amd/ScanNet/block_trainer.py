"""ScanNet's training input loop on the device -- reference ScanNet/train_scannet.py (T) :233-276 (`train_one_epoch`) round
`ScannetDataset.__getitem__` (ScanNet/scannet_dataset.py (D) :31-64) with utils/provider.py (P) :71-89 and :8-24.  It is the
loop that trains `pointasnl_sem_seg`, and the one the validation loops of block_tester.py belong to.

`BlockTrainer` is composed over a `BlockTester` (the scenes on the device, their bounds, the persistent batch, the label
weights and the RNG are the tester's; pass split='train' weights as `labelweights`).  One epoch (csrc/block_test.hip):

  host rng.shuffle(arange(S))                                      T:238-239; the validation loops go in index order
  per item:  the tester's chopped item (tries, rng.choice(m, P), pasnl_block_fill, pasnl_block_gather)
  per batch: host B x rng.uniform() -> pasnl_block_train_batch     T:253-254: rotate, ROUND TO FLOAT32, then normalize
             step(data, labels, smpw) -> (B,P,C) f32 logits        the caller's forward, backward and update
             pasnl_block_train_score                               T:264-272

The transform's order is the other way round from `eval_one_epoch` (T:301-302 normalizes the float64 batch, then rotates):
`rotate_point_cloud_z` returns float32, so here the rotated block is rounded before `normalize_data` takes its centroid and
radius, and the two orders do not give the same bits.  The tallies are not the validation ones either: every entry counts,
with no smpw > 0 and no label > 0; total_seen grows by B * P per batch; total_iou_deno is one number, 1 per entry whose
prediction and label agree and 2 per entry where they differ.

Deviations: scenes are arrays, not pickles; nothing is written (no log file, no TensorBoard summary) -- `report` returns the
lines; the classify loss is pasnl_block_score's (a float32 log-sum-exp per entry, float64 sums in a fixed order), not
TensorFlow's `loss_val`, and is compared under a tolerance, never by bits; the model's other loss terms enter
`mean_loss(extra)` as a number.  z is carried through the rotation: numpy's x*0 + y*0 + z*1 is z for finite input up to the
sign of a zero, which the centroid subtraction removes unless the centroid is exactly zero.  The rotated x and y are
x*cos + y*(-sin) and x*sin + y*cos in float64; numpy's dgemm fixes no summation order, so a rotated coordinate may differ
from the reference's by one float32 ulp, which then moves the whole normalized block (measured on the recorded epoch: none
does, see tests/golden/make_block_train_flow.py).  An epoch with fewer scenes than a batch has no batch: the reference
divides by zero in its log lines, here the results raise ValueError.
"""
import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.ScanNet.block_tester import BlockTester
from pointasnl_amd.block_train_loop import BlockTrainLoop

_p = _hip.ptr


class BlockTrainer(BlockTrainLoop):
    """`BlockTrainer(scenes, labels, colors=None, num_classes=21, block_points=8192, batch_size=8, labelweights=None,
    rng=np.random)`, the arguments of `BlockTester`; or `BlockTrainer(tester=a_block_tester)` over an existing one."""

    def __init__(self, scenes=None, labels=None, tester=None, **kwargs):
        if tester is None:
            tester = BlockTester(scenes, labels, **kwargs)
        elif scenes is not None or labels is not None or kwargs:
            raise ValueError("either the tester's arguments or tester=")
        self._compose(tester)

    @property
    def _gather_into(self):
        return self.tester.raw

    def _transform(self, angles):
        return self.train_batch(self.tester.raw, angles)

    def train_batch(self, raw, angles):
        """T:253-254 alone: rotate_point_cloud_z with the given angles, rounded to float32, then normalize_data, of raw
        (B,P,3|6) f32 into the tester's persistent batch.  -> the batch (B,P,3|6) f32"""
        t = self.tester
        src = _hip.as_dev(raw, torch.float32)
        if tuple(src.shape) != (self.B, self.P, self.width) or len(angles) != self.B:
            raise ValueError(f"raw must be ({self.B}, {self.P}, {self.width}) with one angle per block")
        rot = _hip.as_dev(np.stack([np.cos(angles), np.sin(angles)], axis=1).astype(np.float64), torch.float64)
        _hip.launch("pasnl_block_train_batch", "BlockTrainer transform", self.B, self.P, self.width, _p(src), _p(rot), _p(t.batch))
        return t.batch

    def run(self, step):
        """T:233-276, one epoch.  step: ((B,P,3|6) f32, (B,P) i32 labels, (B,P) f32 smpw) device tensors -> (B,P,C) f32
        logits, called once per batch.  -> total_correct / float(total_seen)."""
        return self.run_train(step)
