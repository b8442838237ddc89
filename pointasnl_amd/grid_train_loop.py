"""What the two grid training input loops share on the host (ScanNet/scene_trainer.py, SemanticKITTI/scan_trainer.py):
`train_one_epoch` of ScanNet/train_scannet_grid.py:264-302 and SemanticKITTI/train_semantic_kitti_grid.py:224-263 is the
same code -- per batch the step, np.argmax, the three tallies and the loss; three log lines at the end -- and the tallies
are line for line those of train_scannet.py, so they are `pasnl_block_train_score` and the result methods are
`BlockTrainLoop`'s.

A class built on `GridTrainLoop` supplies B, P (= num_point), C, device, `steps_per_epoch` and
`next_batch() -> (inputs, labels, weights, point_inds, cloud_inds)`.
"""
import numpy as np
import torch

from pointasnl_amd import _hip, grid_augment
from pointasnl_amd.block_train_loop import BlockTrainLoop

_p = _hip.ptr


class GridTrainLoop(BlockTrainLoop):
    rng = None  # the subclass's own RandomState (BlockTrainLoop reads its tester's)

    def _init_tally(self):
        self.counters = torch.zeros((3,), dtype=torch.int64, device=self.device)  # total_correct, total_seen, total_iou_deno
        self.loss = torch.zeros((2,), dtype=torch.float64, device=self.device)
        nbytes = int(_hip.lib().pasnl_block_score_workspace_bytes())
        self.workspace = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device)
        self.reset()

    def _init_augment(self, augment, config, seed):
        """the augmentation's state: its config, the seed, and the running crop number on the host and staged on the device"""
        self.augment, self.seed = bool(augment), int(seed)
        self.augment_config = grid_augment.config_of(config)
        self.item = 0  # crops augmented so far: crop c of a batch draws under (seed, item + c)
        self.item_stage = torch.zeros((1,), dtype=torch.int64, device=self.device)

    def _stage_item(self):
        """the running number of the batch's first crop goes up to the device like the other draws (asynchronous, from
        pinned memory), so a captured chain replays with fresh numbers"""
        self.item_stage.copy_(torch.tensor([self.item], dtype=torch.int64).pin_memory(), non_blocking=True)
        self.item += self.B

    def _augment(self, inputs):
        """tf_map (D:554-571, K:296-300) of one batch, in place, under the staged crop number"""
        grid_augment.launch(self.B, self.P, int(inputs.shape[2]), inputs, inputs, self.augment_config, self.seed, self.item_stage,
                            what=type(self).__name__ + " augment")

    def _gather_labels(self, inds, clouds, labels_out, weights_out):
        _hip.launch("pasnl_scan_train_labels", type(self).__name__ + " labels", self.B, self.P, _p(inds), _p(clouds), _p(self.offsets),
                    _p(self.labels), _p(self.label_weights), int(self.label_weights.shape[0]), _p(labels_out), _p(weights_out))

    def score(self, logits, labels, weights):
        """the three tallies and the loss for one batch: logits (B,P,C) f32 from the step"""
        v = _hip.as_dev(logits, torch.float32)
        if v.numel() != self.B * self.P * self.C or v.shape[-1] != self.C:
            raise ValueError(f"the step must return ({self.B}, {self.P}, {self.C}) logits")
        _hip.launch("pasnl_block_train_score", type(self).__name__ + " score", self.B, self.P, self.C, _p(v), _p(labels), _p(weights),
                    _p(self.counters), _p(self.loss), _p(self.workspace))
        self.forwards += 1

    def run(self, step):
        """One `train_one_epoch`: `steps_per_epoch` batches, each `next_batch()`, `step(inputs, labels, weights) -> (B,P,C) f32
        logits` (device tensors) and the score; no host synchronisation inside, the counters and the loss come down once, at
        the end.  -> total_correct / float(total_seen)."""
        self.reset()
        for _ in range(self.steps_per_epoch):
            x, y, w, _, _ = self.next_batch()
            self.score(step(x, y, w), y, w)
        return self._end_epoch(self.steps_per_epoch)

    def _end_epoch(self, num_batches):
        """the epoch's results after `num_batches` scored batches -> total_correct / float(total_seen)"""
        self.num_batches = num_batches
        c = self.counters.cpu().numpy()  # the epoch's one readback
        self._final = dict(total_correct=int(c[0]), total_seen=int(c[1]), total_iou_deno=int(c[2]),
                           loss_sum=float(self.loss.cpu().numpy()[0]))
        return self.accuracy()

    def report(self, extra=0.0):
        """the three lines both grid scripts log for the last epoch (loss_sum / num_steps; the ratios times 100)"""
        return ["Training Loss: %f" % self.mean_loss(extra), "Training Accuracy: %f" % (self.accuracy() * 100),
                "Training IoU: %f" % (self.iou() * 100)]


def flat_labels(labels, sizes, what):
    """one (n_i,) integer label array per cloud -> the flat (N,) int64 host array beside the flat points"""
    if labels is None or len(labels) != len(sizes):
        raise ValueError(f"one label array per {what}")
    out = []
    for i, (lab, n) in enumerate(zip(labels, sizes)):
        a = lab.cpu().numpy() if isinstance(lab, torch.Tensor) else np.asarray(lab)
        a = a.reshape(-1)
        if a.shape[0] != n or a.dtype.kind not in "iu":
            raise ValueError(f"labels[{i}] must hold {n} integers, one per point of {what} {i}")
        out.append(a.astype(np.int64))
    return np.concatenate(out)

