"""What ScanNet's and SemanticKITTI's training input loops share on the host (ScanNet/block_trainer.py,
SemanticKITTI/block_trainer.py): both references' `train_one_epoch` are the same code round a different transform; the line
numbers in the docstrings below are given by the two classes' own docstrings.

A class built on `BlockTrainLoop` is composed over a `BlockLoop` tester -- its scenes, bounds, buffers, label weights and
RNG are the tester's; the training counters and the loss sum are its own, so a validation epoch of the tester between two
training epochs disturbs neither -- and supplies

  _gather_into                 the tester's buffer the B items of a batch are gathered into
  _transform(angles) -> data   the dataset's transform of that buffer, (B,P,width) f32 on the device
"""
import numpy as np
import torch

from pointasnl_amd import _hip

_p = _hip.ptr


class BlockTrainLoop:
    ACCURACY_LINE = "Training accuracy: %f"

    def _compose(self, tester):
        self.tester = t = tester
        self.S, self.C, self.P, self.B, self.width, self.device = t.S, t.C, t.P, t.B, t.width, t.device
        self.counters = torch.zeros((3,), dtype=torch.int64, device=t.device)  # total_correct, total_seen, total_iou_deno
        self.loss = torch.zeros((2,), dtype=torch.float64, device=t.device)
        self.reset()

    @property
    def rng(self):
        return self.tester.rng

    def reset(self):
        """clears the counters and the loss (an epoch starts with it)"""
        self.counters.zero_()
        self.loss.zero_()
        self.forwards, self.num_batches, self.order, self._final = 0, 0, None, None

    def score(self, logits, seg, smpw):
        """the three tallies and the loss for one batch of B rows: logits (B,P,C) f32 from the step"""
        v = _hip.as_dev(logits, torch.float32)
        if v.numel() != self.B * self.P * self.C or v.shape[-1] != self.C:
            raise ValueError(f"the step must return ({self.B}, {self.P}, {self.C}) logits")
        _hip.launch("pasnl_block_train_score", type(self).__name__ + " score", self.B, self.P, self.C, _p(v), _p(seg), _p(smpw),
                    _p(self.counters), _p(self.loss), _p(self.tester.workspace))
        self.forwards += 1

    def run_train(self, step):
        """One `train_one_epoch` under the tester's RNG, in the reference's order of draws: the shuffle of the S indices; then
        per batch of int(S / B) -- the remainder is dropped -- B items (each its tries, then `rng.choice(m, P)`), B x
        `rng.uniform() * 2 * np.pi`, the transform, `step(data, labels, smpw) -> (B,P,C) f32 logits` (device tensors, the
        tester's persistent buffers, handed over without a copy) and the score.  No host synchronisation but the read-back
        per try that `draw_crop` needs; the counters and the loss come down once, at the end.  -> the training accuracy."""
        t = self.tester
        self.reset()
        self.order = np.arange(0, self.S)
        t.rng.shuffle(self.order)
        num_batches = int(self.S / self.B)
        for b in range(num_batches):
            for k in range(self.B):
                t._item_into(int(self.order[b * self.B + k]), self._gather_into, t.batch_label, t.batch_smpw, k)
            angles = [t.rng.uniform() * 2 * np.pi for _ in range(self.B)]
            self.score(step(self._transform(angles), t.batch_label, t.batch_smpw), t.batch_label, t.batch_smpw)
        self.num_batches = num_batches
        c = self.counters.cpu().numpy()  # the epoch's one readback
        self._final = dict(total_correct=int(c[0]), total_seen=int(c[1]), total_iou_deno=int(c[2]),
                           loss_sum=float(self.loss.cpu().numpy()[0]))
        return self.accuracy()

    # ---- results
    def totals(self):
        """-> dict(total_correct, total_seen, total_iou_deno): the int64 counters of the last epoch"""
        return {k: self._final[k] for k in ("total_correct", "total_seen", "total_iou_deno")}

    def _ratio(self, over):
        if self.num_batches < 1:
            raise ValueError(f"{self.S} items < batch_size = {self.B}: the epoch has no batch and the reference divides by zero")
        return self._final["total_correct"] / float(self._final[over])

    def accuracy(self):
        """total_correct / float(total_seen)"""
        return self._ratio("total_seen")

    def iou(self):
        """total_correct / float(total_iou_deno)"""
        return self._ratio("total_iou_deno")

    def mean_loss(self, extra=0.0):
        """loss_sum / num_batches with num_batches = int(S / B); extra is what the model's other loss terms add to every
        forward"""
        if self.num_batches < 1:
            raise ValueError(f"{self.S} items < batch_size = {self.B}: the reference divides by int(S / B) = 0")
        return (self._final["loss_sum"] + float(extra) * self.forwards) / self.num_batches

    def report(self, extra=0.0):
        """the three lines the reference logs for the last epoch"""
        return ["Training loss: %f" % self.mean_loss(extra), self.ACCURACY_LINE % self.accuracy(), "Training IoU: %f" % self.iou()]
