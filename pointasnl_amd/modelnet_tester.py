"""The ModelNet40 classification evaluation loop on the device -- reference modelnet_dataset.py (D) :9-136 (`pc_normalize`,
`farthest_point_sample`, `ModelNetDataset._get_item` / `next_batch`), test.py (T) :93-174 (`evaluate`'s robustness table and
`eval_one_epoch`) and utils/provider.py (P) :8-24 (`normalize_data`).  It is the loop that evaluates `pointasnl_cls`.

`ModelNetTester` keeps every raw shape in one flat float32 device buffer and the prepared (S, num_point, 3|6) set beside it.
One batch runs on the current stream with no host synchronisation (csrc/modelnet_test.hip):

  [uniform, first visit of a shape: pasnl_modelnet_fps -> pasnl_modelnet_normalize]
  pasnl_modelnet_batch                       -> the persistent (B, num_point, 3|6) batch and (B,) labels
  [num_noisy_point > 0: pasnl_modelnet_noise]
  per vote: forward -> pasnl_cls_vote        -> float64 vote sums, the vote's mean cross-entropy
  pasnl_cls_tally                            -> predictions, int64 counters, sums cleared

Only RNG draws travel up (one start index per sampled shape, the noise uniforms), staged from pinned memory; the counters
come down once, at the end of the epoch.  The draws are the reference's, in its order, from the caller's numpy RNG: with
`uniform` one `randint(0, n_i)` per shape on the batch that first visits it (D draws inside `_get_item`), then
`random((bsize, K, 3))` per batch when K noisy points are asked for, then per vote a `shuffle(np.arange(num_point))` whose
result the reference never uses (T:141-142) but which moves the stream.

The rows past the last real one of an epoch's final batch are not written: they still hold the batch before it (zeros when
there is none), go through the forward and count in the loss and in `total_object`, not in the accuracy -- as in the
reference.

Deviations: the loss is computed here (a float32 log-sum-exp per row, float64 sums), not by TensorFlow, and is compared
under a tolerance, never by bits; the caller's regularisation term enters `mean_loss` as a number.  `shapes` are arrays,
not files.  A shape with fewer than `num_point` rows raises ValueError (the reference fails at the batch assignment).
Coordinates must be finite.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip

NOISE_POINT = (1, 10, 50, 100)  # T:34


_p = _hip.ptr


def fps_cap():
    """the largest raw shape pasnl_modelnet_fps samples (rows that fit a workgroup's LDS)"""
    return int(_hip.lib().pasnl_modelnet_fps_cap())


class ModelNetTester:
    """`ModelNetTester(shapes, labels, num_classes=40, num_point=1024, batch_size=16, normal_channel=True, uniform=False,
    normalize=True, rng=np.random)`.

    shapes: a list of (n_i, 6) float32 raw shapes (xyz then normal; numpy arrays or device tensors) in the order of the
    reference's `datapath`; labels: the class of each.  uniform=False takes the first num_point rows of every shape (all
    prepared here); uniform=True samples num_point rows by farthest point sampling on the first batch that visits a shape,
    drawing `rng.randint(0, n_i)` then.  rng: np.random or a RandomState."""

    def __init__(self, shapes, labels, num_classes=40, num_point=1024, batch_size=16, normal_channel=True, uniform=False,
                 normalize=True, rng=np.random):
        _hip.require_device()
        self.S, self.C, self.P, self.B = len(shapes), int(num_classes), int(num_point), int(batch_size)
        self.ch, self.uniform, self.normalize, self.rng = (6 if normal_channel else 3), bool(uniform), bool(normalize), rng
        if self.S < 1:
            raise ValueError("an empty shape list")
        if self.C < 1 or self.P < 1 or self.B < 1:
            raise ValueError("at least one class, one point per shape and one shape per batch")
        lab = (labels.cpu().numpy() if isinstance(labels, torch.Tensor) else np.asarray(labels)).reshape(-1)
        if lab.shape[0] != self.S or lab.min() < 0 or lab.max() >= self.C:
            raise ValueError(f"labels must hold {self.S} values in [0, {self.C})")
        dev = []
        for i, s in enumerate(shapes):
            t = _hip.as_dev(s, torch.float32)
            if t.dim() != 2 or t.shape[1] != 6:
                raise ValueError(f"shape {i} must be (N, 6): xyz and normal")
            if t.shape[0] < self.P:
                raise ValueError(f"shape {i} has {t.shape[0]} rows < num_point = {self.P}")
            dev.append(t)
        self.sizes = np.array([int(t.shape[0]) for t in dev], np.int64)
        if self.uniform and int(self.sizes.max()) > fps_cap():
            raise _hip.PasnlUnsupported(f"a raw shape of {int(self.sizes.max())} rows > {fps_cap()} (the LDS record of pasnl_modelnet_fps)")
        self.device = dev[0].device
        self.raw = torch.cat(dev).contiguous()
        row0 = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.total_rows = int(row0[-1])
        self.row0 = torch.from_numpy(row0[:-1].copy()).to(self.device)
        self.nraw = torch.from_numpy(self.sizes.astype(np.int32)).to(self.device)
        self.shape_labels = torch.from_numpy(lab.astype(np.int32)).to(self.device)
        self.labels_host = lab.astype(np.int32)
        if self.uniform:
            self.prepared = torch.zeros((self.S, self.P, self.ch), dtype=torch.float32, device=self.device)
            self.ready = np.zeros(self.S, bool)
        else:  # D:92: the first num_point rows
            self.prepared = torch.stack([t[:self.P, :self.ch] for t in dev]).contiguous()
            self.ready = np.ones(self.S, bool)
            if self.normalize:
                _hip.launch("pasnl_modelnet_normalize", "ModelNetTester normalize", self.S, self.P, self.ch, ctypes.c_long(self.S),
                            ctypes.c_void_p(0), _p(self.prepared))
        self.batch = torch.zeros((self.B, self.P, self.ch), dtype=torch.float32, device=self.device)
        self.label = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.sums = torch.zeros((self.B, self.C), dtype=torch.float64, device=self.device)
        self.counters = torch.zeros((3 + 2 * self.C,), dtype=torch.int64, device=self.device)
        self.loss = torch.zeros((2,), dtype=torch.float64, device=self.device)
        self.preds = torch.zeros((self.S,), dtype=torch.int32, device=self.device)
        self.ids_stage = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.start_stage = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.noise_stage = None
        self.num_batches = (self.S + self.B - 1) // self.B
        self.num_votes, self.batches_done, self.bsize, self.results = 1, 0, 0, None
        self.set_order(np.arange(self.S))

    # ---- the dataset's side
    def set_order(self, idxs):
        """D:114-119: the epoch's visiting order (`idxs`, a permutation of the shapes) and the cursor back to the first batch"""
        idxs = np.asarray(idxs).reshape(-1)
        if idxs.shape[0] != self.S or idxs.min() < 0 or idxs.max() >= self.S:
            raise ValueError(f"idxs must hold {self.S} shape numbers")
        self.idxs = idxs.astype(np.int64)
        self.order = torch.from_numpy(idxs.astype(np.int32)).to(self.device)
        self.batch_idx = 0

    def reset(self):
        self.batch_idx = 0

    def has_next_batch(self):
        return self.batch_idx < self.num_batches

    def prepare(self, ids):
        """D:79-100 for the shapes of `ids` not prepared yet, in that order: one rng.randint(0, n_i) each, then the sampling
        and pc_normalize on the device.  Nothing is drawn for a shape that is ready (the reference's cache)."""
        ids = [int(i) for i in ids if not self.ready[int(i)]]
        for at in range(0, len(ids), self.B):
            part = np.array(ids[at:at + self.B], np.int32)
            starts = np.array([self.rng.randint(0, int(self.sizes[i])) for i in part], np.int32)
            s = len(part)
            self.ids_stage[:s].copy_(torch.from_numpy(part).pin_memory(), non_blocking=True)
            self.start_stage[:s].copy_(torch.from_numpy(starts).pin_memory(), non_blocking=True)
            _hip.launch("pasnl_modelnet_fps", "ModelNetTester sampling", s, self.P, 6, ctypes.c_long(self.S), _p(self.ids_stage),
                        _p(self.row0), _p(self.nraw), _p(self.start_stage), int(self.sizes[part].min()), int(self.sizes[part].max()),
                        ctypes.c_long(self.total_rows), _p(self.raw), ctypes.c_void_p(0), _p(self.prepared), self.ch)
            if self.normalize:
                _hip.launch("pasnl_modelnet_normalize", "ModelNetTester normalize", s, self.P, self.ch, ctypes.c_long(self.S),
                            _p(self.ids_stage), _p(self.prepared))
            self.ready[part] = True

    def next_batch(self):
        """D:124-136 into the persistent buffers (T:135-136) -> (batch (B,num_point,3|6) f32, labels (B,) i32, bsize): rows
        bsize.. of both still hold what the batch before left there."""
        if not self.has_next_batch():
            raise IndexError("no batch left in this epoch: reset()")
        start = self.batch_idx * self.B
        bsize = min(self.B, self.S - start)
        if self.uniform:
            self.prepare(self.idxs[start:start + bsize])
        _hip.launch("pasnl_modelnet_batch", "ModelNetTester batch", self.B, bsize, self.P, self.ch, _p(self.order), ctypes.c_long(self.S),
                    ctypes.c_long(start), ctypes.c_long(self.S), _p(self.prepared), _p(self.shape_labels), _p(self.batch), _p(self.label))
        self.batch_idx += 1
        self.bsize, self.batch_start = bsize, start
        return self.batch, self.label, bsize

    def add_noise(self, num_noisy_point):
        """T:129-132 on the current batch: rng.random((bsize, K, 3)), normalised per block in float64 on the device, over
        rows 0..K-1 of the batch's real shapes"""
        k = int(num_noisy_point)
        if k < 1 or k > self.P:
            raise ValueError(f"num_noisy_point must be in [1, num_point = {self.P}]")
        u = self.rng.random((self.bsize, k, 3))
        if self.noise_stage is None or self.noise_stage.numel() < self.B * k * 3:
            self.noise_stage = torch.empty((self.B * k * 3,), dtype=torch.float64, device=self.device)
        self.noise_stage[:u.size].copy_(torch.from_numpy(u.reshape(-1)).pin_memory(), non_blocking=True)
        _hip.launch("pasnl_modelnet_noise", "ModelNetTester noise", self.bsize, k, _p(self.noise_stage), self.P, self.ch, _p(self.batch))

    # ---- the loop's side
    def begin_epoch(self, num_votes=1):
        """T:108-120: the buffers and counters of a new epoch"""
        if num_votes < 1:
            raise ValueError("at least one vote")
        self.num_votes, self.batches_done, self.results = int(num_votes), 0, None
        for t in (self.batch, self.label, self.sums, self.counters, self.loss, self.preds):
            t.zero_()

    def vote(self, logits):
        """T:147-149 for one vote: logits (B, C) f32, all B rows"""
        v = _hip.as_dev(logits, torch.float32)
        if tuple(v.shape) != (self.B, self.C):
            raise ValueError(f"the forward must return ({self.B}, {self.C}) logits")
        _hip.launch("pasnl_cls_vote", "ModelNetTester vote", self.B, self.C, _p(v), _p(self.label), _p(self.sums), _p(self.loss))

    def finish_batch(self):
        """T:150-162: predictions (kept at the batch's place in the epoch's order), counters, sums cleared"""
        _hip.launch("pasnl_cls_tally", "ModelNetTester tally", self.B, self.bsize, self.C, self.num_votes, _p(self.label), _p(self.sums),
                    _p(self.counters), _p(self.counters, 3 * 8), _p(self.counters, (3 + self.C) * 8), _p(self.preds, self.batch_start * 4),
                    _p(self.loss))
        self.batches_done += 1

    def run(self, forward, num_votes=1, num_noisy_point=0):
        """T:105-174, one epoch.  forward: (B,num_point,3|6) f32 device tensor -> (B,C) f32 logits, called once per vote.
        -> total_correct / float(total_seen)."""
        if num_noisy_point < 0 or num_noisy_point > self.P:
            raise ValueError(f"num_noisy_point must be in [0, num_point = {self.P}]")
        self.begin_epoch(num_votes)
        while self.has_next_batch():
            self.next_batch()
            if num_noisy_point > 0:
                self.add_noise(num_noisy_point)
            for _ in range(num_votes):
                self.rng.shuffle(np.arange(self.P))  # T:141-142: drawn, never used
                self.vote(forward(self.batch))
            self.finish_batch()
        self.reset()  # T:173
        return self.accuracy()

    def robustness(self, forward, num_votes=1, noise_points=NOISE_POINT):
        """T:93-103: the clean epoch, then one epoch per noise level -> (acc, [acc per level], the table's text)"""
        acc = self.run(forward, num_votes)
        txt = "Noise    Accuracy\n" + " 000       %.3f\n" % acc
        noise_acc = []
        for k in noise_points:
            noise_acc.append(self.run(forward, num_votes, num_noisy_point=k))
            txt += " %03d       %.3f\n" % (k, noise_acc[-1])
        return acc, noise_acc, txt

    # ---- results: one readback per epoch
    def _read(self):
        if self.results is None:
            c = self.counters.cpu().numpy()
            self.results = dict(total_correct=int(c[0]), total_seen=int(c[1]), total_object=int(c[2]), seen_class=c[3:3 + self.C].copy(),
                                correct_class=c[3 + self.C:].copy(), loss_sum=float(self.loss[0].item()))
        return self.results

    def accuracy(self):
        r = self._read()
        return r["total_correct"] / float(r["total_seen"])

    def totals(self):
        """-> dict(total_correct, total_seen, total_object, seen_class (C,) i64, correct_class (C,) i64)"""
        r = self._read()
        return {k: r[k] for k in ("total_correct", "total_seen", "total_object", "seen_class", "correct_class")}

    def class_accuracy(self):
        """T:170: correct / seen per class as numpy divides (nan for a class the split does not hold)"""
        r = self._read()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.array(r["correct_class"]) / np.array(r["seen_class"], dtype=float)

    def mean_loss(self, reg_loss=0.0):
        """T:166: loss_sum / float(total_object) -- the reference divides by objects, not batches; reg_loss is what the
        model's regularisation adds to every batch's loss"""
        r = self._read()
        return (r["loss_sum"] + float(reg_loss) * self.batches_done) / float(r["total_object"])

    def predictions(self):
        """np.argmax(batch_pred_sum, 1) of every shape, (S,) i32 device tensor in the epoch's visiting order"""
        return self.preds

    def vote_sums(self):
        """the running float64 sums (B, C) of the batch in flight (cleared by finish_batch)"""
        return self.sums

    def report(self, shape_names, reg_loss=0.0):
        """the lines T:166-172 log"""
        acc = self.class_accuracy()
        lines = ["Eval mean loss: %f" % self.mean_loss(reg_loss), "Eval accuracy: %f" % self.accuracy(),
                 "Eval avg class acc: %f" % np.mean(acc)]
        return lines + ["%10s:\t%0.3f" % (name, acc[i]) for i, name in enumerate(shape_names)]
