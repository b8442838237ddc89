"""The SemanticKITTI grid pipeline's per-epoch validation on the device -- reference
SemanticKITTI/train_semantic_kitti_grid.py (K) :265-330 (`eval_one_epoch`: int(len(val_list) / batch_size) batches of the
validation generator, one confusion matrix per crop against the batch's own labels, the IoU table) over
SemanticKITTI/semantic_kitti_dataset_grid.py:193-247 `get_batch_gen('validation')` and :294-300 `tf_map`.

`ScanEvaluator` runs `ScanTrainer`'s generator with symmetries=(False, False, False) -- the validation split's (:198-202) --
in list order; per batch

  ScanTrainer's five ABI calls   pick, crop, order, labels, augment (no symmetry)
  model(points) -> (B,P,C) f32 logits                                                     the caller's forward
  pasnl_scan_eval_confusion      argmax of softmax(logits[..., 1:]) with the ignored column inserted, the per-crop confusions
                                 against the batch's labels, summed                       K:268, 301-308

with no host synchronisation; the (nl,nl) matrix comes down once per epoch and K:310-319 run in numpy on the host as
written.  label_values is arange(num_classes), as the reference's sorted `label_to_names` keys are.

Only crop_pc's k form (in_radius == 0) is covered.

Deviations: scans are arrays in memory, not files; the augmentation's generator is Philox4x32-10
(pointasnl_amd/grid_augment.py), not TF's; the softmax is computed here in float32, not by TensorFlow; nothing is written to
disk and nothing is logged -- `report` returns the lines.
"""
import numpy as np

from pointasnl_amd.SemanticKITTI.scan_trainer import ScanTrainer
from pointasnl_amd.grid_eval_loop import GridEvalLoop


class ScanEvaluator(GridEvalLoop):
    """`ScanEvaluator(scans, labels, num_classes=20, num_point=10240, num_buffer=1024, batch_size=4, ignored_labels=(0,),
    rng=np.random, seed=0, augment=True)`.

    scans: a list of (n_i,3) float32 sub-sampled scans in the order of the reference's val_list; labels: their (n_i,) integer
    class indices (the output of learning_map).  Per item the host draws `rng.choice(n_i, 1)`, `rng.randint(0, num_buffer //
    4)` and `rng.shuffle(arange(k))`, as `ScanTrainer` does.  seed: the augmentation's 64-bit key."""

    def __init__(self, scans, labels, num_classes=20, num_point=10240, num_buffer=1024, batch_size=4, ignored_labels=(0,),
                 rng=np.random, seed=0, augment=True, in_radius=0.0):
        if in_radius > 0:
            raise NotImplementedError("ScanEvaluator covers crop_pc's k form only (in_radius == 0): the radius form of the "
                                      "evaluators is future work")
        self._init_eval(num_classes, None, ignored_labels)
        if len(scans) < int(batch_size):
            raise ValueError(f"{len(scans)} scans < batch_size = {int(batch_size)}: the epoch of int(S / B) batches is empty")
        self.gen = g = ScanTrainer(scans, labels, num_classes=num_classes, num_point=num_point, num_buffer=num_buffer,
                                   batch_size=batch_size, symmetries=(False, False, False), rng=rng, seed=seed, augment=augment)
        self.S, self.B, self.P, self.device = g.S, g.B, g.P, g.device
        self._init_confusion()
        self.mIoU, self.IoUs = None, None

    @property
    def steps_per_epoch(self):
        return int(self.S / self.B)  # K:124: epoch_steps_eval

    def enqueue_batch(self, model, out=None):
        """everything one staged batch puts on the stream: the generator's chain, the forward and the confusions -- no host
        synchronisation.  -> the model's logits"""
        pts, lab, _, _, _ = self.gen.enqueue(out)
        logits = model(pts)
        self.score(logits, lab)  # K:290: the truth is the batch's own labels
        return logits

    def run(self, model):
        """One `eval_one_epoch` (K:265-330) from the head of the list: int(S / B) batches; then the single read-back and
        K:310-319 in numpy.  model: points (B,P,3) f32 -> (B,P,C) f32 logits.  -> mIoU."""
        g = self.gen
        self.reset()
        g.next_item = 0
        for _ in range(self.steps_per_epoch):
            g.stage(g.draw_batch(g.next_item))
            g.next_item += self.B
            self.enqueue_batch(model)
        C = self.drop_ignored(self.confusion().astype(np.float32))  # K:310-316
        self.IoUs = self.iou_from_confusions(C)
        self.mIoU = 100 * np.mean(self.IoUs)
        return self.mIoU

    def report(self, seg_label_to_cat):
        """the lines K:321-328 log for the last `run`"""
        return [self.class_lines(self.IoUs, seg_label_to_cat, self.C), "Eval point avg class IoU: %.3f" % (self.mIoU)]
