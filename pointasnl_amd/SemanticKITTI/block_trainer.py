"""SemanticKITTI's training input loop on the device -- reference SemanticKITTI/train_semantic_kitti.py (T) :223-264
(`train_one_epoch`) round `SemanticKittiDataset.__getitem__` (SemanticKITTI/semantic_kitti_dataset.py (D) :68-109) with
utils/provider.py (P) :71-89.  It is the loop that trains `pointasnl_sem_seg` on lidar scans, and the one the validation
loops of block_tester.py belong to.

`KittiBlockTrainer` is composed over a `KittiBlockTester` (the scans on the device, their bounds, the persistent batch, the
weight table, `reference_quirks`, the remission column and the RNG are the tester's).  One epoch:

  host rng.shuffle(arange(S))                                      T:228-229; the validation loops go in index order
  per item:  the tester's chopped item (tries, rng.choice(m, P), pasnl_kblock_fill, pasnl_kblock_gather)
  per batch: host B x rng.uniform() -> pasnl_kblock_rotate         T:244, in place; there is no normalize_data
             step(data, labels, smpw) -> (B,P,C) f32 logits        the caller's forward, backward and update
             pasnl_block_train_score                               T:253-261

The tallies are not the validation ones: every entry counts, with no smpw > 0 and no label > 0; total_seen grows by B * P
per batch; total_iou_deno is one number, 1 per entry whose prediction and label agree and 2 per entry where they differ.

Deviations: scans are arrays in memory, not files; nothing is written (no log file, no TensorBoard summary) -- `report`
returns the lines, 'Trainingaccuracy: %f' without its space as T:263 has it; the classify loss is pasnl_block_score's (a
float32 log-sum-exp per entry, float64 sums in a fixed order), not TensorFlow's `loss_val`, and is compared under a
tolerance, never by bits; the model's other loss terms enter `mean_loss(extra)` as a number.  z is carried through the
rotation: numpy's x*0 + y*0 + z*1 is z for finite input up to the sign of a zero.  The rotated x and y are x*cos + y*(-sin)
and x*sin + y*cos in float64, rounded to float32; numpy's dgemm fixes no summation order, so a rotated coordinate may differ
from the reference's by one float32 ulp (measured on the recorded epoch: none does, see
tests/golden/make_block_train_flow.py).  An epoch with fewer scans than a batch has no batch: the reference divides by zero
in its log lines, here the results raise ValueError.
"""
from pointasnl_amd.SemanticKITTI.block_tester import KittiBlockTester
from pointasnl_amd.block_train_loop import BlockTrainLoop


class KittiBlockTrainer(BlockTrainLoop):
    """`KittiBlockTrainer(scans, labels, remissions=None, num_classes=20, block_points=8192, batch_size=8, block_size=10,
    padding=0.01, label_weights_lut=None, reference_quirks=True, rng=np.random)`, the arguments of `KittiBlockTester`; or
    `KittiBlockTrainer(tester=a_kitti_block_tester)` over an existing one."""

    ACCURACY_LINE = "Trainingaccuracy: %f"  # T:263

    def __init__(self, scans=None, labels=None, tester=None, **kwargs):
        if tester is None:
            tester = KittiBlockTester(scans, labels, **kwargs)
        elif scans is not None or labels is not None or kwargs:
            raise ValueError("either the tester's arguments or tester=")
        self._compose(tester)

    @property
    def _gather_into(self):
        return self.tester.batch

    def _transform(self, angles):
        return self.rotate(self.tester.batch, angles)

    def rotate(self, raw, angles):
        """T:244 alone: rotate_point_cloud_z with the given angles of raw (B,P,3|4) f32, in place (the tester's `rotate`).
        -> raw"""
        return self.tester.rotate(raw, self.B, angles)

    train_batch = rotate  # the transform alone, under the name ScanNet's trainer gives it

    def run(self, step):
        """T:223-264, one epoch.  step: ((B,P,3|4) f32, (B,P) i32 labels, (B,P) f32 smpw) device tensors -> (B,P,C) f32
        logits, called once per batch.  -> total_correct / float(total_seen)."""
        return self.run_train(step)
