"""The ScanNet grid training input loop on the device -- reference ScanNet/scannet_dataset_grid.py (D) :435-549
(`get_batch_gen('training')`: potentials, the noisy pick, the crop, the potential update, labels through `label_to_idx`, the
sample weights), :551-645 (`tf_map`: `tf_augment_input` and the colour drop) and ScanNet/train_scannet_grid.py (T) :264-302
(`train_one_epoch`).

`SceneTrainer` is `SceneTester`'s generator (scene_tester.SceneCrops: the same kernels, the same host draws in the same
order -- `rng.rand(n_i) * 1e-3` per scene at construction, then per crop `rng.normal(scale=0.35, size=(1, 3))`,
`rng.randint(0, num_buffer // 4)` and `rng.shuffle` of the k indices) with what the training split adds.  One batch:

  B x (pasnl_scene_pick_crop -> pasnl_scene_order_gather -> pasnl_scene_potential_update)     D:484-520
  pasnl_scan_train_labels      labels[select] and label_weights[labels]                        D:525-531
  pasnl_scan_augment           rotation, scale, symmetry, noise, colour drop, in place         D:561-568
  step(inputs, labels, weights) -> (B,P,C) f32 logits                                          the caller's update
  pasnl_block_train_score      the three tallies and the loss                                  T:285-293

with no host synchronisation; the counters come down once per epoch.  The potentials persist across epochs, as the
reference's do (reset_potentials runs when the generator is built, not when it is restarted).

Only the k form (in_radius == 0) is covered here (the radius form: scene_radius.RadiusSceneTrainer) and every scene must
hold at least num_point + num_buffer + num_buffer // 4 - 1 points, as for `SceneTester`.  There is no abs_coords option: `tf_map` keeps the colour columns only (D:562).

Deviations: the augmentation's generator is Philox4x32-10 (pointasnl_amd/grid_augment.py lays out every draw), not TF's, and
the summation order of TF's matmul is not promised; the classify loss is pasnl_block_score's and is compared under a
tolerance, never by bits; the model's other loss terms enter `mean_loss(extra)` as a number; nothing is written (no log
file, no summary) -- `report` returns the lines.
"""
import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.ScanNet.scene_tester import SceneCrops
from pointasnl_amd.grid_train_loop import GridTrainLoop, flat_labels


class SceneTrainer(SceneCrops, GridTrainLoop):
    """`SceneTrainer(scenes, labels, colors=None, num_classes=21, num_point=8192, num_buffer=1024, batch_size=4,
    epoch_steps=1200, label_values=np.arange(21), label_weights=..., with_rgb=True, rng=np.random, seed=0, augment=True)`.

    scenes, colors: as for `SceneTester`, in the order of input_trees['training']; labels: one (n_i,) integer array per scene
    holding values of label_values, mapped to class indices once, here (D:526); label_weights: (num_classes,) the reference's
    `self.label_weights` (default: ones); epoch_steps: T:59's epoch_sample // batch_size = 4800 // 4.  seed: the
    augmentation's 64-bit key; crop number i of this trainer's life draws under (seed, i).  augment_config: a dict or object
    with the reference's augment_* fields (default: D:443-451)."""

    def __init__(self, scenes, labels, colors=None, num_classes=21, num_point=8192, num_buffer=1024, batch_size=4, epoch_steps=1200,
                 label_values=None, label_weights=None, with_rgb=True, rng=np.random, seed=0, augment=True, in_radius=0.0,
                 augment_config=None):
        if in_radius > 0:
            raise NotImplementedError("SceneTrainer covers the k form only (in_radius == 0): the radius form is "
                                      "pointasnl_amd.ScanNet.scene_radius.RadiusSceneTrainer")
        self._init_trainer(scenes, labels, colors, num_classes, num_point, num_buffer, batch_size, epoch_steps, label_values,
                           label_weights, with_rgb, rng, seed, augment, augment_config)

    def _init_trainer(self, scenes, labels, colors, num_classes, num_point, num_buffer, batch_size, epoch_steps, label_values,
                      label_weights, with_rgb, rng, seed, augment, augment_config, k_form=True):
        _hip.require_device()
        self.C, self.epoch_steps = int(num_classes), int(epoch_steps)
        self.label_values = np.arange(self.C, dtype=np.int64) if label_values is None else np.asarray(label_values, np.int64).reshape(-1)
        if len(set(self.label_values.tolist())) != self.label_values.size:
            raise ValueError("label_values must be distinct")
        w = np.ones((self.C,), np.float32) if label_weights is None else np.asarray(label_weights).reshape(-1)
        host = flat_labels(labels, [len(s) for s in scenes], "scene")
        order = np.argsort(self.label_values, kind="stable")
        pos = np.minimum(np.searchsorted(self.label_values[order], host), self.label_values.size - 1)
        if host.size and not (self.label_values[order][pos] == host).all():
            bad = host[self.label_values[order][pos] != host][0]
            raise KeyError(f"label {int(bad)} is not in label_values (label_to_idx, D:526)")
        idx = order[pos]
        if idx.size and int(idx.max()) >= min(w.size, self.C):
            raise IndexError(f"class index {int(idx.max())} is out of bounds for {w.size} label weights and {self.C} classes (D:531)")
        self._init_crops(scenes, colors, num_point, num_buffer, batch_size, epoch_steps, with_rgb, rng, False, k_form)
        self.P = self.num_point
        self.labels = torch.from_numpy(idx.astype(np.int32)).to(self.device)
        self.label_weights = torch.from_numpy(w.astype(np.float32)).to(self.device)
        self._init_augment(augment, augment_config, seed)
        self._init_tally()

    @property
    def steps_per_epoch(self):
        return self.epoch_steps  # D:456: epoch_n = epoch_steps * batch_size crops

    def stage(self, draws):
        """Copy one batch's draws, and the running crop number of the augmentation, into the device buffers the chain reads."""
        SceneCrops.stage(self, draws)
        if self.augment:
            self._stage_item()

    def enqueue(self, out=None):
        """The device chain of the staged batch: `SceneTester`'s, the label gather and the augmentation (augment=True: the xyz
        columns are augmented and the colours multiplied by keep, in place), on the current stream, no host synchronisation,
        capturable.  -> inputs (B,P,3+F) f32, labels (B,P) i32, weights (B,P) f32, point_inds (B,P) i32, cloud_inds (B,) i32.
        `next_batch()` is draw, stage and enqueue (D:482-541 and tf_map for B crops)."""
        inputs, inds, clouds = SceneCrops.enqueue(self, None if out is None else (out[0], out[3], out[4]))
        lab = torch.empty((self.B, self.P), dtype=torch.int32, device=self.device) if out is None else out[1]
        wts = torch.empty((self.B, self.P), dtype=torch.float32, device=self.device) if out is None else out[2]
        self._gather_labels(inds, clouds, lab, wts)
        if self.augment:
            self._augment(inputs)
        return inputs, lab, wts, inds, clouds
