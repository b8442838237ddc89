"""The ScanNet grid loops in the radius form, `--in_radius R` with R > 0 -- reference ScanNet/scannet_dataset_grid.py (D)
:482-541 with `config.in_radius > 0` (D:491-492): the crop is `query_radius(pick_point, r=in_radius)[0]`, shuffled, cut to
num_point and, where the sphere holds fewer points, filled up by `data_rep` (D:533-535, 692-703).

`RadiusSceneTester` and `RadiusSceneTrainer` are `SceneTester` and `SceneTrainer` with another crop chain
(pointasnl_amd/radius_crop.py): votes, `run`, `reproject`, `confusion`, labels and weights, augmentation, tallies and `report`
are the parents'.  Per crop: the host's `rng.normal(scale=0.35, size=(1, 3))`, pasnl_scene_pick, pasnl_scene_radius_members,
ONE read-back of the count, the host's shuffle and duplicates, pasnl_scene_radius_gather, then
pasnl_scene_potential_update over the min(count, num_point) distinct members (the reference updates before data_rep,
D:512-516).  The chain synchronises with the host once per crop and cannot be captured; `draw_batch`, `stage` and `enqueue` of
the k form do not exist here.

A crop whose sphere is empty ends the epoch (D:505-508): the potentials are drawn afresh (`rng.rand(n_i) * 1e-3`, scene after
scene), `next_batch` raises `EpochEnded` and the crops of the unfinished batch are dropped.  `RadiusSceneTester.run` goes on to
the epoch's checkpoint rule and its next epoch; `RadiusSceneTrainer.run` ends there, and `mean_loss` divides by the batches
done (train_scannet_grid.py:294-300).

Deviations, beside the parents': `tree_orders=None` lists a sphere's members by ascending index where sklearn lists them in
its tree's order, so the crops are self-consistent but not a reference run's; hand over `np.asarray(tree.idx_array)` of every
scene's tree (the reference pickles the trees; their leaf_size is 50) for the reference's crops.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.ScanNet.scene_tester import DESC_BYTES, SceneTester
from pointasnl_amd.ScanNet.scene_trainer import SceneTrainer
from pointasnl_amd.radius_crop import EpochEnded, RadiusChain, draw_perm

_p = _hip.ptr


class RadiusSceneCrops(RadiusChain):
    """`SceneCrops`' generator with the radius crop: what the two classes below share."""

    MEMBERS = "pasnl_scene_radius_members"

    def _init_radius(self, in_radius, tree_orders):
        RadiusChain._init_radius(self, in_radius, tree_orders)
        self.noise_host = torch.zeros((3,), dtype=torch.float64).pin_memory()

    def reset_potentials(self):
        """D:472-478: `rng.rand(n_i) * 1e-3` scene after scene, and their minima"""
        pots = [self.rng.rand(n) * 1e-3 for n in self.sizes]
        self.potentials.copy_(torch.from_numpy(np.concatenate(pots)))
        self.min_pots.copy_(torch.tensor([float(np.min(p)) for p in pots], dtype=torch.float64))

    def _crop(self, b, inputs, inds, clouds):
        """crop b of the batch (D:484-541); raises EpochEnded when the sphere is empty"""
        npt = self.num_point
        desc = _p(self.desc, b * DESC_BYTES)
        sel = _p(inds, b * npt * 4)
        self.noise_host.copy_(torch.from_numpy(self.rng.normal(scale=0.35, size=(1, 3))[0]))
        self.noise_stage[b].copy_(self.noise_host, non_blocking=True)
        _hip.launch("pasnl_scene_pick", "radius pick", self.S, _p(self.offsets), _p(self.potentials), _p(self.min_pots), _p(self.points),
                    _p(self.k_stage, b * 4), _p(self.noise_stage, b * 24), desc, _p(clouds, b * 4))
        self._members(desc)
        count = self.read_count()
        if count == 0:  # (the shuffle of an empty list draws nothing)
            self.reset_potentials()
            raise EpochEnded()
        self._stage_perm(b, draw_perm(self.rng, count, npt))
        _hip.launch("pasnl_scene_radius_gather", "radius gather", 1, desc, _p(self.points), _p(self.colors), self.F, _p(self.members),
                    ctypes.c_long(self.nmax), _p(self.count), _p(self.perm_stage, b * npt * 4), npt, 1 if self.abs_coords else 0, sel,
                    _p(inputs, b * npt * self.width * 4))
        _hip.launch("pasnl_scene_potential_update", "radius update", min(count, npt), desc, _p(self.points), sel, _p(self.potentials),
                    _p(self.min_pots), _p(self.win))

    def _crops(self):
        B, npt = self.B, self.num_point
        inputs = torch.empty((B, npt, self.width), dtype=torch.float32, device=self.device)
        inds = torch.empty((B, npt), dtype=torch.int32, device=self.device)
        clouds = torch.empty((B,), dtype=torch.int32, device=self.device)
        for b in range(B):
            self._crop(b, inputs, inds, clouds)
        return inputs, inds, clouds

    def next_batch(self):
        """B crops (D:482-541) -> (inputs, point_inds, cloud_inds) device tensors; B read-backs.  Raises `EpochEnded`."""
        return self._crops()


class RadiusSceneTester(RadiusSceneCrops, SceneTester):
    """`RadiusSceneTester(scenes, colors=colors, in_radius=2.0, tree_orders=orders, ...)`: `SceneTester`'s arguments without
    num_buffer (unused in this form, D:33), with in_radius > 0 and tree_orders -- one `np.asarray(tree.idx_array)` per scene,
    a permutation of arange(n_i) (None: ascending index, see the module's deviations).  Scenes of any size."""

    def __init__(self, scenes, colors=None, num_classes=21, num_point=8192, batch_size=4, split="test", validation_size=500,
                 label_values=None, ignored_labels=(0,), with_rgb=True, rng=np.random, abs_coords=False, test_smooth=None, *,
                 in_radius, tree_orders=None):
        if not float(in_radius) > 0:
            raise ValueError("in_radius must be > 0 (the k form is SceneTester)")
        self._init_tester(scenes, colors, num_classes, num_point, 0, batch_size, split, validation_size, label_values, ignored_labels,
                          with_rgb, rng, abs_coords, test_smooth, k_form=False)
        self._init_radius(in_radius, tree_orders)

    def _epoch(self, forward):
        """one epoch of the generator: validation_size batches, or fewer when a sphere is empty (D:505-508)"""
        try:
            SceneTester._epoch(self, forward)
        except EpochEnded:
            pass


class RadiusSceneTrainer(RadiusSceneCrops, SceneTrainer):
    """`RadiusSceneTrainer(scenes, labels, colors=colors, in_radius=2.0, tree_orders=orders, ...)`: `SceneTrainer`'s arguments
    without num_buffer, with in_radius > 0 and tree_orders as for `RadiusSceneTester`."""

    def __init__(self, scenes, labels, colors=None, num_classes=21, num_point=8192, batch_size=4, epoch_steps=1200, label_values=None,
                 label_weights=None, with_rgb=True, rng=np.random, seed=0, augment=True, augment_config=None, *, in_radius,
                 tree_orders=None):
        if not float(in_radius) > 0:
            raise ValueError("in_radius must be > 0 (the k form is SceneTrainer)")
        self._init_trainer(scenes, labels, colors, num_classes, num_point, 0, batch_size, epoch_steps, label_values, label_weights,
                           with_rgb, rng, seed, augment, augment_config, k_form=False)
        self._init_radius(in_radius, tree_orders)

    def next_batch(self):
        """B crops, their labels and weights (data_rep's duplicates included, D:699-702) and the augmentation ->
        (inputs, labels, weights, point_inds, cloud_inds) device tensors.  Raises `EpochEnded`."""
        inputs, inds, clouds = self._crops()
        if self.augment:
            self._stage_item()
        lab = torch.empty((self.B, self.P), dtype=torch.int32, device=self.device)
        wts = torch.empty((self.B, self.P), dtype=torch.float32, device=self.device)
        self._gather_labels(inds, clouds, lab, wts)
        if self.augment:
            self._augment(inputs)
        return inputs, lab, wts, inds, clouds

    def run(self, step):
        """One `train_one_epoch` (train_scannet_grid.py:264-302): epoch_steps batches, or those before a sphere is empty; the
        results are over the batches done.  -> total_correct / float(total_seen)."""
        self.reset()
        done = 0
        for _ in range(self.steps_per_epoch):
            try:
                x, y, w, _, _ = self.next_batch()
            except EpochEnded:
                break
            self.score(step(x, y, w), y, w)
            done += 1
        return self._end_epoch(done)
