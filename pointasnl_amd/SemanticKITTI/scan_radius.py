"""The SemanticKITTI grid loops in the radius form, `in_radius > 0` -- reference
SemanticKITTI/semantic_kitti_dataset_grid.py (K) :212-241 with `crop_pc`'s radius branch (K:268-269): the crop is
`search_tree.query_radius(center_point, r=in_radius)[0]`, shuffled, cut to num_point and, where the sphere holds fewer
points, filled up with `np.random.choice(num_in, num_point - num_in)` duplicates (K:277-281).

`RadiusScanTester` and `RadiusScanTrainer` are `ScanTester` and `ScanTrainer` with another crop chain
(pointasnl_amd/radius_crop.py): votes, `run`, `reproject`, labels and weights, augmentation, tallies and `report` are the
parents'.  Per crop: the pick (pasnl_scan_pick; the trainer's `rng.choice(n_i, 1)` through pasnl_scan_pick_given),
pasnl_scan_radius_members, ONE read-back of the count, the host's shuffle and duplicates, pasnl_scan_radius_gather, and for
the test split pasnl_scan_possibility_update over all num_point entries, duplicates included (K:231-234: numpy's fancy-index
`+=` lets the last occurrence win, and so does the kernel).  The chain synchronises with the host once per crop and cannot be
captured; `draw_batch`, `stage` and `enqueue` of the k form do not exist here.

A sphere that holds the centre alone (count == 1) is followed as the reference goes: every distance is 0, `dists /
np.max(dists)` is 0/0 and the point's possibility becomes NaN; numpy's argmin then picks that scan and that point for every
later crop.  The update and pick kernels follow numpy's NaN rule, so the loop degenerates exactly as the reference's does
(at r = 3 on scans of a few hundred points this is the common case); choose a radius that holds more than one point.

Deviations, beside the parents': `tree_orders=None` lists a sphere's members by ascending index where sklearn lists them in
its tree's order, so the crops are self-consistent but not a reference run's; hand over `np.asarray(tree.idx_array)` of every
scan's pickled tree for the reference's crops.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.SemanticKITTI.scan_tester import DESC_BYTES, ScanTester
from pointasnl_amd.SemanticKITTI.scan_trainer import ScanTrainer
from pointasnl_amd.radius_crop import RadiusChain, draw_perm

_p = _hip.ptr


class RadiusScanChain(RadiusChain):
    """the part of a crop the two classes below share: members, the read-back, the draws and the gather"""

    MEMBERS = "pasnl_scan_radius_members"

    def _crop_rest(self, b, pts, inds):
        npt = self.num_point
        desc = _p(self.desc, b * DESC_BYTES)
        self._members(desc)
        count = self.read_count()
        if count < 1:  # (only a NaN centre: the reference's np.random.choice(0, num_point) raises too)
            raise ValueError("a crop's sphere is empty: its centre has a NaN coordinate")
        self._stage_perm(b, draw_perm(self.rng, count, npt))
        _hip.launch("pasnl_scan_radius_gather", "radius gather", 1, desc, _p(self.points), _p(self.members), ctypes.c_long(self.nmax),
                    _p(self.count), _p(self.perm_stage, b * npt * 4), npt, _p(inds, b * npt * 4), _p(pts, b * npt * 12))


class RadiusScanTester(RadiusScanChain, ScanTester):
    """`RadiusScanTester(scans, in_radius=10.0, tree_orders=orders, ...)`: `ScanTester`'s arguments without num_buffer (unused
    in this form, K:30), with in_radius > 0 and tree_orders -- one `np.asarray(tree.idx_array)` per scan, a permutation of
    arange(n_i) (None: ascending index, see the module's deviations).  Scans of any size.  A sphere that holds one point
    makes that point's possibility NaN and the loop picks it for ever after, as the reference does (see the module)."""

    def __init__(self, scans, num_classes=20, num_point=10240, batch_size=8, test_smooth=0.98, rng=np.random, *, in_radius,
                 tree_orders=None):
        if not float(in_radius) > 0:
            raise ValueError("in_radius must be > 0 (the k form is ScanTester)")
        self._init_scans(scans, num_classes, num_point, 0, batch_size, test_smooth, rng, k_form=False)
        self._init_radius(in_radius, tree_orders)

    def next_batch(self):
        """B crops (K:224-241) -> (points, point_inds, cloud_inds) device tensors; B read-backs."""
        B, npt = self.B, self.num_point
        pts = torch.empty((B, npt, 3), dtype=torch.float32, device=self.device)
        inds = torch.empty((B, npt), dtype=torch.int32, device=self.device)
        clouds = torch.empty((B,), dtype=torch.int32, device=self.device)
        for b in range(B):
            desc = _p(self.desc, b * DESC_BYTES)
            _hip.launch("pasnl_scan_pick", "radius pick", self.S, _p(self.offsets), _p(self.possibility), _p(self.min_poss),
                        _p(self.points), _p(self.k_stage, b * 4), desc, _p(clouds, b * 4))
            self._crop_rest(b, pts, inds)
            _hip.launch("pasnl_scan_possibility_update", "radius update", npt, desc, _p(self.points), _p(inds, b * npt * 4),
                        _p(self.possibility), _p(self.min_poss), _p(self.win), _p(self.scratch))
        return pts, inds, clouds


class RadiusScanTrainer(RadiusScanChain, ScanTrainer):
    """`RadiusScanTrainer(scans, labels, in_radius=10.0, tree_orders=orders, ...)`: `ScanTrainer`'s arguments without
    num_buffer, with in_radius > 0 and tree_orders as for `RadiusScanTester`.  Per item the host draws `rng.choice(n_i, 1)`
    (K:220), then, once the count is back, the shuffle and the duplicates (K:274-281)."""

    def __init__(self, scans, labels, num_classes=20, num_point=10240, batch_size=4, label_weights=None, symmetries=(True, False, False),
                 rng=np.random, seed=0, augment=True, augment_config=None, *, in_radius, tree_orders=None):
        if not float(in_radius) > 0:
            raise ValueError("in_radius must be > 0 (the k form is ScanTrainer)")
        self._init_scans(scans, labels, num_classes, num_point, 0, batch_size, label_weights, symmetries, rng, seed, augment,
                         augment_config, k_form=False)
        self._init_radius(in_radius, tree_orders)
        self.pick_host = torch.zeros((1,), dtype=torch.int32).pin_memory()

    def next_batch(self):
        """The next B items of the list (K:214-241 and tf_map), as `ScanTrainer.next_batch` walks it -> (points, labels,
        weights, point_inds, cloud_inds) device tensors; B read-backs."""
        if self.steps_per_epoch < 1:
            raise ValueError(f"{self.S} scans < batch_size = {self.B}: the epoch of int(S / B) * B items is empty")
        if self.next_item + self.B > self.steps_per_epoch * self.B:
            self.next_item = 0
        B, npt = self.B, self.num_point
        self.clouds_host = np.arange(self.next_item, self.next_item + B, dtype=np.int32)
        self.next_item += B
        pts = torch.empty((B, npt, 3), dtype=torch.float32, device=self.device)
        inds = torch.empty((B, npt), dtype=torch.int32, device=self.device)
        for b in range(B):
            cloud = self.clouds_host[b:b + 1]
            self.pick_host[0] = int(self.rng.choice(self.sizes[int(cloud[0])], 1)[0])
            self.pick_stage[b:b + 1].copy_(self.pick_host, non_blocking=True)
            _hip.launch("pasnl_scan_pick_given", "radius pick", 1, self.S, _p(self.offsets), _p(self.points),
                        cloud.ctypes.data_as(ctypes.c_void_p), _p(self.pick_stage, b * 4), _p(self.k_stage, b * 4),
                        _p(self.desc, b * DESC_BYTES))
            self._crop_rest(b, pts, inds)
        clouds = torch.from_numpy(self.clouds_host).to(self.device)
        if self.augment:
            self._stage_item()
        lab = torch.empty((B, npt), dtype=torch.int32, device=self.device)
        wts = torch.empty((B, npt), dtype=torch.float32, device=self.device)
        self._gather_labels(inds, clouds, lab, wts)
        if self.augment:
            self._augment(pts)
        return pts, lab, wts, inds, clouds
