"""The SemanticKITTI grid training input loop on the device -- reference SemanticKITTI/semantic_kitti_dataset_grid.py (K)
:193-292 (`get_batch_gen('training')`: scan i of the list, a random pick, `crop_pc`, labels and `labelweights[labels]`),
:294-354 (`tf_map`: `tf_augment_input`) and train_semantic_kitti_grid.py (T) :224-263 (`train_one_epoch`).

`ScanTrainer` holds the scans and their labels in flat device buffers, in the caller's list order.  The epoch is
int(S / B) * B items (K:195): item i is scan i.  Per item the host draws, from the caller's numpy RandomState in the
reference's order, `rng.choice(n_i, 1)` (K:220), `rng.randint(0, num_buffer // 4)` (K:271) and `rng.shuffle(arange(k))`
(K:288-292); a whole batch is then five ABI calls and no read-back:

  pasnl_scan_pick_given        the B descriptors from the staged picks                         K:216-221, 267
  pasnl_knn_crop_indirect      b = B                                                           K:272
  pasnl_crop_order_permute     b = B: nearest-first order, the shuffle, the points             K:274-283
  pasnl_scan_train_labels      labels[select] and labelweights[labels]                         K:222, 284
  pasnl_scan_augment           rotation, scale, symmetry, noise, in place                      K:298

then `step(points, labels, weights) -> (B,P,C) f32 logits` and pasnl_block_train_score (T:242-250).  symmetries=(True, False,
False) is the training split; (False, False, False) gives the validation split's generator (K:198-202).

Only crop_pc's k form (in_radius == 0) is covered here (the radius form: scan_radius.RadiusScanTrainer); a scan smaller
than k raises ValueError with sklearn's message, as
`DeviceScan.query` does.

Deviations: scans are arrays in memory, not files; the augmentation's generator is Philox4x32-10
(pointasnl_amd/grid_augment.py lays out every draw), not TF's, and the summation order of TF's matmul is not promised; the
reference draws one angle, scale and symmetry per tf_map call, which is one crop (the map runs before the batching): so
does this; the classify loss is pasnl_block_score's and is compared under a tolerance, never by bits; nothing is written --
`report` returns the lines.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip, grid_augment
from pointasnl_amd.SemanticKITTI.scan_tester import DESC_BYTES, ORDER_CAP
from pointasnl_amd.grid_train_loop import GridTrainLoop, flat_labels

_p = _hip.ptr


class ScanTrainer(GridTrainLoop):
    """`ScanTrainer(scans, labels, num_classes=20, num_point=10240, num_buffer=1024, batch_size=4, label_weights=...,
    symmetries=(True, False, False), rng=np.random, seed=0, augment=True)`.

    scans: a list of (n_i,3) float32 sub-sampled scans (numpy arrays or device tensors) in the order of the reference's
    train_list; labels: their (n_i,) integer class indices (the output of learning_map); label_weights: (num_classes,) the
    reference's `self.labelweights` (default: ones).  seed: the augmentation's 64-bit key; item number i of this trainer's
    life draws under (seed, i)."""

    def __init__(self, scans, labels, num_classes=20, num_point=10240, num_buffer=1024, batch_size=4, label_weights=None,
                 symmetries=(True, False, False), rng=np.random, seed=0, augment=True, in_radius=0.0, augment_config=None):
        if in_radius > 0:
            raise NotImplementedError("ScanTrainer covers crop_pc's k form only (in_radius == 0): the radius form is "
                                      "pointasnl_amd.SemanticKITTI.scan_radius.RadiusScanTrainer")
        self._init_scans(scans, labels, num_classes, num_point, num_buffer, batch_size, label_weights, symmetries, rng, seed, augment,
                         augment_config)

    def _init_scans(self, scans, labels, num_classes, num_point, num_buffer, batch_size, label_weights, symmetries, rng, seed, augment,
                    augment_config, k_form=True):
        """the scans, labels, weights, augmentation and tallies; k_form: the checks and buffers of crop_pc's k form (scan_radius
        skips them)"""
        _hip.require_device()
        self.S, self.B, self.C = len(scans), int(batch_size), int(num_classes)
        self.num_point, self.num_buffer, self.rng = int(num_point), int(num_buffer), rng
        self.P = self.num_point
        if self.S < 1 or self.B < 1:
            raise ValueError("at least one scan and one crop per batch")
        if k_form and self.num_buffer // 4 < 1:
            raise ValueError("num_buffer // 4 must be >= 1 (crop_pc draws randint(0, num_buffer // 4))")
        self.kcap = self.num_point + self.num_buffer + self.num_buffer // 4 - 1
        if k_form and self.kcap > ORDER_CAP:
            raise _hip.PasnlUnsupported(f"num_point + num_buffer + num_buffer//4 - 1 = {self.kcap} > {ORDER_CAP} (the LDS sort of "
                                        "pasnl_crop_order_permute)")
        dev = []
        for s in scans:
            t = _hip.as_dev(s, torch.float32)
            if t.dim() != 2 or t.shape[1] != 3:
                raise ValueError("every scan must be (N, 3)")
            dev.append(t)
        self.sizes = [int(t.shape[0]) for t in dev]
        for n in self.sizes:
            if k_form and n < self.kcap:  # sklearn/neighbors/_binary_tree.pxi, query(): any k the crop may draw must fit
                raise ValueError("k must be less than or equal to the number of training points")
        w = np.ones((self.C,), np.float32) if label_weights is None else np.asarray(label_weights).reshape(-1)
        host = flat_labels(labels, self.sizes, "scan")
        if host.size and (int(host.min()) < 0 or int(host.max()) >= min(w.size, self.C)):
            raise IndexError(f"labels in [{int(host.min())}, {int(host.max())}] are out of bounds for {w.size} label weights and "
                             f"{self.C} classes (K:222)")
        self.offsets_host = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.N, self.nmax = int(self.offsets_host[-1]), max(self.sizes)
        self.device = dev[0].device
        self.points = torch.cat(dev).contiguous()
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.labels = torch.from_numpy(host.astype(np.int32)).to(self.device)
        self.label_weights = torch.from_numpy(w.astype(np.float32)).to(self.device)
        B = self.B
        self.desc = torch.zeros((B, DESC_BYTES), dtype=torch.uint8, device=self.device)
        if k_form:
            self.idx = torch.empty((B, self.kcap), dtype=torch.int32, device=self.device)
            self.d2 = torch.empty((B, self.kcap), dtype=torch.float64, device=self.device)
            self.cnt = torch.empty((B,), dtype=torch.int32, device=self.device)
            nbytes = int(_hip.lib().pasnl_knn_crop_workspace_bytes(B, ctypes.c_long(self.nmax)))
            self.ws, self.ws_bytes = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device), nbytes
        self.pick_stage = torch.empty((B,), dtype=torch.int32, device=self.device)
        self.k_stage = torch.zeros((B,), dtype=torch.int32, device=self.device)
        self.cloud_stage = torch.empty((B,), dtype=torch.int32, device=self.device)
        self.perm_stage = torch.empty((B, self.num_point), dtype=torch.int32, device=self.device)
        self.next_item = 0  # position in the epoch's list (K:214-216)
        self._init_augment(augment, grid_augment.config_of(augment_config, augment_symmetries=tuple(symmetries)), seed)
        self._init_tally()

    @property
    def steps_per_epoch(self):
        return int(self.S / self.B)  # K:195: int(len(train_list) / batch_size) * batch_size items

    # ---- one batch
    def draw_batch(self, first):
        """The host's RNG draws of the B items first..first+B-1, in the reference's order (K:220, 271, 288-292): the pick, k =
        num_point + buffer, and the first num_point entries of the shuffled arange(k)."""
        clouds = np.arange(first, first + self.B, dtype=np.int32)
        picks = np.empty((self.B,), np.int32)
        ks = np.empty((self.B,), np.int32)
        perms = np.empty((self.B, self.num_point), np.int32)
        for b in range(self.B):
            picks[b] = self.rng.choice(self.sizes[int(clouds[b])], 1)[0]
            k = self.num_point + self.num_buffer + self.rng.randint(0, self.num_buffer // 4)
            idx = np.arange(k)
            self.rng.shuffle(idx)
            ks[b], perms[b] = k, idx[:self.num_point]
        return clouds, picks, ks, perms

    def stage(self, draws):
        """Check the picks and copy one batch's draws into the device buffers the chain reads (asynchronous, from pinned
        memory)."""
        clouds, picks, ks, perms = draws
        for c, p in zip(clouds, picks):
            if not (0 <= int(c) < self.S) or not (0 <= int(p) < self.sizes[int(c)]):
                raise ValueError(f"pick {int(p)} of scan {int(c)} is outside the scan")
        self.clouds_host = np.ascontiguousarray(clouds, np.int32)
        self.cloud_stage.copy_(torch.from_numpy(self.clouds_host).pin_memory(), non_blocking=True)
        self.pick_stage.copy_(torch.from_numpy(np.ascontiguousarray(picks, np.int32)).pin_memory(), non_blocking=True)
        self.k_stage.copy_(torch.from_numpy(np.ascontiguousarray(ks, np.int32)).pin_memory(), non_blocking=True)
        self.perm_stage.copy_(torch.from_numpy(np.ascontiguousarray(perms, np.int32)).pin_memory(), non_blocking=True)
        if self.augment:
            self._stage_item()

    def enqueue(self, out=None):
        """The device chain of the staged batch: five ABI calls on the current stream (four with augment=False), no host
        synchronisation.  The scan indices travel to pasnl_scan_pick_given as kernel arguments: a captured chain holds the
        ones it was captured with (one graph per batch position of the epoch).  -> points (B,P,3) f32, labels (B,P) i32,
        weights (B,P) f32, point_inds (B,P) i32, cloud_inds (B,) i32."""
        B, npt = self.B, self.num_point
        if out is None:
            out = (torch.empty((B, npt, 3), dtype=torch.float32, device=self.device),
                   torch.empty((B, npt), dtype=torch.int32, device=self.device),
                   torch.empty((B, npt), dtype=torch.float32, device=self.device),
                   torch.empty((B, npt), dtype=torch.int32, device=self.device),
                   torch.empty((B,), dtype=torch.int32, device=self.device))
        pts, lab, wts, inds, clouds = out
        clouds.copy_(self.cloud_stage)
        _hip.launch("pasnl_scan_pick_given", "ScanTrainer pick", B, self.S, _p(self.offsets), _p(self.points),
                    self.clouds_host.ctypes.data_as(ctypes.c_void_p), _p(self.pick_stage), _p(self.k_stage), _p(self.desc))
        _hip.launch("pasnl_knn_crop_indirect", "ScanTrainer crop", B, ctypes.c_long(self.nmax), _p(self.points), _p(self.desc),
                    self.kcap, _p(self.idx), _p(self.d2), _p(self.cnt), _p(self.ws), ctypes.c_size_t(self.ws_bytes))
        _hip.launch("pasnl_crop_order_permute", "ScanTrainer order", B, _p(self.desc), _p(self.points), _p(self.idx), _p(self.d2),
                    self.kcap, _p(self.perm_stage), npt, _p(inds), _p(pts))
        self._gather_labels(inds, clouds, lab, wts)
        if self.augment:
            self._augment(pts)
        return pts, lab, wts, inds, clouds

    def next_batch(self):
        """Draw, stage and enqueue the next B items of the list (K:214-241 and tf_map); the list starts over when fewer than B
        items are left, as the epoch's generator does.  -> (points, labels, weights, point_inds, cloud_inds) device tensors."""
        if self.steps_per_epoch < 1:
            raise ValueError(f"{self.S} scans < batch_size = {self.B}: the epoch of int(S / B) * B items is empty")
        if self.next_item + self.B > self.steps_per_epoch * self.B:
            self.next_item = 0
        self.stage(self.draw_batch(self.next_item))
        self.next_item += self.B
        return self.enqueue()

    def run(self, step):
        """T:224-263, one epoch from the head of the list.  step: ((B,P,3) f32, (B,P) i32 labels, (B,P) f32 weights) device
        tensors -> (B,P,C) f32 logits, called once per batch.  -> total_correct / float(total_seen)."""
        self.next_item = 0
        return GridTrainLoop.run(self, step)
