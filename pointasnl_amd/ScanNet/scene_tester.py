"""The ScanNet grid test and validation loops on the device -- reference ScanNet/scannet_dataset_grid.py (D) :435-549
(`get_batch_gen('test' | 'validation')`: potentials, the noisy pick, the crop, the potential update) and
ScanNet/test_scannet_grid.py (T) :95-229 (`ModelTester.test_cloud_segmentation`) and :231-448
(`test_cloud_segmentation_on_val`): float32 votes over C - 1 classes, each split's checkpoint rule, reprojection of labels,
potentials and probabilities, confusion matrices and IoU.

`SceneTester` holds every scene of a split in one flat device buffer with its colours, its potentials (float64) and its
votes (float32) beside it.  `next_batch()` enqueues, crop after crop, pick + crop -> nearest-first order, shuffle and gather
-> potential update on the current stream (csrc/crop.hip, csrc/scene_test.hip: ten launches per crop): no host
synchronisation, capturable.  The RNG draws of the flow -- the potentials' init, the pick's Gaussian noise, the crop's
`buffer` and its shuffle -- depend on lengths the host knows, so they are drawn on the host from the caller's numpy
RandomState in the reference's order, and the crop sequence is the reference's, crop for crop (tests/scene_flow_ref.py
restates the flow in numpy; tests/test_scene_tester_flow.py pins it to the reference's generator).

Only the k form (in_radius == 0, the reference default) is covered here (the radius form: scene_radius.py), and every scene
must hold at least num_point + num_buffer + num_buffer // 4 - 1 points (9 471 at the defaults): a smaller scene would change k and pull
data_rep's np.random.choice into a stream whose length depends on the device-chosen scene.  Whether real ScanNet scenes at
the reference's sub-sampling always clear that count has not been measured.

`SceneCrops` is the part every split shares -- the scenes, the potentials, the draws and the crop chain; `SceneTester` adds
the votes, and `scene_trainer.SceneTrainer` the training split's labels, weights and augmentation.

Deviations: the crops are fed unaugmented (the reference maps tf_augment_input over them with TF's RNG, which cannot be
reproduced; its colour drop is a no-op at augment_color = 1.0); the softmax of a vote is computed here in float32, not by
TensorFlow; proj_inds computed here break distance ties by the lowest index (sklearn: by its tree's order); PLY and txt
files are not written -- `reproject` returns the three arrays the reference writes.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.SemanticKITTI.scan_tester import ORDER_CAP, project

_p = _hip.ptr

DESC_BYTES = 48  # sizeof(pasnl_scene_crop_t)
SMOOTH = {"test": 0.98, "validation": 0.95}  # T:101, 234


class SceneCrops:
    """What the grid generator does for every split (D:464-541): the scenes in one flat device buffer with their colours and
    potentials, the host's draws of a batch and the device chain of its crops.  `SceneTester` adds the votes of the test and
    validation splits, `scene_trainer.SceneTrainer` the labels, weights and augmentation of the training split."""

    def _init_crops(self, scenes, colors, num_point, num_buffer, batch_size, steps, with_rgb, rng, abs_coords, k_form=True):
        """k_form: the checks and buffers of the k form (scene_radius skips them)"""
        self.S, self.B = len(scenes), int(batch_size)
        self.num_point, self.num_buffer, self.rng = int(num_point), int(num_buffer), rng
        self.abs_coords = bool(abs_coords)
        if self.S < 1 or self.B < 1 or int(steps) < 1:
            raise ValueError("at least one scene, one crop per batch and one batch per epoch")
        if k_form and self.num_buffer // 4 < 1:
            raise ValueError("num_buffer // 4 must be >= 1 (the crop draws randint(0, num_buffer // 4))")
        self.kcap = self.num_point + self.num_buffer + self.num_buffer // 4 - 1
        if k_form and self.kcap > ORDER_CAP:
            raise _hip.PasnlUnsupported(f"num_point + num_buffer + num_buffer//4 - 1 = {self.kcap} > {ORDER_CAP} (the LDS sort of "
                                        "pasnl_scene_order_gather)")
        dev = []
        for s in scenes:
            t = _hip.as_dev(s, torch.float32)
            if t.dim() != 2 or t.shape[1] != 3:
                raise ValueError("every scene must be (N, 3)")
            dev.append(t)
        self.sizes = [int(t.shape[0]) for t in dev]
        for i, n in enumerate(self.sizes):
            if k_form and n < self.kcap:
                raise ValueError(f"scene {i} has {n} points < num_point + num_buffer + num_buffer//4 - 1 = {self.kcap}: k would "
                                 "shrink and data_rep's np.random.choice would enter the RNG stream (D:495-496, 533-535)")
        self.F = 3 if with_rgb else 0
        if with_rgb:
            if colors is None or len(colors) != self.S:
                raise ValueError("with_rgb needs one colour array per scene")
            cdev = [_hip.as_dev(c, torch.float32) for c in colors]
            for i, c in enumerate(cdev):
                if c.dim() != 2 or tuple(c.shape) != (self.sizes[i], 3):
                    raise ValueError(f"colors[{i}] must be ({self.sizes[i]}, 3), the rows of scene {i}")
        self.width = 3 + self.F + (3 if self.abs_coords else 0)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.N, self.nmax = int(self.offsets_host[-1]), max(self.sizes)
        self.device = dev[0].device
        self.points = torch.cat(dev).contiguous()
        self.colors = torch.cat(cdev).contiguous() if with_rgb else None
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        pots, mins = [], []
        for n in self.sizes:  # D:472-478, in list order
            pots.append(rng.rand(n) * 1e-3)
            mins.append(float(np.min(pots[-1])))
        self.potentials = torch.from_numpy(np.concatenate(pots)).to(self.device)
        self.min_pots = torch.tensor(mins, dtype=torch.float64, device=self.device)
        self.win = torch.empty((self.nmax,), dtype=torch.int32, device=self.device)
        _hip.launch("pasnl_scan_scratch_init", type(self).__name__, ctypes.c_long(self.nmax), _p(self.win))
        self.desc = torch.zeros((self.B, DESC_BYTES), dtype=torch.uint8, device=self.device)
        if k_form:
            self.idx = torch.empty((self.kcap,), dtype=torch.int32, device=self.device)
            self.d2 = torch.empty((self.kcap,), dtype=torch.float64, device=self.device)
            self.cnt = torch.empty((1,), dtype=torch.int32, device=self.device)
            nbytes = int(_hip.lib().pasnl_knn_crop_workspace_bytes(1, ctypes.c_long(self.nmax)))
            self.ws, self.ws_bytes = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device), nbytes
        self.noise_stage = torch.empty((self.B, 3), dtype=torch.float64, device=self.device)
        self.k_stage = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.perm_stage = torch.empty((self.B, self.num_point), dtype=torch.int32, device=self.device)

    # ---- one batch
    def draw_batch(self):
        """The host's RNG draws of B crops, in the reference's order (D:488, 494, 500): the pick's noise, k = num_point +
        buffer, and the first num_point entries of the shuffled arange(k)."""
        noise = np.empty((self.B, 3), np.float64)
        ks = np.empty((self.B,), np.int32)
        perms = np.empty((self.B, self.num_point), np.int32)
        for b in range(self.B):
            noise[b] = self.rng.normal(scale=0.35, size=(1, 3))[0]
            k = self.num_point + self.num_buffer + self.rng.randint(0, self.num_buffer // 4)
            idx = np.arange(k)
            self.rng.shuffle(idx)
            ks[b], perms[b] = k, idx[:self.num_point]
        return noise, ks, perms

    def stage(self, draws):
        """Copy one batch's draws into the device buffers the chain reads (asynchronous, from pinned memory)."""
        noise, ks, perms = draws
        self.noise_stage.copy_(torch.from_numpy(noise).pin_memory(), non_blocking=True)
        self.k_stage.copy_(torch.from_numpy(ks).pin_memory(), non_blocking=True)
        self.perm_stage.copy_(torch.from_numpy(perms).pin_memory(), non_blocking=True)

    def enqueue(self, out=None):
        """The device chain of the staged batch: B x (pick + crop -> order/gather -> update), on the current stream, no host
        synchronisation.  -> inputs (B,num_point,3+F[+3]) f32, point_inds (B,num_point) i32, cloud_inds (B,) i32."""
        B, npt = self.B, self.num_point
        if out is None:
            out = (torch.empty((B, npt, self.width), dtype=torch.float32, device=self.device),
                   torch.empty((B, npt), dtype=torch.int32, device=self.device),
                   torch.empty((B,), dtype=torch.int32, device=self.device))
        inputs, inds, clouds = out
        for b in range(B):
            desc = _p(self.desc, b * DESC_BYTES)
            sel = _p(inds, b * npt * 4)
            _hip.launch("pasnl_scene_pick_crop", "SceneTester pick+crop", self.S, _p(self.offsets), _p(self.potentials),
                        _p(self.min_pots), _p(self.points), _p(self.k_stage, b * 4), _p(self.noise_stage, b * 24), desc,
                        _p(clouds, b * 4), ctypes.c_long(self.nmax), self.kcap, _p(self.idx), _p(self.d2), _p(self.cnt), _p(self.ws),
                        ctypes.c_size_t(self.ws_bytes))
            _hip.launch("pasnl_scene_order_gather", "SceneTester order", 1, desc, _p(self.points),
                        _p(self.colors) if self.F else ctypes.c_void_p(0), self.F, _p(self.idx), _p(self.d2), self.kcap,
                        _p(self.perm_stage, b * npt * 4), npt, 1 if self.abs_coords else 0, sel, _p(inputs, b * npt * self.width * 4))
            _hip.launch("pasnl_scene_potential_update", "SceneTester update", npt, desc, _p(self.points), sel, _p(self.potentials),
                        _p(self.min_pots), _p(self.win))
        return inputs, inds, clouds

    def next_batch(self):
        """Draw, stage and enqueue one batch (D:482-541 for B crops).  -> (inputs, point_inds, cloud_inds) device tensors."""
        self.stage(self.draw_batch())
        return self.enqueue()

    # ---- state
    def _rows(self, i):
        return slice(int(self.offsets_host[i]), int(self.offsets_host[i + 1]))

    def potentials_of(self, i):
        return self.potentials[self._rows(i)]

    def min_potentials(self):
        return self.min_pots.cpu().numpy()

    def scene_points(self, i):
        return self.points[self._rows(i)]


class SceneTester(SceneCrops):
    """`SceneTester(scenes, colors=colors, num_classes=21, num_point=8192, num_buffer=1024, batch_size=4, split='test',
    validation_size=500, label_values=np.arange(21), ignored_labels=(0,), with_rgb=True, rng=np.random)`.

    scenes: a list of (n_i,3) float32 sub-sampled scenes (numpy arrays or device tensors) in the order of the reference's
    input_trees[split]; colors: their (n_i,3) float32 colour rows (with_rgb).  The model sees C = num_classes logits and the
    tables hold C - 1 classes (T:95, 108); label_values lists every label, ignored ones included, so
    C - 1 + len(ignored_labels) == len(label_values).  Construction draws `rng.rand(n_i) * 1e-3` scene after scene
    (D:472-478); every crop then draws `rng.normal(scale=0.35, size=(1, 3))`, `rng.randint(0, num_buffer // 4)` and
    `rng.shuffle` of its k indices.  abs_coords: append the reference's three extra feature columns float32(xyz + pick)
    (D:539) to the model input."""

    def __init__(self, scenes, colors=None, num_classes=21, num_point=8192, num_buffer=1024, batch_size=4, split="test",
                 validation_size=500, label_values=None, ignored_labels=(0,), with_rgb=True, rng=np.random, in_radius=0.0,
                 abs_coords=False, test_smooth=None):
        if in_radius > 0:
            raise NotImplementedError("SceneTester covers the k form only (in_radius == 0): the radius form is "
                                      "pointasnl_amd.ScanNet.scene_radius.RadiusSceneTester")
        self._init_tester(scenes, colors, num_classes, num_point, num_buffer, batch_size, split, validation_size, label_values,
                          ignored_labels, with_rgb, rng, abs_coords, test_smooth)

    def _init_tester(self, scenes, colors, num_classes, num_point, num_buffer, batch_size, split, validation_size, label_values,
                     ignored_labels, with_rgb, rng, abs_coords, test_smooth, k_form=True):
        if split not in SMOOTH:
            raise ValueError('split must be "test" or "validation"')
        _hip.require_device()
        self.C, self.split, self.validation_size = int(num_classes), split, int(validation_size)
        self.test_smooth = SMOOTH[split] if test_smooth is None else float(test_smooth)
        self.label_values = np.arange(self.C, dtype=np.int32) if label_values is None else np.asarray(label_values, np.int32).reshape(-1)
        self.ignored_labels = tuple(int(v) for v in ignored_labels)
        self.ignored_mask = np.isin(self.label_values, self.ignored_labels).astype(np.int32)
        self.L, self.nc = int(self.label_values.size), self.C - 1
        if len(set(self.label_values.tolist())) != self.L:
            raise ValueError("label_values must be distinct")
        if self.nc < 1 or self.nc + int(self.ignored_mask.sum()) != self.L:
            raise ValueError(f"num_classes - 1 = {self.nc} table columns + {int(self.ignored_mask.sum())} ignored labels != "
                             f"{self.L} label values")
        self._init_crops(scenes, colors, num_point, num_buffer, batch_size, validation_size, with_rgb, rng, abs_coords, k_form)
        self.probs = torch.zeros((self.N, self.nc), dtype=torch.float32, device=self.device)
        self.smooth_old = float(np.float32(self.test_smooth))      # numpy: python_float * float32_array -> float32 product
        self.smooth_new = float(np.float32(1 - self.test_smooth))
        self.labels_dev = torch.from_numpy(self.label_values).to(self.device)
        self.ignored_dev = torch.from_numpy(self.ignored_mask).to(self.device)
        self.checkpoints = []  # (epoch, new_min) of every checkpoint run() fired

    def vote(self, logits, point_inds, cloud_inds, is_logits=True):
        """T:141-149 / 283-291 for one batch, crop after crop: logits (B,num_point,C) f32 -- the table takes
        softmax(logits[..., 1:]) -- or, is_logits=False, probabilities (B,num_point,C-1)."""
        v = _hip.as_dev(logits, torch.float32).reshape(self.B, self.num_point, self.C if is_logits else self.nc)
        pi = _hip.as_dev(point_inds, torch.int32).reshape(self.B, self.num_point)
        ci = _hip.as_dev(cloud_inds, torch.int32).reshape(self.B)
        _hip.launch("pasnl_scene_vote", "SceneTester vote", self.B, self.num_point, self.nc, _p(v), 1 if is_logits else 0, _p(pi),
                    _p(ci), _p(self.offsets), ctypes.c_float(self.smooth_old), ctypes.c_float(self.smooth_new), _p(self.probs),
                    _p(self.win))

    @property
    def crops_per_epoch(self):
        return self.validation_size * self.B  # D:462-465

    def _epoch(self, forward):
        """one epoch of the generator: validation_size batches, each voted"""
        for _ in range(self.validation_size):
            inputs, inds, clouds = self.next_batch()
            self.vote(forward(inputs), inds, clouds)

    def run(self, forward, num_votes=100, on_checkpoint=None, max_epochs=None):
        """The epoch loop of T:128-227 (test) / T:271-446 (validation): epochs of validation_size batches while
        last_min < num_votes; after each, new_min = min(min_potentials) is read back (the only synchronisation) and the
        split's rule decides a checkpoint -- test: last_min + 2 < new_min, then last_min = new_min; validation:
        last_min + 1 < new_min, then last_min += 1 -- where `on_checkpoint(tester, new_min)` is called (the reference
        reprojects there, or scores and reprojects when int(ceil(new_min)) % 4 == 0).  forward: inputs -> (B,num_point,C)
        logits.  -> the number of epochs run; the checkpoints are appended to `self.checkpoints` as (epoch, new_min)."""
        epochs, last_min = 0, -0.5
        while last_min < num_votes:
            self._epoch(forward)
            new_min = float(self.min_pots.min().item())
            step = 2 if self.split == "test" else 1
            if last_min + step < new_min:
                last_min = new_min if self.split == "test" else last_min + 1
                self.checkpoints.append((epochs, new_min))
                if on_checkpoint is not None:
                    on_checkpoint(self, new_min)
            epochs += 1
            if max_epochs is not None and epochs >= max_epochs:
                break
        return epochs

    # ---- state
    def test_probs(self, i):
        """scene i's float32 vote table (n_i, C-1), a device view"""
        return self.probs[self._rows(i)]

    # ---- reprojection and scoring
    def proj_inds(self, i, raw_points):
        """The nearest sub-sampled point of scene i for every mesh vertex (sklearn KDTree(sub).query(vertices), D:405-406),
        ties to the lowest index.  -> (m,) int32 device tensor."""
        return project(self.scene_points(i), raw_points)

    def _proj(self, i, raw_points, proj_inds):
        n = self.sizes[i]
        if proj_inds is None:
            return None if raw_points is None else self.proj_inds(i, raw_points)
        host = proj_inds.cpu().numpy() if isinstance(proj_inds, torch.Tensor) else np.asarray(proj_inds)
        host = host.reshape(-1)
        if host.size and (host.min() < 0 or host.max() >= n):
            raise ValueError(f"proj_inds outside [0, {n})")
        return torch.from_numpy(host.astype(np.int32)).to(self.device)

    def _labels(self, i, proj, want_all):
        m = self.sizes[i] if proj is None else int(proj.shape[0])
        preds = torch.empty((max(m, 1),), dtype=torch.int32, device=self.device)
        pots = torch.empty((max(m, 1),), dtype=torch.float64, device=self.device) if want_all else None
        probs = torch.empty((max(m, 1), self.nc), dtype=torch.float32, device=self.device) if want_all else None
        null = ctypes.c_void_p(0)
        _hip.launch("pasnl_scene_labels", "SceneTester labels", ctypes.c_long(m), _p(proj) if proj is not None else null,
                    _p(self.test_probs(i)), self.nc, _p(self.potentials_of(i)), _p(self.labels_dev), _p(self.ignored_dev), self.L,
                    _p(preds), _p(pots) if want_all else null, _p(probs) if want_all else null)
        return m, preds, pots, probs

    def reproject(self, i, raw_points=None, proj_inds=None):
        """T:183-218 for scene i at proj_inds (computed from raw_points, or given as the reference loads them; neither: the
        sub-sampled points themselves) -> preds (m,) int32 = label_values[argmax(probs with a zero column per ignored label)],
        pots (m,) float64, probs (m,C-1) float32: the arrays the reference writes to its PLY files, as numpy."""
        m, preds, pots, probs = self._labels(i, self._proj(i, raw_points, proj_inds), True)
        return preds[:m].cpu().numpy(), pots[:m].cpu().numpy(), probs[:m].cpu().numpy()

    def confusion(self, targets, proj_inds=None):
        """The summed confusion matrix of every scene (T:319-339 on the sub clouds; with proj_inds, one array per scene,
        T:378-398 on the full meshes): targets[i] holds scene i's labels (n_i of them, or one per proj_inds[i] entry) as
        values of label_values; a label outside them is dropped.  -> (L,L) int64 numpy, rows the truth."""
        if len(targets) != self.S or (proj_inds is not None and len(proj_inds) != self.S):
            raise ValueError("one target array (and one proj_inds array) per scene")
        out = torch.zeros((self.L, self.L), dtype=torch.int64, device=self.device)
        for i in range(self.S):
            m, preds, _, _ = self._labels(i, None if proj_inds is None else self._proj(i, None, proj_inds[i]), False)
            t = _hip.as_dev(np.ascontiguousarray(np.asarray(targets[i]).reshape(-1).astype(np.int32)), torch.int32)
            if int(t.shape[0]) != m:
                raise ValueError(f"scene {i}: {int(t.shape[0])} targets for {m} predictions")
            if m > 0:
                _hip.launch("pasnl_confusion_matrix", "SceneTester confusion", ctypes.c_long(m), _p(t), _p(preds),
                            _p(self.labels_dev), self.L, _p(out))
        return out.cpu().numpy()

    def drop_ignored(self, C):
        """T:341-345: the rows and columns of the ignored labels removed."""
        keep = np.flatnonzero(self.ignored_mask == 0)
        return np.asarray(C)[np.ix_(keep, keep)]


def confusion_matrix(targets, preds, label_values):
    """sklearn.metrics.confusion_matrix(targets, preds, labels=label_values) on the device -> (L,L) int64 numpy."""
    _hip.require_device()
    t, p = _hip.as_dev(targets, torch.int32).reshape(-1), _hip.as_dev(preds, torch.int32).reshape(-1)
    lv = _hip.as_dev(np.asarray(label_values, np.int32).reshape(-1), torch.int32)
    if t.shape != p.shape:
        raise ValueError("targets and preds differ in length")
    out = torch.zeros((int(lv.shape[0]),) * 2, dtype=torch.int64, device=lv.device)
    if int(t.shape[0]) > 0:
        _hip.launch("pasnl_confusion_matrix", "confusion_matrix", ctypes.c_long(int(t.shape[0])), _p(t), _p(p), _p(lv),
                    int(lv.shape[0]), _p(out))
    return out.cpu().numpy()


def val_proportions(labels_per_mesh, label_values, ignored_labels):
    """T:245-251: the number of mesh vertices of every kept class, float32."""
    kept = [v for v in label_values if v not in ignored_labels]
    return np.array([np.sum([np.sum(np.asarray(lab) == v) for lab in labels_per_mesh]) for v in kept], dtype=np.float32)


def rescale_by_proportions(C, proportions):
    """T:337, 348: the sub-cloud confusions (ignored labels dropped) as float32, each truth row scaled to its class's vertex count."""
    C = np.asarray(C).astype(np.float32)
    C *= np.expand_dims(np.asarray(proportions, np.float32) / (np.sum(C, axis=1) + 1e-6), 1)
    return C


def iou_from_confusions(confusions):
    """utils/metrics.py:120-146: per-class IoU of (..., n, n) confusion matrices (rows the truth); a class with no truth
    gets the mean IoU of the present classes, so a later mean is over those."""
    confusions = np.asarray(confusions)
    tp = np.diagonal(confusions, axis1=-2, axis2=-1)
    truth = np.sum(confusions, axis=-1)
    predicted = np.sum(confusions, axis=-2)
    iou = tp / (predicted + truth - tp + 1e-6)
    absent = truth < 1e-3
    present = np.sum(1 - absent, axis=-1, keepdims=True)
    mean = np.sum(iou, axis=-1, keepdims=True) / (present + 1e-6)
    iou += absent * mean
    return iou
