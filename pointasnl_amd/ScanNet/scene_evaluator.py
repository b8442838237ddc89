"""The ScanNet grid pipeline's per-epoch evaluation on the device -- reference ScanNet/train_scannet_grid.py (S) :304-434
(`eval_one_epoch(..., vote)`: the chopped evaluation balanced by `val_proportions`, the persistent float64 table
`validation_probs` smoothed with `val_smooth = 0.95`, and every `snapshot_gap` epochs the voting evaluation through
`validation_proj`) over ScanNet/scannet_dataset_grid.py (D) :435-549 `get_batch_gen('validation')` and D:551-571 `tf_map`.

`SceneEvaluator` is `SceneTrainer`'s generator on the validation split (scene_tester.SceneCrops: the same kernels, the same
host draws in the same order) with what the evaluation adds.  One batch:

  B x (pasnl_scene_pick_crop -> pasnl_scene_order_gather -> pasnl_scene_potential_update)     D:484-520
  pasnl_scan_train_labels      labels[select] as class indices (the weights are zero, D:528-529)  D:525-526
  pasnl_scan_augment           rotation, scale, noise, colour drop, in place; no symmetry         D:450-453, 561-568
  model(inputs) -> (B,P,C) f32 logits                                                             the caller's forward
  pasnl_scene_eval_vote        validation_probs[c_i][inds] = 0.95 * old + 0.05 * softmax          S:346-351
  pasnl_scan_eval_confusion    the per-crop confusions, summed                                    S:359-368

with no host synchronisation; the (nl,nl) matrix comes down once per epoch and S:368-380 run in numpy on the host as
written.  `vote=True` adds one `pasnl_scene_eval_vote_confusion` per scene and a second read-back (S:384-432).  The table
and the potentials persist from one `run` to the next, as the reference's global table and generator state do.

Only the k form (in_radius == 0) is covered; every scene must hold at least num_point + num_buffer + num_buffer // 4 - 1
points, as for `SceneTester`.

Deviations: the augmentation's generator is Philox4x32-10 (pointasnl_amd/grid_augment.py lays out every draw), not TF's;
the softmax is computed here in float32, not by TensorFlow; nothing is written to disk and nothing is logged -- `report`
returns the lines.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip, grid_augment
from pointasnl_amd.ScanNet.scene_tester import SceneCrops
from pointasnl_amd.grid_eval_loop import GridEvalLoop
from pointasnl_amd.grid_train_loop import flat_labels

_p = _hip.ptr


class SceneEvaluator(SceneCrops, GridEvalLoop):
    """`SceneEvaluator(scenes, labels, colors=None, validation_labels=..., validation_proj=None, num_classes=21,
    num_point=8192, num_buffer=1024, batch_size=4, validation_size=500, label_values=np.arange(21), ignored_labels=(0,),
    with_rgb=True, rng=np.random, seed=0, augment=True, val_smooth=0.95)`.

    scenes, colors: as for `SceneTester`, in the order of input_trees['validation']; labels: one (n_i,) integer array per
    scene holding values of label_values (input_labels['validation']), mapped to class indices once, here (D:526);
    validation_labels: one integer array per scene, the labels of its evaluation points (the mesh vertices), and
    validation_proj: for each of them the index of its nearest sub-sampled point (None: the identity, validation_labels[i]
    then holds n_i labels).  seed: the augmentation's 64-bit key; crop number i of this evaluator's life draws under
    (seed, i)."""

    def __init__(self, scenes, labels, colors=None, validation_labels=None, validation_proj=None, num_classes=21, num_point=8192,
                 num_buffer=1024, batch_size=4, validation_size=500, label_values=None, ignored_labels=(0,), with_rgb=True,
                 rng=np.random, seed=0, augment=True, val_smooth=0.95, in_radius=0.0):
        if in_radius > 0:
            raise NotImplementedError("SceneEvaluator covers the k form only (in_radius == 0): the radius form of the evaluators "
                                      "is future work")
        self._init_eval(num_classes, label_values, ignored_labels)
        S = len(scenes)
        host = flat_labels(labels, [len(s) for s in scenes], "scene")
        lv = self.label_values.astype(np.int64)
        order = np.argsort(lv, kind="stable")
        pos = np.minimum(np.searchsorted(lv[order], host), lv.size - 1)
        if host.size and not (lv[order][pos] == host).all():
            bad = host[lv[order][pos] != host][0]
            raise KeyError(f"label {int(bad)} is not in label_values (label_to_idx, D:526)")
        if validation_labels is None or len(validation_labels) != S:
            raise ValueError("one validation_labels array per scene")
        if validation_proj is not None and len(validation_proj) != S:
            raise ValueError("one validation_proj array per scene")
        vl = [np.ascontiguousarray(np.asarray(v).reshape(-1).astype(np.int32)) for v in validation_labels]
        vp = None
        for i in range(S):
            n = len(scenes[i])
            if validation_proj is None:
                if vl[i].size != n:
                    raise ValueError(f"validation_proj=None is the identity: validation_labels[{i}] must hold {n} labels")
            else:
                p = np.asarray(validation_proj[i]).reshape(-1)
                if p.size != vl[i].size:
                    raise ValueError(f"validation_proj[{i}] holds {p.size} indices for {vl[i].size} labels")
                if p.size and (p.min() < 0 or p.max() >= n):
                    raise ValueError(f"validation_proj[{i}] outside [0, {n})")
        if validation_proj is not None:
            vp = [np.ascontiguousarray(np.asarray(p).reshape(-1).astype(np.int32)) for p in validation_proj]
        # S:324-332: the number of evaluation points of every kept class, float32, counted once
        self.val_proportions = np.zeros(self.nc, dtype=np.float32)
        i = 0
        for label_value in self.label_values:
            if label_value not in self.ignored_labels:
                self.val_proportions[i] = np.sum([np.sum(v == label_value) for v in vl])
                i += 1
        _hip.require_device()
        self.validation_size, self.val_smooth = int(validation_size), float(val_smooth)
        self._init_crops(scenes, colors, num_point, num_buffer, batch_size, validation_size, with_rgb, rng, False)
        self.P = self.num_point
        self.labels = torch.from_numpy(order[pos].astype(np.int32)).to(self.device)
        self.label_weights = torch.zeros((self.C,), dtype=torch.float32, device=self.device)  # D:528-529
        self._init_augment(augment, grid_augment.config_of(augment_symmetries=(False, False, False)), seed)  # D:450-453
        self._init_confusion()
        self.probs = torch.zeros((self.N, self.nc), dtype=torch.float64, device=self.device)  # S:325
        self.smooth_new = float(np.float32(1 - self.val_smooth))  # numpy >= 2: python_float * float32_array -> float32
        self.labels_dev = torch.from_numpy(self.label_values).to(self.device)
        self.val_labels = [torch.from_numpy(v).to(self.device) for v in vl]
        self.val_proj = None if vp is None else [torch.from_numpy(p).to(self.device) for p in vp]
        self.sub_preds = torch.empty((self.nmax,), dtype=torch.int32, device=self.device)
        self.vote_confusion_dev = torch.zeros((self.L, self.L), dtype=torch.int64, device=self.device)
        self.mIoU, self.mIoU_vote, self.vote_IoUs = None, None, None

    # ---- one batch
    def stage(self, draws):
        """Copy one batch's draws, and the running crop number of the augmentation, into the device buffers the chain reads."""
        SceneCrops.stage(self, draws)
        if self.augment:
            self._stage_item()

    def enqueue(self, out=None):
        """The generator's device chain of the staged batch: `SceneTester`'s, the label gather and the augmentation, on the
        current stream, no host synchronisation, capturable.  -> inputs (B,P,3+F) f32, labels (B,P) i32, weights (B,P) f32
        (zeros), point_inds (B,P) i32, cloud_inds (B,) i32."""
        inputs, inds, clouds = SceneCrops.enqueue(self, None if out is None else (out[0], out[3], out[4]))
        lab = torch.empty((self.B, self.P), dtype=torch.int32, device=self.device) if out is None else out[1]
        wts = torch.empty((self.B, self.P), dtype=torch.float32, device=self.device) if out is None else out[2]
        self._gather_labels(inds, clouds, lab, wts)
        if self.augment:
            self._augment(inputs)
        return inputs, lab, wts, inds, clouds

    def vote(self, logits, point_inds, cloud_inds, is_logits=True):
        """S:346-351 for one batch, crop after crop, into the float64 table: logits (B,P,C) f32 -- the table takes
        softmax(logits[..., 1:]) -- or, is_logits=False, probabilities (B,P,C-1)."""
        v = _hip.as_dev(logits, torch.float32).reshape(self.B, self.P, self.C if is_logits else self.nc)
        pi = _hip.as_dev(point_inds, torch.int32).reshape(self.B, self.P)
        ci = _hip.as_dev(cloud_inds, torch.int32).reshape(self.B)
        _hip.launch("pasnl_scene_eval_vote", "SceneEvaluator vote", self.B, self.P, self.nc, _p(v), 1 if is_logits else 0, _p(pi),
                    _p(ci), _p(self.offsets), ctypes.c_double(self.val_smooth), ctypes.c_float(self.smooth_new), _p(self.probs),
                    _p(self.win))

    def enqueue_batch(self, model, out=None):
        """everything one staged batch puts on the stream: the generator's chain, the forward, the vote and the confusions --
        no host synchronisation, capturable when the model is.  -> the model's logits"""
        inputs, lab, _, inds, clouds = self.enqueue(out)
        logits = model(inputs)
        self.vote(logits, inds, clouds)
        self.score(logits, lab)
        return logits

    # ---- the epoch
    def run(self, model, vote=False):
        """One `eval_one_epoch` (S:304-434): validation_size batches, each drawn, staged and enqueued; then the single
        read-back, S:368-380 in numpy, and with vote=True the voting evaluation.  model: inputs (B,P,3+F) f32 ->
        (B,P,C) f32 logits.  -> (mIoU, mIoU_vote), mIoU_vote = 0 without the vote."""
        self.reset()
        for _ in range(self.validation_size):
            self.stage(self.draw_batch())
            self.enqueue_batch(model)
        C = self.drop_ignored(self.confusion().astype(np.float32))   # S:368-374
        C *= np.expand_dims(self.val_proportions / (np.sum(C, axis=1) + 1e-6), 1)  # S:377
        self.mIoU = 100 * np.mean(self.iou_from_confusions(C))
        self.mIoU_vote, self.vote_IoUs = 0, None
        if vote:
            Cv = self.drop_ignored(self.vote_confusion())
            self.vote_IoUs = self.iou_from_confusions(Cv)
            self.mIoU_vote = 100 * np.mean(self.vote_IoUs)
        return self.mIoU, self.mIoU_vote

    def vote_confusion(self):
        """S:389-413: the (nl,nl) int64 confusion of every scene's voted predictions reprojected onto its evaluation points,
        scene after scene in list order (two launches each), then one read-back."""
        self.vote_confusion_dev.zero_()
        null = ctypes.c_void_p(0)
        for i in range(self.S):
            _hip.launch("pasnl_scene_eval_vote_confusion", "SceneEvaluator voting", ctypes.c_long(self.sizes[i]),
                        _p(self.validation_probs(i)), self.nc, ctypes.c_long(int(self.val_labels[i].shape[0])),
                        null if self.val_proj is None else _p(self.val_proj[i]), _p(self.val_labels[i]), _p(self.labels_dev),
                        self.ignored_ptr, self.L, _p(self.sub_preds), _p(self.vote_confusion_dev))
        return self.vote_confusion_dev.cpu().numpy()

    def report(self, seg_label_to_cat):
        """the lines S:382 and, after a voting epoch, S:424-432 log for the last `run`"""
        lines = ["Eval point avg class IoU: %.3f" % (self.mIoU)]
        if self.vote_IoUs is not None:
            lines += [self.class_lines(self.vote_IoUs, seg_label_to_cat, self.C), "Eval voting avg class IoU: %.3f \n" % (self.mIoU_vote)]
        return lines

    # ---- state
    def validation_probs(self, i):
        """scene i's float64 table (n_i, C-1), a device view"""
        return self.probs[self._rows(i)]
