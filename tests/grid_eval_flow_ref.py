"""numpy restatement of the two grid pipelines' per-epoch evaluation -- reference ScanNet/train_scannet_grid.py (S) :304-434
`eval_one_epoch(..., vote)` and SemanticKITTI/train_semantic_kitti_grid.py (K) :265-330 `eval_one_epoch` -- the yardstick of
pointasnl_amd.ScanNet.scene_evaluator and pointasnl_amd.SemanticKITTI.scan_evaluator.  The generators are scene_flow_ref.py's
validation split and grid_train_flow_ref.py's scan list (tests/test_scene_tester_flow.py and tests/test_grid_train_flow.py
pin them to the reference's); what is stated here is what the evaluation does with the model's output, line for line and in
numpy's own dtypes (numpy >= 2: a Python float times a float32 array is a float32 product).  tests/test_grid_eval_flow.py
pins this file to the reference's own functions."""
import numpy as np

import philox_ref as P
from grid_train_flow_ref import ScanTrainFlowRef
from scan_flow_ref import softmax_f32
from scene_flow_ref import SceneFlowRef, confusion, iou_from_confusions

VALIDATION = dict(P.DEFAULT, symmetries=(False, False, False))  # D:450-453, K:198-202: a split that is not training


def softmax_f64(logits):
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def gap_logits(x, num_classes):
    """the end-to-end tests' model: integer-valued logits from the BITS of the input's xyz columns, so the device and the
    host compute the same float32 values by integer operations alone; class k in [1, C) gets 9 on top of a base in [0, 7]:
    a per-row top-two gap >= 2.  x (B,P,W) f32 -> (B,P,C) f32"""
    h = np.ascontiguousarray(x, np.float32).view(np.int32)
    u = ((h[:, :, 0] >> 1) ^ (h[:, :, 1] >> 3) ^ (h[:, :, 2] >> 2)) & 0x7FFFFFFF
    c = np.arange(num_classes, dtype=np.int32)
    base = (u[:, :, None] >> (c % 20)) & 7
    k = 1 + (u >> 5) % (num_classes - 1)
    return (base + 9 * (c == k[:, :, None])).astype(np.float32)


def top_two_gap(logits):
    """the smallest distance between the two largest of logits[..., 1:] over all rows"""
    s = np.sort(np.asarray(logits)[..., 1:], axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


def class_lines(IoUs, seg_label_to_cat, NUM_CLASSES):
    """S:424-428, K:321-325"""
    iou_per_class_str = '------- IoU --------\n'
    for l in range(1, NUM_CLASSES):
        iou_per_class_str += 'class %s IoU: %.3f \n' % (
            seg_label_to_cat[l] + ' ' * (14 - len(seg_label_to_cat[l])),
            100 * IoUs[l - 1])
    return iou_per_class_str


def crop_confusions(predictions, targets, label_values, ignored_labels, nc_tot):
    """S:359-368, K:301-310 -> Confs (len, nc_tot, nc_tot) int32 and C float32"""
    Confs = np.zeros((len(predictions), nc_tot, nc_tot), dtype=np.int32)
    for i, (probs, truth) in enumerate(zip(predictions, targets)):
        for l_ind, label_value in enumerate(label_values):
            if label_value in ignored_labels:
                probs = np.insert(probs, l_ind, 0, axis=1)
        preds = label_values[np.argmax(probs, axis=1)]
        Confs[i, :, :] = confusion(truth, preds, label_values)
    return Confs, np.sum(Confs, axis=0).astype(np.float32)


def drop_ignored(C, label_values, ignored_labels):
    """S:370-374"""
    for l_ind, label_value in reversed(list(enumerate(label_values))):
        if label_value in ignored_labels:
            C = np.delete(C, l_ind, axis=0)
            C = np.delete(C, l_ind, axis=1)
    return C


class SceneEvalFlowRef:
    """S:304-434 over D's 'validation' generator; `validation_probs`, `val_proportions` and the potentials persist"""

    def __init__(self, scenes, labels, colors=None, validation_labels=None, validation_proj=None, num_classes=21, num_point=8192,
                 num_buffer=1024, batch_size=4, validation_size=500, label_values=None, ignored_labels=(0,), rng=np.random,
                 softmax=softmax_f32):
        self.gen = SceneFlowRef(scenes, colors=colors, labels=labels, num_classes=num_classes, num_point=num_point,
                                num_buffer=num_buffer, batch_size=batch_size, split="validation", validation_size=validation_size,
                                label_values=label_values, ignored_labels=ignored_labels, rng=rng)
        self.input_labels, self.validation_labels = labels, validation_labels
        self.validation_proj = [np.arange(len(s)) for s in scenes] if validation_proj is None else validation_proj
        self.label_values, self.ignored_labels = self.gen.label_values, self.gen.ignored_labels
        self.NUM_CLASSES, self.B, self.validation_size, self.softmax = num_classes, batch_size, validation_size, softmax
        self.validation_probs = None
        self.val_proportions = None
        self.item = 0  # crops augmented so far

    def eval_one_epoch(self, model, vote=False, seg_label_to_cat=None, seed=None, with_rgb=True):
        """model: inputs (B,P,3+F) f32 -> (B,P,C) logits; seed: augment under it (None: unaugmented).
        -> dict(mIoU, mIoU_vote, log, C, Confs_vote, clouds, inds)"""
        log = ['---- EVALUATION ----']
        val_smooth = 0.95
        nc_tot = self.NUM_CLASSES
        nc_model = self.NUM_CLASSES - 1
        if self.validation_probs is None:
            self.validation_probs = [np.zeros((l.shape[0], nc_model)) for l in self.input_labels]
            self.val_proportions = np.zeros(nc_model, dtype=np.float32)
            i = 0
            for label_value in self.label_values:
                if label_value not in self.ignored_labels:
                    self.val_proportions[i] = np.sum([np.sum(labels == label_value) for labels in self.validation_labels])
                    i += 1
        validation_probs = self.validation_probs
        predictions = []
        targets = []
        out = dict(clouds=[], inds=[], fed=[], logits=[])
        for _ in range(self.validation_size):
            inputs, point_inds, cloud_inds, _ = self.gen.batch(with_rgb=with_rgb)
            if seed is not None:
                inputs = P.augment(inputs, seed, self.item, VALIDATION)
                self.item += self.B
            logits = np.asarray(model(inputs), np.float32)
            stacked_probs = self.softmax(logits[:, :, 1:])
            out["clouds"].append(cloud_inds)
            out["inds"].append(point_inds)
            out["fed"].append(inputs)
            out["logits"].append(logits)
            for b in range(stacked_probs.shape[0]):
                probs = stacked_probs[b]
                inds = point_inds[b]
                c_i = cloud_inds[b]
                validation_probs[c_i][inds] = val_smooth * validation_probs[c_i][inds] + (1 - val_smooth) * probs
                predictions += [probs]
                targets += [self.input_labels[c_i][inds]]
        Confs, C = crop_confusions(predictions, targets, self.label_values, self.ignored_labels, nc_tot)
        out["Confs"] = np.sum(Confs, axis=0)
        C = drop_ignored(C, self.label_values, self.ignored_labels)
        C *= np.expand_dims(self.val_proportions / (np.sum(C, axis=1) + 1e-6), 1)
        IoUs = iou_from_confusions(C)
        mIoU = 100 * np.mean(IoUs)
        log.append('Eval point avg class IoU: %.3f' % (mIoU))
        mIoU_vote = 0
        if vote:
            log.append('---- VOTING EVALUATION ----')
            Confs = np.zeros((nc_tot, nc_tot), dtype=np.int32)
            for i_val in range(len(self.input_labels)):
                sub_probs = validation_probs[i_val]
                for l_ind, label_value in enumerate(self.label_values):
                    if label_value in self.ignored_labels:
                        sub_probs = np.insert(sub_probs, l_ind, 0, axis=1)
                sub_preds = self.label_values[np.argmax(sub_probs, axis=1).astype(np.int32)]
                preds = (sub_preds[self.validation_proj[i_val]]).astype(np.int32)
                labels = self.validation_labels[i_val].astype(np.int32)
                Confs += confusion(labels, preds, self.label_values).astype(np.int32)
            out["Confs_vote"] = Confs.copy()
            Confs = drop_ignored(Confs, self.label_values, self.ignored_labels)
            IoUs = iou_from_confusions(Confs)
            mIoU_vote = 100 * np.mean(IoUs)
            log.append(class_lines(IoUs, seg_label_to_cat, self.NUM_CLASSES))
            log.append('Eval voting avg class IoU: %.3f \n' % (mIoU_vote))
        out.update(mIoU=mIoU, mIoU_vote=mIoU_vote, log=log)
        return out


class ScanEvalFlowRef:
    """K:265-330 over K's 'validation' generator (the training generator's form over val_list, no symmetry)"""

    def __init__(self, scans, labels, num_classes=20, num_point=10240, num_buffer=1024, batch_size=4, ignored_labels=(0,),
                 rng=np.random):
        self.gen = ScanTrainFlowRef(scans, labels, num_classes=num_classes, num_point=num_point, num_buffer=num_buffer,
                                    batch_size=batch_size, rng=rng)
        self.NUM_CLASSES, self.B = num_classes, batch_size
        self.label_values, self.ignored_labels = np.arange(num_classes), np.asarray(ignored_labels)
        self.item = 0

    def eval_one_epoch(self, model, seg_label_to_cat, seed=None):
        log = ['---- EVALUATION ----']
        nc_tot = self.NUM_CLASSES
        predictions = []
        targets = []
        out = dict(clouds=[], inds=[], fed=[], logits=[])
        self.gen.next_item = 0
        for _ in range(self.gen.steps_per_epoch):
            pts, labels, _, point_inds, cloud_inds = self.gen.batch()
            if seed is not None:
                pts = P.augment(pts, seed, self.item, VALIDATION)
                self.item += self.B
            logits = np.asarray(model(pts), np.float32)
            stacked_probs = softmax_f32(logits[:, :, 1:])
            out["clouds"].append(cloud_inds)
            out["inds"].append(point_inds)
            out["fed"].append(pts)
            out["logits"].append(logits)
            for b in range(stacked_probs.shape[0]):
                probs = stacked_probs[b]
                predictions += [probs]
                targets += [labels[b]]
        Confs, C = crop_confusions(predictions, targets, self.label_values, self.ignored_labels, nc_tot)
        out["Confs"] = np.sum(Confs, axis=0)
        C = drop_ignored(C, self.label_values, self.ignored_labels)
        IoUs = iou_from_confusions(C)
        mIoU = 100 * np.mean(IoUs)
        log.append(class_lines(IoUs, seg_label_to_cat, self.NUM_CLASSES))
        log.append('Eval point avg class IoU: %.3f' % (mIoU))
        out.update(mIoU=mIoU, log=log)
        return out


def report_lines(log):
    """what the evaluators' `report` returns: the log without the two section headers"""
    return [l for l in log if not l.startswith('---- ')]
