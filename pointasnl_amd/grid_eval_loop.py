"""What the two grid evaluators share on the host (ScanNet/scene_evaluator.py, SemanticKITTI/scan_evaluator.py):
`eval_one_epoch` of ScanNet/train_scannet_grid.py (S) :304-434 and SemanticKITTI/train_semantic_kitti_grid.py (K) :265-330
both stack every crop's probabilities and truth, build one sklearn confusion matrix per crop (S:359-366, K:301-308), sum
them, drop the ignored labels and take `IoU_from_confusions`.  Here the sum is one (nl,nl) int64 matrix on the device that
`pasnl_scan_eval_confusion` adds a whole batch to in one launch; it comes down once per epoch, and the float32 lines that
follow (S:368-380, K:310-319) are evaluated in numpy on the host as the reference writes them.

A class built on `GridEvalLoop` supplies B, P (= num_point), C, device, and for `_gather_labels` offsets and labels.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.ScanNet.scene_tester import SceneTester, iou_from_confusions
from pointasnl_amd.grid_train_loop import GridTrainLoop

_p = _hip.ptr


class GridEvalLoop:
    # the generator's pieces the evaluators share with the trainers
    _init_augment = GridTrainLoop._init_augment
    _stage_item = GridTrainLoop._stage_item
    _augment = GridTrainLoop._augment
    _gather_labels = GridTrainLoop._gather_labels
    drop_ignored = SceneTester.drop_ignored  # S:370-374, K:312-316: the rows and columns of the ignored labels removed

    def _init_eval(self, num_classes, label_values, ignored_labels):
        """the label set and the device matrix: the model gives C = num_classes logits, the tables hold nc = C - 1 columns
        (S:310, 318; K:268) and nc + the number of ignored labels == len(label_values)"""
        self.C = int(num_classes)
        self.label_values = np.arange(self.C, dtype=np.int32) if label_values is None else np.asarray(label_values, np.int32).reshape(-1)
        self.ignored_labels = tuple(int(v) for v in ignored_labels)
        self.ignored_mask = np.ascontiguousarray(np.isin(self.label_values, self.ignored_labels).astype(np.int32))
        self.L, self.nc = int(self.label_values.size), self.C - 1
        if len(set(self.label_values.tolist())) != self.L:
            raise ValueError("label_values must be distinct")
        if self.nc < 1 or self.nc + int(self.ignored_mask.sum()) != self.L:
            raise ValueError(f"num_classes - 1 = {self.nc} table columns + {int(self.ignored_mask.sum())} ignored labels != "
                             f"{self.L} label values")
        if self.L > 64:
            raise _hip.PasnlUnsupported(f"{self.L} label values > 64 (pasnl_scan_eval_confusion)")
        self.ignored_ptr = self.ignored_mask.ctypes.data_as(ctypes.c_void_p)  # host memory: the entry reads it at the call

    def _init_confusion(self):
        self.confusion_dev = torch.zeros((self.L, self.L), dtype=torch.int64, device=self.device)
        self.scored, self._C = 0, None

    def reset(self):
        """clears the device matrix (an epoch starts with it)"""
        self.confusion_dev.zero_()
        self.scored, self._C = 0, None

    def score(self, logits, labels, is_logits=True):
        """S:359-366 / K:301-308 for one batch, added to the device matrix: logits (B,P,C) f32 -- the prediction is the argmax
        of softmax(logits[..., 1:]) with a zero column per ignored label -- or, is_logits=False, probabilities (B,P,C-1);
        labels (B,P) i32 class indices (one outside [0, nl) is dropped).  One launch, no host synchronisation."""
        width = self.C if is_logits else self.nc
        v = _hip.as_dev(logits, torch.float32)
        if v.numel() != self.B * self.P * width or v.shape[-1] != width:
            raise ValueError(f"the model must return ({self.B}, {self.P}, {width}) values")
        t = _hip.as_dev(labels, torch.int32)
        if t.numel() != self.B * self.P:
            raise ValueError(f"labels must be ({self.B}, {self.P})")
        _hip.launch("pasnl_scan_eval_confusion", type(self).__name__ + " score", self.B, self.P, self.nc, _p(v), 1 if is_logits else 0,
                    _p(t), self.ignored_ptr, self.L, _p(self.confusion_dev))
        self.scored += 1

    def confusion(self):
        """the (nl,nl) int64 sum of the epoch's per-crop confusions, rows the truth: the epoch's single read-back"""
        if self._C is None:
            self._C = self.confusion_dev.cpu().numpy()
        return self._C

    @staticmethod
    def iou_from_confusions(C):
        """utils/metrics.py:120-146 in the dtype of C"""
        return iou_from_confusions(C)

    @staticmethod
    def class_lines(ious, seg_label_to_cat, num_classes):
        """S:424-428 / K:321-325: the per-class block both scripts log as one string"""
        s = "------- IoU --------\n"
        for l in range(1, num_classes):
            s += "class %s IoU: %.3f \n" % (seg_label_to_cat[l] + " " * (14 - len(seg_label_to_cat[l])), 100 * ious[l - 1])
        return s
