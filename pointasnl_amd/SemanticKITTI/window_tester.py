"""The SemanticKITTI sliding-window whole-scan test loop on the device -- reference SemanticKITTI/semantic_kitti_dataset.py
(D) :217-355 (`SemanticKittiDatasetSlidingWindow.__getitem__`: the `block_size` windows at `stride`, the merge of small
blocks, the division into rows of `block_points`) and SemanticKITTI/test_semantic_kitti.py (T) :99-231 (`add_vote`,
`eval_one_epoch`: the optional rotation about z, argmax over classes 1..C-1, integer votes, the uint32 labels, per-class
counts, IoU).  It is the loop that evaluates `pointasnl_sem_seg` on SemanticKITTI; the grid loop of `pointasnl_sem_seg_res`
is scan_tester.py.

`KittiWindowTester` keeps every scan's xyz (and remission) as float32 device buffers.  One vote of one scan runs under the
caller's numpy RNG stream (csrc/kitti_window_test.hip):

  pasnl_window_bounds                    -> six bounds read back
  host: nsubvolume_x / _y                -> pasnl_kwindow_count                      -> per-window counts read back
  host: merge (counts and centres only), rng.shuffle per block -> positions uploaded -> pasnl_kwindow_fill
  per batch, with no synchronisation: [host: batch_size angles] pasnl_kwindow_gather -> forward -> pasnl_window_vote

No per-point data travels down, and only the permutations, one offset per window and the angles travel up.

The host steps shared with the ScanNet loop are `WindowLoop`'s (window_loop.py); in this reference they are grid D:289-292,
count D:296-302, fill D:300-307, centers D:298-299 and 308, merge_blocks D:311-327 with nearest_block D:271-276, draw_rows
D:337-345, blocks D:289-351, vote T:166 and 171-172, run T:123-216, score T:174-175 and 196-231, class_iou T:219.  What
differs from the ScanNet loop (ScanNet/window_tester.py) is what this file holds: the window is `block_size` wide; a lidar
scan has thousands of windows (no limit per axis) and EVERY window, empty or not, enters the merge (D has no `continue`);
there is no noise step and no 0.001-margin mask (every row entry votes); a remission channel and a rotation about z are
optional; a block that cannot be made up to a multiple of block_points is refused.

The merge (D:311-327) finds each nearest block with ONE batched expression over the remaining centres,
np.sqrt(np.matmul(d[:, None, :], d[:, :, None])[:, 0, 0]) with d = centres - centre, instead of the reference's Python loop
of np.linalg.norm calls (thousands of calls per step, thousands of steps per vote).  Both forms end in the BLAS dot and give
the same bits where that holds; `batched_norm_agrees()` checks it at construction on lattice differences and the tester
falls back to the literal loop, with a warning, if they disagree.

Machine dependence: the merge picks the nearest remaining block with `np.argsort(dist)[0]`, called exactly so.  Window
centres sit on a lattice of `stride`, so equal nearest distances are the rule, and which of them numpy's unstable sort
lists first depends on its sort kernel for the CPU at hand.  Calling the same function on the same array is what agrees with
the reference ON THE SAME MACHINE; across machines the blocks (and everything after them) may differ, here as there.

Deviations: the rows past the last real one of a scan's final batch are fed zeros (the reference leaves stale rows there
and never votes them; with `random_rotate` their angles are still drawn); no file is written -- `label_array` returns the
uint32 array the reference writes with `.tofile`; the `.obj` dumps are left out.  Where the reference crashes (a ragged
chunk in the division, an empty argsort in the merge) a ValueError is raised.  Coordinates must be finite.
"""
import ctypes
import warnings

import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.window_loop import (WindowLoop, batched_norm_agrees, batched_norms, draw_rows, merge_blocks,  # noqa: F401
                                       nearest_block, nearest_block_literal)

_p = _hip.ptr


class KittiWindowTester(WindowLoop):
    """`KittiWindowTester(scans, labels=None, remissions=None, num_classes=20, block_points=8192, batch_size=6, block_size=10,
    stride=4, min_block_points=4096, random_rotate=False, rng=np.random, accumulate_votes=False)`.

    scans: a list of (n_i, 3) float32 arrays (numpy or device tensors), copied to the device.  labels: per scan the mapped
    labels in [0, num_classes) (None: split 'test', nothing is scored).  remissions: per scan (n_i,) float32 (None: rows
    are xyz only).  rng: np.random or a RandomState; `blocks(i)` draws per final block rng.shuffle (when its length is no
    multiple of block_points) and rng.shuffle again, and with random_rotate `run` draws batch_size rng.uniform per batch.

    The pool quirk: the reference clears vote_label_pool at the first batch of EVERY vote (T:168-169), so only the last
    vote of a scan decides its labels.  That is mirrored by default; accumulate_votes=True sums the votes instead."""
    ITEM, ENTRY, SCALARS, MASKED, MAX_WINDOWS = "scan", "pasnl_kwindow", ("block_size", "stride"), False, 2 ** 31

    def __init__(self, scans, labels=None, remissions=None, num_classes=20, block_points=8192, batch_size=6, block_size=10, stride=4,
                 min_block_points=4096, random_rotate=False, rng=np.random, accumulate_votes=False):
        _hip.require_device()
        self.S, self.C, self.P, self.B = len(scans), int(num_classes), int(block_points), int(batch_size)
        self.block_size, self.stride, self.min_block_points = float(block_size), float(stride), int(min_block_points)
        self.random_rotate, self.rng, self.accumulate_votes = bool(random_rotate), rng, bool(accumulate_votes)
        if self.S < 1 or self.C < 2 or self.P < 1 or self.B < 1 or not self.stride > 0 or not self.block_size > 0:
            raise ValueError("at least one scan, two classes, one point per row, one row per batch, a positive block_size and stride")
        for name, per_scan in (("labels", labels), ("remissions", remissions)):
            if per_scan is not None and len(per_scan) != self.S:
                raise ValueError(f"one {name} array per scan")
        self.xyz, self.remission, self.labels, self.sizes = [], [], [], []
        for i, s in enumerate(scans):
            t = _hip.as_dev(s, torch.float32)
            if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
                raise ValueError(f"scan {i} must be (N, 3) with N >= 1")
            n = int(t.shape[0])
            self.sizes.append(n)
            self.xyz.append(t.clone())
            if remissions is not None:
                r = _hip.as_dev(remissions[i], torch.float32).reshape(-1)
                if r.shape[0] != n:
                    raise ValueError(f"remissions[{i}] must hold {n} values")
                self.remission.append(r.clone())
            if labels is not None:
                lab = (labels[i].cpu().numpy() if isinstance(labels[i], torch.Tensor) else np.asarray(labels[i])).reshape(-1)
                if lab.shape[0] != n or lab.min() < 0 or lab.max() >= self.C:
                    raise ValueError(f"labels[{i}] must hold {n} values in [0, {self.C})")
                self.labels.append(_hip.as_dev(lab.astype(np.int32), torch.int32))
        self.device = self.xyz[0].device
        self.nfeat = 1 if remissions is not None else 0
        self.width = 3 + self.nfeat
        self.scored = labels is not None
        self.nearest = nearest_block
        if not batched_norm_agrees(self.stride):
            warnings.warn("the batched distance expression does not reproduce np.linalg.norm bit for bit with this BLAS: the merge "
                          "falls back to the reference's per-centre loop (slow at thousands of windows)")
            self.nearest = nearest_block_literal
        self.bounds = torch.zeros((6,), dtype=torch.float32, device=self.device)
        self.ones = torch.ones((self.B, self.P), dtype=torch.int32, device=self.device)
        self.class_values = torch.arange(self.C, dtype=torch.int32, device=self.device)
        self.pools, self.preds, self.counts, self.logged = {}, {}, {}, {}
        self.total = np.zeros((3, self.C), np.int64)
        self.total_correct, self.total_seen = 0, 0
        self.labelweights = np.zeros(self.C)  # T:121, renormalised in place every tenth scan (T:224)

    # ---- one __getitem__, step by step
    def merged(self, counts):
        return np.arange(len(counts))  # D has no `continue`: every window, empty or not

    def _buffers(self, rows):
        return (torch.empty((rows, self.P, self.width), dtype=torch.float32, device=self.device),
                torch.empty((rows, self.P), dtype=torch.int32, device=self.device))

    def gather(self, i, prep, start, rows, out=None, angles=None):
        """D:347-351 / T:157-161 for rows [start, start + rows) of the prepared vote; rows past the last one come out as
        zeros.  angles: (rows,) float64 host array or None.  -> data (rows,P,3|4) f32, indices (rows,P) i32, device tensors."""
        data, idx = self._buffers(rows) if out is None else out
        real = max(0, min(rows, prep["rows"] - start))
        ang = None if angles is None else _hip.as_dev(np.asarray(angles, np.float64).reshape(rows), torch.float64)
        _hip.launch("pasnl_kwindow_gather", "KittiWindowTester gather", rows, real, self.P, _p(prep["rowpos"], start * self.P * 4),
                    ctypes.c_long(prep["cap"]), _p(prep["cat_idx"]), ctypes.c_long(self.sizes[i]), _p(self.xyz[i]),
                    _p(self.remission[i]) if self.nfeat else ctypes.c_void_p(0), self.nfeat,
                    ctypes.c_void_p(0) if ang is None else _p(ang), _p(data), _p(idx))
        return data, idx

    # ---- the loop
    def begin_vote(self, i, vote):
        if vote > 0 and not self.accumulate_votes:
            self.pools[i].zero_()  # T:168-169: the pool is made anew at the first batch of every vote

    def _batch(self, i, prep, start, out):
        angles = None
        if self.random_rotate:  # T:160-161: one uniform per row of the batch, stale rows included
            angles = np.array([self.rng.uniform() * 2 * np.pi for _ in range(self.B)])
        return self.gather(i, prep, start, self.B, out, angles) + (self.ones,)

    def deno(self, m, seen, correct):
        """T:209: (pred == l) | (label == l)"""
        return m.sum(axis=0) + seen - correct

    def tally(self, i, seen, correct):
        """T:196-202 and, every tenth scan, the logged figures"""
        self.total_correct += int(correct.sum())
        self.total_seen += self.sizes[i]
        self.labelweights += seen  # np.histogram(whole_scene_label, range(C + 1))
        if i % 10 == 0:
            self.logged[i] = self._log_figures()

    def _log_figures(self):
        """T:218-231, with T:224's reassignment of the running `labelweights`"""
        seen, correct, deno = (np.array(t) for t in self.total)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = dict(miou=np.mean(np.array(correct[1:]) / (np.array(deno[1:], dtype=float) + 1e-6)),
                       accuracy=self.total_correct / float(self.total_seen),
                       class_accuracy=np.mean(np.array(correct) / (np.array(seen, dtype=float) + 1e-6)))
            self.labelweights = self.labelweights.astype(np.float32) / np.sum(self.labelweights.astype(np.float32))
            out["labelweights"] = self.labelweights[0:self.C - 1].copy()  # 'weight' of class l is labelweights[l - 1]
            out["iou"] = correct[1:] / deno[1:].astype(float)
        return out

    # ---- state and results
    def label_array(self, i):
        """T:174-175: final_preds as the (n_i,) uint32 numpy array the reference writes with `.tofile`"""
        return self.preds[i].cpu().numpy().astype(np.uint32)

    def scan_counts(self, i):
        """-> seen, correct, iou_deno of scan i, (C,) int64 each (T:203-211)"""
        return tuple(self.counts[i])

    def scan_iou(self, i):
        """T:212-214 -> iou of classes 1..C-1 (C-1,) f64 and its mean over the classes the scan holds"""
        seen, correct, deno = self.scan_counts(i)
        iou = np.array(correct[1:]) / (np.array(deno[1:], dtype=float) + 1e-6)
        return iou, np.mean(iou[np.array(seen[1:]) != 0])

    def tenth_scan_figures(self, i):
        """what T:218-231 logs after scan i (i % 10 == 0): dict(miou, accuracy, class_accuracy, labelweights (C-1,) f32 as
        renormalised at that scan, iou (C-1,) f64 without the 1e-6)"""
        return self.logged[i]
