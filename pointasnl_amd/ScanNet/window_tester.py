"""The ScanNet sliding-window whole-scene test loop on the device -- reference ScanNet/scannet_dataset.py (D) :135-300
(`ScannetDatasetWholeSceneSlidingWindow.__getitem__`: the noise step, the 1.5 m windows at `stride`, the merge of small
blocks, the division into rows of `block_points`) and ScanNet/test_scannet.py (T) :96-196 (`add_vote`, `eval_one_epoch`:
argmax over classes 1..C-1, integer votes, per-class counts, IoU, the exported labels).  It is the loop that evaluates
`pointasnl_sem_seg`; the grid loop of `pointasnl_sem_seg_res` is scene_tester.py.

`WindowTester` keeps every scene's xyz as a float32 device buffer that ACCUMULATES the noise step's moves, as the reference's
`point_set_ini` aliases `scene_points_list[index]`: every vote moves a fifth of the scene's points for good.  One vote of one
scene runs block for block under the caller's numpy RNG stream (csrc/window_test.hip):

  host: rng.choice, rng.randn            -> pasnl_window_noise, pasnl_window_bounds  -> six bounds read back
  host: nsubvolume_x / _y                -> pasnl_window_count                       -> per-window counts read back
  host: merge (counts and centres only), rng.shuffle per block -> positions uploaded -> pasnl_window_fill
  per batch, with no synchronisation: pasnl_window_gather -> forward -> pasnl_window_vote

No other per-point data travels down, and only the noise draws, the permutations and one offset per window travel up.

Machine dependence: the merge picks the nearest remaining block with `np.argsort(dist)[0]`, called exactly so.  Window
centres sit on a lattice of `stride`, so equal nearest distances are the rule, and which of them numpy's unstable sort
lists first depends on its sort kernel for the CPU at hand.  Calling the same function on the same array is what agrees with
the reference ON THE SAME MACHINE; across machines the blocks (and everything after them) may differ, here as there.

Deviations: the rows past the last real one of a scene's final batch are fed zeros (the reference leaves stale rows there
and never votes them); split='train' is refused (its label weights can be inf or nan); no file is written -- `export`
returns the array the reference writes line by line.  Coordinates must be finite.

The host steps shared with the SemanticKITTI loop are `WindowLoop`'s (window_loop.py); in this reference they are grid
D:214-217, count D:223-233, fill D:229-241, centers D:225-226 and 242, merged D:232-233, merge_blocks D:244-269 with
nearest_block_literal D:176-181, draw_rows D:281-287 (a make-up longer than its block pads short, as the reference's slice
does), blocks D:183-300, vote T:159-161, run T:122-180, score T:163-170, class_iou T:189.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from pointasnl_amd import _hip, window_loop
from pointasnl_amd.window_loop import WindowLoop, nearest_block_literal

_p = _hip.ptr
TEST_CLASS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])  # T:105
nearest_block = nearest_block_literal  # D:176-181: a few dozen windows, the reference's own loop
merge_blocks = functools.partial(window_loop.merge_blocks, nearest=nearest_block)  # D:244-269; centres as a list or (m,2)


class WindowTester(WindowLoop):
    """`WindowTester(scenes, labels=labels, num_classes=21, block_points=8192, batch_size=6, stride=0.5, with_rgb=True,
    noise_ratio=0.2, min_block_points=4096, rng=np.random)`.

    scenes: a list of (n_i, 3) or (n_i, 6) float32 arrays (numpy or device tensors; xyz, then rgb), the reference's
    scene_points_list -- copied to the device, the caller's arrays are not touched (the drop-in dataset class writes the
    moves back).  labels: the reference's semantic_labels_list, values in [0, num_classes) (None: zeros).  rng: np.random
    or a RandomState; `blocks(i)` draws rng.choice(n, ceil(noise_ratio * n)), rng.randn(that, 3), then per block
    rng.shuffle (when its length is no multiple of block_points) and rng.shuffle again."""
    ITEM, ENTRY, SCALARS, MASKED, PAD_SHORT = "scene", "pasnl_window", ("stride",), True, True
    block_size, scored, nearest = 1.5, True, staticmethod(nearest_block_literal)  # D:226; labelweights are ones; D:176-181

    def __init__(self, scenes, labels=None, num_classes=21, block_points=8192, batch_size=6, stride=0.5, with_rgb=True,
                 noise_ratio=0.2, min_block_points=4096, rng=np.random, split="test"):
        if split == "train":
            raise NotImplementedError("split='train' weights rows by (max / frequency)^(1/3), which is inf or nan for an "
                                      "absent class; WindowTester covers the splits whose labelweights are ones")
        _hip.require_device()
        self.S, self.C, self.P, self.B = len(scenes), int(num_classes), int(block_points), int(batch_size)
        self.stride, self.with_rgb, self.noise_ratio = float(stride), bool(with_rgb), float(noise_ratio)
        self.min_block_points, self.rng = int(min_block_points), rng
        if self.S < 1 or self.C < 2 or self.P < 1 or self.B < 1 or not self.stride > 0:
            raise ValueError("at least one scene, two classes, one point per row, one row per batch and a positive stride")
        if labels is not None and len(labels) != self.S:
            raise ValueError("one label array per scene")
        self.xyz, self.rgb, self.labels, self.stamp, self.sizes = [], [], [], [], []
        for i, s in enumerate(scenes):
            t = _hip.as_dev(s, torch.float32)
            if t.dim() != 2 or t.shape[1] not in (3, 6) or t.shape[0] < 1 or (self.with_rgb and t.shape[1] != 6):
                raise ValueError(f"scene {i} must be (N, 6), or (N, 3) without rgb, with N >= 1")
            n = int(t.shape[0])
            self.sizes.append(n)
            self.xyz.append(t[:, 0:3].contiguous().clone())
            self.rgb.append(t[:, 3:6].contiguous() if self.with_rgb else None)
            if labels is None:
                lab = np.zeros(n, np.int32)
            else:
                lab = (labels[i].cpu().numpy() if isinstance(labels[i], torch.Tensor) else np.asarray(labels[i])).reshape(-1)
                if lab.shape[0] != n or (n and (lab.min() < 0 or lab.max() >= self.C)):
                    raise ValueError(f"labels[{i}] must hold {n} values in [0, {self.C})")
            self.labels.append(_hip.as_dev(lab.astype(np.int32), torch.int32))
            self.stamp.append(torch.zeros((n,), dtype=torch.int32, device=t.device))
        self.device = self.xyz[0].device
        self.width = 6 if self.with_rgb else 3
        self.serial = 0  # one per noise step; a label reads 0 while its stamp equals the step's serial
        self.stats = torch.zeros((4,), dtype=torch.float32, device=self.device)
        self.bounds = torch.zeros((6,), dtype=torch.float32, device=self.device)
        self.class_values = torch.arange(self.C, dtype=torch.int32, device=self.device)
        self.pools, self.preds, self.counts = {}, {}, {}
        self.total = np.zeros((3, self.C), np.int64)

    # ---- one __getitem__, step by step
    def move(self, i):
        """Step 1 (D:192-212): draw on the host, move on the device.  -> the step's serial."""
        n = self.sizes[i]
        num_noise = math.ceil(n * self.noise_ratio)
        choices = self.rng.choice(n, num_noise)
        shift = (self.rng.randn(num_noise, 3) - 0.5) / 0.5 * 0.002
        slot = np.full(n, -1, np.int64)
        slot[choices] = np.arange(num_noise)  # a repeated index keeps its last draw
        last = (slot[choices] == np.arange(num_noise)).astype(np.uint8)
        self.serial += 1
        null = ctypes.c_void_p(0)
        held = [_hip.as_dev(a, dt) for a, dt in ((choices.astype(np.int32), torch.int32), (shift, torch.float64), (last, torch.uint8))]
        draws = [null] * 3 if num_noise == 0 else [_p(t) for t in held]  # (held: alive until the launch is enqueued)
        _hip.launch("pasnl_window_noise", "WindowTester noise", ctypes.c_long(n), _p(self.xyz[i]), num_noise, *draws,
                    self.serial, _p(self.stamp[i]), _p(self.stats))
        return self.serial

    def merged(self, counts):
        return np.flatnonzero(counts > 0)  # D:232-233: empty windows are skipped

    def prepare(self, i):
        """Steps 1-4 up to the gather: the move, then WindowLoop.prepare with the step's `serial` added."""
        serial = self.move(i)
        return dict(WindowLoop.prepare(self, i), serial=serial)

    def _buffers(self, rows):
        return (torch.empty((rows, self.P, self.width), dtype=torch.float32, device=self.device),) + tuple(
            torch.empty((rows, self.P), dtype=torch.int32, device=self.device) for _ in range(3))

    def gather(self, i, prep, start, rows, out=None):
        """D:289-300 for rows [start, start + rows) of the prepared vote; rows past the last one come out as zeros.
        -> data (rows,P,3|6) f32, labels, weights (0/1), indices (rows,P) i32, device tensors."""
        data, lab, wgt, idx = self._buffers(rows) if out is None else out
        real = max(0, min(rows, prep["rows"] - start))
        _hip.launch("pasnl_window_gather", "WindowTester gather", rows, real, self.P, _p(prep["rowpos"], start * self.P * 4),
                    ctypes.c_long(prep["cap"]), _p(prep["cat_idx"]), _p(prep["cat_mask"]), ctypes.c_long(self.sizes[i]), _p(self.xyz[i]),
                    _p(self.rgb[i]) if self.with_rgb else ctypes.c_void_p(0), 3 if self.with_rgb else 0, _p(self.labels[i]),
                    _p(self.stamp[i]), prep["serial"], _p(data), _p(lab), _p(wgt), _p(idx))
        return data, lab, wgt, idx

    def _batch(self, i, prep, start, out):
        data, _, wgt, idx = self.gather(i, prep, start, self.B, out)
        return data, idx, wgt

    def deno(self, m, seen, correct):
        """T:170: ((pred == l) | (label == l)) & (label > 0)"""
        labelled = m[1:].sum(axis=0)  # predictions of l among the points with label > 0
        return labelled + np.where(np.arange(self.C) > 0, seen - correct, 0)

    # ---- state and results
    def points(self, i):
        """scene i's xyz as moved so far, (n_i, 3) f32 device tensor"""
        return self.xyz[i]

    def scene_counts(self, i):
        """-> seen, correct, iou_deno of scene i, (C,) int64 each (T:168-170)"""
        return tuple(self.counts[i])

    def scene_iou(self, i):
        """T:172-175 -> iou_map (C,) f64 and its mean over the classes the scene holds"""
        seen, correct, deno = self.scene_counts(i)
        iou_map = np.array(correct) / (np.array(deno, dtype=float) + 1e-6)
        return iou_map, np.mean(iou_map[np.array(seen) != 0])

    def export(self, i, scene_points_id, scene_points_num, test_class=TEST_CLASS):
        """T:179-180: whole = zeros(scene_points_num); whole[scene_points_id] = test_class[pred_label] -> (num,) f64 numpy,
        the values the reference writes one per line."""
        lut = torch.from_numpy(np.asarray(test_class)).to(self.device)
        values = lut[self.preds[i].long()].cpu().numpy()
        whole = np.zeros(scene_points_num)
        whole[np.asarray(scene_points_id)] = values
        return whole
