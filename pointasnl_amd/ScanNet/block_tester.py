"""ScanNet's two training-time validation loops on the device -- reference ScanNet/scannet_dataset.py (D) :31-64
(`ScannetDataset.__getitem__`: a 1.5 m column round a drawn centre, up to ten tries until 70 % of it is labelled and 2 % of a
31x31x62 voxel grid is occupied, resampled to `block_points` rows) and :92-129 (`ScannetDatasetWholeScene.__getitem__`: every
non-empty column of a non-overlapping 1.5 m grid, resampled likewise), ScanNet/train_scannet.py (T) :279-329
(`eval_one_epoch`) and :333-420 (`eval_whole_scene_one_epoch`), utils/provider.py (P) :8-24 and :71-89.  They are the loops
`train_scannet.py` runs after every epoch of `pointasnl_sem_seg` to pick the checkpoint; both are inference.

`BlockTester` keeps every scene on the device and runs both loops crop for crop under the caller's numpy RNG stream
(csrc/block_test.hip):

  chopped, per try:  host rng.choice(n, 1)          -> pasnl_block_crop_stats            -> four integers read back
           per item: host rng.choice(m, P)          -> pasnl_block_fill, pasnl_block_gather (into the batch's row)
           per batch: host B x rng.uniform()        -> pasnl_block_normalize (+ rotation) -> forward -> pasnl_block_score
  whole,   per scene: pasnl_block_grid_count        -> the columns' counts read back
                      host rng.choice(count, P) per non-empty column -> pasnl_block_fill, pasnl_block_gather
           per batch: pasnl_block_normalize -> forward -> pasnl_block_score

The readback per try cannot be avoided: the next draw is `rng.choice(m, P)`, and a legacy RandomState consumes its stream
differently for different m.  Between a batch's draws and its score there is no other host synchronisation; the counters
come down once, at the end of the epoch.  The carry-over of rows between whole scenes is decided on the host over row counts
only; the rows stay on the device.

Deviations: scenes are arrays, not pickles; nothing is written (no log file, no TensorBoard summary) -- `report` returns the
lines; the classify loss is computed here (a float32 log-sum-exp per entry, float64 sums in a fixed order), not by
TensorFlow, and is compared under a tolerance, never by bits; the model's other loss terms enter `mean_loss(extra)` as a
number.  A class whose IoU denominator is zero reports nan (see `report`).  Coordinates must be finite; a scene with zero z
extent raises ValueError in the chopped loop (the reference divides by zero in the voxel index there), and one whose voxel
keys would span more than the bitmap holds (a z extent below a few micrometres) raises PasnlUnsupported.  With rgb the
reference's whole-scene loop fails after a batch of exactly BATCH_SIZE rows (T:372 resets the carried rows to 3 columns);
here the loop goes on.
"""
import ctypes
import math

import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.block_loop import BlockLoop

_p = _hip.ptr
TRIES = 10  # D:40


def key_span(zext):
    """The voxel keys a try can produce, from the z extent the crop divides by (float64(coordmax_z) - float64(coordmin_z)):
    vx, vy lie in [0, 32] whatever the centre (the 0.01 margin against the 1.5 m side); vz = ceil((z - zmin) / zext * 62) for
    z in [zmin - 0.01, zmax + 0.01], the mask's range -- negative below zmin, and large once zext is small against the
    margin.  One cell of slack on every side.  -> key_lo, span (Python ints)."""
    if not zext > 0.0:
        raise ValueError("zero z extent: the reference divides by zero in the voxel index (D:53)")
    vz_lo = math.floor(-0.01 / zext * 62.0) - 1
    vz_hi = math.ceil((zext + 0.01) / zext * 62.0) + 1
    key_lo = -1 * 31 * 62 - 1 * 62 + vz_lo
    key_hi = 33 * 31 * 62 + 33 * 62 + vz_hi
    return key_lo, key_hi - key_lo + 1


class BlockTester(BlockLoop):
    """`BlockTester(scenes, labels, colors=None, num_classes=21, block_points=8192, batch_size=8, labelweights=None,
    rng=np.random)`.

    scenes: a list of (n_i, 3) float32 arrays (numpy or device tensors), or (n_i, 6) with rgb in columns 3..5; colors: the
    rgb as a list of (n_i, 3) arrays instead.  With rgb the rows are 6 wide (the reference's with_rgb).  labels: the
    reference's semantic_labels_list, values in [0, num_classes).  labelweights: (num_classes,) float64, default ones
    (split='val').  rng: np.random or a RandomState."""

    def __init__(self, scenes, labels, colors=None, num_classes=21, block_points=8192, batch_size=8, labelweights=None, rng=np.random):
        _hip.require_device()
        self.S, self.C, self.P, self.B, self.rng = len(scenes), int(num_classes), int(block_points), int(batch_size), rng
        if self.S < 1 or self.C < 2 or self.P < 1 or self.B < 1:
            raise ValueError("at least one scene, two classes, one point per row and one row per batch")
        if len(labels) != self.S or (colors is not None and len(colors) != self.S):
            raise ValueError("one label array (and one colour array) per scene")
        self.xyz, self.rgb, self.labels, self.sizes = [], [], [], []
        for i, s in enumerate(scenes):
            t = _hip.as_dev(s, torch.float32)
            if t.dim() != 2 or t.shape[1] not in (3, 6) or t.shape[0] < 1 or (colors is not None and t.shape[1] != 3):
                raise ValueError(f"scene {i} must be (N, 3), or (N, 6) with rgb and no `colors`, with N >= 1")
            n = int(t.shape[0])
            self.sizes.append(n)
            self.xyz.append(t[:, 0:3].contiguous())
            if colors is not None:
                c = _hip.as_dev(colors[i], torch.float32)
                if tuple(c.shape) != (n, 3):
                    raise ValueError(f"colors[{i}] must be ({n}, 3)")
                self.rgb.append(c)
            else:
                self.rgb.append(t[:, 3:6].contiguous() if t.shape[1] == 6 else None)
            lab = (labels[i].cpu().numpy() if isinstance(labels[i], torch.Tensor) else np.asarray(labels[i])).reshape(-1)
            if lab.shape[0] != n or lab.min() < 0 or lab.max() >= self.C:
                raise ValueError(f"labels[{i}] must hold {n} values in [0, {self.C})")
            self.labels.append(_hip.as_dev(lab.astype(np.int32), torch.int32))
        self.with_rgb = self.rgb[0] is not None
        if any((r is not None) != self.with_rgb for r in self.rgb):
            raise ValueError("either every scene has rgb or none has")
        self.device = self.xyz[0].device
        self.width = 6 if self.with_rgb else 3
        lw = np.ones(self.C) if labelweights is None else np.asarray(labelweights, np.float64).reshape(-1)
        if lw.shape[0] != self.C:
            raise ValueError(f"labelweights must hold {self.C} values")
        self.labelweights = _hip.as_dev(lw, torch.float64)
        dev = self.device
        self.bounds = torch.zeros((self.S, 6), dtype=torch.float32, device=dev)
        for i in range(self.S):  # D:37-38 / D:98-99, once: a scene never moves
            _hip.launch("pasnl_window_bounds", "BlockTester bounds", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]), _p(self.bounds, i * 24))
        self.bounds_host = self.bounds.cpu().numpy()
        if not np.all(np.isfinite(self.bounds_host)):
            raise ValueError("coordinates must be finite")
        self.key_capacity = int(_hip.lib().pasnl_block_key_capacity())
        self.bitmap = torch.zeros((1 + self.key_capacity // 32,), dtype=torch.int32, device=dev)
        self.stats = torch.zeros((4,), dtype=torch.int32, device=dev)
        self.zero = torch.zeros((1,), dtype=torch.int32, device=dev)  # woff of the chopped column
        self.raw = torch.zeros((self.B, self.P, self.width), dtype=torch.float32, device=dev)
        self.batch = torch.zeros((self.B, self.P, self.width), dtype=torch.float32, device=dev)
        self.batch_label = torch.zeros((self.B, self.P), dtype=torch.int32, device=dev)
        self.batch_smpw = torch.zeros((self.B, self.P), dtype=torch.float32, device=dev)
        self.counters = torch.zeros((2 + 4 * self.C,), dtype=torch.int64, device=dev)
        self.loss = torch.zeros((2,), dtype=torch.float64, device=dev)
        self.workspace = torch.zeros((int(_hip.lib().pasnl_block_score_workspace_bytes()),), dtype=torch.uint8, device=dev)
        self.reset()

    def _hist(self, i, nx, ny):
        nbytes = int(_hip.lib().pasnl_window_hist_bytes(ctypes.c_long(self.sizes[i]), nx, ny))
        if nbytes == 0:
            raise _hip.PasnlUnsupported(f"{nx} x {ny} columns: their positions do not fit an int32")
        return torch.empty((nbytes // 4,), dtype=torch.int32, device=self.device)

    # ---- chopped scenes (D:31-64)
    def crop_stats(self, i, centre, bounds=None):
        """One try (D:42-55) round point `centre` of scene i -> (m, labelled, nuniq, hist): len(cur_semantic_seg),
        np.sum(cur_semantic_seg > 0), len(np.unique(keys)) read back together, and the scanned chunk histogram
        pasnl_block_fill reads.  bounds: six device floats in place of the scene's coordmin / coordmax."""
        b = self.bounds[i] if bounds is None else _hip.as_dev(bounds, torch.float32)
        bh = self.bounds_host[i] if bounds is None else b.cpu().numpy()
        key_lo, span = key_span(float(np.float64(bh[5]) - np.float64(bh[2])))
        if span > self.key_capacity:
            raise _hip.PasnlUnsupported(f"the voxel keys span {span} values: the bitmap holds {self.key_capacity}")
        hist = self._hist(i, 2, 1)
        _hip.launch("pasnl_block_crop_stats", "BlockTester crop statistics", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]),
                    _p(self.labels[i]), _p(b), ctypes.c_long(int(centre)), ctypes.c_longlong(key_lo), ctypes.c_long(span), _p(hist),
                    _p(self.bitmap), _p(self.stats))
        m, labelled, nuniq, flag = (int(v) for v in self.stats.cpu().numpy())
        if flag:
            raise _hip.PasnlError("a voxel key outside the span computed from the extents (non-finite coordinates?)")
        return m, labelled, nuniq, hist

    def draw_crop(self, i):
        """The rejection loop (D:40-57) -> centre, m, hist of the try that is kept, and the number of tries"""
        n = self.sizes[i]
        for t in range(TRIES):
            centre = int(self.rng.choice(n, 1)[0])
            m, labelled, nuniq, hist = self.crop_stats(i, centre)
            if m == 0:
                raise ValueError(f"scene {i}: point {centre} is not in its own column (coordinates must be finite)")
            if labelled / m >= 0.7 and nuniq / 31.0 / 31.0 / 62.0 >= 0.02:
                break
        return centre, m, hist, t + 1

    def _rows(self, i, centre, nx, ny, hist, woff, cap, rowpos, rowbase, data, seg, smpw, row0=0):
        """member lists, then rows: rowpos (rows*P,) positions -> rows row0.. of data / seg / smpw (rowbase: not needed here)"""
        cat_idx = torch.empty((cap,), dtype=torch.int32, device=self.device)
        cat_mask = torch.empty((cap,), dtype=torch.uint8, device=self.device)
        n = ctypes.c_long(self.sizes[i])
        _hip.launch("pasnl_block_fill", "BlockTester fill", n, _p(self.xyz[i]), _p(self.bounds[i]), ctypes.c_long(centre), nx, ny, _p(hist),
                    _p(woff), ctypes.c_long(cap), _p(cat_idx), _p(cat_mask))
        pos = torch.from_numpy(np.ascontiguousarray(rowpos, dtype=np.int32)).to(self.device)
        rows = pos.shape[0] // self.P
        _hip.launch("pasnl_block_gather", "BlockTester gather", rows, self.P, _p(pos), ctypes.c_long(cap), _p(cat_idx), _p(cat_mask), n,
                    _p(self.xyz[i]), _p(self.rgb[i]) if self.with_rgb else ctypes.c_void_p(0), 3 if self.with_rgb else 0,
                    _p(self.labels[i]), self.C, _p(self.labelweights), _p(data, row0 * self.P * self.width * 4),
                    _p(seg, row0 * self.P * 4), _p(smpw, row0 * self.P * 4))

    # ---- whole scenes (D:92-129)
    def grid(self, i):
        """D:100-101 through numpy on the read-back float32 bounds, the reference's own expression -> nx, ny"""
        coordmin, coordmax = self.bounds_host[i, 0:3], self.bounds_host[i, 3:6]
        nx = int(np.ceil((coordmax[0] - coordmin[0]) / 1.5).astype(np.int32))
        ny = int(np.ceil((coordmax[1] - coordmin[1]) / 1.5).astype(np.int32))
        if nx < 1 or ny < 1:
            raise ValueError(f"scene {i} has zero extent in x or y: the reference finds no column")
        return nx, ny

    def column_counts(self, i):
        """D:105-113, counted in one launch -> (nx, ny), counts (nx*ny,) int64 (the one readback of a scene), hist"""
        nx, ny = self.grid(i)
        hist = self._hist(i, nx, ny)
        counts = torch.empty((nx * ny,), dtype=torch.int32, device=self.device)
        _hip.launch("pasnl_block_grid_count", "BlockTester count", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]), _p(self.bounds[i]), nx, ny,
                    _p(hist), _p(counts))
        return (nx, ny), counts.cpu().numpy().astype(np.int64), hist

    def scene_blocks(self, i):
        """One `ScannetDatasetWholeScene.__getitem__(i)` (D:92-129) on the device -> device tensors data (R,P,3|6) f32, seg
        (R,P) i32, smpw (R,P) f32"""
        return self._whole_item(i)

    # ---- the loops
    def normalize(self, src, rows, angles=None):
        """normalize_data (P:8-24) of the first `rows` blocks of src (>= rows,P,3|6) into the persistent batch, then -- with
        angles -- rotate_point_cloud_z (P:71-89) on the float64 result.  -> the batch (B,P,3|6) f32"""
        rot = None
        if angles is not None:
            rot = _hip.as_dev(np.stack([np.cos(angles), np.sin(angles)], axis=1).astype(np.float64), torch.float64)
        _hip.launch("pasnl_block_normalize", "BlockTester normalize", rows, self.P, self.width, _p(src), _hip.ptr(rot), _p(self.batch))
        return self.batch

    def run_chopped(self, forward):
        """T:279-329, one epoch over randomly chopped scenes: scenes in index order, S // B batches (the remainder is
        dropped, as in the reference); a batch draws its B items, then its B rotation angles.  forward: (B,P,3|6) f32 device
        tensor -> (B,P,C) f32 logits.  -> mIoU."""
        self.reset()
        num_batches = int(self.S / self.B)
        for b in range(num_batches):
            for k in range(self.B):
                self._item_into(b * self.B + k, self.raw, self.batch_label, self.batch_smpw, k)
            angles = [self.rng.uniform() * 2 * np.pi for _ in range(self.B)]
            self.score(forward(self.normalize(self.raw, self.B, angles)), self.batch_label, self.batch_smpw)
        return self._finish(num_batches, False)

    def _whole_batch(self, data):
        return self.normalize(data, self.B)  # T:333-420 feeds the whole scenes' rows normalized and unrotated
