"""SemanticKITTI's two training-time validation loops on the device -- reference SemanticKITTI/semantic_kitti_dataset.py (D)
:68-109 (`SemanticKittiDataset.__getitem__`: a `block_size` column round a drawn point, up to ten tries until 70 % of it is
labelled, resampled to `block_points` rows) and :164-211 (`SemanticKittiDataset_whole.__getitem__`: every non-empty column of
a non-overlapping `block_size` grid, resampled likewise), SemanticKITTI/train_semantic_kitti.py (T) :267-328
(`eval_one_epoch`) and :331-418 (`eval_whole_scene_one_epoch`), utils/provider.py (P) :71-89.  They are the loops
`train_semantic_kitti.py` runs after every epoch of `pointasnl_sem_seg` to pick the checkpoint; both are inference.

`KittiBlockTester` keeps every scan on the device and runs both loops crop for crop under the caller's numpy RNG stream
(csrc/kitti_block_test.hip):

  chopped, per try:  host rng.choice(n, 1)          -> pasnl_kblock_crop_stats           -> two integers read back
           per item: host rng.choice(m, P)          -> pasnl_kblock_fill, pasnl_kblock_gather (into the batch's row)
           per batch: host B x rng.uniform()        -> pasnl_kblock_rotate -> forward -> pasnl_block_score
  whole,   per scan: pasnl_kblock_grid_count        -> the columns' counts read back
                     host rng.choice(count, P) per non-empty column -> pasnl_kblock_fill, pasnl_kblock_gather
           per batch: forward -> pasnl_block_score (no rotation, no normalize_data in either loop)

The readback per try cannot be avoided: the next draw is `rng.choice(m, P)`, and a legacy RandomState consumes its stream
differently for different m.  The carry-over of rows between whole scans is decided on the host over row counts only; the rows
stay on the device.

Two behaviours of the reference decide the bits of what is fed and scored, and are reproduced by default
(`reference_quirks=True`), because these loops promise the reference's rows bit for bit:

  * Sample weight.  `label_weights = lut[label]` (D:77) is a per-point array, and `sample_weight = label_weights[semantic_seg]`
    (D:104, D:202) indexes it by label value: smpw[e] = lut[label[seg[e]]] * mask, the weight of the label of scan point
    number seg[e].  A scan with n <= max(label) raises ValueError (the reference raises IndexError).
  * Remission.  The remission column is `self.scan.remissions[choice]` (D:107, D:198): the remission of scan point number
    choice[e], the raw draw, not of member choice[e].

`reference_quirks=False` gives the evident intent: lut[seg[e]] * mask and the members' own remissions.

Deviations: scans are arrays in memory, not files; nothing is written (no log file, no TensorBoard summary) -- `report`
returns the lines; the classify loss is computed here (pasnl_block_score: a float32 log-sum-exp per entry, float64 sums in a
fixed order), not by TensorFlow, and is compared under a tolerance, never by bits; the model's other loss terms enter
`mean_loss(extra)` as a number.  A class whose IoU denominator is zero reports nan.  Coordinates must be finite; a scan with
zero extent in x or y raises ValueError in the whole-scan loop (the reference finds no column and fails in np.concatenate).
With remission the reference's whole-scan loop fails after a batch of exactly BATCH_SIZE rows (T:369 resets the carried rows
to 3 columns); here the loop goes on.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip
from pointasnl_amd.block_loop import BlockLoop

_p = _hip.ptr
TRIES = 10  # D:81


def label_weights_from_content(content):
    """D:54-58 with its dtypes: content {label: frequency} (the reference's `mapped_content`; the caller supplies the table)
    -> (len(content),) float32 = np.power(max(lut[1:]) / lut, 1 / 3.0) on a float32 table"""
    num_keys = len(content.keys())
    lut = np.zeros((num_keys), dtype=np.float32)
    lut[list(content.keys())] = list(content.values())
    return np.power(np.amax(lut[1:]) / lut, 1 / 3.0)


class KittiBlockTester(BlockLoop):
    """`KittiBlockTester(scans, labels, remissions=None, num_classes=20, block_points=8192, batch_size=8, block_size=10,
    padding=0.01, label_weights_lut=None, reference_quirks=True, rng=np.random)`.

    scans: a list of (n_i, 3) float32 arrays (numpy or device tensors), the reference's scan.points; labels: the already
    mapped per-point labels, values in [0, num_classes); remissions: a list of (n_i,) float32 arrays -- the rows are then 4
    wide (the reference's with_remission).  block_size: the column's side as the reference holds it (an int or a float: the
    half side is Python's block_size / 2).  label_weights_lut: (num_classes,) float32, default ones
    (`label_weights_from_content` evaluates the reference's table).  rng: np.random or a RandomState."""

    TABLE_IN_CHOPPED = True  # T:315-325: both loops print the per-class table

    def __init__(self, scans, labels, remissions=None, num_classes=20, block_points=8192, batch_size=8, block_size=10, padding=0.01,
                 label_weights_lut=None, reference_quirks=True, rng=np.random):
        _hip.require_device()
        self.S, self.C, self.P, self.B, self.rng = len(scans), int(num_classes), int(block_points), int(batch_size), rng
        self.block_size, self.padding, self.quirks = block_size, float(padding), bool(reference_quirks)
        if self.S < 1 or self.C < 2 or self.P < 1 or self.B < 1 or not block_size > 0:
            raise ValueError("at least one scan, two classes, one point per row, one row per batch and a positive block_size")
        if len(labels) != self.S or (remissions is not None and len(remissions) != self.S):
            raise ValueError("one label array (and one remission array) per scan")
        self.with_remission = remissions is not None
        self.width = 4 if self.with_remission else 3
        self.xyz, self.rem, self.labels, self.sizes = [], [], [], []
        for i, s in enumerate(scans):
            t = _hip.as_dev(s, torch.float32)
            if t.dim() != 2 or t.shape[1] != 3 or t.shape[0] < 1:
                raise ValueError(f"scan {i} must be (N, 3) with N >= 1")
            if not bool(torch.isfinite(t).all()):  # (once, at construction: the bounds kernel's min / max pass over a NaN)
                raise ValueError(f"scan {i}: coordinates must be finite")
            n = int(t.shape[0])
            self.sizes.append(n)
            self.xyz.append(t)
            if self.with_remission:
                r = _hip.as_dev(remissions[i], torch.float32).reshape(-1)
                if r.shape[0] != n:
                    raise ValueError(f"remissions[{i}] must hold {n} values")
                self.rem.append(r)
            lab = (labels[i].cpu().numpy() if isinstance(labels[i], torch.Tensor) else np.asarray(labels[i])).reshape(-1)
            if lab.shape[0] != n or lab.min() < 0 or lab.max() >= self.C:
                raise ValueError(f"labels[{i}] must hold {n} values in [0, {self.C})")
            if self.quirks and n <= int(lab.max()):
                raise ValueError(f"scan {i} has {n} points and a label {int(lab.max())}: the reference indexes its per-point weights by "
                                 "label value and raises IndexError (reference_quirks=False looks the table up by label)")
            self.labels.append(_hip.as_dev(lab.astype(np.int32), torch.int32))
        self.device = self.xyz[0].device
        lut = np.ones(self.C, np.float32) if label_weights_lut is None else np.asarray(label_weights_lut, np.float32).reshape(-1)
        if lut.shape[0] != self.C:
            raise ValueError(f"label_weights_lut must hold {self.C} values")
        self.label_weights_lut = lut
        self.lut = _hip.as_dev(lut, torch.float32)
        dev = self.device
        self.bounds = torch.zeros((self.S, 6), dtype=torch.float32, device=dev)
        for i in range(self.S):  # D:78-79 / D:174-175, once: a scan never moves
            _hip.launch("pasnl_window_bounds", "KittiBlockTester bounds", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]), _p(self.bounds, i * 24))
        self.bounds_host = self.bounds.cpu().numpy()
        if not np.all(np.isfinite(self.bounds_host)):
            raise ValueError("coordinates must be finite")
        self.half = ctypes.c_double(block_size / 2)  # D:83: Python's block_size / 2
        self.stats = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.zero = torch.zeros((1,), dtype=torch.int32, device=dev)  # woff of the chopped column
        self.batch = torch.zeros((self.B, self.P, self.width), dtype=torch.float32, device=dev)
        self.batch_label = torch.zeros((self.B, self.P), dtype=torch.int32, device=dev)
        self.batch_smpw = torch.zeros((self.B, self.P), dtype=torch.float32, device=dev)
        self.counters = torch.zeros((2 + 4 * self.C,), dtype=torch.int64, device=dev)
        self.loss = torch.zeros((2,), dtype=torch.float64, device=dev)
        self.workspace = torch.zeros((int(_hip.lib().pasnl_block_score_workspace_bytes()),), dtype=torch.uint8, device=dev)
        self.reset()

    # ---- chopped scans (D:68-109)
    def crop_stats(self, i, centre):
        """One try (D:82-97) round point `centre` of scan i -> (m, labelled, hist): len(cur_semantic_seg) and
        np.sum(cur_semantic_seg > 0) read back together, and the scanned chunk histogram pasnl_kblock_fill reads"""
        nbytes = int(_hip.lib().pasnl_window_hist_bytes(ctypes.c_long(self.sizes[i]), 2, 1))
        hist = torch.empty((nbytes // 4,), dtype=torch.int32, device=self.device)
        _hip.launch("pasnl_kblock_crop_stats", "KittiBlockTester crop statistics", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]),
                    _p(self.labels[i]), _p(self.bounds, i * 24), ctypes.c_long(int(centre)), self.half, _p(hist), _p(self.stats))
        m, labelled = (int(v) for v in self.stats.cpu().numpy())
        return m, labelled, hist

    def draw_crop(self, i):
        """The rejection loop (D:81-99) -> centre, m, hist of the try that is kept, and the number of tries"""
        n = self.sizes[i]
        for t in range(TRIES):
            centre = int(self.rng.choice(n, 1)[0])
            m, labelled, hist = self.crop_stats(i, centre)
            if m == 0:
                raise ValueError(f"scan {i}: point {centre} is not in its own column (coordinates must be finite)")
            if labelled / m >= 0.7:
                break
        return centre, m, hist, t + 1

    def _rows(self, i, centre, nx, ny, hist, woff, cap, rowpos, rowbase, data, seg, smpw, row0=0):
        """member lists, then rows: rowpos (rows*P,) positions, rowbase (rows,) -> rows row0.. of data / seg / smpw"""
        cat_idx = torch.empty((cap,), dtype=torch.int32, device=self.device)
        cat_mask = torch.empty((cap,), dtype=torch.uint8, device=self.device)
        n = ctypes.c_long(self.sizes[i])
        _hip.launch("pasnl_kblock_fill", "KittiBlockTester fill", n, _p(self.xyz[i]), _p(self.bounds, i * 24), ctypes.c_long(centre), self.half,
                    nx, ny, ctypes.c_double(self.block_size), ctypes.c_double(self.padding), _p(hist), _p(woff), ctypes.c_long(cap),
                    _p(cat_idx), _p(cat_mask))
        pos = torch.from_numpy(np.ascontiguousarray(rowpos, dtype=np.int32)).to(self.device)
        base = torch.from_numpy(np.ascontiguousarray(rowbase, dtype=np.int32)).to(self.device)
        rows = pos.shape[0] // self.P
        _hip.launch("pasnl_kblock_gather", "KittiBlockTester gather", rows, self.P, _p(pos), _p(base), ctypes.c_long(cap), _p(cat_idx),
                    _p(cat_mask), n, _p(self.xyz[i]), _p(self.rem[i]) if self.with_remission else ctypes.c_void_p(0),
                    1 if self.with_remission else 0, _p(self.labels[i]), self.C, _p(self.lut), 1 if self.quirks else 0,
                    _p(data, row0 * self.P * self.width * 4), _p(seg, row0 * self.P * 4), _p(smpw, row0 * self.P * 4))

    # ---- whole scans (D:164-211)
    def grid(self, i):
        """D:177-178 through numpy on the read-back float32 bounds, the reference's own expression -> nx, ny"""
        coordmin, coordmax = self.bounds_host[i, 0:3], self.bounds_host[i, 3:6]
        nx = int(np.ceil((coordmax[0] - coordmin[0]) / self.block_size).astype(np.int32))
        ny = int(np.ceil((coordmax[1] - coordmin[1]) / self.block_size).astype(np.int32))
        if nx < 1 or ny < 1:
            raise ValueError(f"scan {i} has zero extent in x or y: the reference finds no column")
        return nx, ny

    def column_counts(self, i):
        """D:182-192, counted in one call -> (nx, ny), counts (nx*ny,) int64 (the one readback of a scan), hist"""
        nx, ny = self.grid(i)
        nbytes = int(_hip.lib().pasnl_kwindow_hist_bytes(ctypes.c_long(self.sizes[i]), nx, ny))
        if nbytes == 0:
            raise _hip.PasnlUnsupported(f"{nx} x {ny} columns: their positions do not fit an int32")
        hist = torch.empty((nbytes // 4,), dtype=torch.int32, device=self.device)
        counts = torch.empty((nx * ny,), dtype=torch.int32, device=self.device)
        _hip.launch("pasnl_kblock_grid_count", "KittiBlockTester count", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]), _p(self.bounds, i * 24),
                    nx, ny, ctypes.c_double(self.block_size), _p(hist), _p(counts))
        return (nx, ny), counts.cpu().numpy().astype(np.int64), hist

    def scan_blocks(self, i):
        """One `SemanticKittiDataset_whole.__getitem__(i)` (D:164-211) on the device -> device tensors data (R,P,3|4) f32, seg
        (R,P) i32, smpw (R,P) f32"""
        return self._whole_item(i)

    # ---- the loops
    def rotate(self, src, rows, angles, out=None):
        """rotate_point_cloud_z (P:71-89) of the first `rows` blocks of src (>= rows,P,3|4) with the host's angles, as T:290
        applies it to the float64 batch.  -> out (default: in place)"""
        rot = _hip.as_dev(np.stack([np.cos(angles), np.sin(angles)], axis=1).astype(np.float64), torch.float64)
        out = src if out is None else out
        _hip.launch("pasnl_kblock_rotate", "KittiBlockTester rotate", rows, self.P, self.width, _p(src), _p(rot), _p(out))
        return out

    def run_chopped(self, forward):
        """T:267-328, one epoch over randomly chopped scans: scans in index order, S // B batches (the remainder is dropped,
        as in the reference); a batch draws its B items, then its B rotation angles.  forward: (B,P,3|4) f32 device tensor ->
        (B,P,C) f32 logits.  -> mIoU."""
        self.reset()
        num_batches = int(self.S / self.B)
        for b in range(num_batches):
            for k in range(self.B):
                self._item_into(b * self.B + k, self.batch, self.batch_label, self.batch_smpw, k)
            angles = [self.rng.uniform() * 2 * np.pi for _ in range(self.B)]
            self.score(forward(self.rotate(self.batch, self.B, angles)), self.batch_label, self.batch_smpw)
        return self._finish(num_batches, False)

    def _whole_batch(self, data):
        return data  # T:331-418 feeds the whole scans' rows as they are
