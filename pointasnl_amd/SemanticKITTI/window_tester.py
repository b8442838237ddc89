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

What differs from the ScanNet loop (ScanNet/window_tester.py): the window is `block_size` wide; a lidar scan has thousands
of windows (no limit per axis) and EVERY window, empty or not, enters the merge (D has no `continue`); there is no noise
step and no 0.001-margin mask (every row entry votes); a remission channel and a rotation about z are optional.

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
from pointasnl_amd.SemanticKITTI.scan_tester import _p


def nearest_block_literal(center, centers):
    """D:271-276, through numpy exactly so"""
    dist = np.zeros(len(centers))
    for i in range(len(centers)):
        dist[i] = np.linalg.norm(centers[i] - center, ord=2)
    return np.argsort(dist)[0]


def batched_norms(d):
    """per row of d (m,2) f64 what np.linalg.norm(d[k], ord=2) gives: sqrt of the BLAS dot of the row with itself"""
    return np.sqrt(np.matmul(d[:, None, :], d[:, :, None])[:, 0, 0])


def nearest_block(center, centers):
    """D:271-276 with the distances from one batched expression; argsort is called as the reference calls it"""
    return np.argsort(batched_norms(centers - center))[0]


def batched_norm_agrees(stride=4.0, side=18):
    """whether batched_norms has the bits of the per-centre np.linalg.norm on this machine's BLAS: side^2 lattice
    differences around an off-lattice origin (microseconds on the host)"""
    ii, jj = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij")
    origin = np.array([-77.29800415039062, 51.06399917602539])
    centers = np.stack([origin[0] + ii.ravel() * stride + 5.0, origin[1] + jj.ravel() * float(stride) + 5.0], 1)
    center = centers[side + 3].copy()
    want = np.array([np.linalg.norm(c - center, ord=2) for c in centers])
    return np.array_equal(batched_norms(centers - center).view(np.int64), want.view(np.int64))


def merge_blocks(sizes, centers, min_block_points=4096, nearest=nearest_block):
    """D:311-327 over counts and centres: a block of at most min_block_points points (an empty window included) is popped
    and appended to the nearest remaining block, and the cursor does not advance.  centers: (m,2) f64.  -> per final block,
    the ordered positions (into `sizes`) of the windows whose member lists are concatenated."""
    sizes = [int(s) for s in sizes]
    centers = np.ascontiguousarray(np.asarray(centers, np.float64).reshape(len(sizes), 2))
    parts = [[k] for k in range(len(sizes))]
    at = 0
    while at < len(sizes):
        if sizes[at] > min_block_points:
            at += 1
            continue
        size, part, center = sizes.pop(at), parts.pop(at), centers[at].copy()
        centers = np.delete(centers, at, axis=0)
        if not sizes:
            raise ValueError(f"every block holds at most min_block_points = {min_block_points} points: the reference's "
                             "nearest_dist would index an empty argsort")
        to = int(nearest(center, centers))
        sizes[to] += size
        parts[to] = parts[to] + part
    return parts


def draw_rows(length, block_points, rng):
    """D:337-345 for one block of `length` points -> the padded, shuffled positions (a multiple of block_points): two
    shuffles where length is no multiple of block_points, one otherwise"""
    order = np.arange(length)
    if length % block_points != 0:
        makeup = block_points - length % block_points
        if makeup > length:
            raise ValueError(f"a block of {length} points cannot be made up to a multiple of block_points = {block_points}: the "
                             f"make-up slice is shorter than {makeup} and the reference's chunks come out ragged")
        rng.shuffle(order)
        order = np.concatenate((order, order[0:makeup].copy()))
    rng.shuffle(order)
    return order


class KittiWindowTester:
    """`KittiWindowTester(scans, labels=None, remissions=None, num_classes=20, block_points=8192, batch_size=6, block_size=10,
    stride=4, min_block_points=4096, random_rotate=False, rng=np.random, accumulate_votes=False)`.

    scans: a list of (n_i, 3) float32 arrays (numpy or device tensors), copied to the device.  labels: per scan the mapped
    labels in [0, num_classes) (None: split 'test', nothing is scored).  remissions: per scan (n_i,) float32 (None: rows
    are xyz only).  rng: np.random or a RandomState; `blocks(i)` draws per final block rng.shuffle (when its length is no
    multiple of block_points) and rng.shuffle again, and with random_rotate `run` draws batch_size rng.uniform per batch.

    The pool quirk: the reference clears vote_label_pool at the first batch of EVERY vote (T:168-169), so only the last
    vote of a scan decides its labels.  That is mirrored by default; accumulate_votes=True sums the votes instead."""

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
    def grid(self, i):
        """D:289-292: coordmin / coordmax on the device, read back (the first of a vote's two readbacks), and the number of
        windows per axis by the reference's own float32 expression.  -> coordmin (3,) f32, coordmax (3,) f32, nx, ny."""
        _hip.launch("pasnl_window_bounds", "KittiWindowTester bounds", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]), _p(self.bounds))
        b = self.bounds.cpu().numpy()
        if not np.all(np.isfinite(b)):
            raise ValueError(f"scan {i} has no finite extent")
        coordmin, coordmax = b[0:3].copy(), b[3:6].copy()
        nx = int(np.ceil((coordmax[0] - coordmin[0]) / self.stride).astype(np.int32))
        ny = int(np.ceil((coordmax[1] - coordmin[1]) / self.stride).astype(np.int32))
        if nx < 1 or ny < 1:
            raise ValueError(f"scan {i} has zero extent in x or y: the reference finds no window")
        if nx * ny >= 2 ** 31:
            raise _hip.PasnlUnsupported(f"{nx} x {ny} windows do not fit int32 positions")
        return coordmin, coordmax, nx, ny

    def count(self, i, nx, ny):
        """D:296-302, counted: -> the scanned histogram (a device buffer pasnl_kwindow_fill reads) and the per-window counts
        (nx*ny,) as numpy, empty windows as 0: the second readback."""
        n = self.sizes[i]
        nbytes = int(_hip.lib().pasnl_kwindow_hist_bytes(ctypes.c_long(n), nx, ny))
        hist = torch.empty((nbytes // 4,), dtype=torch.int32, device=self.device)
        counts = torch.empty((nx * ny,), dtype=torch.int32, device=self.device)
        _hip.launch("pasnl_kwindow_count", "KittiWindowTester count", ctypes.c_long(n), _p(self.xyz[i]), _p(self.bounds), nx, ny,
                    ctypes.c_double(self.block_size), ctypes.c_double(self.stride), _p(hist), _p(counts))
        return hist, counts.cpu().numpy().astype(np.int64)

    def fill(self, i, nx, ny, hist, woff, cap):
        """D:300-307: the member lists, each at woff[w] (-1: skipped) -> cat_idx (cap,) i32 device tensor"""
        cat_idx = torch.empty((cap,), dtype=torch.int32, device=self.device)
        w = _hip.as_dev(np.asarray(woff, np.int32), torch.int32)
        _hip.launch("pasnl_kwindow_fill", "KittiWindowTester fill", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]), _p(self.bounds), nx, ny,
                    ctypes.c_double(self.block_size), ctypes.c_double(self.stride), _p(hist), _p(w), ctypes.c_long(cap), _p(cat_idx))
        return cat_idx

    def centers(self, coordmin, coordmax, nx, ny):
        """D:298-299, 308 for every window in i-major order -> (nx*ny, 2) float64 block centres (the reference's float64
        expressions, evaluated per axis)"""
        out = np.empty((nx, ny, 2))
        for a, count in ((0, nx), (1, ny)):
            curmin = np.float64(coordmin[a]) + np.arange(count) * self.stride
            curmax = curmin + self.block_size
            axis = (curmin + curmax) / 2.0
            out[:, :, a] = axis[:, None] if a == 0 else axis[None, :]
        return out.reshape(-1, 2)

    def prepare(self, i):
        """D:289-349 up to the gather: windows, merge, the rows' positions.  -> dict(rows, rowpos, cat_idx, cap, blocks,
        counts, grid) where `blocks` lists per final block its windows in concatenation order."""
        coordmin, coordmax, nx, ny = self.grid(i)
        hist, counts = self.count(i, nx, ny)
        cap = int(counts.sum())
        if cap >= 2 ** 31:
            raise _hip.PasnlUnsupported("the windows hold 2^31 or more members")
        parts = merge_blocks(counts, self.centers(coordmin, coordmax, nx, ny), self.min_block_points, self.nearest)
        woff = np.full(nx * ny, -1, np.int64)
        at, rowpos = 0, []
        for part in parts:
            start = at
            for w in part:
                if counts[w] > 0:
                    woff[w] = at
                    at += int(counts[w])
            rowpos.append((draw_rows(at - start, self.P, self.rng) + start).astype(np.int32))
        rowpos = np.concatenate(rowpos)
        cat_idx = self.fill(i, nx, ny, hist, woff, cap)
        return dict(rows=rowpos.shape[0] // self.P, rowpos=torch.from_numpy(rowpos).to(self.device), cat_idx=cat_idx, cap=cap,
                    blocks=parts, counts=counts, grid=(nx, ny))

    def gather(self, i, prep, start, rows, out=None, angles=None):
        """D:347-351 / T:157-161 for rows [start, start + rows) of the prepared vote; rows past the last one come out as
        zeros.  angles: (rows,) float64 host array or None.  -> data (rows,P,3|4) f32, indices (rows,P) i32, device tensors."""
        if out is None:
            out = (torch.empty((rows, self.P, self.width), dtype=torch.float32, device=self.device),
                   torch.empty((rows, self.P), dtype=torch.int32, device=self.device))
        data, idx = out
        real = max(0, min(rows, prep["rows"] - start))
        ang = None if angles is None else _hip.as_dev(np.asarray(angles, np.float64).reshape(rows), torch.float64)
        _hip.launch("pasnl_kwindow_gather", "KittiWindowTester gather", rows, real, self.P, _p(prep["rowpos"], start * self.P * 4),
                    ctypes.c_long(prep["cap"]), _p(prep["cat_idx"]), ctypes.c_long(self.sizes[i]), _p(self.xyz[i]),
                    _p(self.remission[i]) if self.nfeat else ctypes.c_void_p(0), self.nfeat,
                    ctypes.c_void_p(0) if ang is None else _p(ang), _p(data), _p(idx))
        return data, idx

    def blocks(self, i):
        """One `__getitem__(i)` of the reference on the device: advances the RNG by the blocks' shuffles.  -> device tensors
        data (R,P,3|4) f32 (div_blocks) and indices (R,P) i32 (div_blocks_idxs)."""
        prep = self.prepare(i)
        return self.gather(i, prep, 0, prep["rows"])

    def window_lists(self, i):
        """The windows of scan i (no RNG draw), every window's list in window order -> coordmin, coordmax, (nx, ny), counts
        (nx*ny,) int64, members i32 (numpy; the lists back to back)."""
        coordmin, coordmax, nx, ny = self.grid(i)
        hist, counts = self.count(i, nx, ny)
        woff = np.where(counts > 0, np.cumsum(counts) - counts, -1)
        total = int(counts.sum())
        cat_idx = self.fill(i, nx, ny, hist, woff, max(total, 1))
        return coordmin, coordmax, (nx, ny), counts, cat_idx[:total].cpu().numpy()

    # ---- the loop
    def vote(self, i, logits, idx, rows):
        """T:166, 171-172 for the first `rows` rows of a batch: logits (B,P,C) f32; every row entry votes"""
        v = _hip.as_dev(logits, torch.float32)
        if v.numel() < rows * self.P * self.C or v.shape[-1] != self.C:
            raise ValueError(f"the forward must return (B, {self.P}, {self.C}) logits")
        _hip.launch("pasnl_window_vote", "KittiWindowTester vote", rows, self.P, self.C, _p(v), _p(idx), _p(self.ones),
                    ctypes.c_long(self.sizes[i]), _p(self.pools[i]))

    def run(self, forward, num_votes=1):
        """T:123-216: scans in order, num_votes votes of each inside (the reference's RNG order).  forward: (B,P,3|4) f32
        device tensor -> (B,P,C) f32 logits.  Within a vote, gather -> forward -> vote runs batch after batch with no host
        synchronisation.  -> the number of rows fed."""
        fed = 0
        out = (torch.empty((self.B, self.P, self.width), dtype=torch.float32, device=self.device),
               torch.empty((self.B, self.P), dtype=torch.int32, device=self.device))
        for i in range(self.S):
            self.pools[i] = torch.zeros((self.sizes[i], self.C), dtype=torch.int32, device=self.device)
            for vote in range(num_votes):
                prep = self.prepare(i)
                if vote > 0 and not self.accumulate_votes:
                    self.pools[i].zero_()  # T:168-169: the pool is made anew at the first batch of every vote
                for start in range(0, prep["rows"], self.B):
                    angles = None
                    if self.random_rotate:  # T:160-161: one uniform per row of the batch, stale rows included
                        angles = np.array([self.rng.uniform() * 2 * np.pi for _ in range(self.B)])
                    data, idx = self.gather(i, prep, start, self.B, out, angles)
                    self.vote(i, forward(data), idx, min(self.B, prep["rows"] - start))
                fed += prep["rows"]
            self.score(i)
        return fed

    def score(self, i):
        """T:174-175 for scan i: final_preds on the device; with labels, T:196-231: the counts from the confusion matrix of
        (labels, final_preds), added to the totals, and every tenth scan the logged figures."""
        n = self.sizes[i]
        pred = torch.empty((n,), dtype=torch.int32, device=self.device)
        _hip.launch("pasnl_window_pool_labels", "KittiWindowTester labels", ctypes.c_long(n), self.C, _p(self.pools[i]), _p(pred))
        self.preds[i] = pred
        if not self.scored:
            return
        cm = torch.zeros((self.C, self.C), dtype=torch.int64, device=self.device)
        _hip.launch("pasnl_confusion_matrix", "KittiWindowTester counts", ctypes.c_long(n), _p(self.labels[i]), _p(pred),
                    _p(self.class_values), self.C, _p(cm))
        m = cm.cpu().numpy()  # rows: the truth
        seen, correct = m.sum(axis=1), np.diagonal(m).copy()
        deno = m.sum(axis=0) + seen - correct  # (pred == l) | (label == l)
        self.counts[i] = np.stack([seen, correct, deno])
        self.total += self.counts[i]
        self.total_correct += int(correct.sum())
        self.total_seen += n
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
    def pool(self, i):
        """scan i's vote counters (n_i, C) i32, device tensor"""
        return self.pools[i]

    def pred_label(self, i):
        """np.argmax(vote_label_pool, axis=1) of scan i, (n_i,) i32 device tensor"""
        return self.preds[i]

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

    def totals(self):
        """-> total_seen_class, total_correct_class, total_iou_deno_class over the scans scored so far"""
        return tuple(self.total.copy())

    def class_iou(self):
        """T:219: the IoU of classes 1..C-1 over all scans; its mean is the reference's 'eval point avg class IoU'"""
        _, correct, deno = self.totals()
        return np.array(correct[1:]) / (np.array(deno[1:], dtype=float) + 1e-6)

    def tenth_scan_figures(self, i):
        """what T:218-231 logs after scan i (i % 10 == 0): dict(miou, accuracy, class_accuracy, labelweights (C-1,) f32 as
        renormalised at that scan, iou (C-1,) f64 without the 1e-6)"""
        return self.logged[i]
