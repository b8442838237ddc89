"""What ScanNet's and SemanticKITTI's sliding-window whole-cloud test loops share on the host (ScanNet/window_tester.py,
SemanticKITTI/window_tester.py): the grid of windows, their counts and member lists, the merge of small blocks, the division
into rows of `block_points`, the vote, the run over clouds and votes, the score and the results.  Both references'
`__getitem__` / `eval_one_epoch` are the same code round these; the line numbers are given by the two classes' own docstrings.

A class built on `WindowLoop` supplies the buffers its constructor allocates (xyz, sizes, labels, bounds, class_values, pools,
preds, counts, total, C, P, B, S, width, stride, block_size, min_block_points, nearest, rng, scored, device) and

  ITEM                      'scene' or 'scan', for the messages
  ENTRY, SCALARS            the prefix of its hist_bytes / count / fill entry points, and the attributes they take as doubles
  MASKED                    whether fill writes a 0.001-margin mask next to every member
  MAX_WINDOWS               the window count `grid` refuses (None: `count` refuses, from hist_bytes == 0)
  PAD_SHORT                 what draw_rows does where the make-up is longer than the block
  merged(counts) -> the windows that enter the merge, ascending
  _buffers(rows) -> what gather fills for `rows` rows
  _batch(i, prep, start, out) -> data, idx, wgt of one batch of B rows (what draws a batch needs come here)
  deno(m, seen, correct) -> iou_deno per class from the confusion matrix m (rows: the truth)
  begin_vote(i, vote), tally(i, seen, correct)   optional: before a vote's first batch, after a cloud's counts
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip

_p = _hip.ptr


def nearest_block_literal(center, centers):
    """the reference's nearest_dist, through numpy exactly so (see the testers' docstrings on ties)"""
    dist = np.zeros(len(centers))
    for i in range(len(centers)):
        dist[i] = np.linalg.norm(centers[i] - center, ord=2)
    return np.argsort(dist)[0]


def batched_norms(d):
    """per row of d (m,2) f64 what np.linalg.norm(d[k], ord=2) gives: sqrt of the BLAS dot of the row with itself"""
    return np.sqrt(np.matmul(d[:, None, :], d[:, :, None])[:, 0, 0])


def nearest_block(center, centers):
    """nearest_dist with the distances from one batched expression; argsort is called as the reference calls it"""
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
    """The merge over counts and centres: a block of at most min_block_points points (an empty window included) is popped
    and appended to the nearest remaining block, and the cursor does not advance.  centers: (m,2) f64.  -> per final block,
    the ordered positions (into `sizes`) of the windows whose member lists are concatenated."""
    sizes = [int(s) for s in sizes]
    if not sizes:
        raise ValueError("no window to merge")
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


def draw_rows(length, block_points, rng, pad_short=False):
    """One block of `length` points -> the padded, shuffled positions: two shuffles where length is no multiple of
    block_points, one otherwise.  Where the make-up is longer than the block the reference's chunks come out ragged:
    a ValueError, or with pad_short what the slice gives (fewer than a multiple of block_points; the caller floors)."""
    order = np.arange(length)
    if length % block_points != 0:
        makeup = block_points - length % block_points
        if makeup > length and not pad_short:
            raise ValueError(f"a block of {length} points cannot be made up to a multiple of block_points = {block_points}: the "
                             f"make-up slice is shorter than {makeup} and the reference's chunks come out ragged")
        rng.shuffle(order)
        order = np.concatenate((order, order[0:makeup].copy()))
    rng.shuffle(order)
    return order


class WindowLoop:
    MAX_WINDOWS = None
    PAD_SHORT = False

    def _launch(self, entry, what, *args):
        _hip.launch(entry, type(self).__name__ + " " + what, *args)

    # ---- one __getitem__, step by step
    def grid(self, i):
        """coordmin / coordmax on the device, read back (the first of a vote's two readbacks), and the number of windows per
        axis by the reference's own float32 expression.  -> coordmin (3,) f32, coordmax (3,) f32, nx, ny."""
        self._launch("pasnl_window_bounds", "bounds", ctypes.c_long(self.sizes[i]), _p(self.xyz[i]), _p(self.bounds))
        b = self.bounds.cpu().numpy()
        if not np.all(np.isfinite(b)):
            raise ValueError(f"{self.ITEM} {i} has no finite extent (a scene whose points coincide divides by zero in the noise step)")
        coordmin, coordmax = b[0:3].copy(), b[3:6].copy()
        nx = int(np.ceil((coordmax[0] - coordmin[0]) / self.stride).astype(np.int32))
        ny = int(np.ceil((coordmax[1] - coordmin[1]) / self.stride).astype(np.int32))
        if nx < 1 or ny < 1:
            raise ValueError(f"{self.ITEM} {i} has zero extent in x or y: the reference finds no window")
        if self.MAX_WINDOWS is not None and nx * ny >= self.MAX_WINDOWS:
            raise _hip.PasnlUnsupported(f"{nx} x {ny} windows do not fit int32 positions")
        return coordmin, coordmax, nx, ny

    def _window_args(self, i, nx, ny):
        return (ctypes.c_long(self.sizes[i]), _p(self.xyz[i]), _p(self.bounds), nx, ny) + tuple(
            ctypes.c_double(getattr(self, name)) for name in self.SCALARS)

    def count(self, i, nx, ny):
        """The windows, counted: -> the scanned histogram (a device buffer `fill` reads) and the per-window counts (nx*ny,) as
        numpy, empty windows as 0: the second readback."""
        nbytes = int(getattr(_hip.lib(), self.ENTRY + "_hist_bytes")(ctypes.c_long(self.sizes[i]), nx, ny))
        if nbytes == 0:
            raise _hip.PasnlUnsupported(f"{nx} x {ny} windows: their positions do not fit an int32")
        hist = torch.empty((nbytes // 4,), dtype=torch.int32, device=self.device)
        counts = torch.empty((nx * ny,), dtype=torch.int32, device=self.device)
        self._launch(self.ENTRY + "_count", "count", *self._window_args(i, nx, ny), _p(hist), _p(counts))
        return hist, counts.cpu().numpy().astype(np.int64)

    def fill(self, i, nx, ny, hist, woff, cap):
        """The member lists, each at woff[w] (-1: skipped) -> cat_idx (cap,) i32 and, where MASKED, cat_mask (cap,) u8 device
        tensors (None otherwise)"""
        cat_idx = torch.empty((cap,), dtype=torch.int32, device=self.device)
        cat_mask = torch.empty((cap,), dtype=torch.uint8, device=self.device) if self.MASKED else None
        w = _hip.as_dev(np.asarray(woff, np.int32), torch.int32)
        self._launch(self.ENTRY + "_fill", "fill", *self._window_args(i, nx, ny), _p(hist), _p(w), ctypes.c_long(cap), _p(cat_idx),
                     *((_p(cat_mask),) if self.MASKED else ()))
        return cat_idx, cat_mask

    def centers(self, coordmin, coordmax, nx, ny):
        """every window's centre in i-major order -> (nx*ny, 2) float64 (the reference's float64 expressions for curmin and
        curmax, block_size wide, evaluated per axis)"""
        out = np.empty((nx, ny, 2))
        for a, count in ((0, nx), (1, ny)):
            curmin = np.float64(coordmin[a]) + np.arange(count) * self.stride
            curmax = curmin + self.block_size
            axis = (curmin + curmax) / 2.0
            out[:, :, a] = axis[:, None] if a == 0 else axis[None, :]
        return out.reshape(-1, 2)

    def prepare(self, i):
        """Up to the gather: windows, merge, the rows' positions.  -> dict(rows, rowpos, cat_idx, cat_mask, cap, blocks,
        counts, grid) where `blocks` lists per final block its windows in concatenation order."""
        coordmin, coordmax, nx, ny = self.grid(i)
        hist, counts = self.count(i, nx, ny)
        cap = int(counts.sum())
        if cap >= 2 ** 31:
            raise _hip.PasnlUnsupported("the windows hold 2^31 or more members")
        windows = self.merged(counts)
        parts = merge_blocks(counts[windows], self.centers(coordmin, coordmax, nx, ny)[windows], self.min_block_points, self.nearest)
        blocks = [windows[part].tolist() for part in parts]
        woff = np.full(nx * ny, -1, np.int64)
        at, rowpos = 0, []
        for block in blocks:
            start = at
            for w in block:
                if counts[w] > 0:
                    woff[w] = at
                    at += int(counts[w])
            rowpos.append((draw_rows(at - start, self.P, self.rng, self.PAD_SHORT) + start).astype(np.int32))
        rowpos = np.concatenate(rowpos)
        cat_idx, cat_mask = self.fill(i, nx, ny, hist, woff, cap)
        return dict(rows=rowpos.shape[0] // self.P, rowpos=torch.from_numpy(rowpos).to(self.device), cat_idx=cat_idx, cat_mask=cat_mask,
                    cap=cap, blocks=blocks, counts=counts, grid=(nx, ny))

    def blocks(self, i):
        """One `__getitem__(i)` of the reference on the device: advances the RNG.  -> what `gather` returns for all its rows."""
        prep = self.prepare(i)
        return self.gather(i, prep, 0, prep["rows"])

    def window_lists(self, i):
        """The windows of cloud i as it stands (no RNG draw), every non-empty window's list in window order -> coordmin,
        coordmax, (nx, ny), counts (nx*ny,) int64, members i32 and, where MASKED, masks u8 (numpy; the lists back to back)."""
        coordmin, coordmax, nx, ny = self.grid(i)
        hist, counts = self.count(i, nx, ny)
        woff = np.where(counts > 0, np.cumsum(counts) - counts, -1)
        total = int(counts.sum())
        lists = self.fill(i, nx, ny, hist, woff, max(total, 1))
        return (coordmin, coordmax, (nx, ny), counts) + tuple(t[:total].cpu().numpy() for t in lists if t is not None)

    # ---- the loop
    def vote(self, i, logits, idx, *wgt_rows):
        """`vote(i, logits, idx, wgt, rows)`, or `vote(i, logits, idx, rows)` where every row entry votes (the class's buffer
        of ones): the first `rows` rows of a batch, logits (B,P,C) f32"""
        wgt, rows = wgt_rows if len(wgt_rows) == 2 else (self.ones, wgt_rows[0])
        v = _hip.as_dev(logits, torch.float32)
        if v.numel() < rows * self.P * self.C or v.shape[-1] != self.C:
            raise ValueError(f"the forward must return (B, {self.P}, {self.C}) logits")
        self._launch("pasnl_window_vote", "vote", rows, self.P, self.C, _p(v), _p(idx), _p(wgt), ctypes.c_long(self.sizes[i]),
                     _p(self.pools[i]))

    def begin_vote(self, i, vote):
        pass

    def run(self, forward, num_votes=1):
        """Clouds in order, num_votes votes of each inside (the reference's RNG order).  forward: (B,P,width) f32 device tensor
        -> (B,P,C) f32 logits.  Within a vote, gather -> forward -> vote runs batch after batch with no host synchronisation.
        -> the number of rows fed."""
        fed = 0
        out = self._buffers(self.B)
        for i in range(self.S):
            self.pools[i] = torch.zeros((self.sizes[i], self.C), dtype=torch.int32, device=self.device)
            for vote in range(num_votes):
                prep = self.prepare(i)
                self.begin_vote(i, vote)
                for start in range(0, prep["rows"], self.B):
                    data, idx, wgt = self._batch(i, prep, start, out)
                    self.vote(i, forward(data), idx, wgt, min(self.B, prep["rows"] - start))
                fed += prep["rows"]
            self.score(i)
        return fed

    def tally(self, i, seen, correct):
        pass

    def score(self, i):
        """Cloud i's labels from its pool on the device; where labels were given, seen / correct / iou_deno from the confusion
        matrix of (labels, predictions), added to the totals."""
        n = self.sizes[i]
        pred = torch.empty((n,), dtype=torch.int32, device=self.device)
        self._launch("pasnl_window_pool_labels", "labels", ctypes.c_long(n), self.C, _p(self.pools[i]), _p(pred))
        self.preds[i] = pred
        if not self.scored:
            return
        cm = torch.zeros((self.C, self.C), dtype=torch.int64, device=self.device)
        self._launch("pasnl_confusion_matrix", "counts", ctypes.c_long(n), _p(self.labels[i]), _p(pred), _p(self.class_values), self.C,
                     _p(cm))
        m = cm.cpu().numpy()  # rows: the truth
        seen, correct = m.sum(axis=1), np.diagonal(m).copy()
        self.counts[i] = np.stack([seen, correct, self.deno(m, seen, correct)])
        self.total += self.counts[i]
        self.tally(i, seen, correct)

    # ---- state and results
    def pool(self, i):
        """cloud i's vote counters (n_i, C) i32, device tensor"""
        return self.pools[i]

    def pred_label(self, i):
        """np.argmax(vote_label_pool, 1) of cloud i, (n_i,) i32 device tensor"""
        return self.preds[i]

    def totals(self):
        """-> total_seen_class, total_correct_class, total_iou_deno_class over the clouds scored so far"""
        return tuple(self.total.copy())

    def class_iou(self):
        """the IoU of classes 1..C-1 over all clouds; its mean is the reference's 'point avg class IoU'"""
        _, correct, deno = self.totals()
        return np.array(correct[1:]) / (np.array(deno[1:], dtype=float) + 1e-6)
