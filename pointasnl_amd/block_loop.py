"""What ScanNet's and SemanticKITTI's training-time validation loops share on the host (ScanNet/block_tester.py,
SemanticKITTI/block_tester.py): the item of a chopped cloud, the item of a whole cloud, the carry-over of rows between whole
clouds, the score and the results.  Both references' `eval_one_epoch` / `eval_whole_scene_one_epoch` are the same code round
these; the line numbers in the docstrings below are given by the two classes' own docstrings.

A class built on `BlockLoop` supplies the buffers its constructor allocates (xyz, sizes, zero, counters, loss, workspace,
C, P, B, S, width, rng, device) and

  draw_crop(i) -> centre, m, hist, tries          the rejection loop of a chopped item
  column_counts(i) -> (nx, ny), counts, hist      the grid of a whole cloud, counted
  _rows(i, centre, nx, ny, hist, woff, cap, rowpos, rowbase, data, seg, smpw, row0=0)
                                                  member lists, then rows; rowbase[r] is the offset row r's draws were shifted by
  _whole_batch(data) -> what the forward is fed   from the first B rows of a whole-cloud batch
"""
import numpy as np
import torch

from pointasnl_amd import _hip

_p = _hip.ptr


class BlockLoop:
    TABLE_IN_CHOPPED = False  # whether `report` prints the per-class table after the chopped loop too

    def reset(self):
        """clears the counters and the loss (both loops start with it)"""
        self.counters.zero_()
        self.loss.zero_()
        self.forwards, self.num_batches, self.whole, self.left, self._final = 0, 0, False, 0, None

    # ---- items
    def _item_into(self, i, data, seg, smpw, row):
        centre, m, hist, _ = self.draw_crop(i)
        choice = self.rng.choice(m, self.P, replace=True)
        self._rows(i, centre, 1, 1, hist, self.zero, m, choice, [0], data, seg, smpw, row)

    def item(self, i):
        """One `__getitem__(i)` of the reference's chopped dataset on the device: advances the RNG.  -> device tensors data
        (P,width) f32, seg (P,) i32, smpw (P,) f32."""
        data = torch.empty((1, self.P, self.width), dtype=torch.float32, device=self.device)
        seg = torch.empty((1, self.P), dtype=torch.int32, device=self.device)
        smpw = torch.empty((1, self.P), dtype=torch.float32, device=self.device)
        self._item_into(i, data, seg, smpw, 0)
        return data[0], seg[0], smpw[0]

    def _whole_item(self, i):
        """One `__getitem__(i)` of the reference's whole-cloud dataset on the device: one `rng.choice(count, P)` per non-empty
        column in the reference's order, one fill, one gather.  -> device tensors data (R,P,width) f32, seg (R,P) i32, smpw
        (R,P) f32."""
        (nx, ny), counts, hist = self.column_counts(i)
        found = np.flatnonzero(counts > 0)  # empty columns are skipped and draw nothing
        cap = int(counts.sum())
        if cap >= 2 ** 31:
            raise _hip.PasnlUnsupported("the columns hold 2^31 or more members")
        woff = np.where(counts > 0, np.cumsum(counts) - counts, -1)
        rowpos = np.concatenate([self.rng.choice(int(counts[w]), self.P, replace=True) + woff[w] for w in found])
        rows = len(found)
        data = torch.empty((rows, self.P, self.width), dtype=torch.float32, device=self.device)
        seg = torch.empty((rows, self.P), dtype=torch.int32, device=self.device)
        smpw = torch.empty((rows, self.P), dtype=torch.float32, device=self.device)
        self._rows(i, -1, nx, ny, hist, _hip.as_dev(woff.astype(np.int32), torch.int32), cap, rowpos, woff[found], data, seg, smpw)
        return data, seg, smpw

    # ---- the loops
    def score(self, logits, seg, smpw):
        """the counters and the loss for one batch of B rows: logits (B,P,C) f32 from the forward"""
        v = _hip.as_dev(logits, torch.float32)
        if v.numel() != self.B * self.P * self.C or v.shape[-1] != self.C:
            raise ValueError(f"the forward must return ({self.B}, {self.P}, {self.C}) logits")
        _hip.launch("pasnl_block_score", type(self).__name__ + " score", self.B, self.P, self.C, _p(v), _p(seg), _p(smpw),
                    _p(self.counters), _p(self.loss), _p(self.workspace))
        self.forwards += 1

    def _finish(self, num_batches, whole, left=0):
        self.num_batches, self.whole, self.left = num_batches, whole, left
        c = self.counters.cpu().numpy()  # the epoch's one readback of the counters
        C = self.C
        self._final = dict(total_correct=int(c[0]), total_seen=int(c[1]), seen=c[2:2 + C].copy(), correct=c[2 + C:2 + 2 * C].copy(),
                           deno=c[2 + 2 * C:2 + 3 * C].copy(), hist=c[2 + 3 * C:2 + 4 * C].copy(),
                           loss_sum=float(self.loss.cpu().numpy()[0]))
        return self.miou()

    def run_whole(self, forward):
        """One epoch over whole clouds with the reference's carry-over: a cloud's rows go in front of the carried ones when no
        batch is being continued and behind the accumulated ones when one is; fewer than B rows wait for the next cloud; of
        more than B the first B are fed and the rest carried, even when B or more remain -- at most one forward per cloud --
        and what is left at the end is never scored.  -> mIoU."""
        self.reset()
        continuing, rows, carried = False, None, None
        for i in range(self.S):
            new = self._whole_item(i)
            if continuing:
                rows = tuple(torch.cat((r, a), dim=0) for r, a in zip(rows, new))
            else:
                rows = new if carried is None else tuple(torch.cat((a, c), dim=0) for a, c in zip(new, carried))
            continuing = rows[0].shape[0] < self.B
            if continuing:
                continue
            carried = tuple(r[self.B:] for r in rows) if rows[0].shape[0] > self.B else None
            data, seg, smpw = (r[:self.B].contiguous() for r in rows)
            self.score(forward(self._whole_batch(data)), seg, smpw)
        left = rows[0].shape[0] if continuing else (0 if carried is None else carried[0].shape[0])
        return self._finish(self.S, True, left)

    # ---- results
    def totals(self):
        """-> dict(total_correct, total_seen, seen (C,), correct (C,), deno (C,), hist (C,)): the int64 counters of the last
        epoch (hist is the label histogram)"""
        return {k: self._final[k] for k in ("total_correct", "total_seen", "seen", "correct", "deno", "hist")}

    def class_iou(self):
        """the IoU of classes 1..C-1, correct / (iou_deno + 1e-6)"""
        f = self._final
        return np.array(f["correct"][1:]) / (np.array(f["deno"][1:], dtype=float) + 1e-6)

    def miou(self):
        return np.mean(self.class_iou())

    def mean_loss(self, extra=0.0):
        """loss_sum / float(num_batches), where num_batches is S // B for the chopped loop and S -- not the number of forwards
        -- for the whole-cloud loop; extra is what the model's other loss terms add to every forward"""
        return (self._final["loss_sum"] + float(extra) * self.forwards) / float(self.num_batches)

    def report(self, names, extra=0.0):
        """The lines the reference logs for the last epoch; names[l] is the class name (seg_label_to_cat).  Where the
        reference divides by a zero count -- the accuracy without a labelled point, the table's IoU of a class with
        iou_deno == 0 -- numpy's scalar division gives nan with a warning there (the counters are numpy integers, so it is not
        a ZeroDivisionError); nan is what is reported here."""
        f = self._final
        head = "Eval whole scene" if self.whole else "Eval"
        with np.errstate(divide="ignore", invalid="ignore"):
            acc = np.float64(f["total_correct"]) / float(f["total_seen"])
            class_acc = np.mean(np.array(f["correct"][1:]) / (np.array(f["seen"][1:], dtype=float) + 1e-6))
            lines = ["%s mean loss: %f" % (head, self.mean_loss(extra)), "Eval point avg class IoU: %f" % self.miou(),
                     "%s point accuracy: %f" % (head, acc), "%s point avg class acc: %f" % (head, class_acc)]
            if self.whole or self.TABLE_IN_CHOPPED:
                hist = f["hist"].astype(np.float64)
                weights = hist[1:].astype(np.float32) / np.sum(hist[1:].astype(np.float32))
                txt = "------- IoU --------\n"
                for l in range(1, self.C):
                    txt += "class %s weight: %.3f, IoU: %.3f \n" % (names[l] + " " * (14 - len(names[l])), weights[l - 1],
                                                                    np.int64(f["correct"][l]) / float(f["deno"][l]))
                lines.append(txt)
        return lines
