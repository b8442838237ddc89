"""numpy restatement of the ScanNet sliding-window whole-scene test loop (reference ScanNet/scannet_dataset.py (D) :135-300
`ScannetDatasetWholeSceneSlidingWindow.__getitem__` and ScanNet/test_scannet.py (T) :96-196 `add_vote` / `eval_one_epoch`),
the yardstick of pointasnl_amd.ScanNet.window_tester.  The flow is cut into the steps the device runs -- move, windows,
merge, rows, vote, counts -- with `min_block_points` (4096 in the reference) as a parameter;
tests/test_window_tester_flow.py pins this file to the reference class and to the literal vote and count expressions.

`merge` calls np.argsort(dist)[0] as the reference does: window centres sit on a lattice, equal nearest distances are the
rule, and which of them numpy's unstable sort lists first depends on its sort kernel for the CPU at hand.  Everything
downstream of the merge is therefore comparable on ONE machine only."""
import math

import numpy as np

from scene_flow_ref import scene  # noqa: F401  (re-exported for the tests)

TEST_CLASS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])  # T:105


def sequential_mean_f32(xyz):
    """what np.mean(raw_xyz, axis=0) computes for a float32 (N,3) view: every column summed front to back in float32, then
    divided by float32(N) -- the chain the device carries in three lanes"""
    acc = np.zeros(3, np.float32)
    for row in np.asarray(xyz, np.float32):
        acc = acc + row
    return acc / np.float32(len(xyz))


def move(xyz, rng, noise_ratio=0.2):
    """D:192-210 on the (N,3) float32 view `xyz`, in place -> (choices, centroid (1,3) f32, max_length f32)"""
    n = xyz.shape[0]
    centroid = np.mean(xyz, axis=0, keepdims=True)
    normalized = xyz - centroid
    hi, lo = np.max(normalized), np.min(normalized)
    max_length = max(abs(hi), abs(lo))
    normalized = normalized / max_length
    num_noise = math.ceil(n * noise_ratio)
    choices = rng.choice(n, num_noise)
    shift = (rng.randn(num_noise, 3) - 0.5) / 0.5 * 0.002
    xyz[choices, 0:3] = (normalized[choices] + shift) * max_length + centroid
    return choices, centroid, max_length


def last_occurrence(choices, n):
    """mask over `choices`: True where no later entry names the same point (numpy's fancy assignment keeps that one)"""
    last = np.full(n, -1, np.int64)
    last[choices] = np.arange(len(choices))  # repeated indices: the last write stays
    return last[choices] == np.arange(len(choices))


def bounds(xyz):
    """D:214-217 -> coordmin (3,) f32, coordmax (3,) f32"""
    return np.min(xyz, axis=0), np.max(xyz, axis=0)


def grid(coordmin, coordmax, stride):
    nx = np.ceil((coordmax[0] - coordmin[0]) / stride).astype(np.int32)
    ny = np.ceil((coordmax[1] - coordmin[1]) / stride).astype(np.int32)
    return int(nx), int(ny)


def window_box(coordmin, coordmax, i, j, stride):
    """D:225-226 -> curmin, curmax float64 (3,)"""
    curmin = coordmin + [i * stride, j * stride, 0]
    curmax = curmin + [1.5, 1.5, coordmax[2] - coordmin[2]]
    return curmin, curmax


def windows(xyz, stride):
    """D:214-242 without the payload: -> coordmin, coordmax, (nx, ny), counts (nx*ny,) int64 in i-major order (empty ones
    included), and per NON-EMPTY window in that order: (w, members ascending, 0.001-margin mask, centre (2,) f64)"""
    coordmin, coordmax = bounds(xyz)
    nx, ny = grid(coordmin, coordmax, stride)
    counts = np.zeros(max(nx, 0) * max(ny, 0), np.int64)
    found = []
    for i in range(nx):
        for j in range(ny):
            curmin, curmax = window_box(coordmin, coordmax, i, j, stride)
            inside = np.sum((xyz >= (curmin - 0.2)) * (xyz <= (curmax + 0.2)), axis=1) == 3
            members = np.where(inside)[0]
            counts[i * ny + j] = len(members)
            if len(members) == 0:
                continue
            sub = xyz[inside, :]
            mask = np.sum((sub >= (curmin - 0.001)) * (sub <= (curmax + 0.001)), axis=1) == 3
            found.append((i * ny + j, members, mask, (curmin[0:2] + curmax[0:2]) / 2.0))
    return coordmin, coordmax, (nx, ny), counts, found


def nearest(center, centers):
    dist = np.zeros(len(centers))
    for i in range(len(centers)):
        dist[i] = np.linalg.norm(centers[i] - center, ord=2)
    return np.argsort(dist)[0]


def merge(sizes, centers, min_block_points=4096):
    """D:244-269 over counts and centres only -> per final block the ordered list of positions (into `sizes`) whose member
    lists are concatenated.  A block at or under min_block_points is popped and appended to the nearest remaining one; the
    cursor stays, so the block that slid into its place is looked at next."""
    sizes, centers = [int(s) for s in sizes], [np.asarray(c, np.float64) for c in centers]
    if len(sizes) == 0:
        raise ValueError("no non-empty window")
    parts = [[k] for k in range(len(sizes))]
    at = 0
    while at < len(sizes):
        if sizes[at] > min_block_points:
            at += 1
            continue
        size, center, part = sizes.pop(at), centers.pop(at), parts.pop(at)
        if len(sizes) == 0:
            raise ValueError("every block holds at most min_block_points points: nothing is left to merge into")
        to = nearest(center, centers)
        sizes[to] += size
        parts[to] = parts[to] + part
    return parts


def draw_rows(length, block_points, rng):
    """D:279-289 for one block of `length` points -> the padded, shuffled positions (a multiple of block_points)"""
    order = np.arange(length)
    if length % block_points != 0:
        makeup = block_points - length % block_points
        rng.shuffle(order)
        order = np.concatenate((order, order[0:makeup].copy()))
    rng.shuffle(order)
    return order


def predict(logits):
    """T:159"""
    return np.argmax(logits[:, :, 1:], 2) + 1


def add_vote(pool, point_idx, pred, weight):
    """T:96-103 (integer increments: order-free)"""
    on = np.asarray(weight) != 0
    np.add.at(pool, (np.asarray(point_idx)[on].astype(np.int64), np.asarray(pred)[on].astype(np.int64)), 1)
    return pool


def class_counts(label, pred, num_classes):
    """T:164-170 -> seen, correct, iou_deno (num_classes,) int64"""
    seen = np.array([np.sum(label == l) for l in range(num_classes)], np.int64)
    correct = np.array([np.sum((pred == l) & (label == l)) for l in range(num_classes)], np.int64)
    deno = np.array([np.sum(((pred == l) | (label == l)) & (label > 0)) for l in range(num_classes)], np.int64)
    return seen, correct, deno


def scene_iou(seen, correct, deno):
    """T:172-175 -> iou_map (C,) f64, its mean over the seen classes"""
    iou_map = np.array(correct) / (np.array(deno, dtype=float) + 1e-6)
    return iou_map, np.mean(iou_map[np.array(seen) != 0])


def class_iou(correct, deno):
    """T:189 -> IoU of classes 1..C-1"""
    return np.array(correct[1:]) / (np.array(deno[1:], dtype=float) + 1e-6)


def export(pred_label, scene_points_id, scene_points_num, test_class=TEST_CLASS):
    """T:179-180"""
    whole = np.zeros(scene_points_num)
    whole[scene_points_id] = test_class[pred_label.astype(np.int32)]
    return whole


class WindowFlowRef:
    """scenes: a list of (N,3|6) float32 arrays, MOVED IN PLACE by every `getitem` as the reference moves
    scene_points_list; labels: a list of (N,) integer arrays."""

    def __init__(self, scenes, labels, num_classes=21, block_points=8192, batch_size=6, stride=0.5, with_rgb=True,
                 noise_ratio=0.2, min_block_points=4096, rng=np.random):
        self.scenes, self.labels, self.C, self.P, self.B = scenes, labels, num_classes, block_points, batch_size
        self.stride, self.with_rgb, self.noise_ratio, self.min_block_points, self.rng = stride, with_rgb, noise_ratio, min_block_points, rng
        self.pools, self.pred, self.counts = {}, {}, {}
        self.total = [np.zeros(num_classes, np.int64) for _ in range(3)]
        self.last = None  # what the latest getitem saw, for the tests

    def getitem(self, i):
        """-> data (R,P,3|6) f32, labels (R,P) i32, weights (R,P) f64, indices (R,P) i64"""
        pts = self.scenes[i] if self.with_rgb else self.scenes[i][:, 0:3]
        seg = self.labels[i].astype(np.int32)
        choices, centroid, max_length = move(pts[:, 0:3], self.rng, self.noise_ratio)
        seg[choices] = 0
        xyz = pts[:, 0:3]
        coordmin, coordmax, (nx, ny), counts, found = windows(xyz, self.stride)
        if nx < 1 or ny < 1:
            raise ValueError("the scene has no extent in x or y")
        parts = merge([len(m) for _, m, _, _ in found], [c for _, _, _, c in found], self.min_block_points)
        self.last = dict(choices=choices, centroid=centroid, max_length=max_length, coordmin=coordmin, coordmax=coordmax,
                         nx=nx, ny=ny, counts=counts, found=found, parts=parts)
        data, lab, wgt, idx = [], [], [], []
        for part in parts:
            members = np.concatenate([found[k][1] for k in part])
            mask = np.concatenate([found[k][2] for k in part])
            order = draw_rows(len(members), self.P, self.rng)
            chosen = members[order].reshape(-1, self.P)
            data.append(pts[chosen])
            lab.append(seg[chosen])
            wgt.append(np.ones(self.C)[seg[chosen]] * mask[order].reshape(-1, self.P))
            idx.append(chosen)
        return np.concatenate(data), np.concatenate(lab), np.concatenate(wgt), np.concatenate(idx)

    def run(self, forward, num_votes=1):
        """T:122-180: scenes in order, votes inside.  forward: (B,P,3|6) f32 -> (B,P,C) f32 logits; the rows past the last
        real one of a scene's final batch are fed zeros (the reference leaves stale rows there and never votes them)."""
        for i in range(len(self.scenes)):
            label = self.labels[i]
            pool = np.zeros((label.shape[0], self.C))
            for _ in range(num_votes):
                data, _, wgt, idx = self.getitem(i)
                for start in range(0, data.shape[0], self.B):
                    real = min(self.B, data.shape[0] - start)
                    batch = np.zeros((self.B,) + data.shape[1:], np.float32)
                    batch[:real] = data[start:start + real]
                    pred = predict(forward(batch))
                    add_vote(pool, idx[start:start + real], pred[:real], wgt[start:start + real])
            self.pools[i] = pool
            self.pred[i] = np.argmax(pool, 1)
            self.counts[i] = class_counts(label, self.pred[i], self.C)
            for acc, c in zip(self.total, self.counts[i]):
                acc += c
