"""numpy restatement of the SemanticKITTI sliding-window whole-scan test loop (reference
SemanticKITTI/semantic_kitti_dataset.py (D) :217-355 `SemanticKittiDatasetSlidingWindow.__getitem__` and
SemanticKITTI/test_semantic_kitti.py (T) :99-231 `add_vote` / `eval_one_epoch`), the yardstick of
pointasnl_amd.SemanticKITTI.window_tester.  The flow is cut into the steps the device runs -- windows, merge, rows, rotation,
vote, counts -- with `min_block_points` (4096 in the reference) as a parameter; tests/test_kitti_window_tester_flow.py pins
this file to the reference class and to the literal vote and count expressions.

`merge` calls np.argsort(dist)[0] as the reference does: window centres sit on a lattice, equal nearest distances are the
rule, and which of them numpy's unstable sort lists first depends on its sort kernel for the CPU at hand.  Everything
downstream of the merge is therefore comparable on ONE machine only."""
import numpy as np


def scan(seed, n, extent_x=24.1, extent_y=19.9, edge=8, snapped=False):
    """a lidar-like patch in metres, swept by azimuth as a lidar's rings are: ground plus a sixth of the points on vertical
    structures, uniform over [0, extent_x - 0.4] x [0, extent_y], and `edge` points in the last 0.25 m of x.  At stride 4 the
    defaults give 7 x 5 windows of which the last column in x is 0.3 m wide and holds only the edge points' memberships
    (fewer than 64 in all) while every other window holds a 4 m share of the patch: whichever way numpy's argsort breaks the
    merge's ties, no merged block ends between min_block_points = 64 and block_points / 2 = 128 points.  `snapped`:
    coordinates on a 0.05 m lattice -> (n,3) f32 points, (n,) f32 remissions"""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)) * [extent_x - 0.4, extent_y]
    u[:edge, 0] = extent_x - 0.25 * rng.random(edge)
    p = np.concatenate([u, rng.standard_normal((n, 1)) * 0.03 - 1.7], 1)
    p[n - n // 6:, 2] += rng.random(n // 6) * 2.5
    p[0, 0], p[n - 1, 0:2], p[n - 2, 1] = extent_x, 0.0, extent_y  # the extent is exact
    p = p[np.argsort(np.arctan2(p[:, 1] - extent_y / 2, p[:, 0] - extent_x / 2), kind="stable")]
    if snapped:
        p = np.round(p / 0.05) * 0.05
    return p.astype(np.float32), rng.random(n).astype(np.float32)


def bounds(xyz):
    """D:289-290 -> coordmin (3,) f32, coordmax (3,) f32"""
    return np.min(xyz[:, 0:3], axis=0), np.max(xyz[:, 0:3], axis=0)


def grid(coordmin, coordmax, stride):
    """D:291-292"""
    nx = np.ceil((coordmax[0] - coordmin[0]) / stride).astype(np.int32)
    ny = np.ceil((coordmax[1] - coordmin[1]) / stride).astype(np.int32)
    return int(nx), int(ny)


def window_box(coordmin, coordmax, i, j, block_size, stride):
    """D:298-299 -> curmin, curmax float64 (3,)"""
    curmin = coordmin + [i * stride, j * stride, 0]
    curmax = curmin + [block_size, block_size, coordmax[2] - coordmin[2]]
    return curmin, curmax


def windows(xyz, block_size, stride, shape=None):
    """D:289-308 without the payload -> coordmin, coordmax, (nx, ny), and per window in i-major order, EMPTY ONES INCLUDED,
    members (ascending scan indices) and centres (2,) f64.  shape: (nx, ny) in place of D:291-292 (for a scan without extent)"""
    coordmin, coordmax = bounds(xyz)
    nx, ny = grid(coordmin, coordmax, stride) if shape is None else shape
    members, centers = [], []
    for i in range(nx):
        for j in range(ny):
            curmin, curmax = window_box(coordmin, coordmax, i, j, block_size, stride)
            curchoice = np.sum((xyz[:, 0:3] >= (curmin - 0.2)) * (xyz[:, 0:3] <= (curmax + 0.2)), axis=1) == 3
            members.append(np.where(curchoice)[0])
            centers.append((curmin[0:2] + curmax[0:2]) / 2.0)
    return coordmin, coordmax, (nx, ny), members, centers


def nearest(center, centers):
    """D:271-276"""
    dist = np.zeros(len(centers))
    for i in range(len(centers)):
        dist[i] = np.linalg.norm(centers[i] - center, ord=2)
    return np.argsort(dist)[0]


def nearest_batched(center, centers):
    """D:271-276 with the distance array from one expression that ends, as np.linalg.norm does, in the BLAS dot"""
    d = np.asarray(centers, np.float64).reshape(-1, 2) - center
    return np.argsort(np.sqrt(np.matmul(d[:, None, :], d[:, :, None])[:, 0, 0]))[0]


def merge(sizes, centers, min_block_points=4096, nearest=nearest):
    """D:311-327 over counts and centres only -> per final block the ordered list of positions (into `sizes`) whose member
    lists are concatenated.  A block at or under min_block_points (an empty window too) is popped and appended to the
    nearest remaining one; the cursor stays, so the block that slid into its place is looked at next."""
    sizes, centers = [int(s) for s in sizes], [np.asarray(c, np.float64) for c in centers]
    parts = [[k] for k in range(len(sizes))]
    at = 0
    while at < len(sizes):
        if sizes[at] > min_block_points:
            at += 1
            continue
        size, center, part = sizes.pop(at), centers.pop(at), parts.pop(at)
        if len(sizes) == 0:
            raise ValueError("every block holds at most min_block_points points: np.argsort of no distance has no [0]")
        to = nearest(center, centers)
        sizes[to] += size
        parts[to] = parts[to] + part
    return parts


def draw_rows(length, block_points, rng):
    """D:337-345 for one block of `length` points -> the padded, shuffled positions (a multiple of block_points)"""
    order = np.array([x for x in range(length)])
    if order.shape[0] % block_points != 0:
        makeup = block_points - order.shape[0] % block_points
        if makeup > length:
            raise ValueError("the make-up slice is shorter than makeup_num: the reference's chunks are ragged")
        rng.shuffle(order)
        order = np.concatenate((order, order[0:makeup].copy()))
    rng.shuffle(order)
    return order


def rotate_z(batch_data, angles):
    """utils/provider.py:71-89 with the angles given (rng.uniform() * 2 * np.pi each) -> float32"""
    rotated = np.zeros(batch_data.shape, dtype=np.float32)
    for k in range(batch_data.shape[0]):
        cosval, sinval = np.cos(angles[k]), np.sin(angles[k])
        rotation_matrix = np.array([[cosval, sinval, 0], [-sinval, cosval, 0], [0, 0, 1]])
        rotated[k, ...] = np.dot(batch_data[k, ...].reshape((-1, 3)), rotation_matrix)
    return rotated


def predict(logits):
    """T:166"""
    return np.argmax(logits[:, :, 1:], 2) + 1


def add_vote(pool, point_idx, pred):
    """T:99-105 (integer increments: order-free)"""
    np.add.at(pool, (np.asarray(point_idx).astype(np.int64).ravel(), np.asarray(pred).astype(np.int64).ravel()), 1)
    return pool


def final_preds(pool):
    """T:174-175"""
    return np.argmax(pool, axis=1).astype(np.uint32)


def class_counts(label, pred, num_classes):
    """T:202-211 -> seen, correct, iou_deno (num_classes,) int64"""
    seen = np.array([np.sum(label == l) for l in range(num_classes)], np.int64)
    correct = np.array([np.sum((pred == l) & (label == l)) for l in range(num_classes)], np.int64)
    deno = np.array([np.sum((pred == l) | (label == l)) for l in range(num_classes)], np.int64)
    return seen, correct, deno


def scan_iou(seen, correct, deno):
    """T:212-214 -> iou of classes 1..C-1, its mean over the classes the scan holds"""
    iou = np.array(correct[1:]) / (np.array(deno[1:], dtype=float) + 1e-6)
    return iou, np.mean(iou[np.array(seen[1:]) != 0])


class KittiWindowFlowRef:
    """scans: a list of (N,3) float32 arrays; labels: a list of (N,) int32 arrays or None (split 'test'); remissions: a list
    of (N,) float32 arrays or None."""

    def __init__(self, scans, labels=None, remissions=None, num_classes=20, block_points=8192, batch_size=6, block_size=10, stride=4,
                 min_block_points=4096, random_rotate=False, rng=np.random, accumulate_votes=False, nearest=nearest):
        self.scans, self.labels, self.remissions, self.C, self.P, self.B = scans, labels, remissions, num_classes, block_points, batch_size
        self.block_size, self.stride, self.min_block_points, self.random_rotate = block_size, stride, min_block_points, random_rotate
        self.rng, self.accumulate_votes, self.nearest = rng, accumulate_votes, nearest
        self.pools, self.pred, self.counts, self.logged = {}, {}, {}, {}
        self.total = [np.zeros(num_classes, np.int64) for _ in range(3)]
        self.total_correct, self.total_seen, self.labelweights = 0, 0, np.zeros(num_classes)
        self.last = None  # what the latest getitem saw, for the tests
        self.seconds = dict(windows=0.0, merge=0.0)

    def getitem(self, i):
        """-> div_blocks (R,P,3|4) f32, div_blocks_idxs (R,P) i64"""
        import time

        pts = self.scans[i]
        t0 = time.perf_counter()
        coordmin, coordmax, (nx, ny), members, centers = windows(pts, self.block_size, self.stride)
        t1 = time.perf_counter()
        parts = merge([len(m) for m in members], centers, self.min_block_points, self.nearest)
        self.seconds["windows"] += t1 - t0
        self.seconds["merge"] += time.perf_counter() - t1
        self.last = dict(coordmin=coordmin, coordmax=coordmax, nx=nx, ny=ny, members=members, centers=centers, parts=parts)
        full = pts if self.remissions is None else np.concatenate((pts, np.expand_dims(self.remissions[i], axis=1)), axis=1)
        data, idx = [], []
        for part in parts:
            mem = np.concatenate([members[k] for k in part])
            chosen = mem[draw_rows(len(mem), self.P, self.rng)].reshape(-1, self.P)
            data.append(full[chosen])
            idx.append(chosen)
        return np.concatenate(data), np.concatenate(idx)

    def run(self, forward, num_votes=1):
        """T:123-231: scans in order, votes inside.  forward: (B,P,3|4) f32 -> (B,P,C) f32 logits; the rows past the last real
        one of a scan's final batch are fed zeros (the reference leaves stale rows there and never votes them)."""
        for i in range(len(self.scans)):
            n = self.scans[i].shape[0]
            pool = np.zeros((n, self.C))
            for vote in range(num_votes):
                data, idx = self.getitem(i)
                if not self.accumulate_votes:
                    pool = np.zeros((n, self.C))  # T:168-169
                for start in range(0, data.shape[0], self.B):
                    real = min(self.B, data.shape[0] - start)
                    batch = np.zeros((self.B,) + data.shape[1:], np.float32)
                    batch[:real] = data[start:start + real]
                    if self.random_rotate:
                        angles = [self.rng.uniform() * 2 * np.pi for _ in range(self.B)]
                        batch[:, :, :3] = rotate_z(batch[:, :, :3].astype(np.float64), angles)
                    pred = predict(forward(batch))
                    add_vote(pool, idx[start:start + real], pred[:real])
            self.pools[i] = pool
            self.pred[i] = final_preds(pool)
            if self.labels is not None:
                self.score(i)

    def score(self, i):
        """T:196-231"""
        label, pred = self.labels[i], self.pred[i]
        self.total_correct += np.sum(pred == label)
        self.total_seen += len(label)
        tmp, _ = np.histogram(label, range(self.C + 1))
        self.labelweights += tmp
        self.counts[i] = class_counts(label, pred, self.C)
        for acc, c in zip(self.total, self.counts[i]):
            acc += c
        if i % 10 == 0:
            seen, correct, deno = self.total
            with np.errstate(divide="ignore", invalid="ignore"):
                out = dict(miou=np.mean(np.array(correct[1:]) / (np.array(deno[1:], dtype=float) + 1e-6)),
                           accuracy=self.total_correct / float(self.total_seen),
                           class_accuracy=np.mean(np.array(correct) / (np.array(seen, dtype=float) + 1e-6)))
                self.labelweights = self.labelweights.astype(np.float32) / np.sum(self.labelweights.astype(np.float32))
                out["labelweights"] = np.array([self.labelweights[l - 1] for l in range(1, self.C)])
                out["iou"] = np.array([correct[l] / float(deno[l]) for l in range(1, self.C)])
            self.logged[i] = out
