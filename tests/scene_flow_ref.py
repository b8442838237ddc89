"""numpy restatement of the ScanNet grid test and validation loops (reference ScanNet/scannet_dataset_grid.py (D) :435-549
and ScanNet/test_scannet_grid.py (T) :95-229 / :231-448, utils/metrics.py:120-146), the yardstick of
pointasnl_amd.ScanNet.scene_tester.  The search tree is replaced by an exact nearest-first order on sklearn's key (the
float64 ((dx*dx)+(dy*dy))+(dz*dz) of the float32 points against the float64 pick), ties by the lowest index;
tests/test_scene_tester_flow.py pins this file to the reference's own generator and metrics."""
import numpy as np

from scan_flow_ref import nearest_first, softmax_f32  # noqa: F401  (re-exported for the tests)


def scene(seed, n, snapped=False):
    """an indoor-like scene in metres: a 6 x 5 m floor, two walls and boxes of furniture, with colours in [0, 1);
    `snapped`: coordinates on a 0.04 m lattice (distance ties by construction) -> (points (n,3) f32, colors (n,3) f32)"""
    rng = np.random.default_rng(seed)
    p = np.empty((n, 3))
    a, b = n // 2, n // 2 + n // 4
    p[:a] = np.stack([rng.random(a) * 6, rng.random(a) * 5, rng.standard_normal(a) * 0.01], 1)         # floor
    w = b - a
    side = rng.random(w) < 0.5
    p[a:b] = np.stack([np.where(side, rng.random(w) * 6, 0.0), np.where(side, 0.0, rng.random(w) * 5), rng.random(w) * 2.6], 1)
    m = n - b
    box = rng.integers(0, 5, m)
    corner = rng.random((5, 2)) * np.array([5.0, 4.0])
    p[b:] = np.stack([corner[box, 0] + rng.random(m), corner[box, 1] + rng.random(m), rng.random(m) * 0.9], 1)
    if snapped:
        p = np.round(p / 0.04) * 0.04
    return p.astype(np.float32), rng.random((n, 3)).astype(np.float32)


def insert_ignored(probs, label_values, ignored_labels):
    """T:196-199: a zero column at the position of every ignored label"""
    probs2 = probs.copy()
    for l_ind, label_value in enumerate(label_values):
        if label_value in ignored_labels:
            probs2 = np.insert(probs2, l_ind, 0, axis=1)
    return probs2


def confusion(targets, preds, label_values):
    """sklearn.metrics.confusion_matrix(targets, preds, labels=label_values): int64 counts, unlisted values dropped"""
    lv = np.asarray(label_values)
    out = np.zeros((len(lv), len(lv)), np.int64)
    t, p = np.asarray(targets).reshape(-1), np.asarray(preds).reshape(-1)
    for i, a in enumerate(lv):
        for j, b in enumerate(lv):
            out[i, j] = np.count_nonzero((t == a) & (p == b))
    return out


def drop_ignored(C, label_values, ignored_labels):
    """T:341-345"""
    for l_ind, label_value in reversed(list(enumerate(label_values))):
        if label_value in ignored_labels:
            C = np.delete(C, l_ind, axis=0)
            C = np.delete(C, l_ind, axis=1)
    return C


def iou_from_confusions(confusions):
    """utils/metrics.py:120-146"""
    TP = np.diagonal(confusions, axis1=-2, axis2=-1)
    TP_plus_FN = np.sum(confusions, axis=-1)
    TP_plus_FP = np.sum(confusions, axis=-2)
    IoU = TP / (TP_plus_FP + TP_plus_FN - TP + 1e-6)
    mask = TP_plus_FN < 1e-3
    counts = np.sum(1 - mask, axis=-1, keepdims=True)
    mIoU = np.sum(IoU, axis=-1, keepdims=True) / (counts + 1e-6)
    IoU += mask * mIoU
    return IoU


class SceneFlowRef:
    def __init__(self, scenes, colors=None, labels=None, num_classes=21, num_point=8192, num_buffer=1024, batch_size=4, split="test",
                 validation_size=500, label_values=None, ignored_labels=(0,), rng=np.random):
        self.scenes = [np.ascontiguousarray(s, np.float32) for s in scenes]
        self.pc = [s.astype(np.float64) for s in self.scenes]  # sklearn's float64 copy (input_trees[...].data)
        self.colors = colors if colors is not None else [np.zeros((len(s), 3), np.float32) for s in scenes]
        self.labels = labels
        self.C, self.npoint, self.buffer, self.B, self.split, self.validation_size, self.rng = (
            num_classes, num_point, num_buffer, batch_size, split, validation_size, rng)
        self.label_values = np.arange(num_classes) if label_values is None else np.asarray(label_values)
        self.ignored_labels = np.asarray(ignored_labels)
        self.label_to_idx = {l: i for i, l in enumerate(self.label_values)}
        self.test_smooth = 0.98 if split == "test" else 0.95  # T:101, 234
        self.potentials, self.min_potentials = [], []
        for s in self.scenes:  # D:472-478
            self.potentials += [rng.rand(s.shape[0]) * 1e-3]
            self.min_potentials += [float(np.min(self.potentials[-1]))]
        self.test_probs = [np.zeros((s.shape[0], num_classes - 1), dtype=np.float32) for s in self.scenes]
        self.checkpoints = []

    def crop(self):
        """one crop of D:482-541 -> dict(cloud_ind, point_ind, pick_point, input_inds, input_points, features, labels)"""
        cloud_ind = int(np.argmin(self.min_potentials))
        point_ind = np.argmin(self.potentials[cloud_ind])
        points = self.pc[cloud_ind]
        center_point = points[point_ind, :].reshape(1, -1)
        noise = self.rng.normal(scale=0.35, size=center_point.shape)
        pick_point = center_point + noise.astype(center_point.dtype)
        buffer = self.buffer + self.rng.randint(0, self.buffer // 4)
        assert len(points) >= self.npoint + buffer, "the restatement covers scenes that hold k points"
        input_inds, _ = nearest_first(points, pick_point[0], self.npoint + buffer)
        idx = np.arange(len(input_inds))
        self.rng.shuffle(idx)
        input_inds = input_inds[idx][:self.npoint]
        dists = np.sum(np.square((points[input_inds] - pick_point).astype(np.float32)), axis=1)
        delta = np.square(1 - dists / np.max(dists))
        self.potentials[cloud_ind][input_inds] += delta
        self.min_potentials[cloud_ind] = float(np.min(self.potentials[cloud_ind]))
        input_points = (points[input_inds] - pick_point).astype(np.float32)
        input_colors = self.colors[cloud_ind][input_inds]
        if self.split == "test" or self.labels is None:
            input_labels = np.zeros(input_points.shape[0])
        else:
            input_labels = np.array([self.label_to_idx[l] for l in self.labels[cloud_ind][input_inds]])
        features = np.hstack((input_colors, input_points + pick_point))
        return dict(cloud_ind=cloud_ind, point_ind=int(point_ind), pick_point=pick_point[0].copy(), input_inds=input_inds,
                    input_points=input_points, features=features, labels=input_labels)

    def batch(self, abs_coords=False, with_rgb=True):
        """-> inputs (B,npoint,3+F[+3]) f32 (what the model is fed), point_inds (B,npoint) i32, cloud_inds (B,) i32, crops"""
        crops = [self.crop() for _ in range(self.B)]
        cols = lambda c: [c["input_points"]] + ([c["features"][:, :3]] if with_rgb else []) + (  # noqa: E731
            [c["features"][:, 3:]] if abs_coords else [])
        inputs = np.stack([np.hstack(cols(c)).astype(np.float32) for c in crops])
        inds = np.stack([c["input_inds"] for c in crops]).astype(np.int32)
        clouds = np.array([c["cloud_ind"] for c in crops], dtype=np.int32)
        return inputs, inds, clouds, crops

    def vote(self, stacked_probs, point_inds, cloud_inds):
        """T:141-149 / 283-291, literally"""
        test_smooth = self.test_smooth
        for b in range(stacked_probs.shape[0]):
            probs = stacked_probs[b]
            inds = point_inds[b]
            c_i = cloud_inds[b]
            self.test_probs[c_i][inds] = test_smooth * self.test_probs[c_i][inds] + (1 - test_smooth) * probs

    def run(self, forward, num_votes=100, on_checkpoint=None, max_epochs=None, log=None, with_rgb=True):
        """T:128-227 / T:271-446: epochs of validation_size batches while last_min < num_votes, each split's checkpoint rule.
        forward: inputs -> (B,npoint,C) logits; the votes take softmax(logits[..., 1:]) (T:95)."""
        epochs, last_min = 0, -0.5
        while last_min < num_votes:
            for _ in range(self.validation_size):
                inputs, inds, clouds, crops = self.batch(with_rgb=with_rgb)
                if log is not None:
                    log.extend(crops)
                self.vote(softmax_f32(forward(inputs)[:, :, 1:]), inds, clouds)
            new_min = np.min(self.min_potentials)
            if self.split == "test":
                if last_min + 2 < new_min:
                    last_min = new_min
                    self.checkpoints.append((epochs, float(new_min)))
                    if on_checkpoint is not None:
                        on_checkpoint(self, new_min)
            else:
                if last_min + 1 < new_min:
                    last_min += 1
                    self.checkpoints.append((epochs, float(new_min)))
                    if on_checkpoint is not None:
                        on_checkpoint(self, new_min)
            epochs += 1
            if max_epochs is not None and epochs >= max_epochs:
                break
        return epochs

    def reproject(self, i, proj_inds=None):
        """T:190-205 -> preds int32, pots float64, probs float32"""
        proj = np.arange(len(self.scenes[i])) if proj_inds is None else np.asarray(proj_inds)
        probs = self.test_probs[i][proj, :]
        probs2 = insert_ignored(probs, self.label_values, self.ignored_labels)
        preds = self.label_values[np.argmax(probs2, axis=1)].astype(np.int32)
        pots = self.potentials[i][proj]
        return preds, pots, probs

    def confusion(self, targets, proj_inds=None):
        """T:319-339 (sub clouds) / T:378-398 (full meshes): the summed confusion matrix"""
        Confs = []
        for i in range(len(self.scenes)):
            preds, _, _ = self.reproject(i, None if proj_inds is None else proj_inds[i])
            Confs += [confusion(targets[i], preds, self.label_values)]
        return np.sum(np.stack(Confs), axis=0)


def stand_in_forward_np(x, w, b):
    """a fixed map of the model input's columns to C logits (the end-to-end tests' model): sin(x @ w + b) * 4, float32"""
    return (np.sin(x.astype(np.float32) @ w + b) * np.float32(4)).astype(np.float32)
