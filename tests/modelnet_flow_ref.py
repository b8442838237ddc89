"""numpy restatement of the ModelNet40 evaluation flow, the yardstick of pointasnl_amd.modelnet_tester: the dataset of the
reference's modelnet_dataset.py (D) -- both sampling modes, pc_normalize, the cache, batches whose last one is short -- and
the epoch of test.py (T) :105-174 with the noisy points of utils/provider.py (P) :8-24.  It works on in-memory shapes,
drives a `forward` callable and takes the RNG (np.random or a RandomState) as an argument; every expression is numpy's own
in the reference's dtypes, so bits can be compared.  tests/test_modelnet_tester_flow.py pins it to the reference's class."""
import numpy as np


def shape(seed, n, kind="blob"):
    """a seeded raw shape (n, 6) float32: xyz and a unit normal.  'blob': an anisotropic off-centre gaussian cloud;
    'lattice': coordinates on multiples of 1/8 (distance ties); 'dup': every point of a small blob repeated about four times"""
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "lattice":
        xyz = np.round(rng.random((n, 3)) * 8) / 8
    elif kind == "dup":
        base = rng.standard_normal((max(1, n // 4), 3))
        xyz = base[rng.integers(0, base.shape[0], n)]
    else:
        xyz = rng.standard_normal((n, 3)) * np.array([1.0, 0.6, 0.3]) + np.array([0.4, -0.2, 1.5])
    nrm = rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.ascontiguousarray(np.hstack([xyz, nrm]).astype(np.float32))


def pc_normalize(pc):
    """D:9-14: centre on the float32 mean, scale by the largest float32 norm"""
    centred = pc - np.mean(pc, axis=0)
    return centred / np.max(np.sqrt(np.sum(centred ** 2, axis=1)))


def fps_indices(point, npoint, rng):
    """D:16-35: numpy's farthest point sampling -> the npoint indices (int64); draws rng.randint(0, N) once"""
    xyz = point[:, :3]
    running = np.ones((point.shape[0],)) * 1e10
    picks = np.zeros((npoint,))
    nxt = rng.randint(0, point.shape[0])
    for r in range(npoint):
        picks[r] = nxt
        d = np.sum((xyz - xyz[nxt, :]) ** 2, -1)
        closer = d < running
        running[closer] = d[closer]
        nxt = np.argmax(running, -1)
    return picks.astype(np.int32).astype(np.int64)


def normalize_data(batch_data):
    """P:8-24: every (N, C) block of a float64 batch centred and scaled on its own"""
    out = np.zeros(batch_data.shape)
    for b in range(batch_data.shape[0]):
        centred = batch_data[b] - np.mean(batch_data[b], axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[b] = centred / np.max(np.sqrt(np.sum(centred ** 2, axis=1)))
    return out


class ModelNetFlowRef:
    """D:39-136 over arrays: shapes a list of (n_i, 6) float32, labels their classes"""

    def __init__(self, shapes, labels, batch_size=32, npoints=1024, normalize=True, normal_channel=False, cache_size=15000,
                 shuffle=False, uniform=False, rng=np.random):
        self.shapes, self.labels = [np.asarray(s, np.float32) for s in shapes], np.asarray(labels)
        self.batch_size, self.npoints, self.normalize, self.normal_channel = batch_size, npoints, normalize, normal_channel
        self.cache_size, self.shuffle, self.uniform, self.rng = cache_size, shuffle, uniform, rng
        self.cache = {}
        self.fps_draws = 0
        self.reset()

    def __len__(self):
        return len(self.shapes)

    def num_channel(self):
        return 6 if self.normal_channel else 3

    def get_item(self, index):
        if index in self.cache:
            return self.cache[index]
        cls = np.array([self.labels[index]]).astype(np.int32)
        raw = self.shapes[index].copy()  # the reference reads the file anew
        if self.uniform:
            self.fps_draws += 1
            point_set = raw[fps_indices(raw, self.npoints, self.rng)]
        else:
            point_set = raw[0:self.npoints, :]
        if self.normalize:
            point_set[:, 0:3] = pc_normalize(point_set[:, 0:3])
        if not self.normal_channel:
            point_set = point_set[:, 0:3]
        if len(self.cache) < self.cache_size:
            self.cache[index] = (point_set, cls)
        return point_set, cls

    def reset(self):
        self.idxs = np.arange(0, len(self.shapes))
        if self.shuffle:
            self.rng.shuffle(self.idxs)
        self.num_batches = (len(self.shapes) + self.batch_size - 1) // self.batch_size
        self.batch_idx = 0

    def has_next_batch(self):
        return self.batch_idx < self.num_batches

    def next_batch(self):
        lo = self.batch_idx * self.batch_size
        hi = min(lo + self.batch_size, len(self.shapes))
        data = np.zeros((hi - lo, self.npoints, self.num_channel()))
        label = np.zeros((hi - lo), dtype=np.int32)
        for i in range(hi - lo):
            data[i], cls = self.get_item(self.idxs[lo + i])
            label[i] = cls[0]
        self.batch_idx += 1
        return data, label


def cross_entropy(logits, labels):
    """mean sparse-softmax cross-entropy of a batch, float64"""
    x = np.asarray(logits, np.float64)
    mx = x.max(axis=1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(axis=1)) + mx[:, 0]
    return float(np.mean(lse - x[np.arange(x.shape[0]), labels]))


def eval_one_epoch(ds, forward, num_classes, num_votes=1, num_noisy_point=0, rng=np.random, reg_loss=0.0):
    """T:105-174 over the dataset `ds`.  forward: (B, N, ch) float32 -> (B, num_classes) float32 logits.  -> dict: accuracy,
    the counters, mean_loss, and per batch what was fed (float32), the labels, the float64 vote sums and the predictions."""
    B, N = ds.batch_size, ds.npoints
    cur_data = np.zeros((B, N, ds.num_channel()))
    cur_label = np.zeros((B), dtype=np.int32)
    out = dict(total_correct=0, total_seen=0, total_object=0, seen_class=np.zeros(num_classes, np.int64),
               correct_class=np.zeros(num_classes, np.int64), fed=[], labels=[], sums=[], preds=[], bsizes=[])
    loss_sum = 0
    while ds.has_next_batch():
        data, label = ds.next_batch()
        bsize = data.shape[0]
        if num_noisy_point > 0:
            noisy = normalize_data(rng.random((bsize, num_noisy_point, 3)))
            data[:bsize, :num_noisy_point, :3] = noisy
        cur_data[0:bsize, ...] = data
        cur_label[0:bsize] = label
        sums = np.zeros((B, num_classes))
        loss_vote = 0
        fed = cur_data.astype(np.float32)  # the feed into a float32 placeholder
        for _ in range(num_votes):
            rng.shuffle(np.arange(N))  # drawn and never used
            logits = np.asarray(forward(fed), np.float32)
            sums += logits
            loss_vote += cross_entropy(logits, cur_label) + reg_loss
        loss_vote /= num_votes
        pred = np.argmax(sums, 1)
        out["total_correct"] += int(np.sum(pred[0:bsize] == label[0:bsize]))
        out["total_seen"] += bsize
        out["total_object"] += B
        loss_sum += loss_vote
        for i in range(bsize):
            out["seen_class"][label[i]] += 1
            out["correct_class"][label[i]] += int(pred[i] == label[i])
        out["fed"].append(fed)
        out["labels"].append(cur_label.copy())
        out["sums"].append(sums)
        out["preds"].append(pred[:bsize].astype(np.int32))
        out["bsizes"].append(bsize)
    ds.reset()
    out["mean_loss"] = loss_sum / float(out["total_object"])
    out["accuracy"] = out["total_correct"] / float(out["total_seen"])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["class_accuracy"] = np.array(out["correct_class"]) / np.array(out["seen_class"], dtype=float)
    return out


def report(out, shape_names):
    """the lines T:166-172 log"""
    lines = ["Eval mean loss: %f" % out["mean_loss"], "Eval accuracy: %f" % out["accuracy"],
             "Eval avg class acc: %f" % np.mean(out["class_accuracy"])]
    return lines + ["%10s:\t%0.3f" % (name, out["class_accuracy"][i]) for i, name in enumerate(shape_names)]


def robustness(ds, forward, num_classes, num_votes=1, noise_points=(1, 10, 50, 100), rng=np.random):
    """T:93-103 -> (acc, [acc per level], the table's text)"""
    acc = eval_one_epoch(ds, forward, num_classes, num_votes, 0, rng)["accuracy"]
    txt = "Noise    Accuracy\n" + " 000       %.3f\n" % acc
    levels = []
    for k in noise_points:
        levels.append(eval_one_epoch(ds, forward, num_classes, num_votes, k, rng)["accuracy"])
        txt += " %03d       %.3f\n" % (k, levels[-1])
    return acc, levels, txt


def stand_in_weights(seed, ch, num_classes):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((ch, num_classes)) * 0.9).astype(np.float32), rng.standard_normal(num_classes).astype(np.float32)


def stand_in_forward_np(data, w, b):
    """a fixed map of a cloud to C logits (the end-to-end tests' model): the per-cloud maximum over the points of
    sin(row @ w + b) * 4, float32 -- every point of the cloud matters, its order does not"""
    x = np.sin(np.nan_to_num(data.astype(np.float32), nan=0.5) @ w + b) * np.float32(4)
    return x.max(axis=1).astype(np.float32)
