"""numpy restatement of the SemanticKITTI test loop (reference SemanticKITTI/semantic_kitti_dataset_grid.py (D) :192-245 and
test_semantic_kitti_grid.py (T) :128-180), the yardstick of pointasnl_amd.SemanticKITTI.scan_tester.  The search tree is
replaced by an exact nearest-first order on sklearn's key (the float64 ((dx*dx)+(dy*dy))+(dz*dz) of the float32 points),
ties by the lowest index; tests/test_scan_tester_flow.py pins this file to the reference's own generator."""
import numpy as np


def scan(seed, n, snapped=False):
    """a lidar-like scan in metres (the generator of tests/test_oracle_crop.py): ground disc with 1/r density + vertical
    walls; `snapped`: coordinates on a 0.06 m lattice (distance ties by construction)"""
    rng = np.random.default_rng(seed)
    r = 2.0 + 38.0 * rng.random(n) ** 2
    th = rng.random(n) * 2 * np.pi
    p = np.stack([r * np.cos(th), r * np.sin(th), rng.standard_normal(n) * 0.02], 1)
    w = n // 6
    p[:w, 2] = rng.random(w) * 2.0
    if snapped:
        p = np.round(p / 0.06) * 0.06
    return p.astype(np.float32)


def nearest_first(pc64, centre, k):
    d = pc64 - centre
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return np.lexsort((np.arange(len(pc64)), d2))[:k], d2


def softmax_f32(logits):
    x = np.asarray(logits, np.float32)
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


class ScanFlowRef:
    def __init__(self, scans, num_classes=20, num_point=10240, num_buffer=1024, batch_size=8, test_smooth=0.98, rng=np.random):
        self.scans = [np.ascontiguousarray(s, np.float32) for s in scans]
        self.pc = [s.astype(np.float64) for s in self.scans]  # sklearn's float64 copy (search_tree.data)
        self.C, self.num_point, self.num_buffer, self.B, self.test_smooth, self.rng = (
            num_classes, num_point, num_buffer, batch_size, test_smooth, rng)
        self.possibility, self.min_possibility = [], []
        for s in self.scans:  # D:206-209
            self.possibility += [rng.rand(s.shape[0]) * 1e-3]
            self.min_possibility += [float(np.min(self.possibility[-1]))]
        self.test_probs = [np.zeros(shape=[len(l), num_classes], dtype=np.float16) for l in self.possibility]

    def crop(self):
        """one crop of D:224-234 -> (cloud_ind, pick_idx, selected_idx)"""
        cloud_ind = int(np.argmin(self.min_possibility))
        pick_idx = np.argmin(self.possibility[cloud_ind])
        pc = self.pc[cloud_ind]
        buffer = self.num_buffer + self.rng.randint(0, self.num_buffer // 4)
        select_idx, _ = nearest_first(pc, pc[pick_idx], self.num_point + buffer)
        idx = np.arange(len(select_idx))
        self.rng.shuffle(idx)
        selected_idx = select_idx[idx][:self.num_point]
        selected_pc = pc[selected_idx]
        dists = np.sum(np.square((selected_pc - pc[pick_idx]).astype(np.float32)), axis=1)
        delta = np.square(1 - dists / np.max(dists))
        self.possibility[cloud_ind][selected_idx] += delta
        self.min_possibility[cloud_ind] = np.min(self.possibility[cloud_ind])
        return cloud_ind, int(pick_idx), selected_idx

    def batch(self):
        crops = [self.crop() for _ in range(self.B)]
        pts = np.stack([self.scans[c][s] for c, _, s in crops])
        inds = np.stack([s for _, _, s in crops]).astype(np.int32)
        clouds = np.array([[c] for c, _, _ in crops], dtype=np.int32)
        return pts, inds, clouds, crops

    def vote(self, stacked_probs, point_inds, cloud_inds):
        """T:147-154, literally"""
        test_smooth = self.test_smooth
        for j in range(np.shape(stacked_probs)[0]):
            probs = stacked_probs[j, :, :]
            inds = point_inds[j, :]
            c_i = np.reshape(cloud_inds, (-1,))[j]
            self.test_probs[c_i][inds] = test_smooth * self.test_probs[c_i][inds] + (1 - test_smooth) * probs

    def run(self, forward, num_votes=1, max_epochs=None, log=None):
        """T:128-160: epochs of int(S/B)*B*4 crops until min(min_possibility) > num_votes.  forward: (B,num_point,3) -> logits."""
        num_per_epoch = int(len(self.scans) / self.B) * self.B * 4
        epochs = 0
        while True:
            for _ in range(num_per_epoch // self.B):
                pts, inds, clouds, crops = self.batch()
                if log is not None:
                    log.extend(crops)
                self.vote(softmax_f32(forward(pts)), inds, clouds)
            epochs += 1
            if np.min(self.min_possibility) > num_votes or (max_epochs is not None and epochs >= max_epochs):
                return epochs

    def reproject(self, i, proj_inds=None, remap_lut=None):
        """T:165-178"""
        probs = self.test_probs[i] if proj_inds is None else self.test_probs[i][proj_inds, :]
        pred = np.argmax(probs, 1).astype(np.uint32)
        upper_half = pred >> 16
        lower_half = pred & 0xFFFF
        if remap_lut is not None:
            lower_half = remap_lut[lower_half]
        return ((upper_half << 16) + lower_half).astype(np.uint32)


def proj_brute(sub, raw):
    """the nearest sub point of every raw point on sklearn's float64 key, ties to the lowest index"""
    s = np.asarray(sub, np.float32).astype(np.float64)
    out = np.empty(len(raw), np.int64)
    for j, q in enumerate(np.asarray(raw, np.float32).astype(np.float64)):
        d = s - q
        out[j] = np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return out


def stand_in_forward_np(pts, w, b):
    """a fixed map of xyz to C logits (the end-to-end tests' model): sin(xyz @ w + b) * 4, float32"""
    return (np.sin(pts.astype(np.float32) @ w + b) * np.float32(4)).astype(np.float32)
