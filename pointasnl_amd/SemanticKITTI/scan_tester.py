"""The SemanticKITTI test loop on the device -- reference SemanticKITTI/semantic_kitti_dataset_grid.py (D) :192-245
(`get_batch_gen('test')`: possibility init, pick, crop, possibility update) and test_semantic_kitti_grid.py (T) :128-180
(`ModelTester.test`: votes into float16 tables, stop rule, reprojection, .label files).

`ScanTester` holds every scan of a sequence in one flat device buffer, with its possibility (float64) and its votes
(float16) beside it.  `next_batch()` enqueues, crop after crop, pick -> crop -> nearest-first order and shuffle -> update on
the current stream (csrc/scan_test.hip, csrc/crop.hip): no host synchronisation, capturable.  The only RNG draws of the
flow -- the possibility init, crop_pc's `buffer` and its shuffle -- depend on lengths the host knows, so they are drawn on
the host from the caller's numpy RandomState in the reference's order, and the crop sequence is the reference's, crop for
crop (tests/scan_flow_ref.py restates the flow in numpy; tests/test_scan_tester_flow.py pins it to the reference's
generator).  Only the k form of crop_pc (in_radius == 0, the reference default) is covered here; the radius form is
scan_radius.RadiusScanTester.

Deviations: the crops are fed unaugmented (the reference maps tf_augment_input over the test crops with TF's RNG, which
cannot be reproduced); the softmax of a vote is computed here in float32, not by TensorFlow (a vote may differ by one
float16 ulp); proj_inds computed here break distance ties by the lowest index (sklearn: by its tree's order).
"""
import ctypes
import math

import numpy as np
import torch

from pointasnl_amd import _hip

DESC_BYTES = 40     # sizeof(pasnl_scan_crop_t)
ORDER_CAP = 14336   # pasnl_crop_order_permute: kcap limit of the LDS sort


_p = _hip.ptr


class ScanTester:
    """`ScanTester(scans, num_classes=20, num_point=10240, num_buffer=1024, batch_size=8, test_smooth=0.98, rng=np.random)`.

    scans: a list of (n_i,3) float32 sub-sampled scans (numpy arrays or device tensors, e.g. grid_subsampling output), in
    the order of the reference's test_list.  The possibility init draws `rng.rand(n_i) * 1e-3` scan after scan here, as
    get_batch_gen('test') does; every crop then draws `rng.randint(0, num_buffer // 4)` and `rng.shuffle` of its k indices."""

    def __init__(self, scans, num_classes=20, num_point=10240, num_buffer=1024, batch_size=8, test_smooth=0.98, rng=np.random,
                 in_radius=0.0):
        if in_radius > 0:
            raise NotImplementedError("ScanTester covers crop_pc's k form only (in_radius == 0): the radius form is "
                                      "pointasnl_amd.SemanticKITTI.scan_radius.RadiusScanTester")
        self._init_scans(scans, num_classes, num_point, num_buffer, batch_size, test_smooth, rng)

    def _init_scans(self, scans, num_classes, num_point, num_buffer, batch_size, test_smooth, rng, k_form=True):
        """the scans, possibilities and votes; k_form: the checks and buffers of crop_pc's k form (scan_radius skips them)"""
        _hip.require_device()
        self.S, self.B, self.C = len(scans), int(batch_size), int(num_classes)
        self.num_point, self.num_buffer, self.test_smooth, self.rng = int(num_point), int(num_buffer), float(test_smooth), rng
        if self.S < self.B:
            raise ValueError(f"{self.S} scans < batch_size {self.B}: an epoch of int(S/B)*B*4 crops would be empty (the reference "
                             "would loop forever)")
        if k_form and self.num_buffer // 4 < 1:
            raise ValueError("num_buffer // 4 must be >= 1 (crop_pc draws randint(0, num_buffer // 4))")
        self.kcap = self.num_point + self.num_buffer + self.num_buffer // 4 - 1
        if k_form and self.kcap > ORDER_CAP:
            raise _hip.PasnlUnsupported(f"num_point + num_buffer + num_buffer//4 - 1 = {self.kcap} > {ORDER_CAP} (the LDS sort of "
                                        "pasnl_crop_order_permute)")
        dev = []
        for s in scans:
            t = _hip.as_dev(s, torch.float32)
            if t.dim() != 2 or t.shape[1] != 3:
                raise ValueError("every scan must be (N, 3)")
            dev.append(t)
        self.sizes = [int(t.shape[0]) for t in dev]
        for i, n in enumerate(self.sizes):
            if k_form and n < self.kcap:
                raise ValueError(f"scan {i} has {n} points < num_point + num_buffer + num_buffer//4 - 1 = {self.kcap} (sklearn's "
                                 "query would raise on k > n)")
        self.offsets_host = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.N, self.nmax = int(self.offsets_host[-1]), max(self.sizes)
        self.device = dev[0].device
        self.points = torch.cat(dev).contiguous()
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        poss = []
        mins = []
        for n in self.sizes:  # D:206-209, in list order
            poss.append(rng.rand(n) * 1e-3)
            mins.append(float(np.min(poss[-1])))
        self.possibility = torch.from_numpy(np.concatenate(poss)).to(self.device)
        self.min_poss = torch.tensor(mins, dtype=torch.float64, device=self.device)
        self.probs = torch.zeros((self.N, self.C), dtype=torch.float16, device=self.device)
        self.win = torch.empty((self.nmax,), dtype=torch.int32, device=self.device)
        _hip.launch("pasnl_scan_scratch_init", "ScanTester", ctypes.c_long(self.nmax), _p(self.win))
        self.scratch = torch.zeros((1,), dtype=torch.float32, device=self.device)
        self.desc = torch.zeros((self.B, DESC_BYTES), dtype=torch.uint8, device=self.device)
        self.k_stage = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        self.perm_stage = torch.empty((self.B, self.num_point), dtype=torch.int32, device=self.device)
        if k_form:
            self.idx = torch.empty((self.kcap,), dtype=torch.int32, device=self.device)
            self.d2 = torch.empty((self.kcap,), dtype=torch.float64, device=self.device)
            self.cnt = torch.empty((1,), dtype=torch.int32, device=self.device)
            nbytes = int(_hip.lib().pasnl_knn_crop_workspace_bytes(1, ctypes.c_long(self.nmax)))
            self.ws, self.ws_bytes = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device), nbytes
        self.smooth_old = int(np.array(self.test_smooth, dtype=np.float16).view(np.uint16))  # numpy: test_smooth * float16 -> f16
        self.smooth_new = float(np.float32(1 - self.test_smooth))                           # (1 - test_smooth) * float32 probs

    # ---- one batch
    def draw_batch(self):
        """The host's RNG draws of B crops, in the reference's order (D:270, 287-291): k = num_point + buffer and the first
        num_point entries of the shuffled arange(k) of every crop."""
        ks = np.empty((self.B,), np.int32)
        perms = np.empty((self.B, self.num_point), np.int32)
        for b in range(self.B):
            k = self.num_point + self.num_buffer + self.rng.randint(0, self.num_buffer // 4)
            idx = np.arange(k)
            self.rng.shuffle(idx)
            ks[b], perms[b] = k, idx[:self.num_point]
        return ks, perms

    def stage(self, draws):
        """Copy one batch's draws into the device buffers the chain reads (asynchronous, from pinned memory)."""
        ks, perms = draws
        self.k_stage.copy_(torch.from_numpy(ks).pin_memory(), non_blocking=True)
        self.perm_stage.copy_(torch.from_numpy(perms).pin_memory(), non_blocking=True)

    def enqueue(self, out=None):
        """The device chain of the staged batch: B x (pick -> crop -> order/permute -> update), on the current stream, no host
        synchronisation.  -> points (B,num_point,3) f32, point_inds (B,num_point) i32, cloud_inds (B,) i32."""
        B, npt = self.B, self.num_point
        if out is None:
            out = (torch.empty((B, npt, 3), dtype=torch.float32, device=self.device),
                   torch.empty((B, npt), dtype=torch.int32, device=self.device),
                   torch.empty((B,), dtype=torch.int32, device=self.device))
        pts, inds, clouds = out
        for b in range(B):
            desc = _p(self.desc, b * DESC_BYTES)
            sel = _p(inds, b * npt * 4)
            _hip.launch("pasnl_scan_pick", "ScanTester pick", self.S, _p(self.offsets), _p(self.possibility), _p(self.min_poss),
                        _p(self.points), _p(self.k_stage, b * 4), desc, _p(clouds, b * 4))
            _hip.launch("pasnl_knn_crop_indirect", "ScanTester crop", 1, ctypes.c_long(self.nmax), _p(self.points), desc, self.kcap,
                        _p(self.idx), _p(self.d2), _p(self.cnt), _p(self.ws), ctypes.c_size_t(self.ws_bytes))
            _hip.launch("pasnl_crop_order_permute", "ScanTester order", 1, desc, _p(self.points), _p(self.idx), _p(self.d2), self.kcap,
                        _p(self.perm_stage, b * npt * 4), npt, sel, _p(pts, b * npt * 12))
            _hip.launch("pasnl_scan_possibility_update", "ScanTester update", npt, desc, _p(self.points), sel, _p(self.possibility),
                        _p(self.min_poss), _p(self.win), _p(self.scratch))
        return pts, inds, clouds

    def next_batch(self):
        """Draw, stage and enqueue one batch (D:220-245 for B crops).  -> (points, point_inds, cloud_inds) device tensors."""
        self.stage(self.draw_batch())
        return self.enqueue()

    def vote(self, logits, point_inds, cloud_inds, is_logits=True):
        """T:147-154 for one batch, crop after crop: logits (B,num_point,C) f32 (is_logits=False: probabilities)."""
        v = _hip.as_dev(logits, torch.float32).reshape(self.B, self.num_point, self.C)
        pi = _hip.as_dev(point_inds, torch.int32).reshape(self.B, self.num_point)
        ci = _hip.as_dev(cloud_inds, torch.int32).reshape(self.B)
        _hip.launch("pasnl_scan_vote", "ScanTester vote", self.B, self.num_point, self.C, _p(v), 1 if is_logits else 0, _p(pi), _p(ci),
                    _p(self.offsets), ctypes.c_ushort(self.smooth_old), ctypes.c_float(self.smooth_new), _p(self.probs), _p(self.win))

    @property
    def crops_per_epoch(self):
        return int(self.S / self.B) * self.B * 4  # D:204

    def run(self, forward, num_votes=1, max_epochs=None):
        """The epoch loop of T:128-160: epochs of int(S/B)*B*4 crops until min(min_possibility) > num_votes, read back once per
        epoch.  forward: (B,num_point,3) f32 -> (B,num_point,C) logits.  -> the number of epochs run."""
        epochs = 0
        while True:
            for _ in range(self.crops_per_epoch // self.B):
                pts, inds, clouds = self.next_batch()
                self.vote(forward(pts), inds, clouds)
            epochs += 1
            if float(self.min_poss.min().item()) > num_votes or (max_epochs is not None and epochs >= max_epochs):
                return epochs

    # ---- state
    def test_probs(self, i):
        """scan i's float16 vote table (n_i, C), a device view"""
        return self.probs[int(self.offsets_host[i]):int(self.offsets_host[i + 1])]

    def possibility_of(self, i):
        return self.possibility[int(self.offsets_host[i]):int(self.offsets_host[i + 1])]

    def min_possibility(self):
        return self.min_poss.cpu().numpy()

    def scan_points(self, i):
        return self.points[int(self.offsets_host[i]):int(self.offsets_host[i + 1])]

    # ---- reprojection
    def proj_inds(self, i, raw_points):
        """The nearest sub-sampled point of scan i for every raw point (sklearn KDTree(sub).query(raw), D:168-169), ties to the
        lowest index.  -> (n_raw,) int32 device tensor."""
        return project(self.scan_points(i), raw_points)

    def reproject(self, i, raw_points=None, proj_inds=None, remap_lut=None):
        """T:165-178 for scan i: argmax of the float16 votes at proj_inds (computed from raw_points, or given as the reference
        loads them; neither: the sub-sampled points themselves), then remap_lut (learning_map_inv) -> (n,) uint32 numpy."""
        n = self.sizes[i]
        if proj_inds is None and raw_points is not None:
            proj = self.proj_inds(i, raw_points)
        elif proj_inds is not None:
            host = proj_inds.cpu().numpy() if isinstance(proj_inds, torch.Tensor) else np.asarray(proj_inds)
            host = host.reshape(-1)
            if host.size and (host.min() < 0 or host.max() >= n):
                raise ValueError(f"proj_inds outside [0, {n})")
            proj = torch.from_numpy(host.astype(np.int32)).to(self.device)
        else:
            proj = None
        m = n if proj is None else int(proj.shape[0])
        lut = np.arange(self.C, dtype=np.int32) if remap_lut is None else np.asarray(remap_lut, dtype=np.int32).reshape(-1)
        if lut.size < self.C:
            raise ValueError(f"remap_lut has {lut.size} entries < {self.C} classes")
        lut_d = torch.from_numpy(lut).to(self.device)
        out = torch.empty((max(m, 1),), dtype=torch.int32, device=self.device)
        _hip.launch("pasnl_scan_labels", "ScanTester labels", ctypes.c_long(m), _p(proj) if proj is not None else ctypes.c_void_p(0),
                    _p(self.test_probs(i)), self.C, _p(lut_d), int(lut.size), _p(out))
        return out[:m].cpu().numpy().view(np.uint32)


def project(sub, raw):
    """proj_inds: for every raw point (m,3) the index of the nearest of the sub points (n,3), exact on the float64 key
    ((dx*dx)+(dy*dy))+(dz*dz) of the float32 coordinates, ties to the lowest index (csrc/scan_test.hip, a counting-sorted grid
    and a ring search).  The grid geometry is read back from the device (one synchronisation).  -> (m,) int32 device tensor."""
    sub = _hip.as_dev(sub, torch.float32).reshape(-1, 3)
    raw = _hip.as_dev(raw, torch.float32).reshape(-1, 3)
    n, m = int(sub.shape[0]), int(raw.shape[0])
    if n == 0:
        raise ValueError("no sub-sampled points")
    out = torch.empty((max(m, 1),), dtype=torch.int32, device=sub.device)
    if m == 0:
        return out[:0]
    fin = sub[torch.isfinite(sub).all(1)]
    lo, hi = (fin.amin(0), fin.amax(0)) if fin.shape[0] else (torch.zeros(3, device=sub.device), torch.zeros(3, device=sub.device))
    lo, hi = lo.double().cpu().numpy(), hi.double().cpu().numpy()
    ext = np.maximum(hi - lo, 1e-6)
    h = max(math.sqrt(ext[0] * ext[1] / n) * 2.0, float(ext.max()) / 4096.0, 1e-6)  # lidar scans are flat: ~2D density
    while True:
        dims = [int(e / h) + 1 for e in ext]
        if dims[0] * dims[1] * dims[2] <= 4 * n + 4096:
            break
        h *= 1.25
    cells = dims[0] * dims[1] * dims[2]
    nbytes = int(_hip.lib().pasnl_scan_reproject_workspace_bytes(ctypes.c_long(n), ctypes.c_long(cells)))
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=sub.device)
    _hip.launch("pasnl_scan_reproject", "project", ctypes.c_long(n), _p(sub), ctypes.c_long(m), _p(raw), ctypes.c_double(lo[0]),
                ctypes.c_double(lo[1]), ctypes.c_double(lo[2]), ctypes.c_double(h), dims[0], dims[1], dims[2], _p(out), _p(ws),
                ctypes.c_size_t(nbytes))
    return out[:m]


def write_label(path, labels):
    """T:171-180: the uint32 prediction of every raw point, raw binary (SemanticKITTI's .label format)."""
    np.asarray(labels).astype(np.uint32).tofile(path)
