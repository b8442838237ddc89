"""The crop stage of the SemanticKITTI "grid" input pipeline on the GPU -- host mirror of
SemanticKITTI/semantic_kitti_dataset_grid.py:265-291 (`crop_pc`, `shuffle_idx`) of the reference.

The reference keeps one pickled sklearn `KDTree` per voxel-subsampled scan (get_data, :248-263) and asks it for the
`num_point + buffer` nearest points of one centre (`search_tree.query`, :271) or for every point within `in_radius`
(`query_radius`, :269).  `DeviceScan` stands where that tree stood: it holds the scan in HBM and answers the two calls
with ONE exact selection (`pasnl_knn_crop`, csrc/crop.hip; no tree is built) -- same argument meaning, same return
structure, the same SET of points (ranked by the float64 squared distance sklearn ranks by); a tie at the k-th distance
goes to the lowest indices (and `query_radius` lists its points by ascending index, sklearn in its tree's order -- crop_pc
shuffles positions of that list, so hand `DeviceScan` the tree's `idx_array` for the reference's radius crop).  `crop_pc` below is the reference's flow on top of it: shuffle, truncate, duplicate-pad with the
caller's numpy RNG, on the host as there.  The test loop around it -- possibility init, pick, crop, possibility update,
votes and reprojection (:192-245 and test_semantic_kitti_grid.py) -- runs on the device in scan_tester.ScanTester.
Datasets and the tf.data plumbing are out of scope.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip


class DeviceScan:
    """One scan in HBM, queried like the reference's `search_tree` (an sklearn.neighbors.KDTree over the same points).

    `DeviceScan(points)`: points (n,3) float32, numpy (copied over PCIe once, like unpickling the tree) or a CUDA tensor
    (e.g. the output rows of grid_subsampling on the device).  `.data` is the (n,3) array view crop_pc indexes.
    tree_order: `np.asarray(tree.idx_array)` of the reference's tree over the same points, a permutation of arange(n); with
    it `query_radius` lists its points in sklearn's order (pasnl_scan_radius_members), so `crop_pc(..., in_radius > 0)` is
    the reference's crop.  None: ascending index, as before."""

    def __init__(self, points, tree_order=None):
        _hip.require_device()
        if isinstance(points, torch.Tensor):
            self.dev = _hip.as_dev(points, torch.float32)
            self._host = None
        else:
            self._host = np.ascontiguousarray(points, dtype=np.float32)
            self.dev = torch.from_numpy(self._host).cuda()
        if self.dev.dim() != 2 or self.dev.shape[1] != 3:
            raise ValueError("points.shape is not (N, 3)")
        self.n = int(self.dev.shape[0])
        nbytes = int(_hip.lib().pasnl_knn_crop_workspace_bytes(1, ctypes.c_long(self.n)))
        self._ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.dev.device)
        self._ws_bytes = nbytes
        self.order = None
        if tree_order is not None:
            from pointasnl_amd.radius_crop import flat_tree_orders

            self.order = torch.from_numpy(flat_tree_orders([tree_order], [self.n])).to(self.dev.device)

    @property
    def data(self):
        if self._host is None:
            self._host = self.dev.cpu().numpy()
        return self._host

    def select(self, centre, k=0, radius=0.0, want_d2=False):
        """Device-side result of one search, no host synchronisation: (idx (kcap,) int32 ascending index, d2 (kcap,) float64
        or None, count (1,) int32).  k form: kcap = min(k, n); radius form: kcap = n."""
        c = centre if isinstance(centre, torch.Tensor) else torch.from_numpy(np.asarray(centre, dtype=np.float32).reshape(1, 3))
        c = c.to(device=self.dev.device, dtype=torch.float32).reshape(1, 3).contiguous()
        kcap = self.n if radius > 0 else max(1, min(int(k), self.n))
        idx = torch.empty((kcap,), dtype=torch.int32, device=self.dev.device)
        d2 = torch.empty((kcap,), dtype=torch.float64, device=self.dev.device) if want_d2 else None
        cnt = torch.empty((1,), dtype=torch.int32, device=self.dev.device)
        kd = None
        if radius <= 0 and int(k) != kcap:  # k <= 0 (an empty result) is passed on as it is
            kd = torch.tensor([int(k)], dtype=torch.int32, device=self.dev.device)
        _hip.launch("pasnl_knn_crop", "crop_pc", 1, ctypes.c_long(self.n), ctypes.c_long(0), _hip.ptr(self.dev), _hip.ptr(c),
                    _hip.ptr(kd), kcap, ctypes.c_double(float(radius) if radius > 0 else 0.0), _hip.ptr(idx), _hip.ptr(d2),
                    _hip.ptr(cnt), _hip.ptr(self._ws), ctypes.c_size_t(self._ws_bytes))
        return idx, d2, cnt

    def query(self, X, k=1, return_distance=True, sort_results=True):
        """sklearn KDTree.query for ONE query point X (1,3): (dist (1,k) float64, ind (1,k) int64), nearest first (ties by index)."""
        X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
        if X.shape[0] != 1:
            raise ValueError("DeviceScan.query answers one centre per call (crop_pc's use, semantic_kitti_dataset_grid.py:271)")
        if k > self.n:
            raise ValueError("k must be less than or equal to the number of training points")  # sklearn's message
        idx, d2, cnt = self.select(X[0].astype(np.float32), k=int(k), want_d2=True)
        m = min(int(k), self.n)
        idx, d2 = idx[:m], d2[:m]
        if sort_results:
            d2, order = torch.sort(d2, stable=True)  # ascending index came in: ties stay in index order
            idx = idx[order]
        ind = idx.cpu().numpy().astype(np.int64)[None]
        if not return_distance:
            return ind
        return np.sqrt(d2.cpu().numpy())[None], ind

    def query_radius(self, X, r):
        """sklearn KDTree.query_radius for ONE query point: an object array holding one int64 index array (ascending index)."""
        X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
        if X.shape[0] != 1:
            raise ValueError("DeviceScan.query_radius answers one centre per call (crop_pc's use, :269)")
        out = np.empty((1,), dtype=object)
        if self.order is not None:
            out[0] = self._members_in_tree_order(X[0].astype(np.float32), float(r))
            return out
        idx, _, cnt = self.select(X[0].astype(np.float32), radius=float(r))
        m = int(cnt.item())
        out[0] = idx[:m].cpu().numpy().astype(np.int64)
        return out

    def _members_in_tree_order(self, centre, r):
        """the points within r of centre in the order of the tree's idx_array (sklearn's), int64"""
        desc = np.zeros(1, np.dtype([("offset", "<i8"), ("cloud", "<i4"), ("pick", "<i4"), ("n", "<i4"), ("k", "<i4"),
                                     ("c", "<f4", 3), ("pad", "<i4")]))  # pasnl_scan_crop_t
        desc["n"], desc["c"] = self.n, centre
        dev = self.dev.device
        d = torch.from_numpy(desc.view(np.uint8)).to(dev)
        members = torch.empty((self.n,), dtype=torch.int32, device=dev)
        cnt = torch.empty((1,), dtype=torch.int32, device=dev)
        nbytes = int(_hip.lib().pasnl_scan_radius_workspace_bytes(1, ctypes.c_long(self.n)))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
        _hip.launch("pasnl_scan_radius_members", "query_radius", 1, ctypes.c_long(self.n), _hip.ptr(self.dev), _hip.ptr(d),
                    ctypes.c_double(r), _hip.ptr(self.order), _hip.ptr(members), ctypes.c_long(self.n), _hip.ptr(cnt), _hip.ptr(ws),
                    ctypes.c_size_t(nbytes))
        return members[:int(cnt.item())].cpu().numpy().astype(np.int64)


def select_batch(points, centres, k=None, kcap=None, radius=0.0, want_d2=False, workspace=None):
    """b searches in ONE call of pasnl_knn_crop, everything on the device, no host synchronisation (capturable once the
    workspace is passed in): points (n,3) -- every crop searches the same scan -- or (b,n,3); centres (b,3); k an int, a
    (b,) int32 device tensor (per-crop counts: crop_pc draws its buffer per crop) or None (= kcap).
    -> idx (b,kcap) int32 ascending index, d2 (b,kcap) float64 or None, count (b,) int32."""
    _hip.require_device()
    pts = _hip.as_dev(points, torch.float32)
    cen = _hip.as_dev(centres, torch.float32).reshape(-1, 3)
    b = int(cen.shape[0])
    if pts.dim() == 2:
        n, stride = int(pts.shape[0]), 0
    else:
        if pts.shape[0] != b:
            raise ValueError("points (b,n,3) and centres (b,3) differ in b")
        n, stride = int(pts.shape[1]), int(pts.shape[1])
    if pts.shape[-1] != 3:
        raise ValueError("points.shape is not (N, 3)")
    kd = None
    if isinstance(k, torch.Tensor):
        kd = _hip.as_dev(k, torch.int32).reshape(b)
        if kcap is None:
            raise ValueError("per-crop k on the device needs kcap (the row length of the result)")
    elif k is not None and kcap is None:
        kcap = int(k)
    elif k is not None:
        kd = torch.full((b,), int(k), dtype=torch.int32, device=pts.device)
    if kcap is None:
        kcap = n
    kcap = max(1, min(int(kcap), n))
    idx = torch.empty((b, kcap), dtype=torch.int32, device=pts.device)
    d2 = torch.empty((b, kcap), dtype=torch.float64, device=pts.device) if want_d2 else None
    cnt = torch.empty((b,), dtype=torch.int32, device=pts.device)
    nbytes = int(_hip.lib().pasnl_knn_crop_workspace_bytes(b, ctypes.c_long(n)))
    if workspace is None:
        workspace = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=pts.device)
    _hip.launch("pasnl_knn_crop", "crop_pc", b, ctypes.c_long(n), ctypes.c_long(stride), _hip.ptr(pts), _hip.ptr(cen), _hip.ptr(kd),
                kcap, ctypes.c_double(float(radius) if radius > 0 else 0.0), _hip.ptr(idx), _hip.ptr(d2), _hip.ptr(cnt),
                _hip.ptr(workspace), ctypes.c_size_t(workspace.numel()))
    return idx, d2, cnt


def shuffle_idx(x, rng=np.random):
    """semantic_kitti_dataset_grid.py:287-291"""
    idx = np.arange(len(x))
    rng.shuffle(idx)
    return x[idx]


def crop_pc(points, labels, search_tree, pick_idx, num_point, num_buffer=0, in_radius=0.0, rng=np.random):
    """crop a fixed size point cloud (semantic_kitti_dataset_grid.py:265-285; `self.args.*` are arguments here).
    points (n,3), labels (n,), search_tree: a DeviceScan over `points` -> (select_points, select_labels, select_idx)."""
    center_point = points[pick_idx, :].reshape(1, -1)
    if in_radius > 0:
        select_idx = search_tree.query_radius(center_point, r=in_radius)[0]
    else:
        buffer = num_buffer + rng.randint(0, num_buffer // 4)
        # (nearest first, as sklearn returns them: under the same RNG state the shuffle below then yields the reference's crop,
        # order included, whenever no two distances are equal)
        select_idx = search_tree.query(center_point, k=num_point + buffer)[1][0]
    select_idx = shuffle_idx(select_idx, rng)
    select_idx = select_idx[:num_point]
    if len(select_idx) < num_point:
        num_in = len(select_idx)
        dup = rng.choice(num_in, num_point - num_in)
        idx_dup = list(range(num_in)) + list(dup)
        select_idx = select_idx[idx_dup]
    return points[select_idx], labels[select_idx], select_idx
