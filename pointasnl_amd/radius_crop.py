"""What the four radius-form grid loops share on the host (ScanNet/scene_radius.py, SemanticKITTI/scan_radius.py): the crop
of `in_radius > 0` -- reference ScanNet/scannet_dataset_grid.py (D) :491-492, 500-501, 533-535 with data_rep (D:692-703), and
SemanticKITTI/semantic_kitti_dataset_grid.py (K) :268-269, 274-281.

`query_radius` returns as many points as lie in the sphere, and the crop draws `shuffle(arange(count))` and, when
count < num_point, `choice(count, num_point - count)`: the host must know the count before it can draw, and the next crop's
pick depends on this crop's update.  So the chain is serial, with ONE 4-byte read-back per crop (`read_count`):

  pick                          the sibling class's entry, one descriptor
  pasnl_sc*_radius_members      the member list in the tree's order, and its count         D:492 / K:269
  read_count                    the crop's one synchronisation
  draw_perm                     shuffle, [:num_point], the duplicated rows, composed        D:500-501, 694, 699 / K:274-281
  pasnl_sc*_radius_gather       select[j] = members[perm[j]] and the model input rows       D:519-520, 539 / K:283
  update                        the sibling class's entry

sklearn lists the members in the positional order of the tree's `idx_array` (a depth-first traversal, left before right), and
the shuffle permutes positions: `tree_orders`, one `np.asarray(tree.idx_array)` per scan, makes the crops the reference's.
`tree_orders=None` lists members by ascending index: self-consistent, but not a reference run's crops.
"""
import ctypes

import numpy as np
import torch

from pointasnl_amd import _hip

_p = _hip.ptr


class EpochEnded(Exception):
    """A ScanNet crop found no point inside the radius (D:505-508): the potentials are drawn afresh and the epoch's
    generator returns; the crops of the unfinished batch are dropped (drop_remainder=True)."""


def flat_tree_orders(tree_orders, sizes):
    """one permutation of arange(n_i) per scan -> the flat (N,) int32 host array beside the flat points (None: None)"""
    if tree_orders is None:
        return None
    if len(tree_orders) != len(sizes):
        raise ValueError("one tree order (np.asarray(tree.idx_array)) per scan")
    out = []
    for i, (o, n) in enumerate(zip(tree_orders, sizes)):
        a = o.cpu().numpy() if isinstance(o, torch.Tensor) else np.asarray(o)
        if a.dtype.kind not in "iu" or a.shape != (n,) or not np.array_equal(np.sort(a), np.arange(n)):
            raise ValueError(f"tree_orders[{i}] must be a permutation of arange({n}), the idx_array of scan {i}'s tree")
        out.append(a.astype(np.int32))
    return np.concatenate(out)


def draw_perm(rng, count, num_point):
    """The crop's draws in the reference's order, composed into one list of positions into the member list: `idx =
    arange(count); rng.shuffle(idx); perm = idx[:num_point]`, then `dup = rng.choice(len(perm), num_point - len(perm))` and
    `perm[list(range(len(perm))) + list(dup)]` when the sphere holds fewer than num_point points.  count >= 1.
    -> perm (num_point,) int32; its first min(count, num_point) entries are distinct."""
    idx = np.arange(count)
    rng.shuffle(idx)
    perm = idx[:num_point]
    if len(perm) < num_point:
        num_in = len(perm)
        dup = rng.choice(num_in, num_point - num_in)
        perm = perm[list(range(num_in)) + list(dup)]
    return perm.astype(np.int32)


class RadiusChain:
    """The buffers and the steps of the radius crop for a class that holds its scans as `SceneCrops` and `ScanTester` do
    (points, offsets, sizes, nmax, desc, perm_stage, device, num_point)."""

    MEMBERS = None  # "pasnl_scan_radius_members" | "pasnl_scene_radius_members"

    def _init_radius(self, in_radius, tree_orders):
        self.in_radius = float(in_radius)
        if not self.in_radius > 0:
            raise ValueError("in_radius must be > 0 (the k form is the sibling class)")
        host = flat_tree_orders(tree_orders, self.sizes)
        self.order = None if host is None else torch.from_numpy(host).to(self.device)
        self.members = torch.empty((self.nmax,), dtype=torch.int32, device=self.device)
        self.count = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.count_host = torch.zeros((1,), dtype=torch.int32).pin_memory()
        self.perm_host = torch.zeros((self.num_point,), dtype=torch.int32).pin_memory()
        nbytes = int(_hip.lib().pasnl_scan_radius_workspace_bytes(1, ctypes.c_long(self.nmax)))
        self.rws, self.rws_bytes = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=self.device), nbytes
        self.readbacks = 0

    def _members(self, desc):
        _hip.launch(self.MEMBERS, type(self).__name__ + " members", 1, ctypes.c_long(self.nmax), _p(self.points), desc,
                    ctypes.c_double(self.in_radius), _p(self.order), _p(self.members), ctypes.c_long(self.nmax), _p(self.count),
                    _p(self.rws), ctypes.c_size_t(self.rws_bytes))

    def read_count(self):
        """the crop's one read-back: the member count, 4 bytes into pinned memory, and a wait for the stream"""
        self.count_host.copy_(self.count, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        self.readbacks += 1
        return int(self.count_host[0])

    def _stage_perm(self, b, perm):
        """crop b's composed permutation into the batch's staging rows (the stream has just been waited for, so the pinned
        buffer of the previous crop is free)"""
        self.perm_host.copy_(torch.from_numpy(perm))
        self.perm_stage[b].copy_(self.perm_host, non_blocking=True)

    def _no_k_form(self, *args, **kwargs):
        raise TypeError("the radius form draws inside its chain (the shuffle's length is the device's count): use next_batch()")

    draw_batch = stage = enqueue = _no_k_form
