"""`SemanticKittiDatasetSlidingWindow` under the reference's name (SemanticKITTI/semantic_kitti_dataset.py:217-358): a thin
wrapper over `KittiWindowTester.blocks`, built from in-memory scans (it reads no yaml and no files).  `ds[i]` returns the
reference's tuple -- float32 div_blocks (R,P,3|4), int64 div_blocks_idxs (R,P), point_set_ini (n,3) float32 and, for every
split but 'test', the int32 labels -- and draws from the same numpy RNG stream.  The blocks depend on numpy's argsort for
the CPU at hand, as the reference's do: see window_tester.py."""
import numpy as np

from pointasnl_amd.SemanticKITTI.window_tester import KittiWindowTester

splits = ["train", "valid", "test"]


class SemanticKittiDatasetSlidingWindow:
    """`SemanticKittiDatasetSlidingWindow(scans, labels=None, remissions=None, sample_points=8192, block_size=10, stride=3.3,
    num_classes=20, split='test', with_remission=False)`: scans is a list of (n_i,3) float32 arrays (the reference's
    scan.points), labels the already mapped per-point labels (needed unless split == 'test'), remissions the (n_i,) float32
    channel appended to every row when with_remission."""

    def __init__(self, scans, labels=None, remissions=None, sample_points=8192, block_size=10, stride=3.3, num_classes=20, split="test",
                 with_remission=False, points_name=None, rng=np.random, min_block_points=4096):
        assert split in splits
        if split != "test" and labels is None:
            raise ValueError(f"split '{split}' returns the labels: pass them")
        if with_remission and remissions is None:
            raise ValueError("with_remission needs the remissions")
        self.split, self.stride, self.block_size, self.block_points = split, stride, block_size, sample_points
        self.with_remission = with_remission
        self.scans = [np.asarray(s, np.float32) for s in scans]
        self.labels = None if labels is None else [np.asarray(l).astype(np.int32) for l in labels]
        self.points_name = list(points_name) if points_name is not None else ["%06d.bin" % i for i in range(len(scans))]
        self.tester = KittiWindowTester(self.scans, labels=self.labels, remissions=remissions if with_remission else None,
                                        num_classes=num_classes, block_points=sample_points, block_size=block_size, stride=stride,
                                        min_block_points=min_block_points, rng=rng)

    def __getitem__(self, index):
        data, idx = self.tester.blocks(index)
        div_blocks, div_blocks_idxs = data.cpu().numpy(), idx.cpu().numpy().astype(np.int64)
        if self.split != "test":
            return div_blocks, div_blocks_idxs, self.scans[index], self.labels[index]
        return div_blocks, div_blocks_idxs, self.scans[index]

    def __len__(self):
        return len(self.scans)
