"""`SemanticKittiDatasetSlidingWindow` under the reference's name (SemanticKITTI/semantic_kitti_dataset.py:217-358): a thin
wrapper over `KittiWindowTester.blocks`, built from in-memory scans (it reads no yaml and no files).  `ds[i]` returns the
reference's tuple -- float32 div_blocks (R,P,3|4), int64 div_blocks_idxs (R,P), point_set_ini (n,3) float32 and, for every
split but 'test', the int32 labels -- and draws from the same numpy RNG stream.  The blocks depend on numpy's argsort for
the CPU at hand, as the reference's do: see window_tester.py.

`SemanticKittiDataset` (:17-112, randomly chopped scans) and `SemanticKittiDataset_whole` (:115-214, every column of a whole
scan) under the reference's names, over in-memory scans likewise: thin wrappers over `KittiBlockTester.item` and
`KittiBlockTester.scan_blocks` (block_tester.py).  `ds[i]` returns the reference's tuple with its dtypes -- float32 rows
(P,3|4) or (R,P,3|4), int32 labels, float32 weights -- and draws from the same numpy RNG stream; `ds.tester` runs the loops of
train_semantic_kitti.py on the device.  `random_sample` / `random_rate` reproduce :47-52: `random.Random(100).shuffle` depends
only on the list's length, so shuffling the indices is exact.  The label frequencies of :54-58 (the reference's
`mapped_content`) are the caller's to supply as `label_frequencies`; without them the weights are ones.  The two reference
behaviours that `reference_quirks=True` reproduces are stated in block_tester.py."""
import random

import numpy as np

from pointasnl_amd.SemanticKITTI.block_tester import KittiBlockTester, label_weights_from_content
from pointasnl_amd.SemanticKITTI.window_tester import KittiWindowTester

seed = 100

splits = ["train", "valid", "test"]


class _BlockDataset:
    """what the two block datasets share: the scans in memory, the :47-52 subset, the weight table and the tester"""

    def __init__(self, scans, labels, remissions, sample_points, block_size, num_classes, split, with_remission, padding, random_sample,
                 random_rate, label_frequencies, reference_quirks, rng, batch_size, points_name):
        assert split in splits
        if with_remission and remissions is None:
            raise ValueError("with_remission needs the remissions")
        self.split, self.padding, self.block_size, self.sample_points = split, padding, block_size, sample_points
        self.random_sample, self.with_remission = random_sample, with_remission
        order = list(range(len(scans)))
        self.points_name = list(points_name) if points_name is not None else ["%06d.bin" % i for i in order]
        if random_sample:  # :47-52
            random.Random(seed).shuffle(order)
            random.Random(seed).shuffle(self.points_name)
            order = order[:int(len(order) * random_rate)]
            self.points_name = self.points_name[:int(len(self.points_name) * random_rate)]
        self.order = order
        self.scans = [np.asarray(scans[k], np.float32) for k in order]
        self.labels = [np.asarray(labels[k]).astype(np.int32) for k in order]
        self.remissions = [np.asarray(remissions[k], np.float32) for k in order] if with_remission else None
        if label_frequencies is None:
            self.label_weights_lut = np.ones(num_classes, np.float32)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                self.label_weights_lut = label_weights_from_content(label_frequencies)  # :54-58
        self.tester = KittiBlockTester(self.scans, self.labels, remissions=self.remissions, num_classes=num_classes,
                                       block_points=sample_points, batch_size=batch_size, block_size=block_size, padding=padding,
                                       label_weights_lut=self.label_weights_lut, reference_quirks=reference_quirks, rng=rng)

    def __len__(self):
        return len(self.scans)


class SemanticKittiDataset(_BlockDataset):
    """`SemanticKittiDataset(scans, labels, remissions=None, sample_points=8192, block_size=10, num_classes=20, split='train',
    with_remission=False, padding=0.01, random_sample=False, random_rate=0.1, label_frequencies=None)`; `ds[i]` is :68-109:
    (sample_points, 3|4) f32, (sample_points,) i32, (sample_points,) f32."""

    def __init__(self, scans, labels, remissions=None, sample_points=8192, block_size=10, num_classes=20, split="train",
                 with_remission=False, padding=0.01, random_sample=False, random_rate=0.1, label_frequencies=None,
                 reference_quirks=True, rng=np.random, batch_size=8, points_name=None):
        super().__init__(scans, labels, remissions, sample_points, block_size, num_classes, split, with_remission, padding, random_sample,
                         random_rate, label_frequencies, reference_quirks, rng, batch_size, points_name)

    def __getitem__(self, index):
        return tuple(a.cpu().numpy() for a in self.tester.item(index))

    @property
    def trainer(self):
        """`train_one_epoch` of train_semantic_kitti.py on the device, over the same tester (block_trainer.py); built on
        first use"""
        if getattr(self, "_trainer", None) is None:
            from pointasnl_amd.SemanticKITTI.block_trainer import KittiBlockTrainer

            self._trainer = KittiBlockTrainer(tester=self.tester)
        return self._trainer


class SemanticKittiDataset_whole(_BlockDataset):
    """`SemanticKittiDataset_whole(...)` with the same arguments; `ds[i]` is :164-211: (R, sample_points, 3|4) f32,
    (R, sample_points) i32, (R, sample_points) f32 for the scan's R non-empty columns."""

    def __init__(self, scans, labels, remissions=None, sample_points=8192, block_size=10, num_classes=20, split="train",
                 with_remission=False, padding=0.01, random_sample=False, random_rate=0.1, label_frequencies=None,
                 reference_quirks=True, rng=np.random, batch_size=8, points_name=None):
        super().__init__(scans, labels, remissions, sample_points, block_size, num_classes, split, with_remission, padding, random_sample,
                         random_rate, label_frequencies, reference_quirks, rng, batch_size, points_name)

    def __getitem__(self, index):
        return tuple(a.cpu().numpy() for a in self.tester.scan_blocks(index))


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
