"""`ScannetDatasetWholeSceneSlidingWindow` under the reference's name (ScanNet/scannet_dataset.py:135-303): a thin wrapper
over `WindowTester.blocks`.  `ds[i]` returns the reference's four numpy arrays -- float32 data (R,P,3|6), int32 labels,
float64 weights, int64 point indices -- draws from the same numpy RNG stream, and leaves `scene_points_list[i]` moved by the
noise step exactly as the reference does (the device holds the moving scene; its xyz is written back after every call, so
edits made to `scene_points_list` from outside after construction are not seen).  The blocks depend on numpy's argsort for
the CPU at hand, as the reference's do: see window_tester.py.

`ScannetDataset` (:6-67, randomly chopped scenes) and `ScannetDatasetWholeScene` (:69-132, every column of a whole scene)
under the reference's names and constructor arguments: thin wrappers over `BlockTester.item` and `BlockTester.scene_blocks`
(block_tester.py).  `ds[i]` returns the reference's three numpy arrays -- float32 data, int32 labels, float64 weights -- and
draws from the same numpy RNG stream; `ds.tester` runs the loops of train_scannet.py on the device.  split='train' computes
the label weights as the reference does: a class the split does not hold gets a non-finite weight ((max / 0)^(1/3) = inf in
`ScannetDataset`), which is the reference's own behaviour and harmless, because no row carries that label."""
import os
import pickle

import numpy as np

from pointasnl_amd.ScanNet.block_tester import BlockTester
from pointasnl_amd.ScanNet.window_tester import WindowTester


class _BlockDataset:
    """what the two block datasets share: the pickle (or the four lists in memory with root=None), the label weights and the
    tester"""

    def __init__(self, root, block_points, split, with_rgb, scene_points_list, semantic_labels_list, scene_points_id, scene_points_num,
                 rng, batch_size):
        self.npoints, self.root, self.with_rgb, self.split = block_points, root, with_rgb, split
        if scene_points_list is None:
            self.data_filename = os.path.join(root, "scannet_%s_rgb21c_pointid.pickle" % split)
            with open(self.data_filename, "rb") as fp:
                scene_points_list = pickle.load(fp)
                semantic_labels_list = pickle.load(fp)
                scene_points_id = pickle.load(fp)
                scene_points_num = pickle.load(fp)
        self.scene_points_list, self.semantic_labels_list = scene_points_list, semantic_labels_list
        self.scene_points_id, self.scene_points_num = scene_points_id, scene_points_num
        if split == "train":
            labelweights = np.zeros(21)
            for seg in semantic_labels_list:
                labelweights += np.histogram(seg, range(22))[0]
            labelweights = labelweights.astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                self.labelweights = self.train_weights(labelweights / np.sum(labelweights))
        elif split == "val":
            self.labelweights = np.ones(21)
        else:
            raise ValueError("split is 'train' or 'val' (the reference sets no label weights for another)")
        scenes = [np.asarray(s, np.float32) if with_rgb else np.asarray(s, np.float32)[:, 0:3] for s in scene_points_list]
        self.tester = BlockTester(scenes, semantic_labels_list, num_classes=21, block_points=block_points, batch_size=batch_size,
                                  labelweights=self.labelweights, rng=rng)

    def _host(self, data, seg, smpw):
        seg = seg.cpu().numpy()
        weight = self.labelweights[seg]
        weight *= smpw.cpu().numpy() != 0  # the device's float32(labelweights[seg] * mask) is 0 exactly where the mask is
        return data.cpu().numpy(), seg, weight

    def __len__(self):
        return len(self.scene_points_list)


class ScannetDataset(_BlockDataset):
    """`ScannetDataset(root, block_points=8192, split='train', with_rgb=False)` reads
    `<root>/scannet_<split>_rgb21c_pointid.pickle` as the reference does (:6-29); or pass the four lists in memory with
    root=None.  `ds[i]` is :31-64: (block_points, 3|6) f32, (block_points,) i32, (block_points,) f64."""

    def __init__(self, root=None, block_points=8192, split="train", with_rgb=False, scene_points_list=None, semantic_labels_list=None,
                 scene_points_id=None, scene_points_num=None, rng=np.random, batch_size=8):
        super().__init__(root, block_points, split, with_rgb, scene_points_list, semantic_labels_list, scene_points_id, scene_points_num,
                         rng, batch_size)

    @staticmethod
    def train_weights(frequency):
        return np.power(np.amax(frequency[1:]) / frequency, 1 / 3.0)  # :26

    def __getitem__(self, index):
        return self._host(*self.tester.item(index))

    @property
    def trainer(self):
        """`train_one_epoch` of train_scannet.py on the device, over the same tester (block_trainer.py); built on first use"""
        if getattr(self, "_trainer", None) is None:
            from pointasnl_amd.ScanNet.block_trainer import BlockTrainer

            self._trainer = BlockTrainer(tester=self.tester)
        return self._trainer


class ScannetDatasetWholeScene(_BlockDataset):
    """`ScannetDatasetWholeScene(root, block_points=8192, split='val', with_rgb=False)` (:69-90); `ds[i]` is :92-129:
    (R, block_points, 3|6) f32, (R, block_points) i32, (R, block_points) f64 for the scene's R non-empty columns."""

    def __init__(self, root=None, block_points=8192, split="val", with_rgb=False, scene_points_list=None, semantic_labels_list=None,
                 scene_points_id=None, scene_points_num=None, rng=np.random, batch_size=8):
        super().__init__(root, block_points, split, with_rgb, scene_points_list, semantic_labels_list, scene_points_id, scene_points_num,
                         rng, batch_size)

    @staticmethod
    def train_weights(frequency):
        return 1 / np.log(1.2 + frequency)  # :88

    def __getitem__(self, index):
        return self._host(*self.tester.scene_blocks(index))


class ScannetDatasetWholeSceneSlidingWindow:
    """`ScannetDatasetWholeSceneSlidingWindow(root, split='test', num_class=21, block_points=8192, with_rgb=True, stride=0.5)`
    reads `<root>/scannet_<split>_rgb21c_pointid.pickle` as the reference does; or pass the four lists in memory
    (`scene_points_list`, `semantic_labels_list`, `scene_points_id`, `scene_points_num`) with root=None.  split='train'
    (label weights that can be inf or nan) raises NotImplementedError."""

    def __init__(self, root=None, split="test", num_class=21, block_points=8192, with_rgb=True, stride=0.5, scene_points_list=None,
                 semantic_labels_list=None, scene_points_id=None, scene_points_num=None, rng=np.random, min_block_points=4096):
        if split == "train":
            raise NotImplementedError("split='train': see WindowTester")
        self.root, self.split, self.stride, self.with_rgb, self.block_points = root, split, stride, with_rgb, block_points
        if scene_points_list is None:
            self.data_filename = os.path.join(root, "scannet_%s_rgb21c_pointid.pickle" % split)
            with open(self.data_filename, "rb") as fp:
                scene_points_list = pickle.load(fp)
                semantic_labels_list = pickle.load(fp)
                scene_points_id = pickle.load(fp)
                scene_points_num = pickle.load(fp)
        self.scene_points_list, self.semantic_labels_list = scene_points_list, semantic_labels_list
        self.scene_points_id, self.scene_points_num = scene_points_id, scene_points_num
        self.labelweights = np.ones(num_class)
        self.point_num = [seg.shape[0] for seg in semantic_labels_list]
        scenes = [np.asarray(s, np.float32) if with_rgb else np.asarray(s, np.float32)[:, 0:3] for s in scene_points_list]
        self.tester = WindowTester(scenes, labels=semantic_labels_list, num_classes=num_class, block_points=block_points, stride=stride,
                                   with_rgb=with_rgb, min_block_points=min_block_points, rng=rng, split=split)

    def __getitem__(self, index):
        data, seg, smpw, idx = self.tester.blocks(index)
        self.scene_points_list[index][:, 0:3] = self.tester.points(index).cpu().numpy()
        return (data.cpu().numpy(), seg.cpu().numpy(), self.labelweights[0] * smpw.cpu().numpy().astype(np.float64),
                idx.cpu().numpy().astype(np.int64))

    def __len__(self):
        return len(self.scene_points_list)
