"""`ScannetDatasetWholeSceneSlidingWindow` under the reference's name (ScanNet/scannet_dataset.py:135-303): a thin wrapper
over `WindowTester.blocks`.  `ds[i]` returns the reference's four numpy arrays -- float32 data (R,P,3|6), int32 labels,
float64 weights, int64 point indices -- draws from the same numpy RNG stream, and leaves `scene_points_list[i]` moved by the
noise step exactly as the reference does (the device holds the moving scene; its xyz is written back after every call, so
edits made to `scene_points_list` from outside after construction are not seen).  The blocks depend on numpy's argsort for
the CPU at hand, as the reference's do: see window_tester.py."""
import os
import pickle

import numpy as np

from pointasnl_amd.ScanNet.window_tester import WindowTester


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
