"""numpy restatement of the two grid training input loops -- reference ScanNet/scannet_dataset_grid.py (D) :435-549
`get_batch_gen('training')` and SemanticKITTI/semantic_kitti_dataset_grid.py (K) :193-292, with the tallies of
ScanNet/train_scannet_grid.py:264-302 and SemanticKITTI/train_semantic_kitti_grid.py:224-263 -- the yardstick of
pointasnl_amd.ScanNet.scene_trainer and pointasnl_amd.SemanticKITTI.scan_trainer.  The crops are those of scene_flow_ref.py
and scan_flow_ref.py (an exact nearest-first order in place of the search tree); what is stated here is what the training
split adds: labels through label_to_idx, the sample weights, K's host-drawn pick in list order, and the epoch.
tests/test_grid_train_flow.py pins this file to the reference's own generators; the augmentation is tests/philox_ref.py."""
import numpy as np

import philox_ref as P
from block_train_flow_ref import new_totals, recount, stand_in_forward_np, stand_in_weights, train_score  # noqa: F401
from scan_flow_ref import nearest_first
from scene_flow_ref import SceneFlowRef


class SceneTrainFlowRef(SceneFlowRef):
    """D's 'training' split: SceneFlowRef's crop with label_weights[input_labels] (D:531)"""

    def __init__(self, scenes, labels, colors=None, label_weights=None, num_classes=21, num_point=8192, num_buffer=1024, batch_size=4,
                 epoch_steps=500, label_values=None, rng=np.random):
        SceneFlowRef.__init__(self, scenes, colors=colors, labels=labels, num_classes=num_classes, num_point=num_point,
                              num_buffer=num_buffer, batch_size=batch_size, split="training", validation_size=epoch_steps,
                              label_values=label_values, rng=rng)
        self.label_weights = np.ones(num_classes) if label_weights is None else np.asarray(label_weights)
        self.epoch_steps = epoch_steps

    def crop(self):
        c = SceneFlowRef.crop(self)
        c["weights"] = self.label_weights[c["labels"]]
        return c

    def batch(self, with_rgb=True):
        """-> inputs (B,npoint,3+F) f32 unaugmented, labels (B,npoint) i32, weights (B,npoint) f32, point_inds i32,
        cloud_inds (B,) i32: what the generator's outputs become under gen_types (D:546)"""
        crops = [self.crop() for _ in range(self.B)]
        inputs = np.stack([np.hstack([c["input_points"]] + ([c["features"][:, :3]] if with_rgb else [])).astype(np.float32)
                           for c in crops])
        labels = np.stack([c["labels"] for c in crops]).astype(np.int32)
        weights = np.stack([c["weights"] for c in crops]).astype(np.float32)
        inds = np.stack([c["input_inds"] for c in crops]).astype(np.int32)
        clouds = np.array([c["cloud_ind"] for c in crops], dtype=np.int32)
        return inputs, labels, weights, inds, clouds

    @property
    def steps_per_epoch(self):
        return self.epoch_steps


class ScanTrainFlowRef:
    """K's 'training' split over scans and labels in memory"""

    def __init__(self, scans, labels, label_weights=None, num_classes=20, num_point=10240, num_buffer=1024, batch_size=8,
                 rng=np.random):
        self.scans = [np.ascontiguousarray(s, np.float32) for s in scans]
        self.pc = [s.astype(np.float64) for s in self.scans]  # sklearn's float64 copy (search_tree.data)
        self.labels = labels
        self.labelweights = np.ones(num_classes) if label_weights is None else np.asarray(label_weights)
        self.C, self.num_point, self.num_buffer, self.B, self.rng = num_classes, num_point, num_buffer, batch_size, rng
        self.next_item = 0

    @property
    def steps_per_epoch(self):
        return int(len(self.scans) / self.B)

    def crop(self, cloud_ind):
        """K:216-222 with crop_pc (K:265-286) -> dict(cloud_ind, pick_idx, selected_idx, selected_pc, labels, weights)"""
        pc, labels = self.pc[cloud_ind], self.labels[cloud_ind]
        pick_idx = self.rng.choice(len(pc), 1)
        center_point = pc[pick_idx, :].reshape(1, -1)
        buffer = self.num_buffer + self.rng.randint(0, self.num_buffer // 4)
        assert len(pc) >= self.num_point + buffer, "sklearn's query raises on k > n"
        select_idx, _ = nearest_first(pc, center_point[0], self.num_point + buffer)
        idx = np.arange(len(select_idx))
        self.rng.shuffle(idx)
        select_idx = select_idx[idx][:self.num_point]
        selected_labels = labels[select_idx]
        return dict(cloud_ind=cloud_ind, pick_idx=int(pick_idx[0]), selected_idx=select_idx, selected_pc=pc[select_idx],
                    labels=selected_labels, weights=self.labelweights[selected_labels])

    def batch(self):
        """the next B items of the list under gen_types (K:237-244) -> points f32, labels i32, weights f32, point_inds i32,
        cloud_inds (B,) i32"""
        if self.next_item + self.B > self.steps_per_epoch * self.B:
            self.next_item = 0
        crops = [self.crop(self.next_item + b) for b in range(self.B)]
        self.next_item += self.B
        return (np.stack([c["selected_pc"] for c in crops]).astype(np.float32), np.stack([c["labels"] for c in crops]).astype(np.int32),
                np.stack([c["weights"] for c in crops]).astype(np.float32),
                np.stack([c["selected_idx"] for c in crops]).astype(np.int32), np.array([c["cloud_ind"] for c in crops], np.int32))


def augment(inputs, seed, item0, cfg=P.DEFAULT):
    """tf_map on the host under the kernel's generator (philox_ref.augment)"""
    return P.augment(inputs, seed, item0, cfg)


def train_epoch(ref, step, num_classes, seed=None, item0=0, cfg=P.DEFAULT, log=None):
    """`train_one_epoch` of both grid scripts over ref.steps_per_epoch batches of ref.batch(); seed: augment under it (None:
    unaugmented).  step(inputs, labels, weights) -> (B,P,C) f32 logits.  -> the totals of block_train_flow_ref.new_totals
    with num_batches and the selected indices"""
    out = new_totals()
    out["inds"], out["clouds"] = [], []
    if hasattr(ref, "next_item"):
        ref.next_item = 0
    for n in range(ref.steps_per_epoch):
        x, y, w, inds, clouds = ref.batch()
        if seed is not None:
            x = augment(x, seed, item0 + n * ref.B, cfg)
        out["fed"].append(x)
        out["labels"].append(y)
        out["smpw"].append(w)
        out["inds"].append(inds)
        out["clouds"].append(clouds)
        if log is not None:
            log.append((x, y, w, inds, clouds))
        train_score(out, np.asarray(step(x, y, w), np.float32), y, w, num_classes)
    out["num_batches"] = ref.steps_per_epoch
    return out


def report(out):
    """train_scannet_grid.py:300-302 and train_semantic_kitti_grid.py:261-263"""
    return ["Training Loss: %f" % (out["loss_sum"] / out["num_batches"]),
            "Training Accuracy: %f" % (out["total_correct"] / float(out["total_seen"]) * 100),
            "Training IoU: %f" % (out["total_correct"] / float(out["total_iou_deno"]) * 100)]
