"""`ModelNetDataset` under the reference's name and method set (modelnet_dataset.py:39-136), built over `ModelNetTester`:
the shapes stay on the device, `next_batch` returns device tensors, and the draws (`np.random.shuffle(idxs)` in `reset`, one
`randint(0, n_i)` per shape sampled with `uniform`) come from the same numpy stream in the same order.  It takes the raw
shapes as arrays instead of a dataset root: reading the text files stays with the caller.  The reference's cache must hold
every shape (`cache_size >= len(shapes)`, its default of 15000 against 9843 / 2468 shapes): a smaller one would re-read and
re-sample a shape on a later visit, and raises NotImplementedError."""
import numpy as np

from pointasnl_amd.modelnet_tester import ModelNetTester


class ModelNetDataset:
    """`ModelNetDataset(shapes, labels, batch_size=32, npoints=1024, split='train', normalize=True, normal_channel=False,
    cache_size=15000, shuffle=None, uniform=False, num_classes=40, rng=np.random)`.  shapes: a list of (n_i, 6) float32
    arrays or device tensors in `datapath` order; labels: their classes.  shuffle=None: True for split 'train'."""

    def __init__(self, shapes, labels, batch_size=32, npoints=1024, split="train", normalize=True, normal_channel=False,
                 cache_size=15000, shuffle=None, uniform=False, num_classes=40, rng=np.random):
        assert split == "train" or split == "test"
        if cache_size < len(shapes):
            raise NotImplementedError(f"cache_size = {cache_size} < {len(shapes)} shapes: every prepared shape is kept")
        self.batch_size, self.npoints, self.normalize, self.uniform = batch_size, npoints, normalize, uniform
        self.normal_channel, self.cache_size, self.rng = normal_channel, cache_size, rng
        self.shuffle = (split == "train") if shuffle is None else shuffle
        self.tester = ModelNetTester(shapes, labels, num_classes=num_classes, num_point=npoints, batch_size=batch_size,
                                     normal_channel=normal_channel, uniform=uniform, normalize=normalize, rng=rng)
        self.reset()

    def _get_item(self, index):
        """-> (point_set (npoints, 3|6) f32 device tensor, cls (1,) i32 numpy)"""
        self.tester.prepare([index])
        return self.tester.prepared[index], self.tester.labels_host[index:index + 1].copy()

    def __getitem__(self, index):
        return self._get_item(index)

    def __len__(self):
        return self.tester.S

    def num_channel(self):
        return 6 if self.normal_channel else 3

    def reset(self):
        self.idxs = np.arange(0, len(self))
        if self.shuffle:
            self.rng.shuffle(self.idxs)
        self.tester.set_order(self.idxs)
        self.num_batches = self.tester.num_batches

    @property
    def batch_idx(self):
        return self.tester.batch_idx

    def has_next_batch(self):
        return self.tester.has_next_batch()

    def next_batch(self):
        """-> (batch_data (bsize, npoints, 3|6) f32, batch_label (bsize,) i32), device tensors: views of the tester's
        persistent batch, overwritten by the next call; the last batch of an epoch may be smaller than batch_size"""
        data, label, bsize = self.tester.next_batch()
        return data[:bsize], label[:bsize]
