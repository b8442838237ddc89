"""The radius form (`in_radius > 0`) of the grid loops, host chain vs the four radius classes: what `--in-radius R` of
tools/scene_test_bench.py, tools/scan_test_bench.py and tools/grid_train_bench.py runs.  Input side only -- no model: the point
is what the crop chain with its one read-back per crop costs.

  host     the generator as written (tests/radius_flow_ref.py, the restatement pinned to the reference's generators) with its
           search answered by the cloud's prebuilt sklearn KDTree (`query_radius`), everything else in numpy; the trainers'
           batches, labels and weights uploaded, the stand-in logits brought down and tallied in numpy
  radius   RadiusSceneTester / RadiusScanTester `.next_batch()`, RadiusSceneTrainer / RadiusScanTrainer `.run(step)` with
           the trees' idx_array as tree_orders, unaugmented
  k form   the sibling class at the same num_point (num_buffer 1024), for what the read-back costs against a chain that has
           none

and the one choice pasnl_sc*_radius_members leaves open: the membership pass over `order` (an indirect read per position)
against the same pass over a tree-ordered copy of the points with order = NULL (kernel time, HIP events).

Every figure is a median of --repeats timed blocks; one JSON line comes out.
"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median(xs):
    return float(np.median(np.asarray(xs)))


def timed(block, warmup, repeats):
    """-> (seconds, crops) of every timed block; block() returns the crops it made"""
    for _ in range(warmup):
        block()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = block()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0, n))
    return out


def rate(samples):
    return round(median([n / s for s, n in samples]), 2)


def tree_search(trees):
    """radius_flow_ref.sphere answered by the cloud's prebuilt tree, as the reference's generators are"""
    def sphere(pc64, centre, r, order, stats=None):
        return trees[id(pc64)].query_radius(np.asarray(centre).reshape(1, -1), r=r)[0]
    return sphere


def members_choice(points, order, radius, reps=50):
    """kernel time of pasnl_scan_radius_members over one cloud: with `order`, and over a tree-ordered copy with order = NULL"""
    from pointasnl_amd import _hip

    n = len(points)
    desc = np.zeros(1, np.dtype([("offset", "<i8"), ("cloud", "<i4"), ("pick", "<i4"), ("n", "<i4"), ("k", "<i4"), ("c", "<f4", 3),
                                 ("pad", "<i4")]))
    desc["n"], desc["c"] = n, points[n // 2]
    d = torch.from_numpy(desc.view(np.uint8)).cuda()
    o = torch.from_numpy(order.astype(np.int32)).cuda()
    members = torch.empty((n,), dtype=torch.int32, device="cuda")
    cnt = torch.empty((1,), dtype=torch.int32, device="cuda")
    nbytes = int(_hip.lib().pasnl_scan_radius_workspace_bytes(1, ctypes.c_long(n)))
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
    out = {}
    for name, pts, op in (("order", torch.from_numpy(points).cuda(), o), ("ordered_copy", torch.from_numpy(points[order]).cuda(), None)):
        def call():
            _hip.launch("pasnl_scan_radius_members", "bench", 1, ctypes.c_long(n), _hip.ptr(pts), _hip.ptr(d), ctypes.c_double(radius),
                        _hip.ptr(op), _hip.ptr(members), ctypes.c_long(n), _hip.ptr(cnt), _hip.ptr(ws), ctypes.c_size_t(nbytes))
        for _ in range(5):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        us = []
        for _ in range(3):
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / reps)
        out[f"members_us_{name}"] = round(median(us), 2)
        out[f"members_count_{name}"] = int(cnt.item())
    return out


def run(pipeline, split, clouds, colors, labels, in_radius, num_point, batch, steps, batches, warmup, repeats, num_classes):
    """pipeline 'scene' | 'scan', split 'test' | 'training' -> the result dict"""
    from sklearn.neighbors import KDTree

    import grid_train_flow_ref as T
    import radius_flow_ref as R
    from pointasnl_amd.radius_crop import EpochEnded
    from pointasnl_amd.ScanNet import scene_radius, scene_tester, scene_trainer
    from pointasnl_amd.SemanticKITTI import scan_radius, scan_tester, scan_trainer

    B, P, C = batch, num_point, num_classes
    scene = pipeline == "scene"
    lv = np.arange(C)
    if scene:
        ref = R.SceneRadiusFlowRef(clouds, colors, labels, in_radius, split=split, num_point=P, batch_size=B, steps=steps,
                                   label_values=lv, label_weights=np.ones(C), rng=np.random.RandomState(0))
    else:
        ref = R.ScanRadiusFlowRef(clouds, labels, in_radius, split=split, num_point=P, batch_size=B, label_weights=np.ones(C),
                                  rng=np.random.RandomState(0))
    trees = {id(p64): KDTree(p64, leaf_size=50) if scene else KDTree(p64) for p64 in ref.pc}
    orders = [np.asarray(trees[id(p64)].idx_array) for p64 in ref.pc]
    R.sphere = tree_search(trees)
    w, b = T.stand_in_weights(1, C)
    wt, bt = torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()

    def step(x, labels_dev=None, weights_dev=None):
        return torch.sin(x[:, :, :3] @ wt + bt) * 4.0

    out = dict(metric="radius_" + pipeline + "_" + split, in_radius=in_radius, clouds=len(clouds), points=len(clouds[0]), batch=B,
               num_point=P, repeats=repeats, step="stand-in, input side only")
    rng = np.random.RandomState(0)
    if split == "training":
        kw = dict(num_classes=C, num_point=P, batch_size=B, rng=rng, augment=False)
        if scene:
            dev = scene_radius.RadiusSceneTrainer(clouds, labels, colors=colors, epoch_steps=steps, label_values=lv, in_radius=in_radius,
                                                  tree_orders=orders, **kw)
            sib = scene_trainer.SceneTrainer(clouds, labels, colors=colors, epoch_steps=steps, label_values=lv, num_buffer=1024, **kw)
        else:
            dev = scan_radius.RadiusScanTrainer(clouds, labels, in_radius=in_radius, tree_orders=orders, **kw)
            sib = scan_trainer.ScanTrainer(clouds, labels, num_buffer=1024, **kw)

        def host_epoch():
            tot, n = T.new_totals(), 0
            items = None if scene else list(ref.epoch())
            for crops in ref.batches() if scene else [items[i:i + B] for i in range(0, len(items), B)]:
                if scene:
                    x = np.stack([np.hstack((c["input_points"], c["features"][:, :3])).astype(np.float32) for c in crops])
                else:
                    x = np.stack([c["points"] for c in crops])
                y = np.stack([c["labels"] for c in crops]).astype(np.int32)
                sw = np.stack([c["weights"] for c in crops]).astype(np.float32)
                logits = step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(sw).cuda()).cpu().numpy()
                T.train_score(tot, logits, y, sw, C)
                n += len(crops)
            return n

        def dev_epoch(t):
            def epoch():
                try:
                    t.run(step)
                except ValueError:  # an epoch that ended before its first batch
                    pass
                return t.num_batches * B
            return epoch

        host_s = timed(host_epoch, warmup, repeats)
        dev_s, sib_s = timed(dev_epoch(dev), warmup, repeats), timed(dev_epoch(sib), warmup, repeats)
    else:
        kw = dict(num_classes=C, num_point=P, batch_size=B, rng=rng)
        if scene:
            dev = scene_radius.RadiusSceneTester(clouds, colors=colors, label_values=lv, validation_size=steps, in_radius=in_radius,
                                                 tree_orders=orders, **kw)
            sib = scene_tester.SceneTester(clouds, colors=colors, label_values=lv, validation_size=steps, num_buffer=1024, **kw)
        else:
            dev = scan_radius.RadiusScanTester(clouds, in_radius=in_radius, tree_orders=orders, **kw)
            sib = scan_tester.ScanTester(clouds, num_buffer=1024, **kw)

        def host_block():
            n = 0
            while n < batches * B:
                n += sum(1 for _ in ref.epoch())
            return n

        def dev_block(t):
            def block():
                n = 0
                for _ in range(batches):
                    try:
                        t.next_batch()
                        n += B
                    except EpochEnded:
                        pass
                return n
            return block

        host_s = timed(host_block, warmup, repeats)
        dev_s, sib_s = timed(dev_block(dev), warmup, repeats), timed(dev_block(sib), warmup, repeats)
    counts = np.asarray(ref.counts)
    out.update(host_crops_per_s=rate(host_s), radius_crops_per_s=rate(dev_s), k_form_crops_per_s=rate(sib_s),
               ratio_to_host=round(rate(dev_s) / rate(host_s), 3), ratio_to_k_form=round(rate(dev_s) / rate(sib_s), 3),
               radius_us_per_crop=round(1e6 / rate(dev_s), 1), k_form_us_per_crop=round(1e6 / rate(sib_s), 1),
               readbacks=dev.readbacks, sphere_count_median=int(np.median(counts)), sphere_count_min=int(counts.min()),
               spheres_under_num_point=int((counts < P).sum()), spheres=int(len(counts)))
    out.update(members_choice(np.ascontiguousarray(clouds[0], np.float32), orders[0], in_radius))
    return out
