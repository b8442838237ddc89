"""The grid pipelines' per-epoch evaluation, host bookkeeping vs SceneEvaluator / ScanEvaluator, behind the same device
generator and the same stand-in model (sin(x[:, :, :3] @ w + b) * 4 on the device) at the reference's shapes -- ScanNet:
4 x 8192 x 21 logits, colours; SemanticKITTI: 4 x 10240 x 20 -- over the synthetic scenes of tools/block_test_bench.py and
the synthetic scans of tools/kitti_window_test_bench.py.  What is compared is what `eval_one_epoch` does with the model's
output (train_scannet_grid.py:334-432, train_semantic_kitti_grid.py:273-328); crops and forward are the device's on both
sides.

  (a) host: per batch the logits, the labels, point_inds and cloud_inds are read back; numpy's float32 softmax, the EMA
      into the float64 per-scene table by fancy indexing (ScanNet), the probabilities and truth stacked; per crop np.insert,
      argmax and sklearn.metrics.confusion_matrix (the numpy restatement where sklearn is not importable), then the IoU
      lines; the voting pass per scene: np.insert, argmax, the projection, one confusion matrix;
  (b) SceneEvaluator.run / ScanEvaluator.run: pasnl_scene_eval_vote and pasnl_scan_eval_confusion per batch, one read-back
      per epoch; SceneEvaluator.vote_confusion(): two launches per scene, one read-back.

Prints one JSON line: batches per second of both for both datasets and voting seconds per scene (medians over --repeats
runs after --warmup).

  python tools/grid_eval_bench.py [--points 150000] [--kitti-points 120000] [--radius 50] [--scenes 8] [--steps 32]
                                  [--mesh 300000] [--warmup 1] [--repeats 3] [--device-epochs 8] [--vote-passes 5 500]

One timed sample is a few tenths of a second on either side: --device-epochs epochs in a row on the device (one on the
host; SemanticKITTI's epoch of int(S / B) batches is repeated to --steps batches first), and --vote-passes voting passes
(host, device).
"""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=150000)
    ap.add_argument("--kitti-points", type=int, default=120000)
    ap.add_argument("--radius", type=float, default=50.0)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--steps", type=int, default=32, help="ScanNet: batches per epoch (validation_size)")
    ap.add_argument("--mesh", type=int, default=300000, help="ScanNet: evaluation points (mesh vertices) per scene")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--device-epochs", type=int, default=8)
    ap.add_argument("--vote-passes", type=int, nargs=2, default=(5, 500), help="voting passes per timed sample: host, device")
    args = ap.parse_args()

    import block_flow_ref as F
    import grid_eval_flow_ref as R
    from kitti_window_test_bench import lidar_scan  # (tools/ is the script's directory)
    from pointasnl_amd.ScanNet.scene_evaluator import SceneEvaluator
    from pointasnl_amd.SemanticKITTI.scan_evaluator import ScanEvaluator
    from scan_flow_ref import softmax_f32
    from scene_flow_ref import confusion, iou_from_confusions

    try:
        from sklearn.metrics import confusion_matrix as sk_confusion

        def confusion_matrix(truth, preds, label_values):
            return sk_confusion(truth, preds, labels=label_values)
        cm_name = "sklearn"
    except ImportError:
        confusion_matrix, cm_name = confusion, "numpy"

    torch.cuda.set_device(0)
    S, B = args.scenes, 4
    ignored = np.array([0])

    def labels_of(k, n, c):
        lab = np.random.default_rng(5 + k).integers(1, c, n)
        lab[np.random.default_rng(50 + k).random(n) < 0.1] = 0
        return lab.astype(np.int32)

    def timed(run):
        for _ in range(args.warmup):
            run()
        secs = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        return secs

    def crop_iou(predictions, targets, label_values, C, proportions=None):
        """S:359-380 / K:301-319"""
        Confs = np.zeros((len(predictions), C, C), dtype=np.int32)
        for i, (probs, truth) in enumerate(zip(predictions, targets)):
            probs = np.insert(probs, 0, 0, axis=1)
            preds = label_values[np.argmax(probs, axis=1)]
            Confs[i, :, :] = confusion_matrix(truth, preds, label_values)
        Cm = R.drop_ignored(np.sum(Confs, axis=0).astype(np.float32), label_values, ignored)
        if proportions is not None:
            Cm *= np.expand_dims(proportions / (np.sum(Cm, axis=1) + 1e-6), 1)
        return 100 * np.mean(iou_from_confusions(Cm))

    out = dict(metric="grid_eval_loops", clouds=S, batch=B, repeats=args.repeats, warmup=args.warmup, model="stand-in",
               host_confusion=cm_name)
    for name in ("scannet", "kitti"):
        if name == "scannet":
            C, P, points = 21, 8192, args.points
            pc = [F.scene(5 + k, points) for k in range(S)]
            clouds, colors = [p for p, _ in pc], [c for _, c in pc]
            labels = [labels_of(k, points, C) for k in range(S)]
            vlab = [labels_of(100 + k, args.mesh, C) for k in range(S)]
            proj = [np.random.default_rng(200 + k).integers(0, points, args.mesh).astype(np.int32) for k in range(S)]
            ev = SceneEvaluator(clouds, labels, colors=colors, validation_labels=vlab, validation_proj=proj, num_classes=C,
                                num_point=P, num_buffer=1024, batch_size=B, validation_size=args.steps, rng=np.random.RandomState(0))
            gen, steps = ev, args.steps
        else:
            C, P, points = 20, 10240, args.kitti_points
            clouds = [lidar_scan(5 + k, points, args.radius) for k in range(S)]
            labels = [labels_of(k, points, C) for k in range(S)]
            ev = ScanEvaluator(clouds, labels, num_classes=C, num_point=P, num_buffer=1024, batch_size=B, rng=np.random.RandomState(0))
            gen, steps = ev.gen, ev.steps_per_epoch
        label_values = np.arange(C)
        rng = np.random.default_rng(1)
        wt = torch.from_numpy((rng.standard_normal((3, C)) * 0.9).astype(np.float32)).cuda()
        bt = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).cuda()

        def model(x):
            return torch.sin(x[:, :, :3] @ wt + bt) * 4.0

        host_tables = [np.zeros((len(c), C - 1)) for c in clouds]
        val_smooth = 0.95

        def host_epoch():
            predictions, targets = [], []
            for n in range(steps):
                gen.stage(gen.draw_batch() if name == "scannet" else gen.draw_batch(n * B))
                x, lab, _, inds, cl = gen.enqueue()
                stacked_probs = softmax_f32(model(x).cpu().numpy()[:, :, 1:])
                lab, point_inds, cloud_inds = lab.cpu().numpy(), inds.cpu().numpy(), cl.cpu().numpy()
                for b in range(B):
                    probs = stacked_probs[b]
                    if name == "scannet":
                        t, i = host_tables[cloud_inds[b]], point_inds[b]
                        t[i] = val_smooth * t[i] + (1 - val_smooth) * probs
                        targets += [labels[cloud_inds[b]][i]]
                    else:
                        targets += [lab[b]]
                    predictions += [probs]
            return crop_iou(predictions, targets, label_values, C, ev.val_proportions if name == "scannet" else None)

        def host_vote():
            Confs = np.zeros((C, C), dtype=np.int32)
            for i in range(S):
                sub_probs = np.insert(host_tables[i], 0, 0, axis=1)
                sub_preds = label_values[np.argmax(sub_probs, axis=1).astype(np.int32)]
                preds = (sub_preds[proj[i]]).astype(np.int32)
                Confs += confusion_matrix(vlab[i].astype(np.int32), preds, label_values).astype(np.int32)
            return 100 * np.mean(iou_from_confusions(R.drop_ignored(Confs, label_values, ignored)))

        epochs = max(1, args.steps // steps)  # SemanticKITTI's epoch is int(S / B) batches: several in a row make one sample
        host_s = timed(lambda: [host_epoch() for _ in range(epochs)])
        dev_s = [s / args.device_epochs for s in timed(lambda: [ev.run(model) for _ in range(epochs * args.device_epochs)])]
        row = dict(points=points, num_point=P, classes=C, batches_per_epoch=steps, host_epochs_per_sample=epochs,
                   device_epochs_per_sample=epochs * args.device_epochs,
                   host_batches_per_s=round(steps * epochs / median(host_s), 2),
                   device_batches_per_s=round(steps * epochs / median(dev_s), 2),
                   ratio=round(median(host_s) / median(dev_s), 3), host_s_per_pass_runs=[round(s, 4) for s in host_s],
                   device_s_per_pass_runs=[round(s, 4) for s in dev_s])
        if name == "scannet":
            hp, dp = args.vote_passes
            hv = [s / hp for s in timed(lambda: [host_vote() for _ in range(hp)])]
            dv = [s / dp for s in timed(lambda: [ev.vote_confusion() for _ in range(dp)])]
            row.update(mesh_points=args.mesh, host_vote_s_per_scene=round(median(hv) / S, 5),
                       device_vote_s_per_scene=round(median(dv) / S, 6), vote_ratio=round(median(hv) / median(dv), 2), vote_passes_per_sample=[hp, dp],
                       host_vote_s_runs=[round(s, 4) for s in hv], device_vote_s_runs=[round(s, 5) for s in dv])
        out[name] = row
        del ev, gen
    print(json.dumps(out))


if __name__ == "__main__":
    main()
