"""numpy restatement of ScanNet's two training-time validation loops (reference ScanNet/scannet_dataset.py (D) :31-64
`ScannetDataset.__getitem__` and :92-129 `ScannetDatasetWholeScene.__getitem__`, ScanNet/train_scannet.py (T) :279-329
`eval_one_epoch` and :333-420 `eval_whole_scene_one_epoch`, utils/provider.py (P) :8-24 and :71-89), the yardstick of
pointasnl_amd.ScanNet.block_tester.  Every expression keeps the dtype numpy gives it there: the scene is float32, a float32
array combined with a Python list is float64, the comparisons and the voxel key are float64.
tests/test_block_tester_flow.py pins this file to the reference's own classes (tests/golden/block_flow.npz)."""
import numpy as np

OUTER = 0.2         # the margin of membership
CHOP_INNER = 0.01   # the margin of the chopped scenes' mask
WHOLE_INNER = 0.001  # ... of the whole scenes'
GRID = [31.0, 31.0, 62.0]
TRIES = 10


def scene(seed, n):
    """tests/scene_flow_ref.scene: a 6 x 5 m indoor scene -> (points (n,3) f32, colors (n,3) f32)"""
    from scene_flow_ref import scene as indoor

    return indoor(seed, n)


def fixture_scenes(num_classes=5):
    """The scenes of tests/golden/block_flow.npz -> [(points (n,6) f32, labels (n,) i64)]: a 40-point patch (less than one
    chunk of 64); a dense 1.9 x 1.7 x 2.2 m room of 2500 points whose low-x third is unlabelled (tries fail or pass by the
    centre drawn); 1000 points over 4.2 x 2.5 m (3 x 2 columns, the last one empty; no multiple of 64); a sparse, mostly
    unlabelled 3 x 3 m floor of 600 points on which no try is ever valid."""
    rng = np.random.default_rng(2024)
    out = []
    for n, ext, unl in ((40, (1.0, 0.8, 0.5), 0.2), (2500, (1.9, 1.7, 2.2), None), (1000, (4.2, 2.5, 2.4), 0.1), (600, (3.0, 3.0, 0.3), 0.6)):
        p = (rng.random((n, 3)) * ext + [-1.3, 0.4, 0.05]).astype(np.float32)
        if n == 1000:
            far = p[:, 0] > np.float32(-1.3 + 2.7)
            p[far, 1] = (0.4 + (p[far, 1] - 0.4) * 0.45).astype(np.float32)
            p[0, 1] = np.float32(0.4 + 2.5)  # (x < 2.7 here: the y extent stays 2.5)
            p[0, 0] = np.float32(-1.0)
        lab = rng.integers(1, num_classes, n)
        if unl is None:
            lab[(p[:, 0] < np.float32(-1.3 + 0.65)) & (rng.random(n) < 0.9)] = 0
        else:
            lab[rng.random(n) < unl] = 0
        out.append((np.ascontiguousarray(np.hstack([p, rng.random((n, 3)).astype(np.float32)])), lab.astype(np.int64)))
    return out


def bounds(xyz):
    """D:37-38 / D:98-99 -> coordmin, coordmax (3,) f32"""
    return np.min(xyz[:, 0:3], axis=0), np.max(xyz[:, 0:3], axis=0)


def inside(xyz, lo, hi, margin):
    """D:46 / D:52: float32 coordinates against float64 bounds -> (n,) bool"""
    return np.sum((xyz[:, 0:3] >= (lo - margin)) * (xyz[:, 0:3] <= (hi + margin)), axis=1) == 3


def crop_box(centre, zmin, zmax):
    """D:42-45 -> lo, hi (3,) f64 round the float32 centre; z spans [zmin, zmax] (the scene's, float32)"""
    lo = centre - [0.75, 0.75, 1.5]
    hi = centre + [0.75, 0.75, 1.5]
    lo[2] = zmin
    hi[2] = zmax
    return lo, hi


def voxel_keys(pts, lo, hi):
    """D:53-54 before the unique: one float64 key per point"""
    v = np.ceil((pts - lo) / (hi - lo) * GRID)
    return v[:, 0] * 31.0 * 62.0 + v[:, 1] * 62.0 + v[:, 2]


def crop_stats(xyz, labels, centre, zmin, zmax):
    """One try (D:42-55) -> dict: members (indices, ascending), mask (over the members), m, labelled, nuniq, keys, valid"""
    lo, hi = crop_box(centre, zmin, zmax)
    members = np.flatnonzero(inside(xyz, lo, hi, OUTER))
    pts = xyz[members, 0:3]
    mask = inside(pts, lo, hi, CHOP_INNER)
    with np.errstate(divide="ignore", invalid="ignore"):
        keys = voxel_keys(pts[mask, :], lo, hi)
    m, labelled, nuniq = len(members), int(np.sum(labels[members] > 0)), len(np.unique(keys))
    valid = m > 0 and labelled / m >= 0.7 and nuniq / 31.0 / 31.0 / 62.0 >= 0.02
    return dict(members=members, mask=mask, m=m, labelled=labelled, nuniq=nuniq, keys=keys, valid=valid, lo=lo, hi=hi)


def chopped_item(points, labels, labelweights, block_points, rng, with_rgb=True):
    """D:31-64 -> data (P,3|6) f32, seg (P,) i32, smpw (P,) f64, and what happened: the tries' centres and statistics, the
    resampling draw"""
    pts = points if with_rgb else points[:, 0:3]
    seg = labels.astype(np.int32)
    coordmin, coordmax = bounds(pts)
    tries, kept = [], None
    for _ in range(TRIES):
        c = int(rng.choice(len(seg), 1)[0])
        st = crop_stats(pts, seg, pts[c, 0:3], coordmin[2], coordmax[2])
        tries.append(dict(centre=c, m=st["m"], labelled=st["labelled"], nuniq=st["nuniq"], valid=st["valid"]))
        if st["m"] == 0:
            continue
        kept = st
        if st["valid"]:
            break
    choice = rng.choice(kept["m"], block_points, replace=True)
    rows = kept["members"][choice]
    smpw = labelweights[seg[rows]]
    smpw *= kept["mask"][choice]
    return pts[rows, :], seg[rows], smpw, dict(tries=tries, choice=choice, members=kept["members"], mask=kept["mask"])


def grid(coordmin, coordmax):
    """D:100-101, through numpy on the float32 bounds -> nx, ny"""
    nx = np.ceil((coordmax[0] - coordmin[0]) / 1.5).astype(np.int32)
    ny = np.ceil((coordmax[1] - coordmin[1]) / 1.5).astype(np.int32)
    return int(nx), int(ny)


def column_box(coordmin, coordmax, i, j):
    """D:107-108 -> lo, hi (3,) f64; the upper bound is coordmin + (i + 1) * 1.5, not lo + 1.5"""
    lo = coordmin + [i * 1.5, j * 1.5, 0]
    hi = coordmin + [(i + 1) * 1.5, (j + 1) * 1.5, coordmax[2] - coordmin[2]]
    return lo, hi


def columns(xyz):
    """D:98-115 without the draws -> (nx, ny), counts (nx*ny,), per non-empty column (w, members, mask)"""
    coordmin, coordmax = bounds(xyz)
    nx, ny = grid(coordmin, coordmax)
    counts, found = np.zeros(max(nx * ny, 0), np.int64), []
    for i in range(nx):
        for j in range(ny):
            lo, hi = column_box(coordmin, coordmax, i, j)
            members = np.flatnonzero(inside(xyz, lo, hi, OUTER))
            counts[i * ny + j] = len(members)
            if len(members):
                found.append((i * ny + j, members, inside(xyz[members, 0:3], lo, hi, WHOLE_INNER)))
    return (nx, ny), counts, found


def whole_item(points, labels, labelweights, block_points, rng, with_rgb=True):
    """D:92-129 -> data (R,P,3|6) f32, seg (R,P) i32, smpw (R,P) f64, and the columns, counts and draws"""
    pts = points if with_rgb else points[:, 0:3]
    seg = labels.astype(np.int32)
    shape, counts, found = columns(pts)
    data, segs, smpws, draws = [], [], [], []
    for _, members, mask in found:
        choice = rng.choice(len(members), block_points, replace=True)
        rows = members[choice]
        w = labelweights[seg[rows]]
        w *= mask[choice]
        data.append(pts[rows, :])
        segs.append(seg[rows])
        smpws.append(w)
        draws.append(choice)
    if not data:
        raise ValueError("no column: the reference concatenates an empty tuple")
    return np.stack(data), np.stack(segs), np.stack(smpws), dict(shape=shape, counts=counts, columns=[f[0] for f in found], choices=draws)


def train_weights(labels_list, whole, num_classes=21):
    """D:19-26 (whole=False) / D:81-88 (whole=True) -> (num_classes,) label weights; a class the split does not hold gets
    inf (chopped) -- the reference's own behaviour"""
    w = np.zeros(num_classes)
    for seg in labels_list:
        w += np.histogram(seg, range(num_classes + 1))[0]
    w = w.astype(np.float32)
    w = w / np.sum(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 1 / np.log(1.2 + w) if whole else np.power(np.amax(w[1:]) / w, 1 / 3.0)


# ---- the loops
def normalize_data(batch):
    """P:8-24 on a float64 (B,N,3) view -> float64"""
    out = np.zeros(batch.shape)
    for b in range(batch.shape[0]):
        pc = batch[b]
        pc = pc - np.mean(pc, axis=0)
        out[b] = pc / np.max(np.sqrt(np.sum(pc ** 2, axis=1)))
    return out


def rotate_z(batch, angles):
    """P:71-89 with the angles given -> float32"""
    out = np.zeros(batch.shape, dtype=np.float32)
    for k in range(batch.shape[0]):
        c, s = np.cos(angles[k]), np.sin(angles[k])
        out[k] = np.dot(batch[k].reshape((-1, 3)), np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]]))
    return out


def classify_loss(logits, labels, smpw):
    """tf.losses.sparse_softmax_cross_entropy(labels, logits, weights=smpw): sum(w * ce) / count(w != 0), 0 without one; float64"""
    x = np.asarray(logits, np.float64).reshape(-1, logits.shape[-1])
    l, w = np.asarray(labels).reshape(-1).astype(np.int64), np.asarray(smpw, np.float32).reshape(-1).astype(np.float64)
    mx = x.max(axis=1)
    ce = np.log(np.exp(x - mx[:, None]).sum(axis=1)) + mx - x[np.arange(x.shape[0]), l]
    present = int(np.sum(w != 0))
    return float(np.sum(np.where(w != 0, w * ce, 0.0)) / present) if present else 0.0


def new_totals(num_classes):
    return dict(total_correct=0, total_seen=0, seen=np.zeros(num_classes, np.int64), correct=np.zeros(num_classes, np.int64),
                deno=np.zeros(num_classes, np.int64), hist=np.zeros(num_classes, np.int64), loss_sum=0.0, fed=[], labels=[], smpw=[],
                losses=[])


def score(out, logits, label, smpw, num_classes, extra=0.0):
    """T:311-321 / T:391-402 for one batch"""
    pred = np.argmax(logits, 2)
    live = smpw > 0
    out["total_correct"] += int(np.sum((pred == label) & (label > 0) & live))
    out["total_seen"] += int(np.sum((label > 0) & live))
    loss = classify_loss(logits, label, smpw)
    out["loss_sum"] += loss + extra
    out["losses"].append(loss)
    out["hist"] += np.histogram(label, range(num_classes + 1))[0]
    for l in range(num_classes):
        out["seen"][l] += np.sum((label == l) & live)
        out["correct"][l] += np.sum((pred == l) & (label == l) & live)
        out["deno"][l] += np.sum(((pred == l) | (label == l)) & live)


def finish(out, num_batches):
    out["num_batches"] = num_batches
    out["mean_loss"] = out["loss_sum"] / float(num_batches)
    out["class_iou"] = np.array(out["correct"][1:]) / (np.array(out["deno"][1:], dtype=float) + 1e-6)
    out["miou"] = np.mean(out["class_iou"])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["accuracy"] = np.float64(out["total_correct"]) / float(out["total_seen"])
    out["class_acc"] = np.mean(np.array(out["correct"][1:]) / (np.array(out["seen"][1:], dtype=float) + 1e-6))
    return out


def eval_chopped(getitem, num_scenes, batch_size, block_points, width, forward, num_classes, rng, extra=0.0):
    """T:279-329.  getitem(i) -> (data, seg, smpw) of one chopped scene; forward: (B,P,width) f32 -> (B,P,C) f32"""
    out = new_totals(num_classes)
    num_batches = int(num_scenes / batch_size)
    for b in range(num_batches):
        data = np.zeros((batch_size, block_points, width))
        label = np.zeros((batch_size, block_points), dtype=np.int32)
        smpw = np.zeros((batch_size, block_points), dtype=np.float32)
        for k in range(batch_size):
            data[k], label[k], smpw[k] = getitem(b * batch_size + k)
        data[:, :, :3] = normalize_data(data[:, :, :3])
        angles = [rng.uniform() * 2 * np.pi for _ in range(batch_size)]
        data[:, :, :3] = rotate_z(data[:, :, :3], angles)
        fed = data.astype(np.float32)
        out["fed"].append(fed)
        out["labels"].append(label)
        out["smpw"].append(smpw)
        score(out, np.asarray(forward(fed), np.float32), label, smpw, num_classes, extra)
    return finish(out, num_batches)


def eval_whole(getitem, num_scenes, batch_size, forward, num_classes, extra=0.0):
    """T:333-420.  getitem(i) -> (data (R,P,w), seg (R,P), smpw (R,P)).  A scene's rows go in front of the carried ones when
    no batch is being continued and behind the accumulated ones when one is; at most one forward per scene; rows past the
    batch are carried; what is left at the end is never scored."""
    out = new_totals(num_classes)
    continuing, rows, carried = False, None, None
    for i in range(num_scenes):
        new = [np.asarray(a, np.float64) for a in getitem(i)]
        if continuing:
            rows = [np.concatenate((r, a), axis=0) for r, a in zip(rows, new)]
        else:
            rows = new if carried is None else [np.concatenate((a, c), axis=0) for a, c in zip(new, carried)]
        continuing = rows[0].shape[0] < batch_size
        if continuing:
            continue
        carried = [r[batch_size:] for r in rows] if rows[0].shape[0] > batch_size else None
        data, label, smpw = (r[:batch_size].copy() for r in rows)
        data[:, :, :3] = normalize_data(data[:, :, :3])
        fed = data.astype(np.float32)
        out["fed"].append(fed)
        out["labels"].append(label.astype(np.int32))
        out["smpw"].append(smpw.astype(np.float32))
        score(out, np.asarray(forward(fed), np.float32), label, smpw.astype(np.float32), num_classes, extra)
    out["left"] = rows[0].shape[0] if continuing else (0 if carried is None else carried[0].shape[0])
    return finish(out, num_scenes)


def report(out, names, whole):
    """the lines T:323-326 / T:405-417 log (a class whose iou_deno is 0 prints numpy's nan)"""
    head = "Eval whole scene" if whole else "Eval"
    lines = ["%s mean loss: %f" % (head, out["mean_loss"]), "Eval point avg class IoU: %f" % out["miou"],
             "%s point accuracy: %f" % (head, out["accuracy"]), "%s point avg class acc: %f" % (head, out["class_acc"])]
    if whole:
        hist = out["hist"].astype(np.float64)
        weights = hist[1:].astype(np.float32) / np.sum(hist[1:].astype(np.float32))
        txt = "------- IoU --------\n"
        with np.errstate(divide="ignore", invalid="ignore"):
            for l in range(1, len(out["seen"])):
                txt += "class %s weight: %.3f, IoU: %.3f \n" % (names[l] + " " * (14 - len(names[l])), weights[l - 1],
                                                                np.int64(out["correct"][l]) / float(out["deno"][l]))
        lines.append(txt)
    return lines


def recount(fed_labels, fed_smpw, logits, num_classes):
    """the counters again, entry by entry -> total_correct, total_seen, seen, correct, deno, hist"""
    tc = ts = 0
    seen, correct, deno, hist = (np.zeros(num_classes, np.int64) for _ in range(4))
    for label, smpw, lg in zip(fed_labels, fed_smpw, logits):
        for l, w, row in zip(label.reshape(-1), smpw.reshape(-1), lg.reshape(-1, lg.shape[-1])):
            p = int(np.argmax(row))
            hist[l] += 1
            if not w > 0:
                continue
            seen[l] += 1
            deno[l] += 1
            if p == l:
                correct[l] += 1
            else:
                deno[p] += 1
            ts += l > 0
            tc += l > 0 and p == l
    return int(tc), int(ts), seen, correct, deno, hist


def stand_in_weights(seed, num_classes):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((3, num_classes)) * 0.9).astype(np.float32), rng.standard_normal(num_classes).astype(np.float32)


def stand_in_forward_np(data, w, b):
    """a fixed map of every point to C logits (the end-to-end tests' model), float32"""
    return (np.sin(data[:, :, :3].astype(np.float32) @ w + b) * np.float32(4)).astype(np.float32)
