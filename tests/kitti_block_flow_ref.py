"""numpy restatement of SemanticKITTI's two training-time validation loops (reference SemanticKITTI/semantic_kitti_dataset.py
(D) :68-109 `SemanticKittiDataset.__getitem__` and :164-211 `SemanticKittiDataset_whole.__getitem__`,
SemanticKITTI/train_semantic_kitti.py (T) :267-328 `eval_one_epoch` and :331-418 `eval_whole_scene_one_epoch`,
utils/provider.py (P) :71-89), the yardstick of pointasnl_amd.SemanticKITTI.block_tester.  Every expression keeps the dtype
numpy gives it there: the scan is float32, a float32 array combined with a Python list is float64, the comparisons are float64,
the weight table and the weights are float32.  `reference_quirks=True` restates two behaviours of the reference literally:

  * label_weights = lut[label] is a per-POINT array and sample_weight = label_weights[semantic_seg] indexes it by label VALUE:
    the weight of the label of scan point number seg[e] (IndexError when n <= max(label));
  * the remission column is scan.remissions[choice]: the remission of scan point number choice[e], the raw draw.

`reference_quirks=False` is the evident intent: lut[semantic_seg] and the members' own remissions.
tests/test_kitti_block_tester_flow.py pins this file to the reference's own classes (tests/golden/kitti_block_flow.npz)."""
import numpy as np

from block_flow_ref import classify_loss, new_totals, recount, rotate_z, score, stand_in_forward_np, stand_in_weights  # noqa: F401

OUTER = 0.2  # the margin of membership
TRIES = 10
NUM_CLASSES = 20


def fixture_scans():
    """The scans of tests/golden/kitti_block_flow.npz -> [(points (n,3) f32, remissions (n,) f32, labels (n,) i32)]: 40 points
    over 6 x 5 x 3 m (less than one chunk of 64, one column); 3000 over 38 x 27 x 6 m whose low-x band is mostly unlabelled
    (tries pass or fail by the centre drawn; 4 x 3 columns); 1000 over 41 x 9 x 4 m (5 x 1 columns, no multiple of 64); 600
    over 21 x 21 x 2 m that are 60 % unlabelled (no try is ever valid; 3 x 3 columns); 500 over 25 x 15 x 3 m whose far
    corner is empty (3 x 2 columns, one of them empty)."""
    rng = np.random.default_rng(2025)
    out = []
    for n, ext, unl in ((40, (6.0, 5.0, 3.0), 0.1), (3000, (38.0, 27.0, 6.0), None), (1000, (41.0, 9.0, 4.0), 0.1),
                        (600, (21.0, 21.0, 2.0), 0.6), (500, (25.0, 15.0, 3.0), 0.15)):
        origin = np.array([-17.3, 4.6, -1.9])
        p = (rng.random((n, 3)) * ext + origin).astype(np.float32)
        p[0] = (origin + [0.0, 0.0, 0.0]).astype(np.float32)  # the extents are the nominal ones
        p[1] = (origin + [ext[0], 1.0, ext[2]]).astype(np.float32)
        p[2] = (origin + [1.0, ext[1], 1.0]).astype(np.float32)
        if n == 500:  # nothing within 0.2 of column (2, 1): x >= 19.8 and y >= 9.8 from the origin
            far = (p[:, 0] > np.float32(origin[0] + 19.0)) & (p[:, 1] > np.float32(origin[1] + 9.0))
            p[far, 1] = (origin[1] + (p[far, 1] - origin[1]) * 0.55).astype(np.float32)
        lab = rng.integers(1, NUM_CLASSES, n)
        if unl is None:
            lab[(p[:, 0] < np.float32(origin[0] + 12.0)) & (rng.random(n) < 0.9)] = 0
        else:
            lab[rng.random(n) < unl] = 0
        out.append((p, rng.random(n).astype(np.float32), lab.astype(np.int32)))
    return out


def label_weights_lut(content):
    """D:54-58 with its dtypes -> (len(content),) float32"""
    num_keys = len(content.keys())
    lut = np.zeros((num_keys), dtype=np.float32)
    lut[list(content.keys())] = list(content.values())
    return np.power(np.amax(lut[1:]) / lut, 1 / 3.0)


def bounds(points):
    """D:78-79 / D:174-175 -> coordmin, coordmax (3,) f32"""
    return np.min(points[:, 0:3], axis=0), np.max(points[:, 0:3], axis=0)


def inside(xyz, lo, hi, margin):
    """D:87 / D:95: float32 coordinates against float64 bounds -> (n,) bool"""
    return np.sum((xyz[:, 0:3] >= (lo - margin)) * (xyz[:, 0:3] <= (hi + margin)), axis=1) == 3


def crop_box(centre, block_size, zmin, zmax):
    """D:83-86 -> lo, hi (3,) f64 round the float32 centre; z spans [zmin, zmax] (the scan's, float32)"""
    lo = centre - [block_size / 2, block_size / 2, 14]
    hi = centre + [block_size / 2, block_size / 2, 14]
    lo[2] = zmin
    hi[2] = zmax
    return lo, hi


def crop_stats(points, labels, centre, block_size, padding, zmin, zmax):
    """One try (D:82-97) -> dict: members (indices, ascending), mask (over the members), m, labelled, valid"""
    lo, hi = crop_box(centre, block_size, zmin, zmax)
    members = np.flatnonzero(inside(points, lo, hi, OUTER))
    mask = inside(points[members, 0:3], lo, hi, padding)
    m, labelled = len(members), int(np.sum(labels[members] > 0))
    valid = m > 0 and bool(np.sum(labels[members] > 0) / m >= 0.7)
    return dict(members=members, mask=mask, m=m, labelled=labelled, valid=valid, lo=lo, hi=hi)


def _rows(points, remissions, labels, lut, members, mask, choice, quirks):
    """D:101-107 / D:196-203 for one column -> point_set (P,3|4) f32, semantic_seg (P,) i32, sample_weight (P,) f32"""
    point_set = points[members, :][choice, :]
    semantic_seg = labels[members][choice]
    if quirks:
        label_weights = lut[labels]
        sample_weight = label_weights[semantic_seg]
    else:
        sample_weight = lut[semantic_seg]
    sample_weight *= mask[choice]
    if remissions is not None:
        rem = remissions[choice] if quirks else remissions[members][choice]
        point_set = np.concatenate((point_set, np.expand_dims(rem, axis=1)), axis=1)
    return point_set, semantic_seg, sample_weight


def chopped_item(points, remissions, labels, lut, sample_points, rng, block_size=10, padding=0.01, reference_quirks=True):
    """D:68-109 -> point_set, semantic_seg, sample_weight, and what happened: the tries, the kept crop, the draw"""
    coordmin, coordmax = bounds(points)
    tries, kept = [], None
    for _ in range(TRIES):
        c = int(rng.choice(len(labels), 1)[0])
        st = crop_stats(points, labels, points[c, 0:3], block_size, padding, coordmin[2], coordmax[2])
        tries.append(dict(centre=c, m=st["m"], labelled=st["labelled"], valid=st["valid"]))
        if st["m"] == 0:
            continue
        kept = st
        if st["valid"]:
            break
    choice = rng.choice(kept["m"], sample_points, replace=True)
    return _rows(points, remissions, labels, lut, kept["members"], kept["mask"], choice, reference_quirks) + (
        dict(tries=tries, choice=choice, members=kept["members"], mask=kept["mask"]),)


def grid(coordmin, coordmax, block_size):
    """D:177-178, through numpy on the float32 bounds -> nx, ny"""
    nx = np.ceil((coordmax[0] - coordmin[0]) / block_size).astype(np.int32)
    ny = np.ceil((coordmax[1] - coordmin[1]) / block_size).astype(np.int32)
    return int(nx), int(ny)


def column_box(coordmin, coordmax, i, j, block_size):
    """D:184-185 -> lo, hi (3,) f64; the upper bound is coordmin + (i + 1) * block_size, not lo + block_size"""
    lo = coordmin + [i * block_size, j * block_size, 0]
    hi = coordmin + [(i + 1) * block_size, (j + 1) * block_size, coordmax[2] - coordmin[2]]
    return lo, hi


def columns(points, block_size=10, padding=0.01):
    """D:174-193 without the draws -> (nx, ny), counts (nx*ny,), per non-empty column (w, members, mask)"""
    coordmin, coordmax = bounds(points)
    nx, ny = grid(coordmin, coordmax, block_size)
    counts, found = np.zeros(max(nx * ny, 0), np.int64), []
    for i in range(nx):
        for j in range(ny):
            lo, hi = column_box(coordmin, coordmax, i, j, block_size)
            members = np.flatnonzero(inside(points, lo, hi, OUTER))
            counts[i * ny + j] = len(members)
            if len(members):
                found.append((i * ny + j, members, inside(points[members, 0:3], lo, hi, padding)))
    return (nx, ny), counts, found


def whole_item(points, remissions, labels, lut, sample_points, rng, block_size=10, padding=0.01, reference_quirks=True):
    """D:164-211 -> point_sets (R,P,3|4) f32, semantic_segs (R,P) i32, sample_weights (R,P) f32, and the columns and draws"""
    shape, counts, found = columns(points, block_size, padding)
    data, segs, smpws, draws = [], [], [], []
    for _, members, mask in found:
        choice = rng.choice(len(members), sample_points, replace=True)
        point_set, semantic_seg, sample_weight = _rows(points, remissions, labels, lut, members, mask, choice, reference_quirks)
        data.append(np.expand_dims(point_set, 0))
        segs.append(np.expand_dims(semantic_seg, 0))
        smpws.append(np.expand_dims(sample_weight, 0))
        draws.append(choice)
    if not data:
        raise ValueError("no column: the reference concatenates an empty tuple")
    return (np.concatenate(tuple(data), axis=0), np.concatenate(tuple(segs), axis=0), np.concatenate(tuple(smpws), axis=0),
            dict(shape=shape, counts=counts, columns=[f[0] for f in found], choices=draws))


# ---- the loops
def finish(out, num_batches):
    """T:311-319 / T:402-408"""
    out["num_batches"] = num_batches
    out["mean_loss"] = out["loss_sum"] / float(num_batches)
    out["class_iou"] = np.array(out["correct"][1:]) / (np.array(out["deno"][1:], dtype=float) + 1e-6)
    out["miou"] = np.mean(out["class_iou"])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["accuracy"] = np.float64(out["total_correct"]) / float(out["total_seen"])
    out["class_acc"] = np.mean(np.array(out["correct"][1:]) / (np.array(out["seen"][1:], dtype=float) + 1e-6))
    return out


def eval_chopped(getitem, num_scans, batch_size, sample_points, width, forward, num_classes, rng, extra=0.0):
    """T:267-328.  getitem(i) -> (point_set, seg, smpw) of one chopped scan; the batch is float64 (T:213), rotated about z
    with B angles drawn behind the B items (T:290) and fed as float32; forward: (B,P,width) f32 -> (B,P,C) f32"""
    out = new_totals(num_classes)
    num_batches = int(num_scans / batch_size)
    for b in range(num_batches):
        data = np.zeros((batch_size, sample_points, width))
        label = np.zeros((batch_size, sample_points), dtype=np.int32)
        smpw = np.zeros((batch_size, sample_points), dtype=np.float32)
        for k in range(batch_size):
            data[k, ...], label[k, :], smpw[k, :] = getitem(b * batch_size + k)
        angles = [rng.uniform() * 2 * np.pi for _ in range(batch_size)]
        data[:, :, :3] = rotate_z(data[:, :, :3], angles)
        fed = data.astype(np.float32)
        out["fed"].append(fed)
        out["labels"].append(label)
        out["smpw"].append(smpw)
        score(out, np.asarray(forward(fed), np.float32), label, smpw, num_classes, extra)
    return finish(out, num_batches)


def eval_whole(getitem, num_scans, batch_size, forward, num_classes, extra=0.0):
    """T:331-418.  getitem(i) -> (point_sets (R,P,w), segs (R,P), smpws (R,P)).  A scan's rows go in front of the carried ones
    when no batch is being continued and behind the accumulated ones when one is; fewer than B rows wait for the next scan; of
    more than B the first B are fed and the rest carried -- at most one forward per scan; what is left at the end is never
    scored.  No normalize_data and no rotation (T:381 is commented out).  With remission the reference stops after a batch of
    exactly B rows (T:369 resets the carried rows to 3 columns); here the loop goes on."""
    out = new_totals(num_classes)
    continuing, rows, carried = False, None, None
    out["rows"] = []
    for i in range(num_scans):
        new = [np.asarray(a, np.float64) for a in getitem(i)]
        if continuing:
            rows = [np.concatenate((r, a), axis=0) for r, a in zip(rows, new)]
        else:
            rows = new if carried is None else [np.concatenate((a, c), axis=0) for a, c in zip(new, carried)]
        out["rows"].append(rows[0].shape[0])
        continuing = rows[0].shape[0] < batch_size
        if continuing:
            continue
        carried = [r[batch_size:] for r in rows] if rows[0].shape[0] > batch_size else None
        data, label, smpw = (r[:batch_size].copy() for r in rows)
        fed = data.astype(np.float32)
        out["fed"].append(fed)
        out["labels"].append(label.astype(np.int32))
        out["smpw"].append(smpw.astype(np.float32))
        score(out, np.asarray(forward(fed), np.float32), label, smpw.astype(np.float32), num_classes, extra)
    out["left"] = rows[0].shape[0] if continuing else (0 if carried is None else carried[0].shape[0])
    return finish(out, num_scans)


def report(out, names, whole):
    """the lines T:315-325 / T:403-415 log: both loops print the per-class table (a class whose iou_deno is 0 prints nan)"""
    head = "Eval whole scene" if whole else "Eval"
    lines = ["%s mean loss: %f" % (head, out["mean_loss"]), "Eval point avg class IoU: %f" % out["miou"],
             "%s point accuracy: %f" % (head, out["accuracy"]), "%s point avg class acc: %f" % (head, out["class_acc"])]
    hist = out["hist"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        weights = hist[1:].astype(np.float32) / np.sum(hist[1:].astype(np.float32))
        txt = "------- IoU --------\n"
        for l in range(1, len(out["seen"])):
            txt += "class %s weight: %.3f, IoU: %.3f \n" % (names[l] + " " * (14 - len(names[l])), weights[l - 1],
                                                            np.int64(out["correct"][l]) / float(out["deno"][l]))
    lines.append(txt)
    return lines
