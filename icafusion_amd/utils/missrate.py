"""KAIST log-average miss rate (MR^-2 over nine FPPI points) for All / Day / Night and the six scale and occlusion subsets — the
reference's evaluation_script/evaluation_script.py, split as the rest of the validation path is:

* the per-image half (score sort + ignore-aware greedy matching under all seven set-ups, :46-294) runs on the device: one
  icaf_missrate_match launch (icafusion_amd/csrc/missrate.hip, ops.missrate_match);
* the data-set half (`accumulate`: the global score sort, the cumulative TP / FP counts, the FPPI sweep and the log average, :296-395 and
  :432-475) is restated here in numpy fp64, operation for operation.

Quirks of the reference that are kept because published numbers contain them:
  - a detection matched to the annotation whose `id` is 0 counts as UNMATCHED (dtMatches stores the id and is tested for truth);
  - an image without detections contributes nothing, not even its labels, to the number of positives (evaluateImg returns None);
  - an FPPI threshold below the smallest fppi reads the LAST recall value (searchsorted - 1 = -1, Python's negative index);
  - without any non-ignored detection the nine recalls stay 0 (MR = 1 + 1e-5); a subset without an evaluated image or without a
    positive label gives -1;
  - among ignored labels the first one at IoU >= 0.5 wins, not the best one, and ties between regular labels go to the later label.

File formats: the annotation JSON of the reference (images: id, im_name; annotations: id, image_id, bbox [x, y, w, h], height, occlusion,
ignore; a `.gz` of it is read too) and `result.txt` (`frame,x,y,w,h,score`, frame 1-based: what test.py --save-txt writes)."""
import gzip
import json

import numpy as np

from .._lib import MISSRATE_KEEP, MISSRATE_MAX_DET

FPPI_THRS = np.array([0.0100, 0.0178, 0.0316, 0.0562, 0.1000, 0.1778, 0.3162, 0.5623, 1.0000])      # KAISTParams.fppiThrs (:489)
# evaluate() (:546-646): name -> (set-up, subset of the images)
SUBSETS = (("all", 0, "all"), ("day", 0, "day"), ("night", 0, "night"), ("near", 1, "all"), ("medium", 2, "all"), ("far", 3, "all"),
           ("none", 4, "all"), ("partial", 5, "all"), ("heavy", 6, "all"))
KEYS = tuple(k for k, _, _ in SUBSETS) + ("recall_all",)


def _open_text(path):
    return gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)


def load_annotations(json_path):
    """Annotation file -> label table in annotation order, grouped by image in ascending image id (a stable sort: what the reference's
    per-image lists hold).  Returns a dict of numpy arrays: box (G, 4) fp64 [x, y, w, h], height (G,) fp64, occlusion / ignore (G,) int32,
    id (G,) int64, off (I + 1,) int32 (image i owns rows off[i]:off[i + 1]), image_id (I,) int64 ascending, plus im_name (list of str)."""
    with _open_text(json_path) as f:
        data = json.load(f)
    images = sorted(data["images"], key=lambda im: im["id"])
    image_id = np.array([im["id"] for im in images], dtype=np.int64)
    if len(image_id) == 0 or len(np.unique(image_id)) != len(image_id):
        raise ValueError(f"{json_path}: image ids must be unique and at least one image is needed")
    pos = {int(v): i for i, v in enumerate(image_id)}
    anns = [a for a in data["annotations"] if a.get("category_id", 1) == 1]            # evaluate() sets catIds = [1]
    try:
        img_of = np.array([pos[int(a["image_id"])] for a in anns], dtype=np.int64)
    except KeyError as e:
        raise ValueError(f"{json_path}: annotation of unknown image {e}") from None
    keep = np.argsort(img_of, kind="stable")
    anns, img_of = [anns[i] for i in keep], img_of[keep]
    G = len(anns)
    table = {
        "box": np.array([a["bbox"] for a in anns], dtype=np.float64).reshape(G, 4),
        "height": np.array([a["height"] for a in anns], dtype=np.float64),
        "occlusion": np.array([a["occlusion"] for a in anns], dtype=np.int32),
        "ignore": np.array([1 if a.get("ignore", 0) else 0 for a in anns], dtype=np.int32),
        "id": np.array([a["id"] for a in anns], dtype=np.int64),
        "off": np.concatenate(([0], np.cumsum(np.bincount(img_of, minlength=len(images))))).astype(np.int32),
        "image_id": image_id,
        "im_name": [im.get("im_name", str(im["id"])) for im in images],
    }
    return table


def read_result_txt(path):
    """`frame,x,y,w,h,score` lines -> (image (N,) int64 = frame - 1, rows (N, 5) fp64 [x, y, w, h, score]) in file order; every number is
    parsed as the reference parses it (Python's float).  A `.gz` of the file is read too."""
    image, rows = [], []
    with _open_text(path) as f:
        for ln, line in enumerate(f, 1):
            if not line.strip():
                continue
            v = [float(t) for t in line.split(",")]
            if len(v) != 6 or v[0] != int(v[0]):
                raise ValueError(f"{path}:{ln}: expected frame,x,y,w,h,score")
            image.append(int(v[0]) - 1)
            rows.append(v[1:])
    return np.array(image, dtype=np.int64), np.array(rows, dtype=np.float64).reshape(len(rows), 5)


def write_result_txt(path, image, rows, fmt="%.17g"):
    """The inverse of read_result_txt; `%.17g` prints every fp64 so that it reads back to the same bits."""
    with open(path, "w") as f:
        for i, r in zip(np.asarray(image).tolist(), np.asarray(rows, dtype=np.float64).tolist()):
            f.write(",".join(["%d" % (i + 1)] + [fmt % v for v in r]) + "\n")


def pack_detections(n_images, image, rows, cap=None):
    """Detections in arrival order -> the store of icaf_missrate_match: dt (I, cap, 5) fp64 and count (I,) int32, an image's rows in
    arrival order.  An image with more than 1000 detections keeps the reference's stable top 1000 (still in arrival order: the device
    sort then reproduces the reference's order).  cap defaults to the largest count (at least 1)."""
    image, rows = np.asarray(image, dtype=np.int64), np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    if len(image) != len(rows):
        raise ValueError("one image index per detection row")
    if len(image) and (image.min() < 0 or image.max() >= n_images):
        raise ValueError(f"detections name image {int(image.min() if image.min() < 0 else image.max()) + 1}, the annotations hold {n_images}")
    if not np.isfinite(rows[:, 4]).all():
        raise ValueError("non-finite detection score")
    by_image = np.argsort(image, kind="stable")
    count = np.bincount(image, minlength=n_images)
    if count.max(initial=0) > MISSRATE_KEEP:
        start = np.concatenate(([0], np.cumsum(count)))
        drop = np.zeros(len(image), bool)
        for i in np.nonzero(count > MISSRATE_KEEP)[0]:
            mine = by_image[start[i]:start[i + 1]]
            drop[mine[np.argsort(-rows[mine, 4], kind="mergesort")[MISSRATE_KEEP:]]] = True
        image, rows = image[~drop], rows[~drop]
        by_image = np.argsort(image, kind="stable")
        count = np.bincount(image, minlength=n_images)
    cap = max(int(count.max(initial=0)), 1) if cap is None else int(cap)
    if cap > MISSRATE_MAX_DET or count.max(initial=0) > cap:
        raise ValueError(f"cap {cap}: at most {MISSRATE_MAX_DET} rows per image, and at least the largest count ({int(count.max(initial=0))})")
    dt = np.zeros((n_images, cap, 5), dtype=np.float64)
    start = np.concatenate(([0], np.cumsum(count)))[:-1]
    simg = image[by_image]
    dt[simg, np.arange(len(simg)) - start[simg]] = rows[by_image]
    return dt, count.astype(np.int32)


def matched_ids(dt_gt, ann_id):
    """Matched label rows (-1 = none) -> the reference's dtMatches: the annotation's `id`, 0 where unmatched."""
    dt_gt, ann_id = np.asarray(dt_gt), np.asarray(ann_id, dtype=np.int64)
    if ann_id.size == 0:
        return np.zeros(dt_gt.shape, dtype=np.int64)
    return np.where(dt_gt >= 0, ann_id[np.maximum(dt_gt, 0)], 0)


def accumulate(count, score, dt_id, dt_ignore, gt_ignore, gt_off, setup, first=0, last=None):
    """KAISTPedEval.accumulate + summarize (:296-395, :432-475) of one evaluation in numpy fp64: set-up `setup` over the images
    [first, last).  count (I,) kept detections per image (<= 1000), score (I, cap) the scores in sorted order, dt_id (I, cap, 7) matched
    annotation ids (0 = unmatched), dt_ignore (I, cap) and gt_ignore (G,) the 7-bit masks, gt_off (I + 1,).
    Returns (MR, recall): the log-average miss rate (-1 when no image was evaluated or no label counts) and the last raw recall."""
    count, gt_off = np.asarray(count, dtype=np.int64), np.asarray(gt_off, dtype=np.int64)
    last = len(count) if last is None else last
    I0 = last - first                                                   # the subset's image count, evaluated or not
    n = np.minimum(count[first:last], MISSRATE_KEEP)
    if I0 <= 0 or not (n > 0).any():                                    # E is empty: ys stays -1
        return -1.0, -1.0
    bit = np.uint8(1 << setup)
    sel = np.arange(np.asarray(score).shape[1])[None, :] < n[:, None]     # image order, then sorted position: the reference's concatenation
    scores = np.asarray(score, dtype=np.float64)[first:last][sel]
    inds = np.argsort(-scores, kind="mergesort")
    dtm = np.asarray(dt_id)[first:last, :, setup][sel][inds]
    dt_ig = (np.asarray(dt_ignore)[first:last][sel][inds] & bit) != 0
    lab_img = np.repeat(np.arange(len(count)), np.diff(gt_off))
    evaluated = np.zeros(len(count), bool)
    evaluated[first:last] = n > 0                                       # images without detections do not contribute their labels
    npig = int(np.count_nonzero(evaluated[lab_img] & ((np.asarray(gt_ignore) & bit) == 0)))
    if npig == 0:
        return -1.0, -1.0
    tps = np.logical_and(dtm, np.logical_not(dt_ig))[~dt_ig]
    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))[~dt_ig]
    tp = np.cumsum(tps).astype(np.float64)
    fppi = np.cumsum(fps).astype(np.float64) / I0
    recall = tp / npig                                                  # non-decreasing: the reference's monotone clean-up (:376-378) is a no-op
    q = np.zeros(len(FPPI_THRS))
    if len(recall):
        q = recall[np.searchsorted(fppi, FPPI_THRS, side="right") - 1]   # -1 wraps to the last recall value, as Python's index does
    mr = float(np.exp(np.mean(np.log((1 - q) + 1e-5))))
    return mr, (float(1 - (1 - recall[-1])) if len(recall) else -1.0)


def summarize(table, count, score, dt_gt, dt_ignore, gt_ignore, day_images=1455):
    """evaluate() (:546-646) on the match arrays of one launch: the ten numbers as a dict (KEYS)."""
    dt_id = matched_ids(dt_gt, table["id"])
    I = len(table["image_id"])
    day = min(int(day_images), I)
    rng = {"all": (0, I), "day": (0, day), "night": (day, I)}
    out = {}
    for name, setup, subset in SUBSETS:
        out[name], rec = accumulate(count, score, dt_id, dt_ignore, gt_ignore, table["off"], setup, *rng[subset])
        if name == "all":
            recall_all = rec
    out["recall_all"] = recall_all
    return out


def sorted_scores(dt, order, count):
    """Scores of the store in sorted order: score[i, k] = dt[i, order[i, k], 4] for k < count[i] (0 elsewhere)."""
    dt, order, count = np.asarray(dt), np.asarray(order), np.asarray(count)
    valid = np.arange(order.shape[1])[None, :] < count[:, None]
    idx = np.where(valid, order, 0)
    return np.where(valid, np.take_along_axis(dt[:, :, 4], idx, axis=1), 0.0)


def kaist_miss_rate(annotations, detections, day_images=1455, device="cuda"):
    """The reference's evaluate(annotation file, result.txt): annotations = a path or a load_annotations table, detections = a result.txt
    path or (image, rows) in arrival order.  The matching runs on the device (no CPU fallback); returns the dict of KEYS."""
    from .. import ops
    table = load_annotations(annotations) if isinstance(annotations, (str, bytes)) or hasattr(annotations, "__fspath__") else annotations
    image, rows = read_result_txt(detections) if isinstance(detections, (str, bytes)) or hasattr(detections, "__fspath__") else detections
    dt, count = pack_detections(len(table["image_id"]), image, rows)
    res = ops.missrate_evaluate(table, dt, count, device=device)
    return summarize(table, count, sorted_scores(dt, res["order"], count), res["dt_gt"], res["dt_ignore"], res["gt_ignore"], day_images)


def format_lines(mr):
    """The two MR lines of the reference's test.py:306-307."""
    head = ("%20s" + "%11s" * 9) % ("MR-all", "MR-day", "MR-night", "MR-near", "MR-medium", "MR-far", "MR-none", "MR-partial", "MR-heavy",
                                   "Recall-all")
    return [head, ("%20.2f" + "%11.2f" * 9) % tuple(mr[k] * 100 for k in KEYS)]
