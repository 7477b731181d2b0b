"""Scalar numpy statement of the two modes of the reference's non_max_suppression that oracle.non_max_suppression leaves out — apriori
labels (utils/general.py:545-552) and merge-NMS (:594-600) — on top of that oracle's candidate logic and greedy core.  The test oracle of
icaf_nms_ex: it implements exactly the summation rule of include/icaf.h, so the device is compared bit for bit; `exact=True` returns the
quotient of the two fp64 sums instead (no rounding to fp32 before the division), the yardstick for the reference's own fp32 result."""
import numpy as np

from oracle import icaf_oracle as oracle

MERGE_LIMIT = 3000
F = np.float32


def candidates(x, conf_thres, classes, multi_label, labels=None):
    """One image's candidate list (n, 6) [x1, y1, x2, y2, conf, cls] in the reference's order: :543-575 with the label rows of :545-552
    appended behind the rows that pass the objectness test."""
    nc = x.shape[1] - 5
    x = x[x[:, 4] > F(conf_thres)].copy()
    if labels is not None and len(labels):
        l = np.asarray(labels, F).reshape(-1, 5)
        v = np.zeros((len(l), nc + 5), F)
        v[:, :4] = l[:, 1:5]
        v[:, 4] = 1.0
        v[np.arange(len(l)), l[:, 0].astype(np.int64) + 5] = 1.0
        x = np.concatenate((x, v), 0)
    if x.shape[0] == 0:
        return np.zeros((0, 6), F)
    x[:, 5:] *= x[:, 4:5]
    half = x[:, 2:4] / F(2)
    box = np.concatenate((x[:, 0:2] - half, x[:, 0:2] + half), 1)
    if multi_label:
        i, j = np.nonzero(x[:, 5:] > F(conf_thres))
        det = np.concatenate((box[i], x[i, j + 5][:, None], j[:, None].astype(F)), 1)
    else:
        j = x[:, 5:].argmax(1)
        conf = x[np.arange(x.shape[0]), j + 5]
        det = np.concatenate((box, conf[:, None], j[:, None].astype(F)), 1)[conf > F(conf_thres)]
    if classes is not None:
        det = det[np.isin(det[:, 5], np.asarray(classes, F))]
    return det.astype(F)


def _iou_row(bi, boxes):
    """box_iou(boxes[i:i+1], boxes)[0] with the operation order of utils/general.py:455-477, fp32"""
    a1 = (bi[2] - bi[0]) * (bi[3] - bi[1])
    a2 = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    w = np.maximum(np.minimum(bi[2], boxes[:, 2]) - np.maximum(bi[0], boxes[:, 0]), F(0))
    h = np.maximum(np.minimum(bi[3], boxes[:, 3]) - np.maximum(bi[1], boxes[:, 1]), F(0))
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (a1 + a2 - inter)


def _lane_sum(values, hit):
    """THE summation rule: partial sum l takes the hits j = l, l + 64, ... in ascending j from 0.0 (fp64); v[l] += v[l ^ o] for o = 32 .. 1"""
    v = np.zeros(64, np.float64)
    for j in np.nonzero(hit)[0]:
        v[j & 63] = v[j & 63] + values[j]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[idx ^ o]
    return v[0]


def merge(det, keep, iou_thres, agnostic, max_wh=4096.0, redundant=True, exact=False):
    """:594-600 on a candidate list `det` (n, 6) and the kept indices of plain NMS -> (rows (k, 6), kept indices).  exact: fp64 rows whose
    coordinates are the quotient of the fp64 sums."""
    off = det[:, 5:6] * F(0.0 if agnostic else max_wh)
    boxes, scores = (det[:, :4] + off).astype(F), det[:, 4]
    out = det[keep].astype(np.float64 if exact else F)
    nhit = np.zeros(len(keep), np.int64)
    s64, x64 = scores.astype(np.float64), det[:, :4].astype(np.float64)
    for r, i in enumerate(keep):
        hit = _iou_row(boxes[i], boxes) > F(iou_thres)
        nhit[r] = hit.sum()
        sw = _lane_sum(s64, hit)
        sx = [_lane_sum(s64 * x64[:, c], hit) for c in range(4)]             # fp32 x fp32 products: exact in fp64
        with np.errstate(invalid="ignore", divide="ignore"):
            out[r, :4] = [np.float64(s) / np.float64(sw) for s in sx] if exact else [F(s) / F(sw) for s in sx]
    sel = nhit > 1 if redundant else np.ones(len(keep), bool)
    return out[sel], np.asarray(keep)[sel]


def non_max_suppression(pred, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, labels=None, merge_nms=False,
                        redundant=True, max_det=300, max_nms=30000, max_wh=4096.0, exact=False):
    """-> (list of (k, 6) rows, list of kept indices into the image's candidate list, list of candidate counts n)"""
    pred = np.asarray(pred, F)
    multi_label = multi_label and pred.shape[2] - 5 > 1
    outs, idxs, ns = [], [], []
    for b, x in enumerate(pred):
        det = candidates(x, conf_thres, classes, multi_label, labels[b] if labels is not None else None)
        n = det.shape[0]
        ns.append(n)
        if n == 0:
            outs.append(np.zeros((0, 6), F)); idxs.append(np.zeros((0,), np.int64)); continue
        if n > max_nms:
            det = det[np.argsort(-det[:, 4], kind="stable")[:max_nms]]
        off = det[:, 5:6] * F(0.0 if agnostic else max_wh)
        keep = oracle.nms_greedy(det[:, :4] + off, det[:, 4], iou_thres)[:max_det]
        if merge_nms and 1 < n < MERGE_LIMIT:
            rows, keep = merge(det, keep, iou_thres, agnostic, max_wh, redundant, exact)
        else:
            rows = det[keep]
        outs.append(rows); idxs.append(np.asarray(keep, np.int64))
    return outs, idxs, ns


# ----------------------------------------------------------------------------------------------------------------------------------
# The cases: ONE definition for the fixtures recorded from the reference (tests/golden/make_golden_nms_modes.py) and the device tests
# ----------------------------------------------------------------------------------------------------------------------------------
ROWS = 4096 + 37                     # crosses the 4096-row chunk of the keys kernel


def plant(pred, b, rows):
    """Write [cx, cy, w, h, obj, cls conf...] rows into filler rows (objectness 0) of image b, the LAST free rows first — beyond row 4096 —
    and return their row indices."""
    free = np.nonzero(pred[b, :, 4] == 0)[0][::-1]
    at = []
    for k, r in enumerate(rows):
        pred[b, free[k], :] = np.asarray(r, F)
        at.append(int(free[k]))
    return at


def _row(nc, cx, cy, w, h, obj, cls, conf=1.0):
    r = [cx, cy, w, h, obj] + [0.0] * nc
    r[5 + cls] = conf
    return r


def cases(rows=ROWS):
    """name -> dict(pred (B, rows, 5 + nc), labels (list of B (n_i, 5) arrays) or None, kw for non_max_suppression, merge, note)"""
    from icafusion_amd.synth import synth_crowd_prediction
    out = {}

    def labels_case(nc, order, **kw):
        pred = synth_crowd_prediction(3, rows, 40, nc, seed=20 + nc)
        only, both, none = order                                   # which image has labels only / labels and predictions / no labels
        pred[only, :, 4] *= F(0.1)                                  # every prediction below the threshold: the labels are all there is
        last = nc - 1
        strong = _row(nc, 1200.0, 300.0, 40.0, 100.0, 0.99, last, 0.99)
        plant(pred, both, [strong])
        labels = [np.zeros((0, 5), F)] * 3
        labels[only] = np.asarray([[0, 100, 100, 30, 80], [last, 300, 200, 30, 80], [0, 500, 120, 36, 90], [0, 500, 120, 36, 90]], F)   # two identical labels
        labels[both] = np.asarray([[last, 1200, 300, 40, 100],                      # identical to the strong prediction: wins at 1.0
                                   [min(1, last), 320, 256, 50, 120], [last, 900, 400, 44, 96]], F)
        return dict(pred=pred, labels=labels, kw=dict(conf_thres=0.25, iou_thres=0.45, **kw), merge=False)

    out["labels_nc3_multi"] = labels_case(3, (1, 2, 0), multi_label=True)                              # offsets 0 0 4 7: an empty image first
    out["labels_nc1"] = labels_case(1, (2, 0, 1))                                                     # offsets 0 3 3 7: an empty image in the middle
    out["labels_nc3_agnostic_filter"] = labels_case(3, (0, 1, 2), agnostic=True, classes=[0, 2])      # the class-1 label is filtered out

    def merge_base(nc, seed, n=320):
        return synth_crowd_prediction(3, rows, n, nc, seed=seed)

    p = merge_base(1, 31)
    plant(p, 0, [_row(1, 1500.0, 300.0, 40.0, 100.0, 0.9, 0)])                                        # isolated: one hit (itself), dropped by `redundant`
    plant(p, 1, [_row(1, 1026.0, 1026.0, 4.0, 4.0, 0.9, 0), _row(1, 1026.0, 1025.0, 4.0, 2.0, 0.8, 0)])   # IoU = 8 / 16 exactly 0.5: strict >, no hit
    plant(p, 2, [_row(1, 1500.0, 300.0, 0.0, 100.0, 0.97, 0), _row(1, 1500.0, 300.0, 40.0, 100.0, 0.6, 0),
                 _row(1, 1501.0, 300.0, 40.0, 100.0, 0.5, 0)])                                        # zero area: IoU NaN, kept by NMS, no hit at all
    out["merge_nc1"] = dict(pred=p, labels=None, kw=dict(conf_thres=0.1, iou_thres=0.5), merge=True)
    p = merge_base(3, 32)
    for b in range(3):
        at = np.nonzero(p[b, :, 4] > 0)[0][::3]
        p[b, at, 5:] = np.maximum(p[b, at, 5:], F(0.6))                                              # every third box carries all three labels
    out["merge_nc3_multi"] = dict(pred=p, labels=None, kw=dict(conf_thres=0.1, iou_thres=0.5, multi_label=True), merge=True)
    p = merge_base(3, 33)
    for b in range(3):                                                                                # two classes on one spot, far from the crowd:
        plant(p, b, [_row(3, 1500.0, 300.0, 40.0, 100.0, 0.9, 0), _row(3, 1502.0, 301.0, 40.0, 100.0, 0.8, 2)])   # they overlap only without the class offset
    out["merge_nc3_classoff"] = dict(pred=p, labels=None, kw=dict(conf_thres=0.1, iou_thres=0.5), merge=True)
    out["merge_nc3_agnostic"] = dict(pred=p, labels=None, kw=dict(conf_thres=0.1, iou_thres=0.5, agnostic=True), merge=True)
    counts = (0, 1, 2, 2999, 3000)
    p = np.concatenate([synth_crowd_prediction(1, rows, n, 1, seed=40 + i) for i, n in enumerate(counts)], 0)
    out["merge_counts"] = dict(pred=p, labels=None, kw=dict(conf_thres=0.1, iou_thres=0.5), merge=True, counts=counts)
    p = np.zeros((1, rows, 6), F)
    p[..., :4] = (320.0, 256.0, 40.0, 100.0)
    grid = []
    for k in range(360):                                                                              # 360 separate spots, two boxes on each: 300 kept of 720 candidates
        cx, cy = 32.0 + 24.0 * (k % 24), 32.0 + 40.0 * (k // 24)
        grid += [_row(1, cx, cy, 16.0, 32.0, 0.95 - k * 0.001, 0), _row(1, cx + 1.0, cy, 16.0, 32.0, 0.5 - k * 0.001, 0)]
    plant(p, 0, grid)
    out["merge_maxdet"] = dict(pred=p, labels=None, kw=dict(conf_thres=0.1, iou_thres=0.5), merge=True)
    c = labels_case(3, (1, 2, 0), multi_label=True)
    c["labels"][1] = np.concatenate((c["labels"][1], np.asarray([[2, 301, 201, 30, 80]], F)), 0)       # a partner for one label: that pair merges
    c["merge"] = True
    out["merge_labels"] = c
    return out


def run_case(c, exact=False, redundant=True):
    return non_max_suppression(c["pred"], labels=c["labels"], merge_nms=c["merge"], redundant=redundant, exact=exact, **c["kw"])
