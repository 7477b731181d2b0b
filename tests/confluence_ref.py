"""Vectorised CPU statement of the confluence rules (include/icaf.h, the confluence block), written from the rules and not from the kernel:
the proximity matrix of a class is computed once in numpy fp64, in the worded operation order, and every pick re-derives every value from it.
The host tests pin it to the reference's recorded kept indices (tests/golden/confluence); the GPU tests may then use it for inputs that have
no recorded result (poisoned buffers, the decoded rows of a forward)."""
import numpy as np

NEIGHBOUR, START, MIN_CONF = 2.0, 10000.0, 2e-4


def proximity(boxes):
    """(m, 4) fp32 xyxy -> (m, m) fp64 p(i, j); NaN on the diagonal and wherever the four values of an axis coincide."""
    b = np.asarray(boxes, np.float64)
    m = len(b)
    out = np.empty((m, m), np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r0 in range(0, m, 256):
            a = b[r0:r0 + 256, None, :]
            terms = []
            for lo_col, hi_col in ((0, 2), (1, 3)):
                v = np.stack(np.broadcast_arrays(a[..., lo_col], a[..., hi_col], b[None, :, lo_col], b[None, :, hi_col]), -1)
                lo, hi = v.min(-1, keepdims=True), v.max(-1, keepdims=True)
                nv = (v - lo) / (hi - lo)
                terms += [np.abs(nv[..., 0] - nv[..., 2]), np.abs(nv[..., 1] - nv[..., 3])]
            out[r0:r0 + 256] = ((terms[0] + terms[1]) + terms[2]) + terms[3]
    out[np.arange(m), np.arange(m)] = np.nan
    return out


def confluence(dets, class_num, p_thres=0.6, trace=None):
    """dets (n, 6) [x1, y1, x2, y2, conf, cls] -> sorted int64 kept indices; `trace` (a list) receives the picks in order."""
    dets = np.asarray(dets, np.float32)
    keep = []
    for c in range(class_num):
        idx = np.flatnonzero(dets[:, 5] == c)
        if not len(idx):
            continue
        conf = dets[idx, 4].astype(np.float64)
        assert (conf > MIN_CONF).all(), "precondition: conf > 2e-4"
        P = proximity(dets[idx, :4])
        with np.errstate(invalid="ignore"):
            near = P < NEIGHBOUR
            W = np.where(near, P / conf[:, None], np.inf)
        alive = np.ones(len(idx), bool)
        while alive.any():
            value = np.where(alive[None, :], W, np.inf).min(1)
            value[np.isinf(value)] = 0.0                      # no neighbour left: 0
            value[~alive] = np.inf
            pick = int(np.argmin(value))                      # the first of the least values
            assert alive.sum() == 1 or value[pick] < START
            keep.append(int(idx[pick]))
            if trace is not None:
                trace.append(int(idx[pick]))
            with np.errstate(invalid="ignore"):
                alive &= ~(P[pick] < p_thres)
            alive[pick] = False
    return np.unique(np.asarray(keep, np.int64))


def candidates(pred, conf_thres):
    """One image's decoded rows (rows, 5 + nc) fp32 -> its candidate list (n, 6) fp32, in the reference's order."""
    x = np.asarray(pred, np.float32)
    x = x[x[:, 4] > np.float32(conf_thres)]
    conf = x[:, 5:] * x[:, 4:5]
    half = x[:, 2:4] / np.float32(2)
    box = np.concatenate((x[:, :2] - half, x[:, :2] + half), 1)
    i, j = np.nonzero(conf > np.float32(conf_thres))          # row-major; for nc == 1 the best-class branch gives the same list
    return np.concatenate((box[i], conf[i, j, None], j[:, None].astype(np.float32)), 1).astype(np.float32).reshape(-1, 6)


def confluence_process(prediction, conf_thres=0.1, p_thres=0.6):
    """(B, rows, 5 + nc) -> per image the kept candidates (k, 6) fp32 in ascending candidate order, or None."""
    prediction = np.asarray(prediction, np.float32)
    nc = prediction.shape[2] - 5
    out = []
    for x in prediction:
        cand = candidates(x, conf_thres)
        out.append(cand[confluence(cand, nc, p_thres)] if len(cand) else None)
    return out
