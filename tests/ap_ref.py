"""Scalar restatement of ap_per_class (reference utils/metrics.py:18-82, compute_ap :85-110) with a DEFINED order: class ascending, confidence
descending, equal confidences in arrival order.  Python floats are IEEE doubles and nothing here is fused, so every value is what numpy's
float64 expressions give; `interp` is np.interp rule for rule.  Pinned to the reference's recorded outputs (tests/golden/stats/) on inputs with
distinct confidences by tests/test_val_stats_host.py; with ties it is the yardstick of the device kernels."""
import numpy as np

PX = 1000
AP_POINTS = 101


def linspace(k, num):
    """np.linspace(0, 1, num)[k]"""
    return 1.0 if k == num - 1 else k * (1.0 / (num - 1))


def interp(x, xp, fp, left=None):
    """np.interp(x, xp, fp, left=left) for one x; xp ascending (equal neighbours allowed), finite."""
    n = len(xp)
    if x < xp[0]:
        return fp[0] if left is None else left
    if x > xp[n - 1]:
        return fp[n - 1]
    lo, hi = 0, n - 1                                   # the LARGEST j with xp[j] <= x
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if xp[mid] <= x:
            lo = mid
        else:
            hi = mid - 1
    j = lo
    if j == n - 1 or xp[j] == x:
        return fp[j]
    slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
    return slope * (x - xp[j]) + fp[j]


def stable_order(conf, cls):
    """Sorted position -> arrival index: class ascending, confidence descending, ties by arrival index."""
    conf, cls = np.asarray(conf, np.float32), np.asarray(cls).astype(np.int64)
    by_conf = np.argsort(-conf.astype(np.float64), kind="stable")
    return by_conf[np.argsort(cls[by_conf], kind="stable")]


def compute_ap(recall, precision):
    """recall / precision: float64 arrays of one class and threshold.  The envelope is a reverse running maximum (exact in any order)."""
    mrec = np.concatenate(([0.0], recall, [recall[-1] + 0.01])).tolist()
    mpre = np.maximum.accumulate(np.concatenate(([1.0], precision, [0.0]))[::-1])[::-1].tolist()
    y = [interp(linspace(k, AP_POINTS), mrec, mpre) for k in range(AP_POINTS)]
    acc = 0.0
    for k in range(AP_POINTS - 1):                      # np.trapz's terms d * (y1 + y0) / 2, summed in index order
        acc += (linspace(k + 1, AP_POINTS) - linspace(k, AP_POINTS)) * (y[k + 1] + y[k]) / 2.0
    return acc


def ap_per_class(tp, conf, pred_cls, unique_classes, n_l):
    """tp (n, T) bool, conf (n,) fp32, pred_cls (n,) ints, unique_classes ascending with label counts n_l.  Returns a dict: perm (n,), tpc
    (T, n) (inclusive TP count inside the class by sorted position, 0 for rows of classes without labels), ap (nc, T), p / r / f1 (nc, 1000),
    best, tp / fp / fn (nc,)."""
    tp = np.asarray(tp).astype(bool)
    tp = tp.reshape(len(conf), tp.shape[1] if tp.ndim == 2 else 1)
    conf, pred_cls = np.asarray(conf, np.float32), np.asarray(pred_cls).astype(np.int64)
    n, T = tp.shape
    nc = len(unique_classes)
    perm = stable_order(conf, pred_cls)
    stp, sconf, scls = tp[perm], conf[perm].astype(np.float64), pred_cls[perm]
    tpc_all = np.zeros((T, n), np.int64)
    ap, p, r = np.zeros((nc, T)), np.zeros((nc, PX)), np.zeros((nc, PX))
    nl_last = 0
    for ci, c in enumerate(unique_classes):
        rows = np.flatnonzero(scls == int(c))
        nl_last = int(n_l[ci])                          # the reference's loop variable survives the loop (:45, :78)
        if len(rows) == 0 or nl_last == 0:
            continue
        tpc = stp[rows].astype(np.int64).cumsum(0)      # (np, T)
        tpc_all[:, rows] = tpc.T
        npred = len(rows)
        nld = nl_last + 1e-16
        # element-wise IEEE divisions of exact integers: one rounding each, the same value as the scalar expression
        rows1 = np.arange(1, npred + 1, dtype=np.float64)
        xp = (-sconf[rows]).tolist()
        rec0, pre0 = (tpc[:, 0] / nld).tolist(), (tpc[:, 0] / rows1).tolist()
        for k in range(PX):
            x = -linspace(k, PX)
            r[ci, k] = interp(x, xp, rec0, left=0.0)
            p[ci, k] = interp(x, xp, pre0, left=1.0)
        for t in range(T):
            ap[ci, t] = compute_ap(tpc[:, t] / nld, tpc[:, t] / rows1)
    f1 = np.zeros((nc, PX))
    mean = np.zeros(PX)
    for k in range(PX):
        acc = 0.0
        for ci in range(nc):
            f1[ci, k] = 2.0 * p[ci, k] * r[ci, k] / (p[ci, k] + r[ci, k] + 1e-16)
            acc += f1[ci, k]
        mean[k] = acc / nc if nc else 0.0
    best = 0
    for k in range(1, PX):
        if mean[k] > mean[best]:
            best = k
    tpn = np.array([float(np.round(r[ci, best] * float(nl_last))) for ci in range(nc)])
    fpn = np.array([float(np.round(tpn[ci] / (p[ci, best] + 1e-16) - tpn[ci])) for ci in range(nc)])
    return {"perm": perm, "tpc": tpc_all, "ap": ap, "p": p, "r": r, "f1": f1, "best": best, "tp": tpn, "fp": fpn, "fn": float(nl_last) - tpn}
