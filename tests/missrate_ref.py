"""Scalar restatement of the KAIST miss-rate matching rules (include/icaf.h, icaf_missrate_match), written from the rules and not from the
kernel: plain Python floats (fp64), one detection and one label at a time, the labels walked sequentially exactly as the rules are
worded.  The host tests pin it to the reference evaluator's recorded per-image results; the GPU tests may then use it for inputs that
have no recorded result (staged fp32 boxes, poisoned stores)."""
import numpy as np

HT_RNG = ((55, 1e10), (115, 1e10), (45, 115), (1, 45), (1, 1e10), (1, 1e10), (1, 1e10))
OCC_RNG = ((0, 1), (0,), (0,), (0,), (0,), (1,), (2,))
KEEP = 1000


def label_ignore(box, height, occlusion, base, s):
    x, y, w, h = box
    lo, hi = HT_RNG[s]
    if height < lo or height > hi or occlusion not in OCC_RNG[s] or x < 5 or y < 5 or x + w > 635 or y + h > 507:
        return 1
    return 1 if base else 0


def iou(d, g, ignored):
    dx1, dy1, dx2, dy2 = d[0], d[1], d[0] + d[2], d[1] + d[3]
    gx1, gy1, gx2, gy2 = g[0], g[1], g[0] + g[2], g[1] + g[3]
    darea, garea = d[2] * d[3], g[2] * g[3]
    iw = min(dx2, gx2) - max(dx1, gx1)
    if iw <= 0:
        return 0.0
    ih = min(dy2, gy2) - max(dy1, gy1)
    if ih <= 0:
        return 0.0
    t = iw * ih
    union = darea if ignored else darea + garea - t
    return t / union


def match_image(gt_box, gt_height, gt_occ, gt_base, dets):
    """One image: labels (G rows) and detections (n, 5) [x, y, w, h, score] in arrival order ->
    order (min(n, 1000),) sorted position -> arrival index, dt_gt (m, 7) matched LOCAL label index or -1, dt_ignore (m,) and
    gt_ignore (G,) 7-bit masks."""
    G, n = len(gt_box), len(dets)
    boxes = [[float(v) for v in b] for b in np.asarray(gt_box).reshape(G, 4)]
    dets = [[float(v) for v in d] for d in np.asarray(dets).reshape(n, 5)]
    order = sorted(range(n), key=lambda i: -dets[i][4])[:KEEP]           # Python's sort is stable: equal scores keep arrival order
    m = len(order)
    dt_gt = np.full((m, 7), -1, dtype=np.int32)
    dt_ignore, gt_ignore = np.zeros(m, dtype=np.uint8), np.zeros(G, dtype=np.uint8)
    for s in range(7):
        flag = [label_ignore(boxes[j], float(gt_height[j]), int(gt_occ[j]), int(gt_base[j]), s) for j in range(G)]
        for j in range(G):
            gt_ignore[j] |= flag[j] << s
        labels = [j for j in range(G) if not flag[j]] + [j for j in range(G) if flag[j]]
        taken = set()
        for k, a in enumerate(order):
            best, got, got_ignored = 0.5, -1, False
            for j in labels:
                if not flag[j] and j in taken:
                    continue
                if got >= 0 and flag[j]:
                    break
                v = iou(dets[a], boxes[j], flag[j])
                if v < best:
                    continue
                best, got, got_ignored = v, j, bool(flag[j])
            if got < 0:
                continue
            dt_gt[k, s] = got
            if got_ignored:
                dt_ignore[k] |= 1 << s
            else:
                taken.add(got)
    return np.array(order, dtype=np.int32), dt_gt, dt_ignore, gt_ignore


def match_all(table, dt, count):
    """The arrays of ops.missrate_match from the packed store: order (I, cap), dt_gt (I, cap, 7) global label rows, dt_ignore (I, cap),
    gt_ignore (G,); rows beyond the kept count are -1 / 0."""
    I, cap, _ = dt.shape
    off = table["off"]
    order = np.full((I, cap), -1, dtype=np.int32)
    dt_gt = np.full((I, cap, 7), -1, dtype=np.int32)
    dt_ignore = np.zeros((I, cap), dtype=np.uint8)
    gt_ignore = np.zeros(len(table["id"]), dtype=np.uint8)
    for i in range(I):
        a, b = int(off[i]), int(off[i + 1])
        o, g, di, gi = match_image(table["box"][a:b], table["height"][a:b], table["occlusion"][a:b], table["ignore"][a:b], dt[i, :int(count[i])])
        m = len(o)
        order[i, :m], dt_ignore[i, :m], gt_ignore[a:b] = o, di, gi
        dt_gt[i, :m] = np.where(g >= 0, g + a, -1)
    return order, dt_gt, dt_ignore, gt_ignore
