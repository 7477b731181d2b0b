"""Builders and references of the boundary tests for the Detect decode (csrc/detect.hip) and the NMS walk (csrc/nms.hip), CPU only.
tests/test_detect_nms_edges_host.py pins them (and shows that the checks fail on planted defects); tests/test_gpu_exact_detect.py and
tests/test_gpu_nms_edges.py run the same cases on the device.

Decode: decode64 is a float64 statement of the eval branch of the reference's Detect.forward; decode_exact gives the values that follow
exactly from the fp32 expressions (logit >= 17: sigmoid rounds to 1; logit <= -104: expf overflows and the quotient is 0);
emulate_decode32 restates the device's fp32 expressions in numpy and is where the decode defects are planted.

NMS: the oracle is oracle.icaf_oracle.non_max_suppression.  emulate_nms restates the device's decision (iou_gt: two products outside a
+-2^-20 band, the division inside it) and its candidate order; the builders make the inputs on which that decision and the counted
edges of the walk (rounds, max_nms, max_det, bin edges, threshold equality) can differ from the oracle's."""
import numpy as np

F = np.float32
RTOL, ATOL = 1e-6, 1e-5                               # z against decode64: the tolerance test_detect_decode always used
ONE_LO, ZERO_HI = 17.0, -104.0                        # logits >= 17: sg == 1 in fp32 (e^-17 < 2^-24); <= -104: expf(104) = +Inf, sg == +0


# ------------------------------------------------------------------------------------------------------------------------------------
# Detect decode
# ------------------------------------------------------------------------------------------------------------------------------------
LOGIT_VALUES = np.array([0.0, -0.0] + [s * v for v in (2.0 ** -30, 1.0, 16.5, 17.0, 20.0, 87.0, 88.5, 89.0, 103.0, 104.5, 1e4, 3e38, np.inf)
                                       for s in (1.0, -1.0)], dtype=F)
ANCHORS3 = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]


def sweep_map(B, ny, nx, na, no):
    """(B, ny, nx, na * no) fp32: every element one of LOGIT_VALUES, index = pixel + 7 * anchor + 11 * o — for a fixed (anchor, o) the
    pixels run through every value (B * ny * nx >= len(LOGIT_VALUES)), so each value meets each o index and each anchor"""
    assert B * ny * nx >= len(LOGIT_VALUES)
    pix = np.arange(B * ny * nx).reshape(B, ny, nx, 1, 1)
    a = np.arange(na).reshape(1, 1, 1, na, 1)
    o = np.arange(no).reshape(1, 1, 1, 1, no)
    return LOGIT_VALUES[(pix + 7 * a + 11 * o) % len(LOGIT_VALUES)].reshape(B, ny, nx, na * no)


def random_map(B, ny, nx, na, no, seed, scale=4.0, tails=True):
    """Gaussian logits, with (tails) one element in sixteen drawn from LOGIT_VALUES"""
    g = np.random.default_rng(seed)
    p = g.normal(0, scale, (B, ny, nx, na * no)).astype(F)
    if tails:
        m = g.random(p.shape) < 1.0 / 16
        p[m] = LOGIT_VALUES[g.integers(0, len(LOGIT_VALUES), int(m.sum()))]
    return p


def to_raw(p, na, no):
    B, ny, nx, _ = p.shape
    return np.ascontiguousarray(p.reshape(B, ny, nx, na, no).transpose(0, 3, 1, 2, 4))


def decode64(p, na, no, stride, anchors):
    """p (B, ny, nx, na * no) fp32 -> z (B, na * ny * nx, no) float64, logits (B, na * ny * nx, no - 5) fp32, raw (B, na, ny, nx, no) fp32"""
    B, ny, nx, _ = p.shape
    raw = to_raw(p, na, no)
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-raw.astype(np.float64)))
    gx = np.arange(nx, dtype=np.float64).reshape(1, 1, 1, nx)
    gy = np.arange(ny, dtype=np.float64).reshape(1, 1, ny, 1)
    anc = np.asarray(anchors, np.float64).reshape(na, 2)
    z = sg.copy()
    z[..., 0] = (sg[..., 0] * 2.0 - 0.5 + gx) * stride
    z[..., 1] = (sg[..., 1] * 2.0 - 0.5 + gy) * stride
    z[..., 2] = (sg[..., 2] * 2.0) ** 2 * anc[:, 0].reshape(1, na, 1, 1)
    z[..., 3] = (sg[..., 3] * 2.0) ** 2 * anc[:, 1].reshape(1, na, 1, 1)
    return z.reshape(B, -1, no), raw[..., 5:].reshape(B, -1, no - 5).copy(), raw


def decode_exact(p, na, no, stride, anchors):
    """(mask, values): the elements of z whose fp32 value follows exactly — sg = 1: xy = ((1.5) + x) * stride, wh = 4 * anchor, conf = 1;
    sg = 0: xy = (x - 0.5) * stride, wh = 0, conf = 0 — as (B, na * ny * nx, no) bool / fp32 (fp32 steps as the device takes them)"""
    B, ny, nx, _ = p.shape
    raw = to_raw(p, na, no)
    one, zero = raw >= F(ONE_LO), raw <= F(ZERO_HI)
    sg = np.where(one, F(1), F(0)).astype(F)
    gx = np.arange(nx, dtype=F).reshape(1, 1, 1, nx)
    gy = np.arange(ny, dtype=F).reshape(1, 1, ny, 1)
    anc = np.asarray(anchors, F).reshape(na, 2)
    st = F(stride)
    v = sg.copy()
    v[..., 0] = ((sg[..., 0] * F(2) - F(0.5)) + gx) * st
    v[..., 1] = ((sg[..., 1] * F(2) - F(0.5)) + gy) * st
    for k in (2, 3):
        d = sg[..., k] * F(2)
        v[..., k] = (d * d) * anc[:, k - 2].reshape(1, na, 1, 1)
    return (one | zero).reshape(B, -1, no), v.reshape(B, -1, no)


DECODE_DEFECTS = ("anchor_swap", "row_past")


def emulate_decode32(p, na, no, stride, anchors, defect=None, fma=False):
    """The device's expressions in numpy fp32 (np.exp stands in for expf) -> z (B, na * ny * nx, no) fp32.  fma: sg * 2 - 0.5 rounded
    once, as a contracting compiler would emit it — the doubling is exact, so the bits cannot change (the host test asserts that)."""
    B, ny, nx, _ = p.shape
    raw = to_raw(p, na, no)
    with np.errstate(over="ignore"):
        sg = (F(1) / (F(1) + np.exp(-raw).astype(F))).astype(F)
    gx = np.arange(nx, dtype=F).reshape(1, 1, 1, nx)
    gy = np.arange(ny, dtype=F).reshape(1, 1, ny, 1)
    anc = np.asarray(anchors, F).reshape(na, 2)
    if defect == "anchor_swap":
        anc = anc[:, ::-1]
    st = F(stride)
    z = sg.copy()
    for k, g in ((0, gx), (1, gy)):
        t = (sg[..., k].astype(np.float64) * 2.0 - 0.5).astype(F) if fma else sg[..., k] * F(2) - F(0.5)
        z[..., k] = (t + g) * st
    for k in (2, 3):
        d = sg[..., k] * F(2)
        z[..., k] = (d * d) * anc[:, k - 2].reshape(1, na, 1, 1)
    return z.reshape(B, -1, no)


def write_level(zbuf, z, row_offset, defect=None):
    """what a level's launch does to the shared z (B, rows_total, no): its rows, nothing else (row_past: one row more)"""
    n = z.shape[1]
    zbuf[:, row_offset:row_offset + n] = z
    if defect == "row_past" and row_offset + n < zbuf.shape[1]:
        zbuf[:, row_offset + n] = z[:, -1]


def u32(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_level(zbuf, sentinel_bits, row_offset, p, na, no, stride, anchors, what=""):
    """zbuf (B, rows_total, no) fp32 after ONE level ran into a buffer that held sentinel_bits everywhere: rows outside the level intact,
    every element inside written, no NaN that the input does not hold, exact values in bits, the rest within RTOL / ATOL of decode64"""
    z64, _, _ = decode64(p, na, no, stride, anchors)
    n = z64.shape[1]
    zb = u32(zbuf)
    inside = np.zeros(zbuf.shape[1], bool)
    inside[row_offset:row_offset + n] = True
    stray = zb[:, ~inside] != np.uint32(sentinel_bits)
    assert not stray.any(), f"{what}: {int(stray.sum())} elements outside rows [{row_offset}, {row_offset + n}) were written"
    got = zbuf[:, row_offset:row_offset + n]
    missed = zb[:, row_offset:row_offset + n] == np.uint32(sentinel_bits)
    assert not missed.any(), f"{what}: {int(missed.sum())} elements of the level still hold the sentinel; first at {np.argwhere(missed)[0]}"
    nan_in = np.isnan(z64)
    assert np.array_equal(np.isnan(got), nan_in), f"{what}: NaN at {int(np.isnan(got).sum())} elements, the input has it at {int(nan_in.sum())}"
    mask, val = decode_exact(p, na, no, stride, anchors)
    ne = mask & (u32(got) != u32(val))
    assert not ne.any(), f"{what}: {int(ne.sum())} exactly derivable elements differ; first at {np.argwhere(ne)[0]}: {got[ne][0]!r} != {val[ne][0]!r}"
    ok = ~nan_in
    err = np.abs(got[ok].astype(np.float64) - z64[ok])
    bad = err > ATOL + RTOL * np.abs(z64[ok])
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond rtol {RTOL} atol {ATOL}; largest error {err.max():.3e}"
    return float((err / (ATOL + RTOL * np.abs(z64[ok]))).max()) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# NMS: the decision
# ------------------------------------------------------------------------------------------------------------------------------------
BAND_HI, BAND_LO = F(1.0 + 2.0 ** -20), F(1.0 - 2.0 ** -20)
DECISION_DEFECTS = ("ge", "naive", "fused_union")
WALK_DEFECTS = ("offset_after_area", "cut_by_slot", "rank_edge")


def xywh2xyxy(b):
    half = b[..., 2:4] / F(2)
    return np.concatenate((b[..., 0:2] - half, b[..., 0:2] + half), -1)


def box_area(b):
    with np.errstate(all="ignore"):
        return (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])


def pair_terms(a, b, area_a, area_b, fused=False):
    """inter and union of xyxy boxes in fp32, the oracle's operation order (fused: the union with one rounding, a + b - w * h contracted)"""
    with np.errstate(all="ignore"):
        dx = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
        dy = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
        w, h = np.where(dx > 0, dx, F(0)).astype(F), np.where(dy > 0, dy, F(0)).astype(F)
        inter = w * h
        s = (area_a + area_b).astype(F)
        uni = (s.astype(np.float64) - w.astype(np.float64) * h.astype(np.float64)).astype(F) if fused else (s - inter).astype(F)
    return inter.astype(F), uni


def band_terms(inter, uni, thr):
    with np.errstate(all="ignore"):
        t = (F(thr) * uni).astype(F)
        yes, no = inter > t * BAND_HI, inter < t * BAND_LO
        regular = (uni > 0) & (F(thr) > 0)
    return yes, no, regular


def in_band(inter, uni, thr):
    """the pairs whose decision the device leaves to the division although the union is regular"""
    yes, no, regular = band_terms(inter, uni, thr)
    return regular & ~(yes | no)


def decide(inter, uni, thr, mode="oracle"):
    """does the kept box suppress the other?  oracle: the division; device: iou_gt of nms.hip; ge / naive: planted"""
    with np.errstate(all="ignore"):
        q = inter / uni
        if mode == "oracle":
            return q > F(thr)
        if mode == "naive":
            return inter > (F(thr) * uni).astype(F)
        yes, no, regular = band_terms(inter, uni, thr)
        return np.where(regular & (yes | no), yes, (q >= F(thr)) if mode == "ge" else (q > F(thr)))


def emulate_nms(pred, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300, max_nms=30000,
                max_wh=4096.0, defect=None):
    """The device's walk in numpy: candidates in slot order, visited by (score descending, slot ascending), cut at max_nms by rank, each
    kept box suppressing the later ones through decide(..., "device").  Returns (rows, indices) like the oracle with return_indices."""
    pred = np.asarray(pred, F)
    nc = pred.shape[2] - 5
    multi = multi_label and nc > 1
    conf = F(conf_thres)
    mode = defect if defect in ("ge", "naive") else "device"
    outs, idxs = [], []
    for x in pred:
        obj = x[:, 4]
        with np.errstate(all="ignore"):
            sc = (x[:, 5:] * obj[:, None]).astype(F)
        if multi:
            r, j = np.nonzero((obj > conf)[:, None] & (sc > conf))
        else:
            ja = sc.argmax(1)
            best = sc[np.arange(len(x)), ja]
            r = np.nonzero((obj > conf) & (best > conf))[0]
            j = ja[r]
        if classes is not None:
            sel = np.isin(j, np.asarray(classes))
            r, j = r[sel], j[sel]
        n_all = len(r)
        if n_all == 0:
            outs.append(np.zeros((0, 6), F)); idxs.append(np.zeros((0,), np.int64)); continue
        s = sc[r, j]
        box = xywh2xyxy(x[r, :4])
        if defect == "cut_by_slot" and n_all > max_nms:
            order = np.argsort(-s[:max_nms], kind="stable")
        else:
            order = np.argsort(-s, kind="stable")[:max_nms]
        if defect == "rank_edge":
            order = np.delete(order, [k for k in (1024, 4096) if k < len(order)])
        with np.errstate(all="ignore"):
            ob = (box + (j.astype(F) * F(0.0 if agnostic else max_wh))[:, None]).astype(F)
        area = box_area(box if defect == "offset_after_area" else ob)
        bo, ar = ob[order], area[order]
        alive = np.ones(len(order), bool)
        kept, pos = [], 0
        while len(kept) < max_det:
            nz = np.nonzero(alive[pos:])[0]
            if len(nz) == 0:
                break
            p = pos + int(nz[0])
            kept.append(p)
            alive[p] = False
            rest = p + 1 + np.nonzero(alive[p + 1:])[0]
            if len(rest):
                inter, uni = pair_terms(bo[p], bo[rest], ar[p], ar[rest], fused=defect == "fused_union")
                alive[rest[decide(inter, uni, iou_thres, mode)]] = False
            pos = p + 1
        kp = np.asarray(kept, np.int64)
        cand = order[kp]
        outs.append(np.concatenate((box[cand], s[cand][:, None], j[cand][:, None].astype(F)), 1).astype(F))
        idxs.append(kp if n_all > max_nms else cand.astype(np.int64))
    return outs, idxs


def same_result(a, b):
    """two (rows, indices) results: the same bits and the same indices in every image"""
    return all(x.shape == y.shape and np.array_equal(u32(x), u32(y)) for x, y in zip(a[0], b[0])) and \
        all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


# ------------------------------------------------------------------------------------------------------------------------------------
# NMS (a): IoU ulp ladders
# ------------------------------------------------------------------------------------------------------------------------------------
LADDER_THR = (0.45, 0.5, 0.6, 0.05)
LADDER_K = 12
LADDER_BASE = {0.45: 160, 0.5: 160, 0.6: 160, 0.05: 320}  # base pairs: 160 * 25 = 4000 points = 8 images of 500 pairs; at 0.05 the band is a
#                                                       ninth as wide (thr * union), so twice the pairs keep >= 10 exact-equality points
PAIRS_PER_IMAGE = 500                                 # <= 1000 kept boxes per image: below MAX_KEEP = 1024
CELL = 4096.0                                         # one pair per cell along y; heights <= 3400, so pairs never meet
LADDER_CONF = 0.25


def _oracle_pair(a, b, off, thr):
    """a, b (n, 4) xywh, off (n,) class offset -> inter, union, decision of the oracle on the offset xyxy boxes"""
    with np.errstate(all="ignore"):
        A = (xywh2xyxy(a) + off[:, None]).astype(F)
        B = (xywh2xyxy(b) + off[:, None]).astype(F)
    inter, uni = pair_terms(A, B, box_area(A), box_area(B))
    return inter, uni, decide(inter, uni, thr)


def iou_ladder(thr, seed, nc=1, agnostic=False, max_wh=4096.0, n_base=None, K=LADDER_K):
    """n_base * (2K + 1) isolated pairs (A, B) around the place where the oracle's fp32 decision inter / union > thr flips: for every base
    pair the bit pattern of B's cx is bisected between 'concentric' (suppressed) and 'disjoint' (kept), on the boxes as the reference
    forms them (xywh -> xyxy, plus class * max_wh unless agnostic), and the 2K + 1 neighbours in ulps of cx are emitted.  Point q lives
    in image q // PAIRS_PER_IMAGE at cy = CELL * (1 + q % PAIRS_PER_IMAGE): cy and the (even, integer) heights make every y exact, and x
    stays inside (0, 4000), below the class offset — pairs never meet pairs.  Widths of 500 .. 1500 and heights of 500 .. 3000 keep the
    band (2^-20 of thr * union) a few ulps of cx wide."""
    g = np.random.default_rng(seed)
    n_base = LADDER_BASE[thr] if n_base is None else n_base
    P = n_base * (2 * K + 1)
    q = np.arange(P)
    base = q // (2 * K + 1)
    step = q % (2 * K + 1) - K
    wa = g.uniform(500, 1500, n_base)
    ha = 2 * g.integers(250, 1500, n_base)
    wb = wa * g.uniform(0.85, 1.15, n_base)
    hb = np.minimum(2 * np.round(ha * g.uniform(0.85, 1.15, n_base) / 2), 3400)
    cxa = wa / 2 + g.uniform(1, 200, n_base)
    cls = (np.arange(n_base) % nc)[base]
    off = (cls * (0.0 if agnostic else max_wh)).astype(F)
    cy = (CELL * (1 + q % PAIRS_PER_IMAGE)).astype(F)
    a = np.stack((cxa[base], cy, wa[base], ha[base]), 1).astype(F)
    b = np.stack((cxa[base], cy, wb[base], hb[base]), 1).astype(F)
    lo = a[:, 0].copy().view(np.int32)                                 # concentric: IoU >= 0.85^2 > every threshold
    hi = (a[:, 0] + (a[:, 2] + b[:, 2]) / F(2) + F(1)).astype(F).view(np.int32)       # disjoint
    for _ in range(34):
        mid = lo + (hi - lo) // 2
        b[:, 0] = mid.view(F)
        yes = _oracle_pair(a, b, off, thr)[2]
        lo, hi = np.where(yes, mid, lo), np.where(yes, hi, mid)
    assert (hi - lo == 1).all()
    b[:, 0] = (lo + step.astype(np.int32)).view(F)
    inter, uni, sup = _oracle_pair(a, b, off, thr)
    assert float(xywh2xyxy(b)[:, 2].max()) < 4000.0 and float(xywh2xyxy(a)[:, 0].min()) > 0.0
    with np.errstate(all="ignore"):
        eq = (inter / uni) == F(thr)
    return dict(thr=thr, nc=nc, agnostic=agnostic, a=a, b=b, cls=cls, inter=inter, uni=uni, suppressed=sup, band=in_band(inter, uni, thr),
                equal=eq, seed=seed)


def ladder_counts(lad):
    band = lad["band"]
    return dict(points=len(band), band=int(band.sum()), band_suppressed=int((band & lad["suppressed"]).sum()),
                band_kept=int((band & ~lad["suppressed"]).sum()), equal=int(lad["equal"].sum()))


def assert_ladder_reach(lad, what=""):
    """the conditions under which a ladder tests the band at all"""
    c = ladder_counts(lad)
    assert c["band"] >= 100 and c["band_suppressed"] >= 30 and c["band_kept"] >= 30 and c["equal"] >= 10, f"{what}: {c}"
    return c


def _rank_score(rank):
    return ((3900 - rank) * 2.0 ** -12).astype(F)     # exact, distinct, 0.95 .. 0.70 for ranks below 1024


def ladder_ranks(npairs, arrangement):
    i = np.arange(npairs)
    return (2 * i, 2 * i + 1) if arrangement == "adjacent" else (i, npairs + i)


def ladder_pred(lad, arrangement):
    """the pairs as prediction rows (images, 2 * PAIRS_PER_IMAGE, 5 + nc), obj = 1, score in the pair's class column, rows shuffled.
    adjacent: A_i > B_i > A_i+1; split: every A above every B"""
    nc, P = lad["nc"], len(lad["a"])
    imgs = -(-P // PAIRS_PER_IMAGE)
    pred = np.zeros((imgs, 2 * PAIRS_PER_IMAGE, 5 + nc), F)
    g = np.random.default_rng(lad["seed"] + 1)
    for im in range(imgs):
        sl = slice(im * PAIRS_PER_IMAGE, min(P, (im + 1) * PAIRS_PER_IMAGE))
        n = sl.stop - sl.start
        ra, rb = ladder_ranks(n, arrangement)
        rows = g.permutation(2 * PAIRS_PER_IMAGE)[:2 * n]
        for boxes, rank, rr in ((lad["a"][sl], ra, rows[:n]), (lad["b"][sl], rb, rows[n:])):
            pred[im, rr, :4] = boxes
            pred[im, rr, 4] = 1.0
            pred[im, rr, 5 + lad["cls"][sl]] = _rank_score(rank)
    return pred


def same_step_share(npairs, arrangement):
    """smallest / largest share of pairs whose two ranks fall into one 64-candidate step, over every alignment of the steps"""
    ra, rb = ladder_ranks(npairs, arrangement)
    shares = [float((((ra + s) // 64) == ((rb + s) // 64)).mean()) for s in range(64)]
    return min(shares), max(shares)


# ------------------------------------------------------------------------------------------------------------------------------------
# NMS (c, d, f): candidates placed by score rank
# ------------------------------------------------------------------------------------------------------------------------------------
def ranked_pred(scores, distinct, seed, nc=1, multi=False, extra=7, dup_wh=(40.0, 40.0)):
    """One image whose candidates have `scores` (descending, by rank).  The candidates at the ranks in `distinct` are boxes far from
    everything; all others are near-duplicates of one box (per class), so the oracle keeps the first duplicate and every distinct box it
    reaches.  Ranks are dealt to candidate slots at random, equal scores in ascending slot order (the stable sort's order); `extra`
    rows are no candidates (obj = 0).  multi (nc = 3): a duplicate row is a candidate in up to three classes, a distinct row in one.
    Returns (pred (1, rows, 5 + nc), info) with info: n, distinct ranks, cand_of_rank (index in the candidate list), box_of_rank."""
    g = np.random.default_rng(seed)
    scores = np.asarray(scores, F)
    n = len(scores)
    assert (np.diff(scores.astype(np.float64)) <= 0).all()
    distinct = sorted({int(r) for r in distinct if 0 <= r < n})
    m = len(distinct)
    ncm = nc if multi else 1
    if multi:
        nd = n - m
        per_row = [1] * m + [3] * (nd // 3) + ([nd % 3] if nd % 3 else [])
    else:
        assert nc == 1
        per_row = [1] * n
    rows = len(per_row) + extra
    place = g.permutation(rows)[:len(per_row)]
    slot_row, slot_cls = [], []
    for i, k in enumerate(per_row):
        for c in sorted(g.choice(nc, k, replace=False)):
            slot_row.append(place[i]); slot_cls.append(int(c))
    slot_row, slot_cls = np.asarray(slot_row), np.asarray(slot_cls)
    slot_id = slot_row * ncm + (slot_cls if multi else 0)
    sor = np.empty(n, np.int64)                                        # slot (index into slot_row) of every rank
    if multi:
        others = np.setdiff1d(np.arange(n), distinct)
        sor[distinct] = np.arange(m)
        sor[others] = m + g.permutation(n - m)
    else:
        sor[:] = g.permutation(n)
    start = 0
    for end in list(np.nonzero(np.diff(scores.view(np.int32)) != 0)[0] + 1) + [n]:       # equal scores: ascending slot
        seg = sor[start:end]
        sor[start:end] = seg[np.argsort(slot_id[seg], kind="stable")]
        start = end
    pred = np.zeros((1, rows, 5 + nc), F)
    pred[0, :, 0] = 20000.0 + 100.0 * np.arange(rows)                  # non-candidates: anywhere, never looked at
    pred[0, :, 1:4] = (50.0, 10.0, 10.0)
    pred[0, :, 5:] = 0.5
    isd = np.zeros(n, bool)
    isd[distinct] = True
    box_of_rank = np.empty((n, 4), F)
    box_of_rank[:, 0] = 100.0 + g.uniform(-0.05, 0.05, n)
    box_of_rank[:, 1] = 100.0 + g.uniform(-0.05, 0.05, n)
    box_of_rank[:, 2:] = dup_wh
    box_of_rank[isd] = np.stack((1000.0 + 100.0 * np.arange(m), np.full(m, 1000.0), np.full(m, 30.0), np.full(m, 30.0)), 1)
    if multi:                                                          # one box per ROW: the box of its first-dealt rank
        first = {}
        for r in range(n):
            first.setdefault(int(slot_row[sor[r]]), r)
        box_of_rank = box_of_rank[[first[int(slot_row[sor[r]])] for r in range(n)]]
    rr = slot_row[sor]
    pred[0, rr, :4] = box_of_rank
    pred[0, rr, 4] = 1.0
    pred[0, np.unique(rr), 5:] = 0.0
    pred[0, rr, 5 + slot_cls[sor]] = scores
    cand_of_slot = np.argsort(np.argsort(slot_id, kind="stable"), kind="stable")
    return pred, dict(n=n, distinct=distinct, cand_of_rank=cand_of_slot[sor], box_of_rank=box_of_rank, cls_of_rank=slot_cls[sor])


TAIL_N = (1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 4097 + 1024)


def tail_ranks(n):
    return [r for r in (0, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, n - 1) if r < n]


def tail_scores(n, kind):
    """spread: 0.99 .. 0.01 geometrically, over ~850 histogram bins; onebin: distinct scores 0.5 + k * 2^-21, k <= n (below 0.5 + 2^-8: the upper 16
    bits of the word are equal, asserted below), so one bin holds them all and the radix refinement cuts it at 4096; ties: all equal — the order is the slot's"""
    r = np.arange(n, dtype=np.float64)
    if kind == "spread":
        s = (0.99 * (0.01 / 0.99) ** (r / max(n, 2))).astype(F)
    elif kind == "onebin":
        s = (0.5 + (n - r) * 2.0 ** -21).astype(F)
        assert len(set((s.view(np.uint32) >> 16).tolist())) == 1
    else:
        s = np.full(n, 0.5, F)
    if kind != "ties":
        assert (np.diff(s.astype(np.float64)) < 0).all()
    return s


def tail_case(n, kind, seed=0):
    return ranked_pred(tail_scores(n, kind), tail_ranks(n), 1000 + 7 * n + seed)


MAX_NMS = 5000
MAX_NMS_N = (4999, 5000, 5001, 9000)


def max_nms_case(n, multi):
    """a distinct box at ranks 0, max_nms - 1 and max_nms (where they exist); spread scores"""
    return ranked_pred(tail_scores(n, "spread"), (0, MAX_NMS - 1, MAX_NMS), 2000 + n, nc=3 if multi else 1, multi=multi)


MAX_DET = (1, 63, 64, 65, 299, 300, 301, 1024)


def disjoint_pred(n=1000, seed=5):
    """n boxes that never overlap, distinct scores dealt at random"""
    g = np.random.default_rng(seed)
    i = np.arange(n)
    pred = np.zeros((1, n, 6), F)
    pred[0, :, 0] = 50.0 + 100.0 * (i % 40)
    pred[0, :, 1] = 50.0 + 100.0 * (i // 40)
    pred[0, :, 2:4] = 40.0
    pred[0, :, 4] = 1.0
    pred[0, :, 5] = tail_scores(n, "spread")[g.permutation(n)]
    return pred


def threshold_pred(conf=0.25):
    """disjoint boxes around conf_thres: obj == conf and obj * cls == conf are no candidates, one ulp above is; returns (pred, accepted)"""
    c, up, dn = F(conf), np.nextafter(F(conf), F(1)), np.nextafter(F(conf), F(0))
    rows = [(c, 1.0, False), (up, 1.0, True), (dn, 1.0, False), (1.0, c, False), (1.0, up, True), (1.0, dn, False), (0.5, 0.5, False),
            (0.5, np.nextafter(F(0.5), F(1)), True), (up, up, False), (1.0, 1.0, True), (c, c, False), (0.9, 0.7, True)]
    pred = np.zeros((1, len(rows), 6), F)
    for i, (o, s, _) in enumerate(rows):
        pred[0, i] = (50.0 + 100.0 * i, 50.0, 40.0, 40.0, o, s)
    return pred, np.array([r[2] for r in rows])


def bin_edge_case(seed=77):
    """conf_thres = 0.  By rank: three scores above 1; 5100 of exactly 1.0 (one bin beyond the 4096 keys of a round: refined down to the
    slot); a spread of 900; 2^-17 exactly; and about 5400 distinct scores in (0, 2^-17) that reach into the subnormals (5600 drawn,
    duplicates dropped; the counts are returned) — histogram bin 0, refined.  Distinct boxes at the first and last rank of every group and
    around rank 4096 inside the two refined groups."""
    g = np.random.default_rng(seed)
    top = np.array([1e30, 3.0, 1.5], F)
    ones = np.ones(5100, F)
    mid = tail_scores(900, "spread")
    edge = np.array([2.0 ** -17], F)
    tiny = (2.0 ** -(17.0 + g.uniform(0.01, 131.0, 5600))).astype(F)
    tiny = np.unique(tiny)[::-1]
    assert tiny[0] < F(2.0 ** -17) and tiny[-1] > 0 and (tiny < F(2.0 ** -126)).sum() > 100
    scores = np.concatenate((top, ones, mid, edge, tiny))
    b1, b2, b3 = len(top), len(top) + len(ones), len(top) + len(ones) + len(mid)
    distinct = [0, 2, b1, b1 + 4095, b1 + 4096, b2 - 1, b2, b3 - 1, b3, b3 + 1, b3 + 4095, b3 + 4096, b3 + 4097, len(scores) - 1]
    return ranked_pred(scores, distinct, seed), dict(above_one=len(top), ones=len(ones), tiny=len(tiny), subnormal=int((tiny < F(2.0 ** -126)).sum()))


# ------------------------------------------------------------------------------------------------------------------------------------
# NMS (b): degenerate boxes, decided by the oracle
# ------------------------------------------------------------------------------------------------------------------------------------
def degenerate_pred(seed=3):
    """pairs (and a few triples) of boxes far from each other: zero width, zero area on both (0 / 0), negative w, w = inf alone and against
    another inf box (inf - inf), identical boxes, and 400 pairs with areas in the fp32 subnormal range (widths 1e-22 .. 1e-18)"""
    g = np.random.default_rng(seed)
    groups = [
        [(0, 0, 0.0, 40.0), (0, 0, 30.0, 40.0)],                        # zero width inside a box
        [(0, 0, 0.0, 0.0), (0, 0, 0.0, 0.0)],                           # union 0: 0 / 0
        [(0, 0, 0.0, 40.0), (0, 0, 0.0, 40.0)],
        [(0, 0, -30.0, 40.0), (0, 0, 30.0, 40.0)],                      # negative w: x1 > x2, negative area
        [(0, 0, -30.0, 40.0), (0, 0, -30.0, 40.0)],
        [(0, 0, -30.0, -40.0), (2, 1, 30.0, 40.0)],
        [(0, 0, 40.0, 40.0), (0, 0, 40.0, 40.0), (0, 0, 40.0, 40.0)],   # identical
        [(0, 0, 40.0, 40.0), (20, 0, 40.0, 40.0)],                      # IoU 1 / 3
        [(0, 0, 40.0, 40.0), (0, 0, 40.0, 20.0)],                       # IoU 0.5
    ]
    rows = []
    for k, grp in enumerate(groups):
        rows += [(dx + 200.0 * (k % 4), dy + 200.0 * (k // 4), w, h) for dx, dy, w, h in grp]
    n = len(rows)
    pred = np.zeros((1, n, 6), F)
    pred[0, :, :4] = np.asarray(rows, F)
    pred[0, :, 4] = 1.0
    pred[0, :, 5] = tail_scores(n, "spread")[g.permutation(n)]
    return pred


def subnormal_pred(seed=4, pairs=400):
    """(pairs, 2, 6): one pair per image, both boxes around the origin (a centre of 200 would swallow a width of 1e-20), widths and heights
    1e-22 .. 1e-18: areas, intersections and unions are fp32 subnormals or 0, and thr * union is below the normal range"""
    g = np.random.default_rng(seed)
    pred = np.zeros((pairs, 2, 6), F)
    wh = 10.0 ** g.uniform(-22, -18, (pairs, 2, 2))
    pred[:, :, 2:4] = wh
    pred[:, 1, 0:2] = g.uniform(-0.3, 0.3, (pairs, 2)) * wh[:, 0]
    pred[:, :, 4] = 1.0
    pred[:, 0, 5], pred[:, 1, 5] = 0.9, 0.8
    return pred


def inf_pred():
    """w = inf: alone among ordinary boxes, and two of them (union inf - inf = NaN: nobody suppresses anybody)"""
    pred = np.zeros((2, 6, 6), F)
    for b in range(2):
        for i in range(6):
            pred[b, i] = (100.0 + 300.0 * i, 100.0, 40.0, 40.0, 1.0, 0.9 - 0.1 * i)
        pred[b, 1, 2] = np.inf
        pred[b, 2, :2] = pred[b, 0, :2]                                 # a duplicate of box 0: suppressed
    pred[1, 4, 2] = np.inf
    return pred


# ------------------------------------------------------------------------------------------------------------------------------------
# the NMS cases, by name: builder() -> pred, and the keyword arguments of non_max_suppression
# ------------------------------------------------------------------------------------------------------------------------------------
_LADDERS = {}


def ladder(thr, nc=1, agnostic=False):
    key = (thr, nc, agnostic)
    if key not in _LADDERS:
        _LADDERS[key] = iou_ladder(thr, 11 + int(1000 * thr), nc, agnostic)
    return _LADDERS[key]


def nms_cases():
    cases = {}
    for thr in LADDER_THR:
        for arr in ("adjacent", "split"):
            for nc, ag in ((1, False), (3, False), (3, True)):
                name = f"ladder-{thr}-{arr}-nc{nc}" + ("-agnostic" if ag else "")
                cases[name] = (lambda thr=thr, arr=arr, nc=nc, ag=ag: ladder_pred(ladder(thr, nc, ag), arr),
                               dict(conf_thres=LADDER_CONF, iou_thres=thr, agnostic=ag, max_det=1024))
    for thr in (0.45, 0.0, 1.0):
        cases[f"degenerate-thr{thr}"] = (degenerate_pred, dict(conf_thres=0.005, iou_thres=thr))
        cases[f"subnormal-thr{thr}"] = (subnormal_pred, dict(conf_thres=0.25, iou_thres=thr))
        cases[f"disjoint-thr{thr}"] = (lambda: disjoint_pred(200), dict(conf_thres=0.005, iou_thres=thr))
    cases["inf-width"] = (inf_pred, dict(conf_thres=0.25, iou_thres=0.45))
    for kind in ("spread", "onebin", "ties"):
        for n in TAIL_N:
            cases[f"tail-{kind}-{n}"] = (lambda n=n, kind=kind: tail_case(n, kind)[0], dict(conf_thres=0.005, iou_thres=0.45))
    for multi in (False, True):
        for n in MAX_NMS_N:
            cases[f"max_nms-{'multi' if multi else 'single'}-{n}"] = (lambda n=n, multi=multi: max_nms_case(n, multi)[0],
                                                                      dict(conf_thres=0.005, iou_thres=0.45, multi_label=multi, max_nms=MAX_NMS))
    for md in MAX_DET:
        cases[f"max_det-{md}"] = (disjoint_pred, dict(conf_thres=0.005, iou_thres=0.45, max_det=md))
    cases["threshold"] = (lambda: threshold_pred()[0], dict(conf_thres=0.25, iou_thres=0.45))
    cases["bin-edges"] = (lambda: bin_edge_case()[0][0], dict(conf_thres=0.0, iou_thres=0.45))
    return cases


def ladder_decisions(lad, defect=None):
    """every point of a ladder decided pair by pair: the device's iou_gt (defect None) or a planted variant of it"""
    off = (lad["cls"] * (0.0 if lad["agnostic"] else 4096.0)).astype(F)
    A = (xywh2xyxy(lad["a"]) + off[:, None]).astype(F)
    B = (xywh2xyxy(lad["b"]) + off[:, None]).astype(F)
    inter, uni = pair_terms(A, B, box_area(A), box_area(B), fused=defect == "fused_union")
    return decide(inter, uni, lad["thr"], defect if defect in ("ge", "naive") else "device")


# ------------------------------------------------------------------------------------------------------------------------------------
# the decode cases shared by the host test and the device test
# ------------------------------------------------------------------------------------------------------------------------------------
LEVELS = ((8.0, ANCHORS3[0]), (13.0, ANCHORS3[1]), (33.0, ANCHORS3[2]))      # an even and two odd strides; the last holds 373 x 326
SWEEP_SHAPE = (2, 5, 7)                                                      # B, ny, nx of the launched level
NEIGHBOUR_SHAPES = ((3, 4), (2, 3))                                          # ny, nx of the two levels that are NOT launched
SENTINELS = (0x7FC0BEEF, 0xC29A8000)                                         # numerics.NAN_BITS[F32]; -77.25
SWEEP_NC = (1, 3, 9, 2)                                                      # no = 6, 8, 14 (per-pixel heads) and 7 (the general kernel)


def three_levels(pos, na, ny, nx):
    """rows of a z that holds three levels with the launched one ((ny, nx)) at position pos -> (rows_total, row_offset)"""
    dims = list(NEIGHBOUR_SHAPES)
    dims.insert(pos, (ny, nx))
    rows = [na * h * w for h, w in dims]
    return sum(rows), sum(rows[:pos])


def nan_map(B, ny, nx, na, no, seed=21):
    """ordinary logits with NaN at one element in eleven -> (p, mask (B, ny, nx, na * no))"""
    p = random_map(B, ny, nx, na, no, seed, scale=2.0, tails=False)
    m = (np.arange(p.size).reshape(p.shape) % 11) == 3
    p[m] = np.nan
    return p, m
