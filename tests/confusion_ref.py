"""Scalar restatement of ConfusionMatrix.process_batch (reference utils/metrics.py:121-159) with DEFINED IoU ties: the lowest label index
wins, then the lowest detection index (the reference's order comes from an unstable argsort).  fp32 box_iou in the operation order of
utils/general.py:455-477.  Pinned to the reference's recorded matrices (tests/golden/stats/) on inputs without IoU ties by
tests/test_val_stats_host.py; the yardstick of icaf_confusion_matrix."""
import numpy as np

f32 = np.float32


def box_iou(lab, det):
    """lab (4,), det (4,) xyxy fp32 -> fp32 IoU: inter / (area_lab + area_det - inter)"""
    area_l = f32(f32(lab[2] - lab[0]) * f32(lab[3] - lab[1]))
    area_d = f32(f32(det[2] - det[0]) * f32(det[3] - det[1]))
    iw = max(f32(min(lab[2], det[2]) - max(lab[0], det[0])), f32(0))
    ih = max(f32(min(lab[3], det[3]) - max(lab[1], det[1])), f32(0))
    inter = f32(iw * ih)
    with np.errstate(invalid="ignore", divide="ignore"):
        return f32(inter / f32(f32(area_l + area_d) - inter))


def process_batch(matrix, nc, detections, labels, conf=0.25, iou_thres=0.45):
    """matrix (nc + 1, nc + 1) is updated in place.  detections (N, 6) [x1, y1, x2, y2, conf, cls], labels (M, 5) [cls, x1, y1, x2, y2]."""
    det, lab = np.asarray(detections, f32).reshape(-1, 6), np.asarray(labels, f32).reshape(-1, 5)
    det = det[det[:, 4] > f32(conf)]
    D, L = len(det), len(lab)
    best_l, best_iou = np.full(D, -1), np.zeros(D, f32)
    for d in range(D):
        for j in range(L):
            iou = box_iou(lab[j, 1:], det[d, :4])
            if iou > f32(iou_thres) and (best_l[d] < 0 or iou > best_iou[d]):
                best_l[d], best_iou[d] = j, iou
    lab_det = np.full(L, -1)
    for j in range(L):
        for d in range(D):
            if best_l[d] == j and (lab_det[j] < 0 or best_iou[d] > best_iou[lab_det[j]]):
                lab_det[j] = d
    for j in range(L):
        gc = int(lab[j, 0])
        if lab_det[j] >= 0:
            matrix[int(det[lab_det[j], 5]), gc] += 1
        else:
            matrix[nc, gc] += 1
    if (lab_det >= 0).any():                              # the reference's `if n:`
        used = set(lab_det[lab_det >= 0].tolist())
        for d in range(D):
            if d not in used:
                matrix[int(det[d, 5]), nc] += 1


def process_images(matrix, nc, predn, det, count, labels, label_off, conf=0.25, iou_thres=0.45):
    """The batch form as test.py drives it: an image without detections or without labels contributes nothing (test.py:151-153, 198-206)."""
    for b in range(len(count)):
        n, l0, l1 = int(count[b]), int(label_off[b]), int(label_off[b + 1])
        if n <= 0 or l1 <= l0:
            continue
        rows = np.concatenate((np.asarray(predn[b, :n], f32), np.asarray(det[b, :n, 4:6], f32)), 1)
        process_batch(matrix, nc, rows, labels[l0:l1], conf, iou_thres)
