"""Detection metrics on the host (numpy), same entry points as the reference's utils/metrics.py."""
import numpy as np


def fitness(x):
    """Weighted combination used for model selection: only mAP@0.5 counts (reference utils/metrics.py:12-15)."""
    w = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    return (x[:, :8] * w).sum(1)


def compute_ap(recall, precision):
    """101-point interpolated AP of one precision/recall curve (reference utils/metrics.py:85-110)."""
    mrec = np.concatenate(([0.0], recall, [recall[-1] + 0.01]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    ap = np.trapezoid(np.interp(x, mrec, mpre), x) if hasattr(np, "trapezoid") else np.trapz(np.interp(x, mrec, mpre), x)
    return ap, mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, save_dir=".", names=()):
    """Per-class AP at every IoU threshold plus P/R/F1 at the best-F1 confidence (reference utils/metrics.py:18-82).
    Returns (tp, fp, fn, p, r, ap, f1, classes) like the reference; plotting is not provided."""
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes = np.unique(target_cls)
    nc = unique_classes.shape[0]
    px = np.linspace(0, 1, 1000)
    ap, p, r = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    n_l = 0
    for ci, c in enumerate(unique_classes):
        sel = pred_cls == c
        n_l = (target_cls == c).sum()
        n_p = sel.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[sel]).cumsum(0)
        tpc = tp[sel].cumsum(0)
        recall = tpc / (n_l + 1e-16)
        r[ci] = np.interp(-px, -conf[sel], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p[ci] = np.interp(-px, -conf[sel], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j], _, _ = compute_ap(recall[:, j], precision[:, j])
    f1 = 2 * p * r / (p + r + 1e-16)
    i = f1.mean(0).argmax()
    tpn = (r * n_l).round()
    fn = n_l - tpn
    fp = (tpn / (p + 1e-16) - tpn).round()
    return tpn[:, i], fp[:, i], fn[:, i], p[:, i], r[:, i], ap, f1[:, i], unique_classes.astype("int32")


def match_predictions(det, labels, iouv):
    """TP flags of one image's detections at every IoU threshold (reference test.py:196-230).

    det: (n, 6) [x1, y1, x2, y2, conf, cls]; labels: (m, 5) [cls, x1, y1, x2, y2] in the same pixel space; iouv: (T,).
    Per class each prediction is paired with its best-IoU target; predictions are visited in index order and a target
    is claimed by the first prediction above iouv[0] that reaches it.  Returns bool (n, T)."""
    det, labels, iouv = np.asarray(det, np.float32), np.asarray(labels, np.float32), np.asarray(iouv, np.float32)
    correct = np.zeros((det.shape[0], iouv.shape[0]), bool)
    if not len(det) or not len(labels):
        return correct
    claimed_total = 0
    for cls in np.unique(labels[:, 0]):
        ti = np.flatnonzero(labels[:, 0] == cls)
        pi = np.flatnonzero(det[:, 5] == cls)
        if not len(pi):
            continue
        a, b = det[pi, :4], labels[ti, 1:5]
        inter = (np.minimum(a[:, None, 2:], b[None, :, 2:]) - np.maximum(a[:, None, :2], b[None, :, :2])).clip(0).prod(2)
        area_a, area_b = (a[:, 2:] - a[:, :2]).prod(1), (b[:, 2:] - b[:, :2]).prod(1)
        iou = inter / (area_a[:, None] + area_b[None, :] - inter)
        best, arg = iou.max(1), iou.argmax(1)
        claimed = set()
        for j in np.flatnonzero(best > iouv[0]):
            t = int(ti[arg[j]])
            if t in claimed:
                continue
            claimed.add(t)
            claimed_total += 1
            correct[pi[j]] = best[j] > iouv
            if claimed_total == len(labels):
                break
    return correct


def ap_per_class_device(tp, conf, pred_cls, target_cls, plot=False, save_dir=".", names=()):
    """ap_per_class on the device (icaf_ap_per_class; reference utils/metrics.py:18-82): the reference's signature and return tuple, device
    tensors or numpy in, numpy out.  The order is DEFINED where the reference's np.argsort(-conf) is not: class ascending, confidence
    descending, equal confidences in arrival order — with distinct confidences the two agree.  tp (n, T) bool, conf (n,), pred_cls (n,),
    target_cls (m,).  Classes must be integers in [0, 256), confidences finite and not negative (checked here, on the device)."""
    import torch
    from .. import ops
    dev = next((a.device for a in (tp, conf, pred_cls) if isinstance(a, torch.Tensor) and a.is_cuda), torch.device("cuda"))
    tp, conf, pred_cls = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)) for a in (tp, conf, pred_cls))
    tp, conf, pred_cls = tp.to(dev), conf.to(dev, torch.float32).contiguous(), pred_cls.to(dev)
    n, T = int(tp.shape[0]), int(tp.shape[1])
    if n and (not bool(torch.isfinite(conf).all()) or float(conf.min()) < 0 or float(pred_cls.min()) < 0 or float(pred_cls.max()) > 255):
        raise ValueError("ap_per_class_device: confidences must be finite and >= 0, classes in [0, 256)")
    weights = torch.bitwise_left_shift(torch.ones((), dtype=torch.int32, device=dev), torch.arange(T, dtype=torch.int32, device=dev))
    mask = ((tp != 0).to(torch.int32) * weights[None, :]).sum(1).to(torch.int16).contiguous() if T <= 16 else torch.zeros((n,), dtype=torch.int16, device=dev)
    target_cls = target_cls.cpu().numpy() if isinstance(target_cls, torch.Tensor) else np.asarray(target_cls)
    unique_classes, n_l = np.unique(target_cls, return_counts=True)
    if not len(unique_classes):                                   # the reference's loop never runs; nothing to launch
        z = np.zeros(0)
        return z, z, z, z, z, np.zeros((0, T)), z, unique_classes.astype("int32")
    out = ops.ap_per_class_device((mask, conf, pred_cls.to(torch.int32).contiguous(), n), unique_classes, n_l, T=T)
    i = out["best"]
    return out["tp"], out["fp"], out["fn"], out["p"][:, i], out["r"][:, i], out["ap"], out["f1"][:, i], unique_classes.astype("int32")


class ConfusionMatrix:
    """The reference's ConfusionMatrix (utils/metrics.py:113-186) on the device: rows = predicted class, columns = true class, index nc =
    background.  The counts live in an int32 matrix on the device (icaf_confusion_matrix, integer atomics: deterministic); `.matrix` is the
    reference's float64 numpy array, filled when read.  IoU ties (the reference leaves them to an unstable argsort): the lowest label index
    wins, then the lowest detection index."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45, device="cuda"):
        import torch
        self.nc, self.conf, self.iou_thres = int(nc), conf, iou_thres
        self._dev = torch.zeros((self.nc + 1, self.nc + 1), dtype=torch.int32, device=device)

    @property
    def matrix(self):
        return self._dev.cpu().numpy().astype(np.float64)

    def process_images(self, predn, det, count, labels, label_off):
        """A batch in one launch: predn (B, max_det, 4) native-space boxes, det (B, max_det, 6), count (B,) int32, labels (L, 5) fp32
        [cls, x1, y1, x2, y2] sorted by image, label_off (B + 1,) int32 — what test.py hands to ops.match_predictions."""
        from .. import ops
        ops.confusion_matrix(predn, det, count, labels, label_off, self._dev, self.conf, self.iou_thres)(ops.current_stream_ptr())

    def process_batch(self, detections, labels):
        """One image, the reference's signature: detections (N, 6) [x1, y1, x2, y2, conf, cls], labels (M, 5) [cls, x1, y1, x2, y2]."""
        import torch
        dev = self._dev.device
        det = torch.as_tensor(detections, dtype=torch.float32).to(dev).reshape(-1, 6)
        lab = torch.as_tensor(labels, dtype=torch.float32).to(dev).reshape(-1, 5).contiguous()
        n = det.shape[0]
        if lab.shape[0] == 0:                                    # no label: nothing is counted (:149, :156)
            return
        if n == 0:                                               # called without detections the reference counts every label as missed
            det, n = torch.tensor([[0.0, 0.0, 0.0, 0.0, float("-inf"), 0.0]], device=dev), 1      # (:149-154): one row that is never kept
        det = det[None].contiguous()
        self.process_images(det[..., :4].contiguous(), det, torch.tensor([n], dtype=torch.int32, device=dev), lab,
                            torch.tensor([0, lab.shape[0]], dtype=torch.int32, device=dev))

    def print(self):
        m = self.matrix
        for i in range(self.nc + 1):
            print(" ".join(map(str, m[i])))

    def plot(self, save_dir="", names=()):
        """Best effort, like the reference's (:164-181, which needs seaborn and swallows every error): confusion_matrix.txt — the counts, then
        every column as shares of its true class — always; confusion_matrix.png beside it when matplotlib is importable."""
        import os
        m = self.matrix
        share = m / np.maximum(m.sum(0, keepdims=True), 1.0)
        ticks = list(names) + ["background"] if len(names) == self.nc else [str(i) for i in range(self.nc)] + ["background"]
        try:
            os.makedirs(str(save_dir) or ".", exist_ok=True)
            with open(os.path.join(str(save_dir), "confusion_matrix.txt"), "w") as f:
                f.write("# rows: predicted class, columns: true class, last of each: background\n# classes: " + ", ".join(ticks) + "\n# counts\n")
                f.writelines(" ".join("%d" % v for v in row) + "\n" for row in m)
                f.write("# share of the true class (column sums to 1)\n")
                f.writelines(" ".join("%.4f" % v for v in row) + "\n" for row in share)
        except Exception:
            pass
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
            side = min(max(4.0, 0.5 * (self.nc + 1) + 2.0), 16.0)
            fig, ax = plt.subplots(figsize=(side + 1.0, side))
            fig.colorbar(ax.imshow(share, vmin=0.0, vmax=1.0, cmap="Blues"), ax=ax)
            if self.nc < 30:
                ax.set_xticks(range(self.nc + 1), ticks, rotation=90)
                ax.set_yticks(range(self.nc + 1), ticks)
                for (y, x), v in np.ndenumerate(share):
                    if v >= 0.005:
                        ax.text(x, y, "%.2f" % v, ha="center", va="center", fontsize=7, color="white" if v > 0.5 else "black")
            ax.set_xlabel("true class")
            ax.set_ylabel("predicted class")
            fig.tight_layout()
            fig.savefig(os.path.join(str(save_dir), "confusion_matrix.png"), dpi=150)
            plt.close(fig)
        except Exception:
            pass
