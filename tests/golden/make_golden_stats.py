"""Record the reference's validation statistics as fixtures:  python tests/golden/make_golden_stats.py /path/to/reference

Imports the reference's utils/metrics.py (modules only its plots and loaders need are stubbed; no bytecode is written beside it), runs its
`ap_per_class` and `ConfusionMatrix.process_batch` on the cases below and stores DATA only under tests/golden/stats/: the inputs and the
reference's outputs, one small .npz each.  The inputs are chosen so that the reference is well defined — distinct fp32 confidences, no two
candidate pairs of an image with equal IoU — and both conditions are asserted before anything is written (README_stats.md)."""
import os
import sys
import types

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


class _Dummy:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return None

    def __getattr__(self, k):
        return _Dummy()


def load_reference(root):
    for name in ("cv2", "seaborn", "thop", "torchvision", "torchvision.ops", "torchvision.transforms", "torchvision.utils", "torchvision.models",
                 "pandas", "matplotlib", "matplotlib.pyplot", "PIL", "PIL.Image", "PIL.ImageDraw", "PIL.ImageFont", "scipy", "scipy.signal"):
        try:
            __import__(name)
        except Exception:
            m = types.ModuleType(name)
            m.__getattr__ = lambda k: _Dummy()
            sys.modules[name] = m
    if not hasattr(np, "trapz"):
        np.trapz = np.trapezoid
    sys.path.insert(0, root)
    for k in [k for k in sys.modules if k == "utils" or k.startswith("utils.")]:
        del sys.modules[k]
    import utils.general                                   # noqa: F401  (first: it and utils.metrics import each other)
    import utils.metrics as metrics
    assert os.path.abspath(metrics.__file__).startswith(os.path.abspath(root))
    return metrics


def lattice_conf(g, n):
    """n DISTINCT fp32 confidences in (0, 1)"""
    conf = ((g.permutation(n) + 1) / (n + 1)).astype(np.float32)
    assert len(np.unique(conf)) == n
    return conf


def ap_cases():
    """name -> (tp (n, 10) bool, conf (n,) fp32, pred_cls (n,) fp32, target_cls (m,) fp32)"""
    g = np.random.default_rng(20)
    cases = {}

    def rand(n, nc, m, p_tp=0.5):
        tp = g.random((n, 10)) < (p_tp * np.linspace(1.0, 0.3, 10))[None, :]
        tp = np.logical_and.accumulate(tp, 1)                          # a TP at a threshold is one at every lower threshold
        return tp, lattice_conf(g, n), g.integers(0, nc, n).astype(np.float32), g.integers(0, nc, m).astype(np.float32)
    cases["nc1_n300"] = rand(300, 1, 120)
    cases["nc3_n900"] = rand(900, 3, 250)
    cases["nc1_n5000"] = rand(5000, 1, 700, 0.3)
    tp, conf, pc, tc = rand(400, 3, 200)
    pc[pc == 1] = 0.0                                                     # class 1: labels, no predictions
    cases["labels_no_predictions"] = (tp, conf, pc, tc)
    tp, conf, pc, tc = rand(400, 3, 200)
    tc[tc == 2] = 0.0                                                     # class 2: predictions, no labels
    cases["predictions_no_labels"] = (tp, conf, pc, tc)
    tp, conf, pc, tc = rand(400, 3, 200)
    tp[pc == 0] = True                                                    # class 0 all TP, class 1 all FP
    tp[pc == 1] = False
    cases["all_tp_all_fp"] = (tp, conf, pc, tc)
    tp, conf, pc, tc = rand(400, 3, 200)
    keep = tc != 2                                                        # the LAST class (3) has 2 labels and no prediction: TP / FN use ITS n_l
    cases["last_class_gap"] = (tp, conf, pc, np.concatenate((tc[keep], [3.0, 3.0])).astype(np.float32))
    cases["single_row_tp"] = (np.ones((1, 10), bool), np.array([0.75], np.float32), np.zeros(1, np.float32), np.zeros(3, np.float32))
    cases["single_row_fp"] = (np.zeros((1, 10), bool), np.array([0.25], np.float32), np.zeros(1, np.float32), np.zeros(2, np.float32))
    return cases


def cm_images(seed, count, nc=3):
    """Random images in the mould of the issue's CPU check: 1-11 labels, 1-39 detections jittered around them."""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        L, D = int(g.integers(1, 12)), int(g.integers(1, 40))
        lc, lw = g.uniform(50, 450, (L, 2)), g.uniform(20, 120, (L, 2))
        lab = np.concatenate([g.integers(0, nc, (L, 1)), lc - lw / 2, lc + lw / 2], 1).astype(np.float32)
        box = lab[g.integers(0, L, D), 1:] + g.normal(0, 15, (D, 4))
        det = np.concatenate([box, g.uniform(0, 1, (D, 1)), g.integers(0, nc, (D, 1))], 1).astype(np.float32)
        out.append((det, lab))
    return out


def cm_cases():
    """name -> (nc, [(det (N, 6), labels (M, 5))])"""
    cases = {"random_nc3": (3, cm_images(31, 24, 3)), "random_nc1": (1, cm_images(32, 12, 1))}
    lab = np.array([[0, 10, 10, 60, 90], [1, 200, 50, 260, 150]], np.float32)
    far = np.array([[300, 300, 340, 380, 0.9, 0], [400, 20, 430, 70, 0.8, 1]], np.float32)
    low = np.array([[10, 10, 60, 90, 0.2, 0]], np.float32)                                    # a perfect box below conf
    hit = np.array([[11, 12, 61, 91, 0.9, 1], [300, 300, 340, 380, 0.9, 0]], np.float32)     # one match (wrong class) + one unmatched
    cases["no_match"] = (3, [(far, lab)])                   # the `if n:` quirk: unmatched detections are NOT counted
    cases["below_conf"] = (3, [(low, lab)])
    cases["match_and_unmatched"] = (3, [(hit, lab)])
    cases["no_labels"] = (3, [(far, np.zeros((0, 5), np.float32))])
    cases["no_detections"] = (3, [(np.zeros((0, 6), np.float32), lab)])
    return cases


def assert_distinct_ious(det, lab, conf=0.25, thr=0.45):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import confusion_ref
    kept = det[det[:, 4] > np.float32(conf)]
    ious = [confusion_ref.box_iou(l[1:], d[:4]) for l in lab for d in kept]
    cand = [v for v in ious if v > np.float32(thr)]
    assert len(set(cand)) == len(cand), "two candidate pairs of an image share their IoU"


def main(root):
    ref = load_reference(root)
    outdir = os.path.join(HERE, "stats")
    os.makedirs(outdir, exist_ok=True)
    for name, (tp, conf, pc, tc) in ap_cases().items():
        assert len(np.unique(conf)) == len(conf)
        tpn, fpn, fnn, p, r, ap, f1, classes = ref.ap_per_class(tp.copy(), conf.copy(), pc.copy(), tc.copy())
        np.savez_compressed(os.path.join(outdir, f"ap_{name}.npz"), tp_in=tp, conf=conf, pred_cls=pc, target_cls=tc, tp=tpn, fp=fpn, fn=fnn, p=p, r=r,
                            ap=ap, f1=f1, classes=classes)
        print(f"ap_{name}: n {len(conf)} classes {classes.tolist()} mAP50 {ap[:, 0].mean():.4f}")
    for name, (nc, images) in cm_cases().items():
        cm = ref.ConfusionMatrix(nc)
        blob = {"nc": np.int64(nc), "images": np.int64(len(images))}
        for k, (det, lab) in enumerate(images):
            assert_distinct_ious(det, lab)
            before = cm.matrix.copy()
            if name not in ("no_labels", "no_detections"):                 # test.py never calls process_batch for these (:151-153, 198-206)
                cm.process_batch(torch.from_numpy(det.copy()), torch.from_numpy(lab.copy()))
            blob[f"det{k}"], blob[f"lab{k}"], blob[f"delta{k}"] = det, lab, (cm.matrix - before).astype(np.int64)
        blob["matrix"] = cm.matrix.astype(np.int64)
        np.savez_compressed(os.path.join(outdir, f"cm_{name}.npz"), **blob)
        print(f"cm_{name}: {len(images)} images, matrix sum {int(cm.matrix.sum())}")


if __name__ == "__main__":
    main(sys.argv[1])
