#!/usr/bin/env python3
"""Validation loop (mAP@0.5, mAP@0.5:0.95) of the two-stream detector on MI355X — the reference's test.py:23-330 reduced
to its metric path: paired RGB/IR loader -> forward -> NMS(multi_label) -> per-image TP matching at 10 IoU thresholds ->
ap_per_class.  `test(...)` keeps the reference's return value ((mp, mr, map50, map, lbox, lobj, lcls), maps, times); the three losses are 0
unless a loss is asked for (ValLoss).

    python test.py --data data/multispectral/kaist.yaml --weights best.pt --batch-size 32 --img-size 640
    python test.py --data ... --cfg models/transformer/yolov5s_Transfusion_kaist.yaml      (synthetic weights: plumbing)

Protocol as the reference's: rectangular batches with pad 0.5 (test.py:100 — KAIST's 512x640 frames become 544x672
batches), conf 0.001 / IoU 0.5 multi-label NMS, boxes mapped back to native image space before matching.  Every distinct
batch shape compiles its own execution plan (hipGraph); Model keeps them in a byte-capped LRU (Model.plan_cache_bytes).
`--task speed` runs at conf 0.25 / IoU 0.45 as the reference does and saves nothing.

test() is a set-up, one loop — forward, loss, suppress, labels, match, record, consumers — and the finish.  Each step of the loop is a
function below (to_device / forward, suppress, native_labels, match); what the matching leaves goes into one ValBatch, and every output of
the pass is a consumer of those records with `add(batch)` per batch and `finish()` after the loop, built only when its flag asks for it:
MissRate, Confusion, HostStats or DeviceStats, ResultFiles (they see a batch in this order) and ValLoss, which is fed the raw maps before
the labels go to pixels.  Each one's docstring describes its flag.  Without a flag the loop runs the code it always ran.

Not carried over (all outside the metric): the PR / F1 / P / R curve images and `plot_images` / wandb / `--task study` / the pycocotools
call / MR curves and plots; `--augment` raises (the help text says test-time augmentation is not built; Model.forward(augment=True) is by
now — test() still refuses it)."""
import argparse
import collections
import functools
import os

import numpy as np
import torch
import yaml

from icafusion_amd.models.experimental import load_detector
from icafusion_amd.utils.datasets import create_dataloader_rgb_ir
from icafusion_amd import ops
from icafusion_amd.utils.general import check_img_size, increment_path, nms_device, scale_coords, xywh2xyxy
from icafusion_amd.utils import missrate
from icafusion_amd.utils.confluence import confluence_device
from icafusion_amd.utils.loss import ComputeLoss, scale_hyp
from icafusion_amd.utils.results import ResultWriter, frame_index, label_listing
from icafusion_amd.utils.metrics import ConfusionMatrix, ap_per_class
from icafusion_amd.utils.torch_utils import select_device, time_synchronized

MATCH_MAX_DET = 1024                                             # detections per image icaf_match_predictions takes (valstats.hip)
IOUV = np.linspace(0.5, 0.95, 10)                                # the IoU thresholds of mAP@0.5:0.95


# ---- the statistics of a pass -> numbers and the result table -----------------------------------------------------------------------------------
def _numbers(nt, tp=None, fp=None, fn=None, p=None, r=None, f1=None, ap=None, ap_class=None):
    """-> tp, fp, fn, p, r, f1, ap, ap_class, nt, (mp, mr, map50, map75, map): what summarize() formats.  Without the curves — no
    detection, or no TP at all — every metric is 0."""
    if ap is None:
        return np.zeros(1), np.zeros(1), np.zeros(1), np.zeros(0), np.zeros(0), np.zeros(1), np.zeros((0, 10)), np.zeros(0, int), nt, (0.0,) * 5
    return tp, fp, fn, p, r, f1, ap, ap_class, nt, (p.mean(), r.mean(), ap[:, 0].mean(), ap[:, 5].mean(), ap.mean())


def host_numbers(stats, nc):
    """The numbers of the host lists: numpy ap_per_class (utils/metrics.py) on the concatenated rows."""
    if not stats:
        return _numbers(np.zeros(nc, int))
    cat = [np.concatenate([np.asarray(s[k]) for s in stats], 0) for k in range(4)]
    nt = np.bincount(cat[3].astype(np.int64), minlength=nc)
    if not (len(cat[0]) and cat[0].any()):
        return _numbers(nt)
    tp, fp, fn, p, r, ap, f1, ap_class = ap_per_class(cat[0], cat[1], cat[2], cat[3])
    return _numbers(nt, tp, fp, fn, p, r, f1, ap, ap_class)


def store_numbers(tcls_all, store, nc):
    """The numbers of an ops.StatsStore: icaf_ap_per_class on the device; "no TP at all" reads the store's any_tp flag."""
    tcls = np.concatenate([np.asarray(t, np.float64) for t in tcls_all]) if tcls_all else np.zeros(0)
    nt = np.bincount(tcls.astype(np.int64), minlength=nc)
    if not (store.rows() and store.any_tp()):
        return _numbers(nt)
    ap_class, n_l = np.unique(tcls, return_counts=True)
    res = ops.ap_per_class_device(store, ap_class, n_l)
    i = res["best"]
    return _numbers(nt, res["tp"], res["fp"], res["fn"], res["p"][:, i], res["r"][:, i], res["f1"][:, i], res["ap"], ap_class.astype("int32"))


def summarize(stats, nc, names, seen, verbose=False, store=None):
    """Statistics -> (mp, mr, map50, map, maps) + the reference's result table (test.py:287-313): for one class the columns are
    TP / FP / FN / F1 / P / R / mAP@.5 / mAP@.5:.95, otherwise P / R / mAP@.5 / mAP@.75 / mAP@.5:.95 with one row per class when
    `verbose`.  stats: list of (correct (n, 10) bool, conf (n,), pcls (n,), tcls list) per image — or, with `store` (an ops.StatsStore, the
    `device_stats` path), the list of the images' label classes."""
    tp, fp, fn, p, r, f1, ap, ap_class, nt, (mp, mr, map50, map75, map_) = (host_numbers(stats, nc) if store is None else
                                                                            store_numbers(stats, store, nc))
    lines = []
    if nc == 1:
        lines.append(("%20s" + "%12s" * 10) % ("Class", "Images", "Labels", "TP", "FP", "FN", "F1", "P", "R", "mAP@.5", "mAP@.5:.95"))
        lines.append(("%20s" + "%12i" * 2 + "%12.4g" * 8) % ("all", seen, nt.sum(), np.sum(tp), np.sum(fp), np.sum(fn), np.mean(f1), mp, mr,
                                                           map50, map_))
    else:
        pf = "%20s" + "%12i" * 2 + "%12.3g" * 5
        lines.append(("%20s" + "%12s" * 7) % ("Class", "Images", "Labels", "P", "R", "mAP@.5", "mAP@.75", "mAP@.5:.95"))
        lines.append(pf % ("all", seen, nt.sum(), mp, mr, map50, map75, map_))
        if verbose:
            for i, c in enumerate(ap_class):
                lines.append(pf % (names[c], seen, nt[c], p[i], r[i], ap[i, 0], ap[i, 5], ap[i].mean()))
    maps = np.zeros(nc) + map_
    for i, c in enumerate(ap_class):
        maps[c] = ap[i].mean()
    return (mp, mr, map50, map_), maps, lines


# ---- one batch after the matching, and the consumers of a pass ------------------------------------------------------------------------------------
class ValBatch:
    """What the matching step leaves of one batch, built once and read by every consumer: paths, shapes, nb; on the device det (nb, max_det, 6),
    count (nb,), predn (the native-space boxes; None when no consumer reads them), correct (nb, max_det, 10), lab_dev (native-space label
    rows) and off_dev (their offsets per image); tcls_all, the label classes per image, on the host.  The host copies are taken on first
    use and kept, so each block is read back at most once per batch however many consumers ask — and not at all when none does."""

    def __init__(self, paths, shapes, nb, det, count, predn, correct, lab_dev, off_dev, tcls_all):
        self.paths, self.shapes, self.nb, self.tcls_all = paths, shapes, nb, tcls_all
        self.det, self.count, self.predn, self.correct, self.lab_dev, self.off_dev = det, count, predn, correct, lab_dev, off_dev

    @functools.cached_property
    def count_host(self):
        return self.count.cpu().numpy()

    @functools.cached_property
    def conf_cls_host(self):
        return self.det[..., 4:6].cpu().numpy()

    @functools.cached_property
    def predn_host(self):
        return self.predn.cpu().numpy()

    @functools.cached_property
    def correct_host(self):
        return self.correct.cpu().numpy().astype(bool)


class HostStats:
    """The default statistics: flags / conf / cls of every image come back and join the list summarize() hands to numpy's ap_per_class
    (reference test.py:144-230).  `out` (test(stats_out=[...])) receives the list."""
    store = None

    def __init__(self, out):
        self.rows, self.out = [], out

    def match_options(self, tcls_all):
        return {}

    def add(self, b):
        correct, cc, count = b.correct_host, b.conf_cls_host, b.count_host
        for si, tcls in enumerate(b.tcls_all):
            n = int(count[si])
            if n:
                self.rows.append((correct[si, :n] if tcls else np.zeros((n, 10), bool), cc[si, :n, 0], cc[si, :n, 1], tcls))
            elif tcls:
                self.rows.append((np.zeros((0, 10), bool), np.zeros(0), np.zeros(0), tcls))

    def finish(self):
        if isinstance(self.out, list):
            self.out.extend(self.rows)


class DeviceStats:
    """`--device-stats` keeps the statistics of the pass on the device: every batch is appended to an ops.StatsStore in the host loop's
    order, nothing is read back per batch (result files excepted), the four synchronisations per batch become event pairs (EventStopwatch),
    and ap_per_class runs as kernels with a DEFINED order at equal confidences (arrival order; the host's np.argsort leaves it to the numpy
    build).  `rows` holds the label classes per image; `out` (test(stats_out=[...])) receives the store."""

    def __init__(self, dataloader, dev, out):
        self.rows, self.store, self.dataloader, self.dev, self.out = [], None, dataloader, dev, out

    def match_options(self, tcls_all):
        return {"max_labels": max(len(t) for t in tcls_all)}             # spares the matching its label_off read-back

    def add(self, b):
        if self.store is None:                                           # images x max_det rows: an upper bound of the cursor, it cannot overflow
            self.store = ops.StatsStore(len(self.dataloader.dataset) * b.det.shape[1], len(IOUV), self.dev)
        self.store.stage(b.correct, b.det, b.count)
        self.rows += b.tcls_all

    def finish(self):
        if isinstance(self.out, list):
            self.out.append(self.store)


class ResultFiles:
    """`--save-txt` / `--save-conf` / `--save-json` leave the reference's result files (per-image `frame,x,y,w,h[,conf]` lines + `result.txt`,
    the input of the KAIST miss-rate evaluator; `<weights>_predictions.json`) under `--project/--name` (icafusion_amd/utils/results.py).
    They are written on the host: count, conf / cls and the native-space boxes of every batch come back for them."""

    def __init__(self, dataset, save_dir, save_txt, save_conf, save_json, weights):
        listing = label_listing(os.path.dirname(dataset.label_files[0])) if save_txt else None
        self.writer = ResultWriter(save_dir if save_dir is not None else increment_path("runs/test/exp"), save_txt=save_txt, save_conf=save_conf,
                                   save_json=save_json, label_names=listing, weights=weights)

    def add(self, b):
        count, cc, predn = b.count_host, b.conf_cls_host, b.predn_host
        for si in range(b.nb):
            n = int(count[si])
            if n:
                self.writer.add(b.paths[si], predn[si, :n], cc[si, :n, 0], cc[si, :n, 1])

    def finish(self):
        for f in self.writer.close():
            if f is not None:
                print(f"saved {f}")


class Confusion:
    """`--plots` builds the reference's ConfusionMatrix (test.py:103,205-206,320-321; conf 0.25 / IoU 0.45) on the device, every image of a
    batch in one launch, prints it and saves confusion_matrix.txt (and confusion_matrix.png when matplotlib is there)."""

    def __init__(self, nc, dev, names, save_dir):
        self.matrix, self.names, self.save_dir = ConfusionMatrix(nc, device=dev), names, save_dir

    def add(self, b):
        self.matrix.process_images(b.predn, b.det, b.count, b.lab_dev, b.off_dev)

    def finish(self):
        self.matrix.print()
        plot_dir = str(self.save_dir) if self.save_dir is not None else str(increment_path("runs/test/exp"))
        os.makedirs(plot_dir, exist_ok=True)
        self.matrix.plot(save_dir=plot_dir, names=list(self.names))


class MissRate:
    """KAIST log-average miss rate of one validation pass (`miss_rate=` / `--miss-rate ANNOTATIONS`; the evaluator of the reference's
    `evaluation_script/`): every batch's native-space boxes are staged on the device into the store the matching kernel reads
    (icaf_missrate_stage, at the image's position in the sorted label directory: the `frame - 1` of result.txt), one icaf_missrate_match
    launch follows the loop, and utils.missrate.summarize runs the FPPI sweep in numpy.  test() returns the dict as a fourth element;
    `--task speed` ignores the flag."""

    def __init__(self, ann_path, dataset, dev):
        self.table = missrate.load_annotations(ann_path)
        self.listing = label_listing(os.path.dirname(dataset.label_files[0]))
        n_img, n_ann = len(dataset.label_files), len(self.table["image_id"])
        if n_img != n_ann or len(self.listing) != n_ann:
            raise ValueError(f"{ann_path} describes {n_ann} images, the data set holds {n_img} ({len(self.listing)} label files)")
        stems = [os.path.splitext(n)[0].replace("_", "/") for n in self.listing]
        if set(stems) <= set(self.table["im_name"]) and stems != list(self.table["im_name"]):
            bad = next(i for i, (a, b) in enumerate(zip(stems, self.table["im_name"])) if a != b)
            raise ValueError(f"frame {bad + 1} is {stems[bad]} in the label directory and {self.table['im_name'][bad]} in {ann_path}")
        self.dev, self.tab, self.dt, self.count = dev, ops.missrate_table(self.table, dev), None, None

    def add(self, b):
        if self.dt is None:                                                     # cap = NMS's max_det
            self.dt = torch.zeros((self.tab.images, b.det.shape[1], 5), dtype=torch.float64, device=self.dev)
            self.count = torch.zeros((self.tab.images,), dtype=torch.int32, device=self.dev)
        index = [frame_index(self.listing, os.path.splitext(os.path.basename(p))[0]) for p in b.paths]
        ops.missrate_stage(b.predn, b.det, b.count, index, torch.tensor(index, dtype=torch.int32, device=self.dev), self.dt,
                           self.count)(ops.current_stream_ptr())

    def finish(self):
        if self.dt is None:
            raise ValueError("no batch was staged")
        outs = ops.missrate_outputs(self.tab, self.dt.shape[1], self.dev)
        ops.missrate_match(self.tab, self.dt, self.count, *outs)(ops.current_stream_ptr())
        order, dt_gt, dt_ignore, gt_ignore = (o.cpu().numpy() for o in outs)
        dt, count = self.dt.cpu().numpy(), self.count.cpu().numpy()
        res = missrate.summarize(self.table, count, missrate.sorted_scores(dt, order, count), dt_gt, dt_ignore, gt_ignore[:self.tab.labels])
        print("\n".join(missrate.format_lines(res)))
        return res


class ValLoss:
    """`--hyp PATH` (or `test(compute_loss=...)`, as the reference's train.py:257,393 calls it) adds the validation loss — the forward value
    of the reference's ComputeLoss on the raw Detect maps of every batch (utils/loss.py:325-463; icaf_loss, no gradients), averaged over the
    batches as test.py:132-133,364-367 do, with the hyp gains scaled as train.py:238-241 scales them (loss_from_hyp) — fills the three
    trailing values and prints one `Loss:` line; there is no default hyp file, and without the flag nothing changes.  It is fed the raw
    maps and the unscaled targets, so it is the one consumer with a call site of its own."""

    def __init__(self, compute_loss, dev, batches):
        self.compute_loss, self.dev, self.batches = compute_loss, dev, batches
        self.sum = torch.zeros(3, device=dev)                            # box, obj, cls: summed on the device, read once after the loop

    def add(self, maps, targets):
        self.sum += self.compute_loss(maps, targets.to(self.dev))[1][:3]

    def finish(self):
        lbox, lobj, lcls = (self.sum.cpu() / self.batches).tolist()      # test.py:364-367
        print("Loss: %.5g box, %.5g obj, %.5g cls (mean of %d batches)" % (lbox, lobj, lcls, self.batches))
        return lbox, lobj, lcls


# ---- timing ------------------------------------------------------------------------------------------------------------------------------------
class Stopwatch:
    """Synchronised host time: start() and stop(bucket) each synchronise the device and read the host clock; totals() -> seconds per bucket."""

    def __init__(self):
        self.laps = []

    def mark(self):
        return time_synchronized()

    def seconds(self, a, b):
        return b - a

    def start(self):
        self.t0 = self.mark()

    def stop(self, bucket):
        self.laps.append((bucket, self.t0, self.mark()))

    def totals(self):
        out = collections.defaultdict(float)
        for bucket, a, b in self.laps:
            out[bucket] += self.seconds(a, b)
        return out


class EventStopwatch(Stopwatch):
    """The same laps as events on the stream: nothing synchronises during the pass, totals() reads the pairs once it is over."""

    def mark(self):
        e = ops.Event()
        e.record(ops.current_stream_ptr())
        return e

    def seconds(self, a, b):
        return a.elapsed_ms(b) / 1e3


# ---- the steps of the loop body -------------------------------------------------------------------------------------------------------------------
def to_device(img, dev, native):
    """One loader item on the device -> (what forward() takes, images in the batch, (height, width) of the network's input).  `native`
    (`--device-letterbox`): the frames go up as decoded, as lists of uint8 BGR images."""
    if native:
        rgb, ir, (height, width) = img
        return ([f.to(dev, non_blocking=True) for f in rgb], [f.to(dev, non_blocking=True) for f in ir]), len(rgb), (height, width)
    img = img.to(dev, non_blocking=True)                         # uint8 (B, 6, H, W): cat(rgb, ir), test.py:116-123
    return img, img.shape[0], (img.shape[2], img.shape[3])


def forward(model, x, net_hw, imgsz):
    """-> the model's outputs ([0] predictions, [2] raw Detect maps).  Native frames (`--device-letterbox`): the loader's longest-side resize
    (pixel-area average when shrinking) and the padding run on the device (Model.forward_frames(val_size=...))."""
    if isinstance(x, tuple):
        return model.forward_frames(x[0], x[1], img_size=net_hw, val_size=imgsz)[0]
    return model.forward_u8(x)


def suppress(out, targets, nb, paths, conf_thres, iou_thres, agnostic=False, confluence=None, save_hybrid=False, merge_nms=False):
    """Predictions -> det (nb, max_det, 6), count (nb,) on the device.  NMS, with two modes: `--save-hybrid` (test.py:137-139, 414) hands the
    batch's pixel-space labels (`targets`) to it as apriori candidates at conf 1 and forces `--save-txt`; `--merge-nms` runs the reference's
    merge-NMS (utils/general.py:594-600: score-weighted mean of the overlapping candidates, images with 1 < n < 3000 candidates, fp64 sums in
    the fixed order of include/icaf.h).  `--confluence P_THRES` swaps the step for the reference's confluence (its commented line
    test.py:140; utils/confluence.py) and leaves everything downstream as it is; neither NMS mode goes with it.  An image whose candidates
    exceed the confluence cap, or that keeps more than MATCH_MAX_DET boxes, raises."""
    if confluence is None:
        lb = [targets[targets[:, 0] == si, 1:] for si in range(nb)] if save_hybrid else None
        det, count, _ = nms_device(out, conf_thres, iou_thres, multi_label=True, agnostic=agnostic, labels=lb, merge=merge_nms)
        return det, count
    det, count, _ = confluence_device(out, conf_thres, confluence)
    for si, n in enumerate(count.tolist()):                      # the matching kernel takes MATCH_MAX_DET rows per image
        if n < 0 or n > MATCH_MAX_DET:
            raise ValueError(f"{paths[si]}: confluence " + (f"met {-n} candidates, above its cap of {det.shape[1]}" if n < 0 else
                                                            f"kept {n} detections, the matching takes {MATCH_MAX_DET}") +
                             "; raise --conf-thres")
    return det[:, :MATCH_MAX_DET].contiguous(), count


def native_labels(targets, nb, net_hw, shapes, dev):
    """Pixel-space targets of a batch -> lab_dev (rows of class + xyxy in native image space), off_dev (nb + 1 row offsets), scale (nb, 5:
    gain, padw, padh, w0, h0 — what maps a detection to native space), all on the device, and tcls_all (the classes per image, host)."""
    lab_rows, off, scale, tcls_all = [], [0], [], []
    for si in range(nb):
        labels = targets[targets[:, 0] == si, 1:]
        tcls_all.append(labels[:, 0].tolist())
        tbox = xywh2xyxy(labels[:, 1:5])
        scale_coords(net_hw, tbox, shapes[si][0], shapes[si][1])
        lab_rows.append(torch.cat((labels[:, :1], tbox), 1))
        off.append(off[-1] + len(labels))
        (h0, w0), ((gain, _), (padw, padh)) = shapes[si][0], shapes[si][1]
        scale.append([gain, padw, padh, w0, h0])
    return (torch.cat(lab_rows).float().contiguous().to(dev), torch.tensor(off, dtype=torch.int32, device=dev),
            torch.tensor(scale, dtype=torch.float32, device=dev), tcls_all)


def match(det, count, lab_dev, off_dev, scale, want_predn, **options):
    """Statistics per image (reference test.py:144-230) on the device: one kernel maps the detections to native space (scale_coords +
    clip_coords) and matches them against the labels -> predn (nb, max_det, 4) when a consumer wants the boxes, correct (nb, max_det, 10)."""
    predn = torch.zeros((det.shape[0], det.shape[1], 4), dtype=torch.float32, device=det.device) if want_predn else None
    correct = ops.match_predictions(det, count, lab_dev, off_dev, torch.from_numpy(IOUV.astype(np.float32)).to(det.device), scale=scale,
                                    predn=predn, **options)
    return predn, correct


@torch.no_grad()
def test(data, weights=None, batch_size=32, imgsz=640, conf_thres=0.001, iou_thres=0.5, single_cls=False, model=None,
         dataloader=None, device="0", compute_dtype=None, cfg=None, verbose=False, save_json=False, save_txt=False, save_conf=True,
         save_dir=None, augment=False, compute_loss=None, confluence=None, plots=False, device_stats=False, stats_out=None, save_hybrid=False,
         merge_nms=False, miss_rate=None, device_letterbox=False):
    if augment:
        raise NotImplementedError("test-time augmentation (models/yolo_test.py:116-132) is outside the inference hot path")
    if confluence is not None and (save_hybrid or merge_nms):
        raise ValueError("--save-hybrid and --merge-nms are modes of NMS: they do not go with --confluence")
    save_txt = save_txt or save_hybrid                                   # reference test.py:414
    if isinstance(data, str):
        with open(data) as f:
            data = yaml.safe_load(f)
    nc = 1 if single_cls else int(data["nc"])
    if miss_rate and nc > 1:
        raise ValueError(f"the KAIST miss rate is a one-class (person) metric: {nc} classes need --single-cls")
    if model is None:
        model = load_model(weights, cfg, nc, device, compute_dtype)
    dev = next(model.parameters()).device
    if dataloader is None:
        gs = int(max(float(model.stride.max()), 32))                      # grid size = max stride (test.py:68)
        # the reference passes `opt` (test.py:100), whose single_cls makes the dataset zero the label classes (utils/datasets.py:465-466)
        dataloader = create_dataloader_rgb_ir(data["val_rgb"], data["val_ir"], imgsz, batch_size, gs, argparse.Namespace(single_cls=single_cls),
                                              pad=0.5, rect=True, native=device_letterbox)[0]
    names = data.get("names", [str(i) for i in range(nc)])
    files = ResultFiles(dataloader.dataset, save_dir, save_txt, save_conf, save_json, weights) if save_txt or save_json else None
    mr_eval = MissRate(miss_rate, dataloader.dataset, dev) if miss_rate else None
    cmatrix = Confusion(nc, dev, names, save_dir) if plots else None     # test.py:103
    stats = DeviceStats(dataloader, dev, stats_out) if device_stats else HostStats(stats_out)
    watch = EventStopwatch() if device_stats else Stopwatch()
    loss = ValLoss(compute_loss, dev, len(dataloader)) if compute_loss else None
    consumers = [c for c in (mr_eval, cmatrix, stats, files) if c is not None]
    want_predn = bool(files or mr_eval or cmatrix)
    seen = 0
    for img, targets, paths, shapes in dataloader:
        x, nb, (height, width) = to_device(img, dev, device_letterbox)
        watch.start()
        res = forward(model, x, (height, width), imgsz)
        watch.stop("inference")
        if loss:                                                 # on the raw maps, before the labels go to pixels (test.py:132-133)
            loss.add(res[2], targets)
        targets = targets.clone()
        targets[:, 2:] *= torch.tensor([width, height, width, height])
        watch.start()
        det, count = suppress(res[0], targets, nb, paths, conf_thres, iou_thres, single_cls, confluence, save_hybrid, merge_nms)
        watch.stop("nms")
        if single_cls:
            det[..., 5] = 0
        lab_dev, off_dev, scale, tcls_all = native_labels(targets, nb, (height, width), shapes, dev)
        predn, correct = match(det, count, lab_dev, off_dev, scale, want_predn, **stats.match_options(tcls_all))
        batch = ValBatch(paths, shapes, nb, det, count, predn, correct, lab_dev, off_dev, tcls_all)
        seen += nb
        for c in consumers:
            c.add(batch)
    if files:
        files.finish()
    stats.finish()
    (mp, mr, map50, map_), maps, lines = summarize(stats.rows, nc, names, seen, verbose, store=stats.store)
    print("\n".join(lines))
    if cmatrix:                                                  # test.py:320-321
        cmatrix.finish()
    t = watch.totals()
    tt = tuple(x / max(seen, 1) * 1e3 for x in (t["inference"], t["nms"], t["inference"] + t["nms"])) + (imgsz, imgsz, batch_size)
    print("Speed: %.1f/%.1f/%.1f ms inference/NMS/total per %gx%g image at batch-size %g" % tt)
    lbox, lobj, lcls = loss.finish() if loss else (0.0, 0.0, 0.0)
    if mr_eval:
        return (mp, mr, map50, map_, lbox, lobj, lcls), maps, tt, mr_eval.finish()
    return (mp, mr, map50, map_, lbox, lobj, lcls), maps, tt


def parse_opt(argv=None):
    ap_ = argparse.ArgumentParser(prog="test.py")
    ap_.add_argument("--weights", nargs="+", type=str, default=None)
    ap_.add_argument("--cfg", type=str, default="models/transformer/yolov5s_Transfusion_kaist.yaml")
    ap_.add_argument("--data", type=str, default="data/multispectral/kaist.yaml")
    ap_.add_argument("--batch-size", type=int, default=32)
    ap_.add_argument("--img-size", type=int, default=640)
    ap_.add_argument("--conf-thres", type=float, default=0.001)
    ap_.add_argument("--iou-thres", type=float, default=0.5)
    ap_.add_argument("--device", default="0")
    ap_.add_argument("--single-cls", action="store_true")
    ap_.add_argument("--half", action="store_true")
    ap_.add_argument("--bf16", action="store_true")
    ap_.add_argument("--verbose", action="store_true")
    ap_.add_argument("--task", default="val", help="val / test / train: one validation pass (the reference reads val_rgb / val_ir for all three); "
                                                   "speed: conf 0.25 / IoU 0.45, nothing saved")
    ap_.add_argument("--augment", action="store_true", help="test-time augmentation: not built, raises")
    ap_.add_argument("--device-letterbox", action="store_true", help="upload the native frames; the loader's resize (area average when "
                                                                     "shrinking) and the padding run on the device")
    ap_.add_argument("--miss-rate", type=str, default=None, metavar="ANNOTATIONS",
                     help="KAIST annotation JSON: also report the log-average miss rate (All / Day / Night, scale and occlusion subsets)")
    ap_.add_argument("--confluence", type=float, default=None, metavar="P_THRES",
                     help="suppress with confluence (normalised Manhattan proximity below P_THRES, utils/confluence.py) instead of NMS")
    ap_.add_argument("--hyp", type=str, default=None, metavar="PATH",
                     help="hyperparameter yaml: also report the validation loss (box / obj / cls, the forward value of ComputeLoss)")
    ap_.add_argument("--plots", action="store_true", help="confusion matrix of the pass (conf 0.25 / IoU 0.45): printed, and saved as "
                                                          "confusion_matrix.txt (+ .png with matplotlib) under <project>/<name>")
    ap_.add_argument("--device-stats", action="store_true", help="keep the statistics on the device: nothing is read back per batch, "
                                                                 "ap_per_class runs as kernels with a stable order at equal confidences")
    ap_.add_argument("--save-txt", action="store_true", help="per-image result lines + result.txt under <project>/<name>/labels")
    ap_.add_argument("--save-conf", action="store_true", help="append the confidence to every --save-txt line")
    ap_.add_argument("--save-json", action="store_true", help="<project>/<name>/<weights>_predictions.json")
    ap_.add_argument("--save-hybrid", action="store_true", help="auto-labelling: the labels join the NMS candidates at conf 1 (implies --save-txt)")
    ap_.add_argument("--merge-nms", action="store_true", help="merge-NMS: every kept box becomes the score-weighted mean of the candidates "
                                                              "overlapping it (images with fewer than 3000 candidates)")
    ap_.add_argument("--project", default="runs/test")
    ap_.add_argument("--name", default="exp")
    ap_.add_argument("--exist-ok", action="store_true")
    return ap_.parse_args(argv)


def loss_from_hyp(path, model, nc, imgsz):
    """`--hyp PATH`: the yaml with the gains scaled as train.py:238-241 scales them, set on the model as train.py:243-245 does (model.hyp,
    model.gr = 1.0), and the ComputeLoss built from it."""
    with open(path) as f:
        hyp = yaml.safe_load(f)
    model.hyp, model.gr = scale_hyp(hyp, model.model[-1].nl, nc, imgsz), 1.0
    return ComputeLoss(model)


def load_model(weights, cfg, nc, device, compute_dtype):
    """The model test() would build itself — the CLI needs it beforehand when a ComputeLoss is to be made from it."""
    return load_detector(weights, cfg, select_device(device), compute_dtype, nc=nc)


if __name__ == "__main__":
    o = parse_opt()
    print(o)
    if o.task not in ("val", "test", "train", "speed"):
        raise NotImplementedError(f"--task {o.task}: only val / test / train / speed are built (study = image-size sweep + plots)")
    dtype = torch.float16 if o.half else torch.bfloat16 if o.bf16 else None
    imgsz = check_img_size(o.img_size, 32)
    if o.task == "speed":                                                   # test.py:420-422
        for w in (o.weights or [None]):
            test(o.data, [w] if w else None, o.batch_size, imgsz, 0.25, 0.45, o.single_cls, device=o.device, compute_dtype=dtype, cfg=o.cfg,
                 device_letterbox=o.device_letterbox)
    else:
        save_dir = increment_path(os.path.join(o.project, o.name), exist_ok=o.exist_ok)      # a name only: test() makes it when a flag saves
        model, compute_loss = None, None
        if o.hyp:
            with open(o.data) as f:
                nc = 1 if o.single_cls else int(yaml.safe_load(f)["nc"])
            model = load_model(o.weights, o.cfg, nc, o.device, dtype)
            compute_loss = loss_from_hyp(o.hyp, model, nc, imgsz)
        test(o.data, o.weights, o.batch_size, imgsz, o.conf_thres, o.iou_thres, o.single_cls, device=o.device, compute_dtype=dtype, cfg=o.cfg,
             verbose=o.verbose, save_json=o.save_json, save_txt=o.save_txt, save_conf=o.save_conf, save_dir=save_dir, augment=o.augment,
             miss_rate=o.miss_rate, device_letterbox=o.device_letterbox, confluence=o.confluence, model=model, compute_loss=compute_loss,
             plots=o.plots, device_stats=o.device_stats, save_hybrid=o.save_hybrid, merge_nms=o.merge_nms)
