#!/usr/bin/env python3
"""Validation loop (mAP@0.5, mAP@0.5:0.95) of the two-stream detector on MI355X — the reference's test.py:23-330 reduced
to its metric path: paired RGB/IR loader -> forward -> NMS(multi_label) -> per-image TP matching at 10 IoU thresholds ->
ap_per_class.  `test(...)` keeps the reference's return value ((mp, mr, map50, map, lbox, lobj, lcls), maps, times); the three losses are 0
unless a loss is asked for (below).

    python test.py --data data/multispectral/kaist.yaml --weights best.pt --batch-size 32 --img-size 640
    python test.py --data ... --cfg models/transformer/yolov5s_Transfusion_kaist.yaml      (synthetic weights: plumbing)

Protocol as the reference's: rectangular batches with pad 0.5 (test.py:100 — KAIST's 512x640 frames become 544x672
batches), conf 0.001 / IoU 0.5 multi-label NMS, boxes mapped back to native image space before matching.  Every distinct
batch shape compiles its own execution plan (hipGraph); Model keeps them in a byte-capped LRU (Model.plan_cache_bytes).
`--save-txt` / `--save-conf` / `--save-json` leave the reference's result files (per-image `frame,x,y,w,h[,conf]` lines + `result.txt`,
the input of the KAIST miss-rate evaluator; `<weights>_predictions.json`) under `--project/--name` (icafusion_amd/utils/results.py);
`--miss-rate ANNOTATIONS` adds the KAIST log-average miss rate (the evaluator of the reference's `evaluation_script/`: matching on the
device, FPPI sweep in numpy; icafusion_amd/utils/missrate.py) and returns its dict as a fourth element; `--task speed` ignores it.
`--task speed` runs at conf 0.25 / IoU 0.45 as the reference does.  `--device-letterbox` uploads the frames as decoded: the loader's
longest-side resize (pixel-area average when shrinking) and the padding run on the device (Model.forward_frames(val_size=...)).
`--confluence P_THRES` swaps the suppression step for the reference's confluence (its commented line test.py:140; utils/confluence.py) and leaves
everything downstream as it is; `--hyp PATH` (or `test(compute_loss=...)`, as the reference's train.py:257,393 calls it) adds the validation
loss — the forward value of the reference's ComputeLoss on the raw Detect maps of every batch (utils/loss.py:325-463; icaf_loss, no gradients),
averaged over the batches as test.py:132-133,364-367 do, with the hyp gains scaled as train.py:238-241 scales them — fills the three trailing
values and prints one `Loss:` line; there is no default hyp file, and without the flag nothing changes.  An image whose candidates exceed the confluence cap, or that keeps more than 1024 boxes, raises.
`--save-hybrid` (test.py:137-139, 414) hands every batch's pixel-space labels to NMS as apriori candidates at conf 1 and forces `--save-txt`;
`--merge-nms` runs the reference's merge-NMS (utils/general.py:594-600: score-weighted mean of the overlapping candidates, images with
1 < n < 3000 candidates, fp64 sums in the fixed order of include/icaf.h); neither goes with `--confluence`.
`--plots` builds the reference's ConfusionMatrix (test.py:103,205-206,320-321; conf 0.25 / IoU 0.45) on the device, one launch per batch, prints
it and saves confusion_matrix.txt (and confusion_matrix.png when matplotlib is there); `--device-stats` keeps the statistics of the pass on the device: every batch is
appended to an ops.StatsStore, nothing is read back per batch (result files excepted), the four synchronisations per batch become event pairs, and
ap_per_class runs as kernels with a DEFINED order at equal confidences (arrival order; the host's np.argsort leaves it to the numpy build).  Without
the two flags the loop runs the code it always ran.  Not carried over (all outside the metric): the PR / F1 / P / R curve images and `plot_images` /
wandb / `--task study` / the pycocotools call / MR curves and plots; `--augment` raises (the help text says
test-time augmentation is not built; Model.forward(augment=True) is by now — test() still refuses it)."""
import argparse
import os
import time

import numpy as np
import torch
import yaml

from icafusion_amd.models.experimental import attempt_load
from icafusion_amd.models.yolo import Model
from icafusion_amd.utils.datasets import create_dataloader_rgb_ir
from icafusion_amd import ops
from icafusion_amd.utils.general import check_img_size, increment_path, nms_device, scale_coords, xywh2xyxy
from icafusion_amd.utils import missrate
from icafusion_amd.utils.confluence import confluence_device
from icafusion_amd.utils.loss import ComputeLoss, scale_hyp
from icafusion_amd.utils.results import ResultWriter, frame_index, label_listing
from icafusion_amd.utils.metrics import ConfusionMatrix, ap_per_class
from icafusion_amd.utils.torch_utils import select_device, time_synchronized

MATCH_MAX_DET = 1024                                             # detections per image icaf_match_predictions takes (nms.hip)


def summarize(stats, nc, names, seen, verbose=False, store=None):
    """Statistics -> (mp, mr, map50, map, maps) + the reference's result table (test.py:287-313): for one class the columns are
    TP / FP / FN / F1 / P / R / mAP@.5 / mAP@.5:.95, otherwise P / R / mAP@.5 / mAP@.75 / mAP@.5:.95 with one row per class when
    `verbose`.  stats: list of (correct (n, 10) bool, conf (n,), pcls (n,), tcls list) per image — or, with `store` (an ops.StatsStore, the
    `device_stats` path), the list of the images' label classes: the numbers then come from icaf_ap_per_class, and "no TP at all means
    every metric is 0" reads the store's any_tp flag."""
    mp = mr = map50 = map75 = map_ = 0.0
    tp = fp = fn = f1 = np.zeros(1)
    p = r = np.zeros(0)
    ap, ap_class, nt = np.zeros((0, 10)), np.zeros(0, int), np.zeros(nc, int)
    if store is not None:
        tcls = np.concatenate([np.asarray(t, np.float64) for t in stats]) if stats else np.zeros(0)
        if store.rows() and store.any_tp():
            ap_class, n_l = np.unique(tcls, return_counts=True)
            res = ops.ap_per_class_device(store, ap_class, n_l)
            i, ap, ap_class = res["best"], res["ap"], ap_class.astype("int32")
            tp, fp, fn, p, r, f1 = res["tp"], res["fp"], res["fn"], res["p"][:, i], res["r"][:, i], res["f1"][:, i]
            mp, mr, map50, map75, map_ = p.mean(), r.mean(), ap[:, 0].mean(), ap[:, 5].mean(), ap.mean()
        nt = np.bincount(tcls.astype(np.int64), minlength=nc)
    elif stats:
        cat = [np.concatenate([np.asarray(s[k]) for s in stats], 0) for k in range(4)]
        if len(cat[0]) and cat[0].any():
            tp, fp, fn, p, r, ap, f1, ap_class = ap_per_class(cat[0], cat[1], cat[2], cat[3])
            mp, mr, map50, map75, map_ = p.mean(), r.mean(), ap[:, 0].mean(), ap[:, 5].mean(), ap.mean()
        nt = np.bincount(cat[3].astype(np.int64), minlength=nc)
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


class MissRate:
    """KAIST log-average miss rate of one validation pass (`miss_rate=` / `--miss-rate`): every batch's native-space boxes are staged on
    the device into the store the matching kernel reads (icaf_missrate_stage, at the image's position in the sorted label directory:
    the `frame - 1` of result.txt), one icaf_missrate_match launch follows the loop, and utils.missrate.summarize runs the FPPI sweep."""

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

    def stage(self, predn, det, count, paths):
        if self.dt is None:                                                     # cap = NMS's max_det
            self.dt = torch.zeros((self.tab.images, det.shape[1], 5), dtype=torch.float64, device=self.dev)
            self.count = torch.zeros((self.tab.images,), dtype=torch.int32, device=self.dev)
        index = [frame_index(self.listing, os.path.splitext(os.path.basename(p))[0]) for p in paths]
        ops.missrate_stage(predn, det, count, index, torch.tensor(index, dtype=torch.int32, device=self.dev), self.dt,
                           self.count)(ops.current_stream_ptr())

    def finish(self):
        if self.dt is None:
            raise ValueError("no batch was staged")
        outs = ops.missrate_outputs(self.tab, self.dt.shape[1], self.dev)
        ops.missrate_match(self.tab, self.dt, self.count, *outs)(ops.current_stream_ptr())
        order, dt_gt, dt_ignore, gt_ignore = (o.cpu().numpy() for o in outs)
        dt, count = self.dt.cpu().numpy(), self.count.cpu().numpy()
        return missrate.summarize(self.table, count, missrate.sorted_scores(dt, order, count), dt_gt, dt_ignore, gt_ignore[:self.tab.labels])


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
    writer = None
    if save_txt or save_json:                                           # result files of the reference (utils/results.py)
        listing = label_listing(os.path.dirname(dataloader.dataset.label_files[0])) if save_txt else None
        writer = ResultWriter(save_dir if save_dir is not None else increment_path("runs/test/exp"), save_txt=save_txt, save_conf=save_conf,
                              save_json=save_json, label_names=listing, weights=weights)
    mr_eval = MissRate(miss_rate, dataloader.dataset, dev) if miss_rate else None
    iouv = np.linspace(0.5, 0.95, 10)
    names = data.get("names", [str(i) for i in range(nc)])
    stats, seen, t_inf, t_nms = [], 0, 0.0, 0.0
    cmatrix = ConfusionMatrix(nc, device=dev) if plots else None          # test.py:103
    store, events = None, []                                             # device_stats: the statistics stay on the device until the pass is over

    def clock():                                                         # device_stats: an event on the stream instead of a synchronisation
        if not device_stats:
            return time_synchronized()
        events.append(ops.Event())
        events[-1].record(ops.current_stream_ptr())
        return 0.0
    loss = torch.zeros(3, device=dev) if compute_loss else None          # box, obj, cls: summed on the device, read once after the loop
    for img, targets, paths, shapes in dataloader:
        if device_letterbox:                                     # native BGR frames as decoded: resized and padded on the device
            rgb, ir, (height, width) = img
            rgb, ir, nb = [f.to(dev, non_blocking=True) for f in rgb], [f.to(dev, non_blocking=True) for f in ir], len(rgb)
            t = clock()
            res = model.forward_frames(rgb, ir, img_size=(height, width), val_size=imgsz)[0]
        else:
            img = img.to(dev, non_blocking=True)                 # uint8 (B, 6, H, W): cat(rgb, ir), test.py:116-123
            nb, _, height, width = img.shape
            t = clock()
            res = model.forward_u8(img)
        out = res[0]
        t_inf += clock() - t
        if compute_loss:                                         # on the raw maps, before the labels go to pixels (test.py:132-133)
            loss += compute_loss(res[2], targets.to(dev))[1][:3]
        targets = targets.clone()
        targets[:, 2:] *= torch.tensor([width, height, width, height])
        t = clock()
        if confluence is not None:                               # the reference's one-line swap (test.py:139-140)
            det, count, _ = confluence_device(out, conf_thres, confluence)
            for si, n in enumerate(count.tolist()):              # the matching kernel takes MATCH_MAX_DET rows per image
                if n < 0 or n > MATCH_MAX_DET:
                    raise ValueError(f"{paths[si]}: confluence " + (f"met {-n} candidates, above its cap of {det.shape[1]}" if n < 0 else
                                                                    f"kept {n} detections, the matching takes {MATCH_MAX_DET}") +
                                     "; raise --conf-thres")
            det = det[:, :MATCH_MAX_DET].contiguous()
        else:
            # --save-hybrid: the batch's pixel-space targets join the candidates as apriori labels (reference test.py:137-139)
            lb = [targets[targets[:, 0] == si, 1:] for si in range(nb)] if save_hybrid else None
            det, count, _ = nms_device(out, conf_thres, iou_thres, multi_label=True, agnostic=single_cls, labels=lb, merge=merge_nms)
        t_nms += clock() - t
        # statistics per image (reference test.py:144-230) on the device: labels go up in native image space, one kernel
        # maps the detections there (scale_coords + clip_coords) and matches them; only flags / conf / cls come back
        if single_cls:
            det[..., 5] = 0
        lab_rows, off, scale, tcls_all = [], [0], [], []
        for si in range(nb):
            labels = targets[targets[:, 0] == si, 1:]
            tcls_all.append(labels[:, 0].tolist())
            tbox = xywh2xyxy(labels[:, 1:5])
            scale_coords((height, width), tbox, shapes[si][0], shapes[si][1])                 # native-space labels
            lab_rows.append(torch.cat((labels[:, :1], tbox), 1))
            off.append(off[-1] + len(labels))
            (h0, w0), ((gain, _), (padw, padh)) = shapes[si][0], shapes[si][1]
            scale.append([gain, padw, padh, w0, h0])
        predn = torch.zeros((nb, det.shape[1], 4), dtype=torch.float32, device=dev) if writer or mr_eval or cmatrix else None     # native-space boxes
        lab_dev, off_dev = torch.cat(lab_rows).float().contiguous().to(dev), torch.tensor(off, dtype=torch.int32, device=dev)
        correct = ops.match_predictions(det, count, lab_dev, off_dev, torch.from_numpy(iouv.astype(np.float32)).to(dev),
                                        scale=torch.tensor(scale, dtype=torch.float32, device=dev), predn=predn,
                                        **({"max_labels": max(len(t) for t in tcls_all)} if device_stats else {}))     # no label_off read-back
        if mr_eval:
            mr_eval.stage(predn, det, count, paths)
        if cmatrix:                                              # test.py:205-206, every image of the batch in one launch
            cmatrix.process_images(predn, det, count, lab_dev, off_dev)
        if device_stats:                                         # nothing comes back: the rows go to the store in the host loop's order
            if store is None:                                    # images x max_det rows: an upper bound of the cursor, it cannot overflow
                store = ops.StatsStore(len(dataloader.dataset) * det.shape[1], len(iouv), dev)
            store.stage(correct, det, count)
            stats += tcls_all
            seen += nb
            if writer:                                           # the result files are written on the host: their rows still come back
                cnt, cc, pn = count.cpu().numpy(), det[..., 4:6].cpu().numpy(), predn.cpu().numpy()
                for si in range(nb):
                    if cnt[si]:
                        writer.add(paths[si], pn[si, :cnt[si]], cc[si, :cnt[si], 0], cc[si, :cnt[si], 1])
            continue
        correct, cc, count = correct.cpu().numpy().astype(bool), det[..., 4:6].cpu().numpy(), count.cpu().numpy()
        predn = predn.cpu().numpy() if writer else None
        for si in range(nb):
            n, tcls = int(count[si]), tcls_all[si]
            seen += 1
            if writer and n:
                writer.add(paths[si], predn[si, :n], cc[si, :n, 0], cc[si, :n, 1])
            if n == 0:
                if tcls:
                    stats.append((np.zeros((0, 10), bool), np.zeros(0), np.zeros(0), tcls))
                continue
            stats.append((correct[si, :n] if tcls else np.zeros((n, 10), bool), cc[si, :n, 0], cc[si, :n, 1], tcls))
    if writer:
        result_txt, pred_json = writer.close()
        for f in (result_txt, pred_json):
            if f is not None:
                print(f"saved {f}")
    if device_stats:                                             # the event pairs of every batch, read once the pass is over
        ms = [a.elapsed_ms(b) for a, b in zip(events[0::2], events[1::2])]
        t_inf, t_nms = sum(ms[0::2]) / 1e3, sum(ms[1::2]) / 1e3
    if isinstance(stats_out, list):
        stats_out.append(store) if device_stats else stats_out.extend(stats)
    (mp, mr, map50, map_), maps, lines = summarize(stats, nc, names, seen, verbose, store=store)
    print("\n".join(lines))
    if cmatrix:                                                  # test.py:320-321
        cmatrix.print()
        plot_dir = str(save_dir) if save_dir is not None else str(increment_path("runs/test/exp"))
        os.makedirs(plot_dir, exist_ok=True)
        cmatrix.plot(save_dir=plot_dir, names=list(names))
    tt = tuple(x / max(seen, 1) * 1e3 for x in (t_inf, t_nms, t_inf + t_nms)) + (imgsz, imgsz, batch_size)
    print("Speed: %.1f/%.1f/%.1f ms inference/NMS/total per %gx%g image at batch-size %g" % tt)
    lbox, lobj, lcls = (loss.cpu() / len(dataloader)).tolist() if compute_loss else (0.0, 0.0, 0.0)       # test.py:364-367
    if compute_loss:
        print("Loss: %.5g box, %.5g obj, %.5g cls (mean of %d batches)" % (lbox, lobj, lcls, len(dataloader)))
    if mr_eval:
        mr_dict = mr_eval.finish()
        print("\n".join(missrate.format_lines(mr_dict)))
        return (mp, mr, map50, map_, lbox, lobj, lcls), maps, tt, mr_dict
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
    dev = select_device(device)
    if weights:
        model = attempt_load(weights, map_location="cpu")
    else:
        from icafusion_amd.synth import synth_state_dict
        model = Model(cfg, nc=nc).eval()
        model.load_state_dict(synth_state_dict(model, seed=0))
        model = model.fuse().eval()
    model = model.to(dev)
    model.compute_dtype = compute_dtype
    model.use_graph = True
    return model


if __name__ == "__main__":
    o = parse_opt()
    print(o)
    o.save_txt |= o.save_hybrid                                             # reference test.py:414
    if o.task not in ("val", "test", "train", "speed"):
        raise NotImplementedError(f"--task {o.task}: only val / test / train / speed are built (study = image-size sweep + plots)")
    dtype = torch.float16 if o.half else torch.bfloat16 if o.bf16 else None
    imgsz = check_img_size(o.img_size, 32)
    if o.task == "speed":                                                   # test.py:420-422
        for w in (o.weights or [None]):
            test(o.data, [w] if w else None, o.batch_size, imgsz, 0.25, 0.45, o.single_cls, device=o.device, compute_dtype=dtype, cfg=o.cfg,
                 device_letterbox=o.device_letterbox)
    else:
        save_dir = increment_path(os.path.join(o.project, o.name), exist_ok=o.exist_ok) if (o.save_txt or o.save_json or o.plots) else None
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
