#!/usr/bin/env python3
"""Paired-folder RGB / IR inference on MI355X — the front end of the reference's detect_twostream.py (same flags for the
image-folder path: `--source1` visible images, `--source2` infrared images, zipped in sorted order, :56-66).

    python detect_twostream.py --weights best.pt --source1 visible/ --source2 infrared/ [--save-txt] [--half | --bf16]
    python detect_twostream.py --cfg models/transformer/yolov5s_Transfusion_kaist.yaml --source1 ... --source2 ...
                               (no trained ICAFusion weights ship with the reference: --cfg builds the network with
                                deterministic synthetic weights so that the whole path can be exercised)

Per pair: letterbox to --img-size (utils/datasets.py), uint8 -> device, one forward (hipGraph replay) + device NMS,
boxes scaled back to the original image, optional YOLO-format txt / annotated images.  `--augment` runs the reference's test-time
augmentation (three passes per pair, merged before NMS).  `--device-letterbox` hands the decoded frames over as they are: the letterbox and the
mapping of the boxes back to the image then run on the device (Model.forward_frames, ops.scale_detections), same outputs.  The per-frame
`--align-ir FILE|stretch` serves a calibrated rig whose thermal camera differs in size and pose from the visible one: FILE holds the 3 x 3 matrix
that maps visible (aligned) pixel coordinates to thermal pixel coordinates (utils.datasets.load_alignment; --align-inverse: the file maps thermal to
visible), `stretch` is "same field of view, other resolution".  With --device-letterbox the matrix goes to Model.forward_frames(align=...) and the
thermal frame is registered at the letterbox's taps; without it the host calls utils.datasets.warp_perspective in front of letterbox.  Same outputs.
`--ir-16bit` reads --source2 as 16-bit greyscale PNG / TIFF files of raw thermal counts (utils.datasets.imread_u16).  Automatic gain control maps them
to the 8-bit image the network was trained on: a percentile window per frame (`--ir-agc-clip LO_PCT HI_PCT`, default 1 1) or a fixed one
(`--ir-window LO HI`, raw counts).  With --device-letterbox the counts go to Model.forward_frames(formats=(None, "y16")) and are mapped at the
letterbox's taps; without it the host calls utils.datasets.agc_window / agc_u16_to_u8 in front of letterbox.  Same outputs; the annotated thermal
picture is the host-mapped frame on either path.
`Done. (…s, …Hz)` and final `Average Speed` lines are the reference's (:160,198).  Webcam / video sources, the
second-stage classifier and --view-img need OpenCV and are out of scope."""
import argparse
import time
from pathlib import Path

import numpy as np
import torch

from icafusion_amd import ops
from icafusion_amd.models.experimental import load_detector
from icafusion_amd.utils.confluence import confluence_process
from icafusion_amd.utils.datasets import LoadImages, agc_u16_to_u8, agc_window, imwrite_bgr, letterbox, load_alignment, stretch_alignment, warp_perspective
from icafusion_amd.utils.general import increment_path, non_max_suppression, scale_coords, xyxy2xywh
from icafusion_amd.utils.torch_utils import select_device, time_synchronized


def draw_boxes(img_bgr, det, names, thickness=2, hide_labels=False):
    from PIL import Image, ImageDraw
    im = Image.fromarray(np.ascontiguousarray(img_bgr[:, :, ::-1]))
    d = ImageDraw.Draw(im)
    for *xyxy, conf, cls in det.tolist():
        c = int(cls)
        color = ((37 * c + 60) % 256, (91 * c + 160) % 256, (151 * c + 30) % 256)
        d.rectangle(xyxy, outline=color, width=thickness)
        if not hide_labels:
            d.text((xyxy[0] + 2, max(xyxy[1] - 11, 0)), names[c], fill=color)
    return np.asarray(im)[:, :, ::-1]


def load_model(opt, device):
    return load_detector(opt.weights, opt.cfg, device, torch.float16 if opt.half else torch.bfloat16 if opt.bf16 else None)


@torch.no_grad()
def detect(opt):
    if getattr(opt, "merge_nms", False) and getattr(opt, "confluence", None) is not None:
        raise ValueError("--merge-nms is a mode of NMS: it does not go with --confluence")
    device = select_device(opt.device)
    save_img = not opt.nosave
    save_dir = increment_path(Path(opt.project) / opt.name, exist_ok=opt.exist_ok)
    (save_dir / "labels" if opt.save_txt else save_dir).mkdir(parents=True, exist_ok=True)
    model = load_model(opt, device)
    stride = int(model.stride.max())
    names = model.names
    on_device = bool(getattr(opt, "device_letterbox", False))      # native frames in, native boxes out: no host letterbox / scale_coords
    align = getattr(opt, "align_ir", None)                         # a calibrated rig: the thermal frame is registered onto the visible one
    border = int(getattr(opt, "align_border", 0))
    if align is not None and align != "stretch":
        align = load_alignment(align, inverse=bool(getattr(opt, "align_inverse", False)))
    raw16 = bool(getattr(opt, "ir_16bit", False))                  # --source2 holds raw 16-bit thermal counts: gain control in front of the network
    ir_window = getattr(opt, "ir_window", None)
    ir_clip = getattr(opt, "ir_agc_clip", None)
    if not raw16 and (ir_window is not None or ir_clip is not None):
        raise ValueError("--ir-window / --ir-agc-clip describe 16-bit thermal frames: pass --ir-16bit with them")
    if raw16 and align is not None:
        raise ValueError("--ir-16bit does not go with --align-ir yet: the registration reads 8-bit frames")
    if ir_window is not None and ir_clip is not None:
        raise ValueError("--ir-window fixes the gain-control window, --ir-agc-clip picks it per frame: pass one of them")
    if ir_window is not None and not 0 <= ir_window[0] <= ir_window[1] <= 65535:
        raise ValueError(f"--ir-window LO HI must satisfy 0 <= LO <= HI <= 65535, got {ir_window}")
    ir_clip = (100, 100) if ir_clip is None else tuple(int(round(100 * p)) for p in ir_clip)      # per cent -> basis points
    if not all(0 <= c <= 4999 for c in ir_clip):
        raise ValueError("--ir-agc-clip LO_PCT HI_PCT: each between 0 and 49.99 per cent")
    dataset = LoadImages(opt.source1, opt.img_size, stride, native=on_device)
    dataset2 = LoadImages(opt.source2, opt.img_size, stride, native=on_device or align is not None, raw16=raw16)
    if len(dataset) != len(dataset2):
        raise ValueError(f"{len(dataset)} visible images vs {len(dataset2)} infrared images")
    t0, img_num, fps_sum = time.time(), 0, 0.0
    for (path, img, im0, _), (path2, img2, im0_, _) in zip(dataset, dataset2):
        if raw16:
            raw = im0_
            if raw.shape != im0.shape[:2]:
                raise ValueError(f"{path2}: the thermal frame is {raw.shape}, the visible one {im0.shape[:2]}")
            if not on_device or save_img:                              # the mapped thermal frame on the host: the network's input, or only the picture
                lo, hi = tuple(ir_window) if ir_window is not None else agc_window(raw, ir_clip)
                im0_ = np.repeat(agc_u16_to_u8(raw, lo, hi)[:, :, None], 3, axis=2)
            if not on_device:
                img2 = np.ascontiguousarray(letterbox(im0_, opt.img_size, stride=stride)[0][:, :, ::-1].transpose(2, 0, 1))
        if align is not None:
            M = stretch_alignment(im0_.shape[:2], im0.shape[:2]) if isinstance(align, str) else align
            if not on_device or save_img:                              # the registered thermal frame on the host: the network's input, or only the picture
                ir_src, im0_ = im0_, warp_perspective(im0_, M, im0.shape[:2], border)
            if not on_device:
                img2 = np.ascontiguousarray(letterbox(im0_, opt.img_size, stride=stride)[0][:, :, ::-1].transpose(2, 0, 1))
        if on_device and align is not None:
            frames = [torch.from_numpy(np.ascontiguousarray(x)).unsqueeze(0).to(device) for x in (im0, ir_src if save_img else im0_)]
            net_shape = (opt.img_size, opt.img_size)
        elif on_device and raw16:                                      # the counts as their bytes, (1, H0, 2 * W0): every torch release has uint8
            frames = [torch.from_numpy(im0).unsqueeze(0).to(device),
                      torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).reshape(raw.shape[0], 2 * raw.shape[1])).unsqueeze(0).to(device)]
            net_shape = (opt.img_size, opt.img_size)
        elif on_device:
            frames = [torch.from_numpy(x).unsqueeze(0).to(device) for x in (im0, im0_)]      # uint8 (1, H0, W0, 3) BGR, as decoded
            net_shape = (opt.img_size, opt.img_size)
        else:
            img6 = torch.from_numpy(np.concatenate((img, img2), 0)).unsqueeze(0).to(device)     # uint8 (1, 6, H, W)
            net_shape = tuple(img6.shape[2:])
        t1 = time_synchronized()
        # /255, RGB/IR split and the cast happen in the staging kernel; --augment: the three passes of models/yolo_test.py:116-131
        if on_device:
            out, geometry = model.forward_frames(frames[0], frames[1], opt.img_size, bgr=True, augment=getattr(opt, "augment", False),
                                                 **({} if align is None else {"align": (None, M), "align_border": border}),
                                                 **({} if not raw16 else {"formats": (None, "y16"), "agc_clip": ir_clip, "agc_window": ir_window}))
            pred = out[0]
        else:
            pred = (model.forward_u8(img6, augment=True) if getattr(opt, "augment", False) else model.forward_u8(img6))[0]
        if getattr(opt, "confluence", None) is not None:               # the reference's one-line swap (test.py:139-140); --classes afterwards
            det = confluence_process(pred, opt.conf_thres, opt.confluence)[0]
            det = torch.zeros((0, 6), device=pred.device) if det is None else det
            if opt.classes is not None:
                det = det[(det[:, 5:6] == torch.tensor(opt.classes, device=det.device)).any(1)]
            pred = [det]
        else:
            pred = non_max_suppression(pred, opt.conf_thres, opt.iou_thres, classes=opt.classes, agnostic=opt.agnostic_nms,
                                       merge=getattr(opt, "merge_nms", False))
        t2 = time_synchronized()
        det = pred[0]
        p = Path(path)
        s = "%gx%g " % net_shape
        if len(det) and on_device:
            block = det.unsqueeze(0).contiguous()
            ops.scale_detections(block, torch.tensor([len(det)], dtype=torch.int32, device=det.device), geometry.scale,
                                 round=True)(ops.current_stream_ptr())
            det = block[0]
        if len(det):
            if not on_device:
                det[:, :4] = scale_coords(img6.shape[2:], det[:, :4], im0.shape).round()
            for c in det[:, -1].unique():
                n = int((det[:, -1] == c).sum())
                s += f"{n} {names[int(c)]}{'s' * (n > 1)}, "
            if opt.save_txt:
                gn = torch.tensor(im0.shape)[[1, 0, 1, 0]].to(det.device)
                with open(save_dir / "labels" / (p.stem + ".txt"), "a") as f:
                    for *xyxy, conf, cls in reversed(det.tolist()):
                        xywh = (xyxy2xywh(torch.tensor(xyxy).view(1, 4)) / gn.cpu()).view(-1).tolist()
                        line = (cls, *xywh, conf) if opt.save_conf else (cls, *xywh)
                        f.write(("%g " * len(line)).rstrip() % line + "\n")
        if save_img:
            d = det.cpu().numpy() if len(det) else np.zeros((0, 6), np.float32)
            imwrite_bgr(str(save_dir / (p.stem + "_rgb" + p.suffix)), draw_boxes(im0, d, names, opt.line_thickness, opt.hide_labels))
            imwrite_bgr(str(save_dir / (p.stem + "_ir" + p.suffix)), draw_boxes(im0_, d, names, opt.line_thickness, opt.hide_labels))
        print(f"image {img_num + 1}/{len(dataset)} {path}: {s}Done. ({t2 - t1:.6f}s, {1 / (t2 - t1):.6f}Hz)")
        img_num += 1
        fps_sum += 1 / (t2 - t1)
    if opt.save_txt or save_img:
        print(f"Results saved to {save_dir}")
    print(f"Done. ({time.time() - t0:.3f}s)")
    print(f"Average Speed: {fps_sum / max(img_num, 1):.6f}Hz")
    return save_dir


def parse_opt(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", nargs="+", type=str, default=None, help="model.pt path(s) (pickled reference checkpoint)")
    ap.add_argument("--cfg", type=str, default="models/transformer/yolov5s_Transfusion_kaist.yaml",
                    help="model yaml used with synthetic weights when --weights is not given")
    ap.add_argument("--source1", type=str, required=True, help="visible images: file / folder / glob")
    ap.add_argument("--source2", type=str, required=True, help="infrared images: file / folder / glob")
    ap.add_argument("--img-size", type=int, default=640)
    ap.add_argument("--conf-thres", type=float, default=0.1)
    ap.add_argument("--iou-thres", type=float, default=0.5)
    ap.add_argument("--device", default="0")
    ap.add_argument("--half", action="store_true", help="fp16 kernels (the reference's GPU default, :33,40)")
    ap.add_argument("--bf16", action="store_true", help="bf16 kernels")
    ap.add_argument("--save-txt", action="store_true")
    ap.add_argument("--save-conf", action="store_true")
    ap.add_argument("--nosave", action="store_true")
    ap.add_argument("--classes", nargs="+", type=int)
    ap.add_argument("--agnostic-nms", action="store_true")
    ap.add_argument("--confluence", type=float, default=None, metavar="P_THRES",
                    help="suppress with confluence (normalised Manhattan proximity below P_THRES, utils/confluence.py) instead of NMS")
    ap.add_argument("--merge-nms", action="store_true", help="merge-NMS (utils/general.py:594-600): every kept box becomes the score-weighted mean "
                    "of the candidates overlapping it; goes with --augment and ensembles, whose passes repeat every box")
    ap.add_argument("--project", default="runs/detect")
    ap.add_argument("--name", default="exp")
    ap.add_argument("--exist-ok", action="store_true")
    ap.add_argument("--line-thickness", default=2, type=int)
    ap.add_argument("--hide-labels", default=False, action="store_true")
    ap.add_argument("--hide-conf", default=True, action="store_true", help="accepted for the reference's command lines: its default is True and "
                    "cannot be switched off (:224), i.e. boxes carry the class name only — which is what is drawn here")
    ap.add_argument("--augment", action="store_true", help="test-time augmentation (models/yolo_test.py:116-131): scales 1 / 0.83 / 0.67, "
                    "the 0.83 pass flipped left-right; needs --img-size >= 448")
    ap.add_argument("--device-letterbox", action="store_true", help="hand the native frames to the device: letterbox and the mapping of the "
                    "boxes back to the image run as HIP kernels (Model.forward_frames, ops.scale_detections) instead of numpy / torch on the host")
    ap.add_argument("--align-ir", type=str, default=None, metavar="FILE|stretch", help="calibrated rig: the 3 x 3 matrix (nine numbers, text or .npy) "
                    "that maps visible pixel coordinates to thermal pixel coordinates, or `stretch` (same field of view, other resolution); the "
                    "thermal frame is registered onto the visible one, boxes are in the visible frame")
    ap.add_argument("--align-inverse", action="store_true", help="the --align-ir file maps thermal to visible coordinates (findHomography(ir, visible)): invert it")
    ap.add_argument("--ir-16bit", action="store_true", help="--source2 holds 16-bit greyscale PNG / TIFF files of raw thermal counts; automatic gain "
                    "control maps them to 8 bits (on the device with --device-letterbox)")
    ap.add_argument("--ir-agc-clip", type=float, nargs=2, default=None, metavar=("LO_PCT", "HI_PCT"), help="per cent of the pixels clipped at the "
                    "low / high end of each thermal frame's histogram (default 1 1)")
    ap.add_argument("--ir-window", type=int, nargs=2, default=None, metavar=("LO", "HI"), help="a fixed gain-control window in raw counts instead of the per-frame percentiles")
    ap.add_argument("--align-border", type=int, default=0, metavar="N", help="grey level 0..255 of registered pixels the thermal frame does not cover")
    return ap.parse_args(argv)


if __name__ == "__main__":
    opt = parse_opt()
    print(opt)
    detect(opt)
