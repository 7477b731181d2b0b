#!/usr/bin/env python3
"""Cost of serving native YUV 4:2:0 frames (icaf_letterbox_yuv_frames; Model.forward_frames(formats=...) / DetectionPipeline(frame_formats=...)).

    python tools/yuv_frames_bench.py [--model s --batch 32 --size 640 --frames 512x640,1080x1920 --rounds 30 --out profiles/yuv_frames_bench.json]

One process, items interleaved round by round in a rotating order, medians reported, every item with an `_again` twin on the same buffers
for the A/A spread (the method of tools/frames_bench.py):
  (1) per frame size, one modality of --batch frames: icaf_letterbox_yuv_frames on NV12 (default path and forced direct) against the
      yardstick icaf_letterbox_frames on the same content as BGR (HIP event pairs around --inner launches); microseconds and algorithmic
      bytes (frames read once, planes written once) per second.  NV12 reads half the bytes and converts four taps per output pixel.
  (2) the status quo for a YUV source: NV12 -> BGR as torch ops on the device into the BGR arena, then icaf_letterbox_frames.  The fused
      launch and this pair are checked to give the same planes before anything is timed.
  (3) the host-fed pipeline at the last frame size, depth --depth: submit_frames from pinned host memory with NV12 + grey against
      BGR + grey in one interleaved loop (wall clock around --steps submits + synchronize), pairs per second and bytes uploaded per step."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import yaml          # noqa: E402

from icafusion_amd import ops                                     # noqa: E402
from icafusion_amd.models.yolo import Model                       # noqa: E402
from icafusion_amd.pipeline import DetectionPipeline              # noqa: E402
from icafusion_amd.synth import synth_state_dict                  # noqa: E402
from icafusion_amd.utils import datasets as D                     # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def nv12_to_bgr_torch(buf, h0, w0, out):
    """The conversion a user writes today: (B, 3 * h0 // 2, w0) NV12 -> (B, h0, w0, 3) BGR with torch ops, BT.601 limited range, the
    integer rule of utils.datasets.yuv420_to_bgr."""
    B = buf.shape[0]
    c = 298 * (buf[:, :h0].to(torch.int32) - 16) + 128
    uv = buf[:, h0:].reshape(B, h0 // 2, w0 // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    d, e = uv[..., 0], uv[..., 1]
    out.copy_(torch.stack(((c + 516 * d) >> 8, (c - 100 * d - 208 * e) >> 8, (c + 409 * e) >> 8), dim=3).clamp_(0, 255))


def kernel_items(B, shape, size, dev, seed):
    """The launches of (1) and (2) for one frame size, on one NV12 arena and one BGR arena of the same content."""
    h0, w0 = shape
    geom1, _ = ops.frame_geometry([shape] * B, size)
    yrows, yend = ops.pack_yuv_frames(geom1, "nv12")
    brows = geom1.copy()
    bend = ops.pack_frames(brows, 3)
    fb = 3 * h0 * w0 // 2
    assert fb % ops.FRAME_ALIGN == 0 and (3 * h0 * w0) % ops.FRAME_ALIGN == 0, "frame sizes whose buffers lie back to back in the arenas"
    g = torch.Generator().manual_seed(seed)
    nv12 = torch.randint(0, 256, (B, 3 * h0 // 2, w0), dtype=torch.uint8, generator=g).to(dev)
    yarena, barena = nv12.reshape(-1), torch.zeros((bend,), dtype=torch.uint8, device=dev)
    assert yarena.numel() == yend
    bgr = barena.view(B, h0, w0, 3)
    nv12_to_bgr_torch(nv12, h0, w0, bgr)
    ytab, btab = ops.geom_tensor(yrows, dev), ops.geom_tensor(brows, dev)

    def planes():
        return torch.zeros((B, 3, size, size), dtype=torch.uint8, device=dev)
    py, pb = planes(), planes()
    yuv = [ops.letterbox_yuv_frames(yarena, yrows, ytab, p) for p in (py, planes())]
    ref = [ops.letterbox_frames(barena, brows, btab, p, swap_rb=True) for p in (pb, planes())]
    sp = ops.current_stream_ptr()
    yuv[0](sp), ref[0](sp)
    torch.cuda.synchronize()
    same = bool(torch.equal(py, pb))
    one = D.yuv420_to_bgr(*D.yuv420_planes(nv12[0].cpu().numpy(), h0, w0, "nv12"), 0)
    same_host = bool(np.array_equal(bgr[0].cpu().numpy(), one))

    def direct(launch):
        def run(s):
            with ops.letterbox_direct(True):
                launch(s)
        return run

    def status_quo(launch):
        def run(s):
            nv12_to_bgr_torch(nv12, h0, w0, bgr)
            launch(s)
        return run
    tag = f"{h0}x{w0}"
    items, nbytes = {}, {}
    for name, pair, nb in (("yuv_staged", yuv, yuv[0].bytes), ("yuv_direct", [direct(l) for l in yuv], yuv[0].bytes),
                           ("bgr_staged", ref, ref[0].bytes), ("bgr_direct", [direct(l) for l in ref], ref[0].bytes),
                           ("torch_convert_then_bgr", [status_quo(l) for l in ref], yuv[0].bytes)):
        items[f"{name}_{tag}"], items[f"{name}_{tag}_again"] = pair
        nbytes[f"{name}_{tag}"] = nbytes[f"{name}_{tag}_again"] = nb
    facts = {"fused_equals_convert_then_letterbox": same, "torch_conversion_equals_host_rule": same_host,
             "yuv_staged_by_budget_rule": bool(ops.yuv_letterbox_staged(yrows[0])), "bgr_staged_by_budget_rule": bool(ops.letterbox_staged(brows[0]))}
    return items, nbytes, facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="s"); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640); ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--frames", default="512x640,1080x1920")
    ap.add_argument("--rounds", type=int, default=30); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="launches inside one event pair")
    ap.add_argument("--steps", type=int, default=8, help="pipeline steps inside one wall-clock interval")
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--no-autotune", action="store_true"); ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_frames_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "yuv_frames_bench.py measures on the GPU only"
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    B, S = a.batch, a.size
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.frames.split(",")]
    sp = ops.current_stream_ptr()

    # ---- (1) + (2): kernels alone -----------------------------------------------------------------------------------------------------
    items, nbytes, facts = {}, {}, {}
    for k, shape in enumerate(shapes):
        it, nb, facts[f"{shape[0]}x{shape[1]}"] = kernel_items(B, shape, S, dev, k + 1)
        items.update(it); nbytes.update(nb)
    names = list(items)
    e0, e1 = ops.Event(), ops.Event()
    times = {n: [] for n in names}
    for r in range(a.warmup + a.rounds):
        for k in range(len(names)):
            n = names[(k + r) % len(names)]
            e0.record(sp)
            for _ in range(a.inner):
                items[n](sp)
            e1.record(sp)
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[n].append(e0.elapsed_ms(e1) / a.inner)
    kern = {n: {"us": median(v) * 1e3, "us_min_max": [min(v) * 1e3, max(v) * 1e3], "algorithmic_bytes": int(nbytes[n]),
                "GB_per_s": nbytes[n] / (median(v) * 1e-3) / 1e9} for n, v in times.items()}
    ratios = {}
    for shape in shapes:
        t = f"{shape[0]}x{shape[1]}"
        us = {n: kern[f"{n}_{t}"]["us"] for n in ("yuv_staged", "yuv_direct", "bgr_staged", "bgr_direct", "torch_convert_then_bgr")}
        ratios[t] = {"yuv_over_bgr_time": us["yuv_staged"] / us["bgr_staged"], "yuv_direct_over_staged_time": us["yuv_direct"] / us["yuv_staged"],
                     "status_quo_over_fused_time": us["torch_convert_then_bgr"] / us["yuv_staged"],
                     "aa_spread": {n: abs(kern[f"{n}_{t}"]["us"] - kern[f"{n}_{t}_again"]["us"]) / kern[f"{n}_{t}"]["us"] for n in us}}
    res = {"batch": B, "size": S, "frames": [list(s) for s in shapes], "device": ops.device_info(),
           "timing": f"kernels: HIP events around {a.inner} launches, median of {a.rounds} interleaved rounds after {a.warmup}; pipelines: wall clock "
                     f"around {a.steps} submits + synchronize, same rounds, interleaved; *_again: a second copy of the item (the A/A spread)",
           "kernels": kern, "ratios": ratios, "checks": facts}

    # ---- (3): host-fed pipelines ------------------------------------------------------------------------------------------------------
    if not a.no_pipeline:
        frame = shapes[-1]
        cfg = yaml.safe_load(open(os.path.join(ROOT, "models", "transformer", f"yolov5{a.model}_Transfusion_kaist.yaml")))
        cache = os.path.join(ROOT, "profiles", "tune_cache.json")
        if not a.no_autotune and os.path.exists(cache):
            ops.load_tune_cache(cache)

        def model():
            m = Model(cfg).eval()
            m.load_state_dict(synth_state_dict(m, 0))
            m = m.to(dev)
            m.compute_dtype, m.use_graph, m.autotune, m.static_outputs = dt, True, not a.no_autotune, True
            return m
        kw = dict(conf_thres=0.25, iou_thres=0.45, depth=a.depth, frames=frame, frame_channels=(3, 1))
        pipes = {"nv12_grey": DetectionPipeline(model(), B, S, S, dev, frame_formats=("nv12", None), **kw),
                 "bgr_grey": DetectionPipeline(model(), B, S, S, dev, **kw),
                 "nv12_grey_again": DetectionPipeline(model(), B, S, S, dev, frame_formats=("nv12", None), **kw),
                 "bgr_grey_again": DetectionPipeline(model(), B, S, S, dev, **kw)}
        gen = torch.Generator().manual_seed(3)
        h0, w0 = frame
        feeds = []                                                       # two sets of pinned buffers, only ever read
        for _ in range(2):
            nv12 = torch.randint(0, 256, (B, 3 * h0 // 2, w0), dtype=torch.uint8, generator=gen)
            bgr = torch.empty((B, h0, w0, 3), dtype=torch.uint8, device=dev)
            nv12_to_bgr_torch(nv12.to(dev), h0, w0, bgr)
            grey = torch.randint(0, 256, (B, h0, w0, 1), dtype=torch.uint8, generator=gen).pin_memory()
            feeds.append({"nv12": (nv12.pin_memory(), grey), "bgr": (bgr.cpu().pin_memory(), grey)})

        def run(name, k0):
            p = pipes[name]
            for k in range(a.steps):
                p.submit_frames(*feeds[(k0 + k) % 2][name.split("_")[0]])
            p.synchronize()
        pn = list(pipes)
        rates = {n: [] for n in pn}
        for r in range(a.warmup + a.rounds):
            for k in range(len(pn)):
                n = pn[(k + r) % len(pn)]
                t0 = time.perf_counter()
                run(n, r * a.steps)
                dtm = time.perf_counter() - t0
                if r >= a.warmup:
                    rates[n].append(a.steps * B / dtm)
        med = {n: median(v) for n, v in rates.items()}
        up = {"nv12_grey": B * (3 * h0 * w0 // 2 + h0 * w0), "bgr_grey": B * 4 * h0 * w0}
        res["pipeline"] = {"frame": list(frame), "depth": a.depth, "nplans": pipes["bgr_grey"].nplans, "pairs_per_s": med,
                           "pairs_per_s_min_max": {n: [min(v), max(v)] for n, v in rates.items()},
                           "aa_spread": {n: abs(med[n] - med[n + "_again"]) / med[n] for n in ("nv12_grey", "bgr_grey")},
                           "nv12_over_bgr": med["nv12_grey"] / med["bgr_grey"], "uploaded_bytes_per_step": up,
                           "upload_GB_per_s": {n: up[n] * med[n] / B / 1e9 for n in up}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
