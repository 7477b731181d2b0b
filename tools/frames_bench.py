#!/usr/bin/env python3
"""Cost of serving NATIVE camera frames (Model.forward_frames / DetectionPipeline.submit_frames) on the GPU.

    python tools/frames_bench.py [--model s --batch 32 --size 640 --frame 512x640 --dtype bf16 --rounds 30 --out profiles/frames_bench.json]

One process, items interleaved round by round in a rotating order, medians reported (the method of tools/tta_bench.py):
  (a) letterbox_staged / letterbox_direct   icaf_letterbox_frames alone on its two paths (HIP event pairs around --inner launches), with
      its algorithmic bytes (frames read once, planes written once) over the time; the same pair for frames that really are resized
      (--resize-frame, default 384x480: the KAIST frame at 640 is a copy between pads); upsample_nearest at a comparable byte volume is
      the project's streaming yardstick.  Each of the four has two companions on the same arena and descriptors: `<item>_again`, a second
      copy of the launch (the A/A spread), and `resize_null_<path>[_resize]`, icaf_resize_frames without a mode table — the other kernel
      that runs the same tile (`tile_ab`: is its median within the letterbox's median plus that spread?)
  (b) scale_detections alone
  (c) the host-fed pipeline at depth 2: submit_frames from pinned native frames against submit_u8 from pinned host-letterboxed batches,
      and a SECOND copy of the submit_u8 configuration for the A/A spread of the call (wall clock around --steps submits + synchronize)
  (d) for context: host letterbox() + scale_coords per pair on one CPU thread — the work that leaves the serving loop."""
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
from icafusion_amd.utils.general import scale_coords              # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def letterbox_launch(B, shape, size, dev, seed):
    """((letterbox, letterbox again, resize without a mode table), geom) of a two-modality batch of B random BGR frames of one shape, in a
    tight arena: three launches on the same arena and device table, each into planes of its own."""
    h0, w0 = shape
    geom1, _ = ops.frame_geometry([shape] * B, size)
    geom = np.concatenate((geom1, geom1))
    end = ops.pack_frames(geom, 3)
    g = torch.Generator().manual_seed(seed)
    arena = torch.randint(0, 256, (end,), dtype=torch.uint8, generator=g).to(dev)
    tab = ops.geom_tensor(geom, dev)

    def planes():
        return torch.zeros((B, 6, size, size), dtype=torch.uint8, device=dev)
    return (ops.letterbox_frames(arena, geom, tab, planes(), swap_rb=True), ops.letterbox_frames(arena, geom, tab, planes(), swap_rb=True),
            ops.resize_frames(arena, geom, None, tab, planes(), swap_rb=True)), geom


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="s"); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640); ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--frame", default="512x640"); ap.add_argument("--resize-frame", default="384x480")
    ap.add_argument("--rounds", type=int, default=30); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="launches inside one event pair")
    ap.add_argument("--steps", type=int, default=12, help="pipeline steps inside one wall-clock interval")
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--no-autotune", action="store_true"); ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "frames_bench.py measures on the GPU only"
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    B, S = a.batch, a.size
    frame, rframe = (tuple(int(v) for v in s.split("x")) for s in (a.frame, a.resize_frame))
    sp = ops.current_stream_ptr()

    # ---- (a) + (b): kernels alone -------------------------------------------------------------------------------------------------
    (lb, lb2, rn), geom = letterbox_launch(B, frame, S, dev, 1)
    (lbr, lbr2, rnr), geomr = letterbox_launch(B, rframe, S, dev, 2)
    up = ops.upsample_nearest(torch.randn((B, 80, 80, 64), device=dev).to(dt), torch.empty((B, 160, 160, 64), dtype=dt, device=dev), 2)
    det = torch.rand((B, 300, 6), device=dev) * S
    count = torch.full((B,), 300, dtype=torch.int32, device=dev)
    sd = ops.scale_detections(det, count, torch.from_numpy(ops.frame_geometry([frame] * B, S)[1]).to(dev), out=torch.empty_like(det))

    def direct(launch):
        def run(s):
            with ops.letterbox_direct(True):
                launch(s)
        return run
    items = {"letterbox_staged": lb, "letterbox_direct": direct(lb), "letterbox_staged_resize": lbr, "letterbox_direct_resize": direct(lbr),
             "upsample_nearest": up, "scale_detections": sd}
    nbytes = {"letterbox_staged": lb.bytes, "letterbox_direct": lb.bytes, "letterbox_staged_resize": lbr.bytes, "letterbox_direct_resize": lbr.bytes,
              "upsample_nearest": up.bytes, "scale_detections": sd.bytes}
    cells = {"letterbox_staged": ("resize_null_staged", lb2, rn), "letterbox_direct": ("resize_null_direct", direct(lb2), direct(rn)),
             "letterbox_staged_resize": ("resize_null_staged_resize", lbr2, rnr),
             "letterbox_direct_resize": ("resize_null_direct_resize", direct(lbr2), direct(rnr))}
    for cell, (null, again, other) in cells.items():
        items[cell + "_again"], items[null] = again, other
        nbytes[cell + "_again"] = nbytes[null] = nbytes[cell]
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
    kern = {n: {"ms": median(v), "ms_min_max": [min(v), max(v)], "algorithmic_bytes": int(nbytes[n]),
                "GB_per_s": nbytes[n] / (median(v) * 1e-3) / 1e9} for n, v in times.items()}
    yard = kern["upsample_nearest"]["GB_per_s"]
    tile_ab = {}
    for cell, (null, _, _) in cells.items():
        ms, again, other = kern[cell]["ms"], kern[cell + "_again"]["ms"], kern[null]["ms"]
        tile_ab[cell] = {"letterbox_ms": ms, "letterbox_again_ms": again, "resize_null_ms": other, "limit_ms": ms + abs(ms - again),
                         "within": bool(other <= ms + abs(ms - again))}
    res = {"model": f"yolov5{a.model}_Transfusion_kaist", "dtype": a.dtype, "batch": B, "size": S, "frame": list(frame), "resize_frame": list(rframe),
           "device": ops.device_info(),
           "timing": f"kernels: HIP events around {a.inner} launches, median of {a.rounds} interleaved rounds after {a.warmup}; pipelines: wall clock "
                     f"around {a.steps} submits + synchronize, same rounds, interleaved",
           "kernels": kern, "tile_ab": tile_ab, "staged_default_by_budget_rule": [bool(ops.letterbox_staged(geom[0])), bool(ops.letterbox_staged(geomr[0]))],
           "staged_over_direct": kern["letterbox_direct"]["ms"] / kern["letterbox_staged"]["ms"],
           "staged_over_direct_resize": kern["letterbox_direct_resize"]["ms"] / kern["letterbox_staged_resize"]["ms"],
           "letterbox_over_yardstick": kern["letterbox_staged"]["GB_per_s"] / yard,
           "letterbox_resize_over_yardstick": kern["letterbox_staged_resize"]["GB_per_s"] / yard,
           "yardstick": "icaf_upsample_nearest, (B, 80, 80, 64) -> (B, 160, 160, 64) in the compute type"}

    # ---- (d): the host work that leaves the loop ------------------------------------------------------------------------------------
    torch.set_num_threads(1)
    g = np.random.default_rng(0)
    host = {}
    for tag, shape in (("frame", frame), ("resize_frame", rframe)):
        a0, b0 = (g.integers(0, 256, (*shape, 3), dtype=np.uint8) for _ in range(2))
        boxes = torch.rand((50, 4)) * S
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            x = D.letterbox(a0, S)[0]
            y = D.letterbox(b0, S)[0]
            np.concatenate((np.ascontiguousarray(x[:, :, ::-1].transpose(2, 0, 1)), np.ascontiguousarray(y[:, :, ::-1].transpose(2, 0, 1))), 0)
            scale_coords((S, S), boxes.clone(), shape).round()
            ts.append((time.perf_counter() - t0) * 1e3)
        host[tag] = {"ms_per_pair": median(ts), "pairs_per_s_one_thread": 1e3 / median(ts)}
    res["host_letterbox_plus_scale_coords"] = host

    # ---- (c): host-fed pipelines ----------------------------------------------------------------------------------------------------
    if not a.no_pipeline:
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
        kw = dict(conf_thres=0.25, iou_thres=0.45, depth=a.depth)
        pipes = {"submit_frames": DetectionPipeline(model(), B, S, S, dev, frames=frame, **kw),
                 "submit_u8": DetectionPipeline(model(), B, S, S, dev, u8=True, **kw),
                 "submit_u8_again": DetectionPipeline(model(), B, S, S, dev, u8=True, **kw)}
        nbuf = pipes["submit_u8"].nplans + 2
        gen = torch.Generator().manual_seed(3)
        frames_h = [tuple(torch.randint(0, 256, (B, *frame, 3), dtype=torch.uint8, generator=gen).pin_memory() for _ in range(2)) for _ in range(nbuf)]
        geom1, _ = ops.frame_geometry([frame], S)
        top, left, nh, nw = (int(geom1[0][k]) for k in ("top", "left", "nh", "nw"))
        assert (nh, nw) == frame, "the pre-letterboxed batches below are built for frames that are copied between pads"
        u8_h = []
        for rgb, ir in frames_h:                                        # the same pixels, letterboxed on the host ahead of time
            t = torch.full((B, 6, S, S), 114, dtype=torch.uint8)
            t[:, :3, top:top + nh, left:left + nw] = rgb.permute(0, 3, 1, 2).flip(1)
            t[:, 3:, top:top + nh, left:left + nw] = ir.permute(0, 3, 1, 2).flip(1)
            u8_h.append(t.pin_memory())

        def run(name, k0):
            p = pipes[name]
            for k in range(a.steps):
                if name == "submit_frames":
                    p.submit_frames(*frames_h[(k0 + k) % nbuf])
                else:
                    p.submit_u8(u8_h[(k0 + k) % nbuf])
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
        step_ms = B / med["submit_u8"] * 1e3
        res["pipeline"] = {"depth": a.depth, "nplans": pipes["submit_u8"].nplans, "pairs_per_s": med,
                           "pairs_per_s_min_max": {n: [min(v), max(v)] for n, v in rates.items()},
                           "aa_spread": abs(med["submit_u8"] - med["submit_u8_again"]) / med["submit_u8"],
                           "frames_over_u8": med["submit_frames"] / med["submit_u8"],
                           "letterbox_share_of_a_step": kern["letterbox_staged"]["ms"] / step_ms, "step_ms_submit_u8": step_ms,
                           "bytes_per_step": {"submit_frames": 2 * B * frame[0] * frame[1] * 3, "submit_u8": B * 6 * S * S}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
