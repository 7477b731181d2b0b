#!/usr/bin/env python3
"""Cost of VALIDATING from native frames (test.py --device-letterbox; Model.forward_frames(val_size=...)) on the GPU.

    python tools/val_frames_bench.py [--batch 32 --frame 1024x1280 --size 640 --rounds 30 --pairs 16 --out profiles/val_frames_bench.json]

One process, items interleaved round by round in a rotating order, medians reported (the method of tools/frames_bench.py):
  (a) kernel rate: icaf_resize_frames in mode 1 on --batch pairs of --frame frames shrunk to --size on their longest side, into the
      loader's rectangular batch shape (LLVIP: 1024x1280 -> 512x640 into 544x672), on its staged and its direct path, a SECOND copy of the
      staged item for the A/A spread, in us and TB/s of algorithmic bytes (frames read once, planes written once).  Two yardsticks in the
      same rounds: icaf_upsample_nearest at a comparable byte volume (the project's streaming yardstick) and icaf_letterbox_frames doing
      the bilinear shrink of the same frames.
  (b) validation loop: test() over --pairs synthetic pairs of such frames written by the tool, host path against device_letterbox=True
      (and the host path a second time: A/A), wall clock per run; and the pieces per pair — decode, host resize (resize_area + letterbox
      on one CPU thread), upload of the native pair against upload of the resized batch item, kernel."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np   # noqa: E402
import torch         # noqa: E402
import yaml          # noqa: E402

from helpers import val_module                                    # noqa: E402
from icafusion_amd import ops                                     # noqa: E402
from icafusion_amd.models.yolo import Model                       # noqa: E402
from icafusion_amd.synth import synth_state_dict                  # noqa: E402
from icafusion_amd.utils import datasets as D                     # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def rect_shape(h0, w0, img_size, stride=32, pad=0.5):
    ar = h0 / w0
    s = [ar, 1.0] if ar < 1 else [1.0, 1.0 / ar] if ar > 1 else [1.0, 1.0]
    return tuple(int(v) for v in np.ceil(np.array(s) * img_size / stride + pad).astype(np.int64) * stride)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="s"); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640); ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--frame", default="1024x1280")
    ap.add_argument("--rounds", type=int, default=30); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="launches inside one event pair")
    ap.add_argument("--pairs", type=int, default=16, help="pairs of the synthetic validation set"); ap.add_argument("--val-batch", type=int, default=8)
    ap.add_argument("--val-rounds", type=int, default=3); ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_frames_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "val_frames_bench.py measures on the GPU only"
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    B, S = a.batch, a.size
    frame = tuple(int(v) for v in a.frame.split("x"))
    out_shape = rect_shape(*frame, S)
    sp = ops.current_stream_ptr()

    # ---- (a): kernels alone ---------------------------------------------------------------------------------------------------------
    geom1, mode1, _ = ops.val_geometry([frame] * B, S, out_shape)
    geom, mode = np.concatenate((geom1, geom1)), np.concatenate((mode1, mode1))
    end = ops.pack_frames(geom, 3)
    arena = torch.randint(0, 256, (end,), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    tab, mdev = ops.geom_tensor(geom, dev), torch.from_numpy(mode).to(dev)

    def planes():
        return torch.zeros((B, 6, *out_shape), dtype=torch.uint8, device=dev)
    area, area2 = (ops.resize_frames(arena, geom, mdev, tab, planes(), mode=mode) for _ in range(2))
    bil = ops.letterbox_frames(arena, geom, tab, planes())
    up = ops.upsample_nearest(torch.randn((2 * B, 80, 80, 64), device=dev).to(dt), torch.empty((2 * B, 160, 160, 64), dtype=dt, device=dev), 2)

    def direct(launch):
        def run(s):
            with ops.area_direct(True):
                launch(s)
        return run
    items = {"area_staged": area, "area_direct": direct(area), "area_staged_again": area2, "letterbox_bilinear_shrink": bil, "upsample_nearest": up}
    nbytes = {"area_staged": area.bytes, "area_direct": area.bytes, "area_staged_again": area2.bytes, "letterbox_bilinear_shrink": bil.bytes,
              "upsample_nearest": up.bytes}
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
                "TB_per_s": nbytes[n] / (median(v) * 1e-3) / 1e12} for n, v in times.items()}
    yard = kern["upsample_nearest"]["TB_per_s"]
    res = {"dtype": a.dtype, "batch": B, "size": S, "frame": list(frame), "batch_shape": list(out_shape),
           "resized": [int(geom[0]["nh"]), int(geom[0]["nw"])], "device": ops.device_info(),
           "timing": f"kernels: HIP events around {a.inner} launches, median of {a.rounds} interleaved rounds after {a.warmup}; loop: wall clock "
                     f"around test(), median of {a.val_rounds} interleaved rounds after one",
           "kernels": kern, "staged_default_by_budget_rule": bool(ops.area_staged(geom[0])),
           "aa_spread": abs(kern["area_staged"]["us"] - kern["area_staged_again"]["us"]) / kern["area_staged"]["us"],
           "direct_over_staged": kern["area_direct"]["us"] / kern["area_staged"]["us"],
           "area_over_yardstick": kern["area_staged"]["TB_per_s"] / yard,
           "area_direct_over_yardstick": kern["area_direct"]["TB_per_s"] / yard,
           "bilinear_shrink_over_yardstick": kern["letterbox_bilinear_shrink"]["TB_per_s"] / yard,
           "yardstick": f"icaf_upsample_nearest, ({2 * B}, 80, 80, 64) -> ({2 * B}, 160, 160, 64) in the compute type"}

    # ---- (b): the validation loop -----------------------------------------------------------------------------------------------------
    if not a.no_loop:
        val = val_module()
        torch.set_num_threads(1)
        with tempfile.TemporaryDirectory() as td:
            g = np.random.default_rng(0)
            for mod in ("visible", "infrared", "labels"):
                os.makedirs(os.path.join(td, mod, "test"))
            for i in range(a.pairs):
                for mod in ("visible", "infrared"):
                    D.imwrite_bgr(os.path.join(td, mod, "test", f"im{i:03d}.png"), g.integers(0, 256, (*frame, 3), dtype=np.uint8))
                k = int(g.integers(1, 5))
                lab = np.concatenate((np.zeros((k, 1), np.float32), g.uniform(0.2, 0.8, (k, 2)), g.uniform(0.1, 0.3, (k, 2))), 1)
                np.savetxt(os.path.join(td, "labels", "test", f"im{i:03d}.txt"), lab, fmt="%g")
            rgb_dir, ir_dir = os.path.join(td, "visible", "test"), os.path.join(td, "infrared", "test")
            data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 1, "names": ["person"]}
            cfg = yaml.safe_load(open(os.path.join(ROOT, "models", "transformer", f"yolov5{a.model}_Transfusion_kaist.yaml")))
            m = Model(cfg, nc=1).eval()
            m.load_state_dict(synth_state_dict(m, 0))
            m = m.to(dev)
            m.compute_dtype, m.use_graph, m.autotune = dt, True, False

            def loop(flag):
                with contextlib.redirect_stdout(io.StringIO()):
                    return val.test(data, batch_size=a.val_batch, imgsz=S, model=m, device_letterbox=flag)[0]
            runs = {"host": False, "device_letterbox": True, "host_again": False}
            rn = list(runs)
            wall = {n: [] for n in rn}
            first = {}
            for r in range(1 + a.val_rounds):
                for k in range(len(rn)):
                    n = rn[(k + r) % len(rn)]
                    t0 = time.perf_counter()
                    first.setdefault(n, loop(runs[n]))
                    if r >= 1:
                        wall[n].append(time.perf_counter() - t0)
            med = {n: median(v) for n, v in wall.items()}
            # the pieces, per pair
            files = sorted(os.listdir(rgb_dir))[:4]

            def per_pair(fn, reps=3):
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    for f in files:
                        fn(f)
                    ts.append((time.perf_counter() - t0) / len(files) * 1e3)
                return median(ts)
            pair = {f: (D.imread_bgr(os.path.join(rgb_dir, f)), D.imread_bgr(os.path.join(ir_dir, f))) for f in files}

            def host_resize(f):
                out = []
                for x in pair[f]:
                    x = D.resize_area(x, (int(geom[0]["nw"]), int(geom[0]["nh"])))
                    x = D.letterbox(x, out_shape, auto=False, scaleup=False)[0]
                    out.append(np.ascontiguousarray(x[:, :, ::-1].transpose(2, 0, 1)))
                return np.concatenate(out, 0)
            item = torch.from_numpy(host_resize(files[0]))
            nat = [torch.from_numpy(x) for x in pair[files[0]]]

            def upload(ts):
                def fn(_):
                    for t in ts:
                        t.to(dev)
                    torch.cuda.synchronize()
                return fn
            res["validation_loop"] = {
                "pairs": a.pairs, "batch": a.val_batch, "model": f"yolov5{a.model}_Transfusion_kaist", "seconds_per_run": med,
                "seconds_min_max": {n: [min(v), max(v)] for n, v in wall.items()},
                "aa_spread": abs(med["host"] - med["host_again"]) / med["host"], "host_over_device": med["host"] / med["device_letterbox"],
                "same_metrics": bool(first["host"] == first["device_letterbox"]),
                "ms_per_pair": {"decode": per_pair(lambda f: (D.imread_bgr(os.path.join(rgb_dir, f)), D.imread_bgr(os.path.join(ir_dir, f)))),
                                "host_resize_one_thread": per_pair(host_resize),
                                "upload_native_pair": per_pair(upload(nat), 5), "upload_resized_item": per_pair(upload([item]), 5),
                                "kernel": kern["area_staged"]["us"] * 1e-3 / B}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
