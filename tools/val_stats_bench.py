#!/usr/bin/env python3
"""Device time of the validation statistics  ->  profiles/val_stats_bench.json

    python tools/val_stats_bench.py [--out profiles/val_stats_bench.json] [--repeats 50] [--groups 5] [--rounds 3]

Four measurements, nothing of which is a pass criterion:
  stage   icaf_stats_stage on a batch of 32 x 300 rows (every row below its count), device events around windows of `repeats` calls, twice
          per group: the second series is the A/A spread.
  ap      icaf_ap_per_class (ops.ap_per_class_device on device tensors, its result download included) at 5,939 / 675,600 / 1,048,576 rows
          with 1 and 3 classes, confidences on a 2^-16 lattice (ties), beside the numpy ap_per_class of utils/metrics.py on the same rows
          on the host; host clock around each call, device series twice (A/A).
  matrix  icaf_confusion_matrix on 32 images x 300 detections x 8 labels, device events.
  loop    root test() over 16 synthetic 512 x 640 pairs (tests/test_frontends.make_dataset) at batch 8, default path and device_stats=True
          alternating, host clock around the call; each variant twice per round, so the default / default difference is the A/A spread the
          other difference has to be read against."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.utils import metrics                                    # noqa: E402

T = 10


def window(fn, repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / repeats


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def aa(a, b):
    return round(abs(statistics.median(a) - statistics.median(b)), 4)


def stage_bench(dev, repeats, groups):
    g = torch.Generator().manual_seed(1)
    B, md = 32, 300
    correct = (torch.rand((B, md, T), generator=g) < 0.3).to(torch.uint8).to(dev)
    det = torch.rand((B, md, 6), generator=g).to(dev)
    count = torch.full((B,), md, dtype=torch.int32, device=dev)
    store = ops.StatsStore(B * md, T, dev)

    def call():
        store.state.zero_()
        store.stage(correct, det, count)
    call()
    a, b = [], []
    for _ in range(groups):
        a.append(window(call, repeats))
        b.append(window(call, repeats))
    return {"rows": B * md, "ms": stats(a), "ms_again": stats(b), "aa_spread_of_medians_ms": aa(a, b), "note": "one cursor reset (a memset) per call included"}


def ap_bench(dev, groups):
    out = []
    for n in (5939, 675600, 1048576):
        for nc in (1, 3):
            g = np.random.default_rng(n + nc)
            tp = np.logical_and.accumulate(g.random((n, T)) < np.linspace(0.6, 0.2, T)[None, :], 1)
            conf = (g.integers(1, 65536, n) / 65536.0).astype(np.float32)
            cls = g.integers(0, nc, n).astype(np.int32)
            tcls = g.integers(0, nc, max(n // 8, 1)).astype(np.float64)
            uc, n_l = np.unique(tcls, return_counts=True)
            mask = (tp.astype(np.uint16) << np.arange(T, dtype=np.uint16)[None, :]).sum(1).astype(np.uint16).view(np.int16)
            dev_in = (torch.from_numpy(mask).to(dev), torch.from_numpy(conf).to(dev), torch.from_numpy(cls).to(dev), n)

            def device():
                t0 = time.perf_counter()
                res = ops.ap_per_class_device(dev_in, uc, n_l, T=T)
                return (time.perf_counter() - t0) * 1e3, res

            def host():
                t0 = time.perf_counter()
                res = metrics.ap_per_class(tp, conf, cls.astype(np.float64), tcls)
                return (time.perf_counter() - t0) * 1e3, res
            device()
            a, b, h, res, ref = [], [], [], None, None
            for _ in range(groups):
                a.append(device()[0])
                ms, ref = host()
                h.append(ms)
                ms, res = device()
                b.append(ms)
            out.append({"rows": n, "classes": nc, "device_ms": stats(a), "device_ms_again": stats(b), "aa_spread_of_medians_ms": aa(a, b),
                        "numpy_ms": stats(h), "map50_device": float(res["ap"][:, 0].mean()), "map50_numpy": float(ref[5][:, 0].mean())})
            print(json.dumps(out[-1]))
    return out


def matrix_bench(dev, repeats, groups):
    g = torch.Generator().manual_seed(2)
    B, md, L = 32, 300, 8
    lab_xy = torch.rand((B * L, 2), generator=g) * 400
    labels = torch.cat((torch.randint(0, 3, (B * L, 1), generator=g).float(), lab_xy, lab_xy + 40 + torch.rand((B * L, 2), generator=g) * 80), 1)
    src = labels.view(B, L, 5)[:, torch.arange(md) % L, 1:]
    predn = (src + torch.randn((B, md, 4), generator=g) * 8).contiguous().to(dev)
    det = torch.cat((predn.cpu(), torch.rand((B, md, 1), generator=g), torch.randint(0, 3, (B, md, 1), generator=g).float()), 2).contiguous().to(dev)
    count = torch.full((B,), md, dtype=torch.int32, device=dev)
    off = (torch.arange(B + 1, dtype=torch.int32) * L).to(dev)
    m = torch.zeros((4, 4), dtype=torch.int32, device=dev)
    launch = ops.confusion_matrix(predn, det, count, labels.to(dev), off, m)
    sp = ops.current_stream_ptr()
    launch(sp)
    a, b = [], []
    for _ in range(groups):
        a.append(window(lambda: launch(sp), repeats))
        b.append(window(lambda: launch(sp), repeats))
    return {"images": B, "detections": md, "labels": L, "ms": stats(a), "ms_again": stats(b), "aa_spread_of_medians_ms": aa(a, b)}


def loop_bench(dev, rounds):
    from helpers import val_module
    from test_frontends import make_dataset
    from icafusion_amd.models.yolo import Model
    from icafusion_amd.synth import synth_state_dict
    val = val_module()
    with open(os.path.join(REPO, "models", "transformer", "yolov5s_Transfusion_kaist.yaml")) as f:
        cfg = yaml.safe_load(f)
    model = Model(cfg).eval()
    model.load_state_dict(synth_state_dict(model, 0))
    model = model.to(dev)
    model.compute_dtype, model.use_graph = torch.bfloat16, True
    with tempfile.TemporaryDirectory() as tmp:
        rgb_dir, ir_dir = make_dataset(os.path.join(tmp, "set"), n=16, size=(512, 640), nc=1, seed=1, mixed=False)
        data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 1, "names": ["person"]}

        def once(device_stats):
            t0 = time.perf_counter()
            res = val.test(data, batch_size=8, imgsz=640, conf_thres=0.001, model=model, device_stats=device_stats)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res[0][:4]
        once(False), once(True)                                   # plans, runners, file cache
        host_a, host_b, dev_a, dev_b = [], [], [], []
        for _ in range(rounds):
            host_a.append(once(False)[0])
            dev_a.append(once(True)[0])
            host_b.append(once(False)[0])
            dev_b.append(once(True)[0])
    return {"pairs": 16, "frame": [512, 640], "batch": 8, "batches": 2, "default_ms": stats(host_a), "default_ms_again": stats(host_b),
            "device_stats_ms": stats(dev_a), "device_stats_ms_again": stats(dev_b), "aa_spread_of_medians_ms": aa(host_a, host_b),
            "device_minus_default_ms": round(statistics.median(dev_a + dev_b) - statistics.median(host_a + host_b), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "val_stats_bench.json"))
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--groups", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_stats_bench measures on the MI355X only: no GPU found")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0),
              "what": "stage / matrix: ms per call over %d groups of %d calls, device events, each series twice (A/A); ap: ms per call, host clock, "
                      "%d groups of device / numpy / device; loop: ms per test() call, host clock, %d alternating rounds" % (o.groups, o.repeats, o.groups, o.rounds)}
    result["stage"] = stage_bench(dev, o.repeats, o.groups)
    print(json.dumps(result["stage"]))
    result["matrix"] = matrix_bench(dev, o.repeats, o.groups)
    print(json.dumps(result["matrix"]))
    result["ap"] = ap_bench(dev, o.groups)
    result["loop"] = loop_bench(dev, o.rounds)
    print(json.dumps(result["loop"]))
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", o.out)


if __name__ == "__main__":
    main()
