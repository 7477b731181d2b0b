#!/usr/bin/env python3
"""Cost of the KAIST miss-rate evaluation (test.py --miss-rate; tools/kaist_mr.py) on the GPU.

    python tools/kaist_mr_bench.py [--rounds 30 --inner 20 --out profiles/kaist_mr_bench.json]

One process, items interleaved round by round in a rotating order, HIP event pairs around --inner launches, medians reported (the method
of tools/frames_bench.py):
  match_mlpd / match_mlpd_again   icaf_missrate_match on the reference's MLPD result file (2,252 images, 5,939 rows); the second copy of
                                  the same item gives the A/A spread
  match_2252x300                  the same launch on a synthetic store at the validation protocol's worst case: 300 detections on every
                                  one of the 2,252 images (boxes scattered over the image's labels and over the frame, seeded)
  stage_b32                       icaf_missrate_stage of one batch of 32 images x 300 rows
  accumulate_*                    the host half (utils.missrate.summarize: nine FPPI sweeps in numpy), wall clock on this host's CPU
Beside them, for context and NOT measured here: the wall time of the reference's pure-Python evaluator on the CPU that generated the
fixtures (tests/golden/kaist_mr/summary.json)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402

from icafusion_amd import ops                  # noqa: E402
from icafusion_amd.utils import missrate       # noqa: E402

MR_DIR = os.path.join(ROOT, "tests", "golden", "kaist_mr")


def median(v):
    return sorted(v)[len(v) // 2]


def synthetic_store(table, per_image, seed):
    """per_image detections on every image: two thirds jittered copies of the image's labels (where it has any), the rest anywhere in
    the 640 x 512 frame; distinct scores."""
    g = np.random.default_rng(seed)
    I = len(table["image_id"])
    dt = np.zeros((I, per_image, 5))
    dt[:, :, 0], dt[:, :, 1] = g.uniform(0, 600, (I, per_image)), g.uniform(0, 450, (I, per_image))
    dt[:, :, 2], dt[:, :, 3] = g.uniform(10, 60, (I, per_image)), g.uniform(20, 120, (I, per_image))
    dt[:, :, 4] = g.permuted(np.tile(np.linspace(0.001, 0.999, per_image), (I, 1)), axis=1)
    for i in range(I):
        a, b = table["off"][i], table["off"][i + 1]
        if b > a:
            k = 2 * per_image // 3
            dt[i, :k, :4] = table["box"][a + g.integers(0, b - a, k)] + g.normal(0, 3, (k, 4))
    return dt, np.full(I, per_image, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="launches inside one event pair")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kaist_mr_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kaist_mr_bench.py measures on the GPU only"
    dev = "cuda:0"
    table = missrate.load_annotations(os.path.join(MR_DIR, "KAIST_annotation.json.gz"))
    tab = ops.missrate_table(table, dev)
    image, rows = missrate.read_result_txt(os.path.join(MR_DIR, "MLPD_result.txt.gz"))
    stores = {"mlpd": missrate.pack_detections(tab.images, image, rows), "2252x300": synthetic_store(table, 300, 0)}
    dev_store = {k: (torch.from_numpy(d).to(dev), torch.from_numpy(c).to(dev)) for k, (d, c) in stores.items()}
    outs = {k: ops.missrate_outputs(tab, d.shape[1], dev) for k, (d, _) in dev_store.items()}
    B, max_det = 32, 300
    g = torch.Generator(device="cpu").manual_seed(0)
    predn = (torch.rand((B, max_det, 4), generator=g) * 500).to(dev)
    det = torch.rand((B, max_det, 6), generator=g).to(dev)
    count = torch.full((B,), max_det, dtype=torch.int32, device=dev)
    index = list(range(100, 100 + B))
    index_dev = torch.tensor(index, dtype=torch.int32, device=dev)
    stage_dt, stage_cnt = torch.zeros((tab.images, max_det, 5), dtype=torch.float64, device=dev), torch.zeros((tab.images,), dtype=torch.int32, device=dev)
    items = {
        "match_mlpd": ops.missrate_match(tab, *dev_store["mlpd"], *outs["mlpd"]),
        "match_mlpd_again": ops.missrate_match(tab, *dev_store["mlpd"], *outs["mlpd"]),
        "match_2252x300": ops.missrate_match(tab, *dev_store["2252x300"], *outs["2252x300"]),
        "stage_b32": ops.missrate_stage(predn, det, count, index, index_dev, stage_dt, stage_cnt),
    }
    s = ops.current_stream_ptr()
    times = {k: [] for k in items}
    names = list(items)
    for r in range(a.warmup + a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                items[k](s)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inner": a.inner, "unit": "us per launch (median of rounds)"}
    for k, v in times.items():
        res[k] = {"median_us": round(median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    res["aa_spread_percent"] = round(abs(res["match_mlpd"]["median_us"] / res["match_mlpd_again"]["median_us"] - 1) * 100, 2)
    res["detections"] = {k: int(c.sum()) for k, (_, c) in stores.items()}
    for k, (d, c) in stores.items():                        # the host half, on the arrays of the launches above
        order, dt_gt, dt_ignore, gt_ignore = (o.cpu().numpy() for o in outs[k])
        wall = []
        for _ in range(5):
            t0 = time.perf_counter()
            mr = missrate.summarize(table, c, missrate.sorted_scores(d, order, c), dt_gt, dt_ignore, gt_ignore[:tab.labels])
            wall.append(time.perf_counter() - t0)
        res["accumulate_" + k] = {"median_ms": round(median(wall) * 1e3, 2), "MR_all_percent": round(mr["all"] * 100, 4)}
    with open(os.path.join(MR_DIR, "summary.json")) as f:
        ref = json.load(f)
    res["reference_evaluator_cpu_wall_s (recorded with the fixtures, another machine's CPU)"] = {
        k: round(v["evaluator_wall_s"], 2) for k, v in ref.items() if k != "synth"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
