#!/usr/bin/env python3
"""Device time of confluence suppression on clustered synthetic scenes  ->  profiles/confluence_bench.json

    python tools/confluence_bench.py [--out profiles/confluence_bench.json] [--repeats 20]

For 48 / 320 / 1024 / 4096 candidates per image and B = 1 / 32 (icafusion_amd.synth.synth_crowd_prediction: one class, clusters of eight,
seeded) three launches are timed with device events around `repeats` back-to-back calls, after a warm-up, in several rounds whose minimum /
median / maximum are kept:
    confluence   icaf_confluence: candidate stage, chip-wide initial sweep, picks, compaction (ops.ConfluenceRunner)
    select       icaf_confluence_select on the same candidate lists: the workgroup of a class sweeps its own rows
    nms          icaf_nms on the same predictions (IoU 0.5, multi-label), the yardstick every validation pass already pays
Beside them: the reference's own CPU seconds for a scene of that many candidates, as recorded with the fixtures
(tests/golden/confluence/summary.json) — present for the sizes the reference finishes in seconds.  Nothing here is a pass criterion; the
file records what the kernels take."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.synth import synth_crowd_prediction                     # noqa: E402

SIZES, BATCHES, CONF, P_THRES = (48, 320, 1024, 4096), (1, 32), 0.1, 0.6


def timed(fn, repeats, rounds):
    """milliseconds per call: [min, median, max] over `rounds` windows of `repeats` calls each, device events around a window"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / repeats)
    return [round(min(out), 4), round(statistics.median(out), 4), round(max(out), 4)]


def candidate_block(pred, conf):
    """the candidate lists of the whole path, built on the host in the same order (one class: one candidate per row above the thresholds)"""
    B = pred.shape[0]
    lists = []
    for x in pred:
        x = x[x[:, 4] > np.float32(conf)]
        c = x[:, 5] * x[:, 4]
        half = x[:, 2:4] / np.float32(2)
        d = np.concatenate((x[:, :2] - half, x[:, :2] + half, c[:, None], np.zeros((len(x), 1), np.float32)), 1)[c > np.float32(conf)]
        lists.append(d.astype(np.float32))
    cap = max(len(d) for d in lists)
    cand = np.zeros((B, cap, 6), np.float32)
    for b, d in enumerate(lists):
        cand[b, :len(d)] = d
    return cand, np.array([len(d) for d in lists], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "confluence_bench.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("confluence_bench measures on the MI355X only: no GPU found")
    dev = "cuda:0"
    with open(os.path.join(REPO, "tests", "golden", "confluence", "summary.json")) as f:
        recorded = {v["n"]: v["reference_seconds"] for k, v in json.load(f)["select"].items() if k.startswith("crowd") and v["nc"] == 1}
    rows = []
    for n in SIZES:
        for B in BATCHES:
            pred = synth_crowd_prediction(B, 25200, n, nc=1, seed=n)             # the decoded rows of a 640 x 640 input
            t = torch.from_numpy(pred).to(dev)
            cand_np, n_np = candidate_block(pred, CONF)
            assert (n_np == n).all()
            cand, nn = torch.from_numpy(cand_np).to(dev), torch.from_numpy(n_np).to(dev)
            runner = ops.ConfluenceRunner(B, t.shape[1], 1, dev, max_cand=n, want_keep=False)
            nms = ops.NmsRunner(B, t.shape[1], 1, dev, multi_label=True, max_det=300, want_keep=False)
            det = torch.zeros((B, n, 6), device=dev)
            count = torch.zeros((B,), dtype=torch.int32, device=dev)
            _, c1, _ = runner.launch(t, CONF, P_THRES)
            _, c2, _ = ops.confluence_select(cand, nn, 1, P_THRES, det=det, count=count, want_keep=False)
            assert torch.equal(c1, c2) and torch.equal(runner.det, det)                 # the two paths agree before anything is timed
            row = {"candidates_per_image": n, "batch": B, "prediction_rows": int(t.shape[1]), "kept_per_image_mean": round(float(c1.float().mean()), 2),
                   "confluence_ms": timed(lambda: runner.launch(t, CONF, P_THRES), o.repeats, o.rounds),
                   "select_ms": timed(lambda: ops.confluence_select(cand, nn, 1, P_THRES, det=det, count=count, want_keep=False), o.repeats, o.rounds),
                   "nms_ms": timed(lambda: nms.launch(t, CONF, 0.5), o.repeats, o.rounds),
                   "reference_cpu_seconds_per_image": recorded.get(n)}
            rows.append(row)
            print(json.dumps(row))
    result = {"device": torch.cuda.get_device_name(0), "what": "ms per launch [min, median, max] over %d windows of %d calls, device events" % (o.rounds, o.repeats),
              "scene": "synth_crowd_prediction: one class, clusters of 8, conf_thres %g, p_thres %g" % (CONF, P_THRES), "rows": rows}
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", o.out)


if __name__ == "__main__":
    main()
