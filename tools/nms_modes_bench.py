#!/usr/bin/env python3
"""Device time of the two NMS modes beside plain NMS  ->  profiles/nms_modes_bench.json

    python tools/nms_modes_bench.py [--out profiles/nms_modes_bench.json] [--repeats 10] [--groups 7]
                                    [--bench-this LINE.json ...] [--bench-parent LINE.json ...]

B = 32 images of 25 200 rows (the decoded rows of a 640 x 640 input), nc = 1 and 3, 48 / 320 / 1 024 / 2 999 candidates per image
(icafusion_amd.synth.synth_crowd_prediction: clusters of eight, seeded).  Timed per size, with device events around `repeats` back-to-back
launches, in `groups` INTERLEAVED groups (plain, plain again, labels, merge, torch — then the next group) whose medians are reported:
    nms          icaf_nms (ops.NmsRunner as every caller builds it)
    nms_again    the same launch a second time per group: the A/A series, |median difference| / median is the spread of this run
    labels       icaf_nms_ex with 8 apriori labels per image
    merge        icaf_nms_ex with merge-NMS (redundant)
    torch_merge  the torch-ops statement of utils/general.py:594-600 (box_iou, the weight matrix, torch.mm, the redundancy filter) on the same
                 GPU, per image on the candidate lists and kept indices already on the device — what the merge kernel replaces; the
                 candidate stage and the greedy walk are NOT in this figure
`--bench-this` / `--bench-parent`: result lines of `bench.py --full` runs of this tree and of its parent commit made in the same call on
the same machine; their NMS-alone figure and pairs/s are recorded side by side with the spread of a tree's own runs (the plain path must not
get slower).  `--append-call` adds the lines of a further call to an existing file without measuring anything.  Nothing here is a pass
criterion; the file records what was measured."""
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
from icafusion_amd.utils.general import box_iou                            # noqa: E402

SIZES, NCS, B, ROWS, CONF, IOU, NLAB = (48, 320, 1024, 2999), (1, 3), 32, 25200, 0.1, 0.5, 8


def window(fn, repeats):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / repeats


def interleaved(fns, repeats, groups):
    """{name: [min, median, max] ms per call} over `groups` rounds that visit every function once, in order"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(groups):
        for k, fn in fns.items():
            out[k].append(window(fn, repeats))
    return {k: [round(min(v), 4), round(statistics.median(v), 4), round(max(v), 4)] for k, v in out.items()}


def candidate_lists(pred, nc, dev):
    """per image (x (n, 6) xyxy conf cls, class-offset boxes) on the device, multi-label order — the inputs of the torch statement"""
    out = []
    for x in pred:
        x = x[x[:, 4] > np.float32(CONF)]
        c = x[:, 5:] * x[:, 4:5]
        half = x[:, 2:4] / np.float32(2)
        box = np.concatenate((x[:, :2] - half, x[:, :2] + half), 1)
        i, j = np.nonzero(c > np.float32(CONF)) if nc > 1 else (np.nonzero(c[:, 0] > np.float32(CONF))[0], None)
        j = np.zeros(len(i), np.int64) if j is None else j
        d = torch.from_numpy(np.concatenate((box[i], c[i, j][:, None], j[:, None].astype(np.float32)), 1).astype(np.float32)).to(dev)
        out.append((d, d[:, :4] + d[:, 5:6] * 4096.0))
    return out


def torch_merge(cands, keeps):
    res = []
    for (x, boxes), i in zip(cands, keeps):
        x = x.clone()
        scores = x[:, 4]
        iou = box_iou(boxes[i], boxes) > IOU
        weights = iou * scores[None]
        x[i, :4] = torch.mm(weights, x[:, :4]).float() / weights.sum(1, keepdim=True)
        res.append(x[i[iou.sum(1) > 1]])
    return res


def bench_lines(paths):
    rows = []
    for p in paths or ():
        with open(p) as f:
            line = [l for l in f.read().splitlines() if l.startswith("{")][-1]
        d = json.loads(line)
        rows.append({"file": os.path.basename(p), "pairs_per_s": d.get("value"), "nms_ms_per_batch_standalone": d.get("nms_ms_per_batch_standalone")})
    return rows


def plain_call(this_paths, parent_paths, label):
    """one entry of plain_path.calls: the bench.py lines of both trees from ONE call, their medians and the spread of a tree's own runs"""
    def summary(rows):
        v, n = [r["pairs_per_s"] for r in rows], [r["nms_ms_per_batch_standalone"] for r in rows]
        return {"pairs_per_s_median": statistics.median(v), "pairs_per_s_range": [min(v), max(v)], "nms_ms_median": statistics.median(n),
                "nms_ms_range": [min(n), max(n)]}
    t, p = bench_lines(this_paths), bench_lines(parent_paths)
    st, sp = summary(t), summary(p)
    spread = {k: round((s["pairs_per_s_range"][1] - s["pairs_per_s_range"][0]) / s["pairs_per_s_median"], 5) for k, s in (("this", st), ("parent", sp))}
    return {"call": label, "this_commit": t, "parent_commit": p, "this_summary": st, "parent_summary": sp,
            "pairs_per_s_this_over_parent": round(st["pairs_per_s_median"] / sp["pairs_per_s_median"], 5), "aa_spread_pairs_per_s": spread}


PLAIN_NOTE = {"command": "bench.py --gpus 1 --steps 50 --warmup 10 --full --no-cpu-baseline --no-latency, alternating pairs, both trees in the same call on the same machine",
              "device_code": "nms_keys_kernel / nms_walk_kernel<false> / nms_rank_kernel: same VGPR / SGPR / spill / LDS figures as the parent's kernels "
                             "(kernel_resources.json of both builds)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nms_modes_bench.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--bench-this", nargs="*", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=None)
    ap.add_argument("--call-label", default="call 1", help="name of the plain_path entry the --bench-* lines become")
    ap.add_argument("--append-call", action="store_true", help="measure nothing: add the --bench-* lines of a further call to the existing --out file")
    o = ap.parse_args()
    if o.append_call:
        with open(o.out) as f:
            result = json.load(f)
        result["plain_path"]["calls"].append(plain_call(o.bench_this, o.bench_parent, o.call_label))
        with open(o.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("nms_modes_bench measures on the MI355X only: no GPU found")
    dev = "cuda:0"
    rows = []
    for nc in NCS:
        for n in SIZES:
            pred = synth_crowd_prediction(B, ROWS, n, nc=nc, seed=n + nc)
            t = torch.from_numpy(pred).to(dev)
            g = np.random.default_rng(n)
            labels = [np.concatenate((g.integers(0, nc, (NLAB, 1)), g.uniform(60, 560, (NLAB, 2)), g.uniform(20, 120, (NLAB, 2))), 1).astype(np.float32)
                      for _ in range(B)]
            table, off, _ = ops.nms_label_table(labels, B, nc, NLAB, device=dev)
            plain = ops.NmsRunner(B, ROWS, nc, dev, multi_label=True)
            lab = ops.NmsRunner(B, ROWS, nc, dev, multi_label=True, max_labels=NLAB)
            mrg = ops.NmsRunner(B, ROWS, nc, dev, multi_label=True, merge=True)
            _, count, keep = plain.launch(t, CONF, IOU)
            torch.cuda.synchronize()
            cands = candidate_lists(pred, nc, dev)
            keeps = [keep[b, :int(count[b])].long() for b in range(B)]
            _, mcount, _ = mrg.launch(t, CONF, IOU)
            tm = torch_merge(cands, keeps)
            same = [len(r) for r in tm] == mcount.tolist()                        # do the two statements keep the same boxes?  (recorded, not asserted)
            err = max([float((r[:, :4] - mrg.det[b, :len(r), :4]).abs().max()) for b, r in enumerate(tm) if len(r)] + [0.0]) if same else None
            fns = {"nms": lambda: plain.launch(t, CONF, IOU), "nms_again": lambda: plain.launch(t, CONF, IOU),
                   "labels": lambda: lab.launch(t, CONF, IOU, labels=table, label_off=off), "merge": lambda: mrg.launch(t, CONF, IOU),
                   "torch_merge": lambda: torch_merge(cands, keeps)}
            ms = interleaved(fns, o.repeats, o.groups)
            row = {"nc": nc, "candidates_per_image": [int(len(c[0])) for c in cands][:2] + ["..."], "planted_rows_per_image": n, "batch": B,
                   "prediction_rows": ROWS, "kept_per_image_mean": round(float(count.float().mean()), 2),
                   "kept_after_merge_mean": round(float(mcount.float().mean()), 2), "torch_keeps_the_same_boxes": same, "merge_max_abs_diff_to_torch": err,
                   "aa_spread": round(abs(ms["nms"][1] - ms["nms_again"][1]) / ms["nms"][1], 4), **{k + "_ms": v for k, v in ms.items()}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0),
              "what": "ms per launch [min, median, max] over %d interleaved groups of %d calls, device events; B = %d" % (o.groups, o.repeats, B),
              "scene": "synth_crowd_prediction: clusters of 8, conf_thres %g, iou_thres %g, multi-label, %d labels per image" % (CONF, IOU, NLAB),
              "rows": rows, "plain_path": dict(PLAIN_NOTE, calls=[plain_call(o.bench_this, o.bench_parent, o.call_label)] if o.bench_this else [])}
    os.makedirs(os.path.dirname(o.out), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", o.out)


if __name__ == "__main__":
    main()
