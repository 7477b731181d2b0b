#!/usr/bin/env python3
"""Device time of the validation loss  ->  profiles/val_loss_bench.json

    python tools/val_loss_bench.py [--out profiles/val_loss_bench.json] [--repeats 200] [--groups 7]

Two measurements, nothing of which is a pass criterion:
  call   icaf_loss (ops.LossRunner) at the KAIST validation shape — B = 32 at 544 x 672 (maps 68 x 84, 34 x 42, 17 x 21), nc = 1, 100 seeded
         targets — beside the same loss written with torch ops on the same GPU (tests/loss_ref.py on device tensors: index gathers, a
         boolean-mask compaction and its host syncs included).  One interleaved loop: every group times `repeats` calls of the kernel path,
         the same again (the A/A spread), then `repeats / 4` calls of the torch formulation, device events around each window; the median,
         minimum and maximum over the groups are kept.  The two agree on the four items before anything is timed.
  loop   root test() over 16 synthetic 512 x 640 pairs (tests/test_frontends.make_dataset) at batch 8, without and with the loss built as
         `--hyp` builds it, alternating, host clock around the call (it ends in device-to-host copies); each variant twice per round, so
         the plain / plain difference is the A/A spread the with / without difference has to be read against.
Bytes: the objectness term needs one fp32 logit per cell and reads, through the stride of `no` floats, every cache line of the maps."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.utils import loss as L                                  # noqa: E402
import loss_ref                                                            # noqa: E402

B, SHAPES, NA, NC, NT = 32, [(68, 84), (34, 42), (17, 21)], 3, 1, 100
ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
HYP = os.path.join(REPO, "tests", "golden", "loss", "hyp.scratch.yaml")


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


def call_bench(dev, repeats, groups):
    g = torch.Generator().manual_seed(7)
    maps = [(torch.randn((B, NA, ny, nx, 5 + NC), generator=g) * 1.5).to(dev) for ny, nx in SHAPES]
    t = torch.rand((NT, 6), generator=g)
    t[:, 0] = torch.randint(0, B, (NT,), generator=g).float().sort()[0]
    t[:, 1] = 0
    t[:, 4:6] = t[:, 4:6] * 0.3 + 0.03
    targets = t.to(dev)
    anchors = torch.tensor(ANCHORS, dtype=torch.float32).view(3, 3, 2) / torch.tensor([8.0, 16.0, 32.0]).view(3, 1, 1)
    with open(HYP) as f:
        prm = L.loss_params(L.scale_hyp(yaml.safe_load(f), 3, NC, 640), 1.0, 3)
    runner = ops.LossRunner(B, SHAPES, NA, NC, anchors, dev)
    anchors_dev = anchors.to(dev)

    def kernel():
        return runner.launch(maps, targets, prm)

    def torch_ops():
        return loss_ref.compute(maps, targets, anchors_dev, prm)["items"]
    got, want = kernel()[0].double().cpu(), torch_ops().cpu()
    assert torch.allclose(got, want, rtol=1e-6, atol=0.0), (got, want)
    for _ in range(5):
        kernel(), torch_ops()
    torch.cuda.synchronize()
    ka, kb, tt = [], [], []
    for _ in range(groups):
        ka.append(window(kernel, repeats))
        kb.append(window(kernel, repeats))
        tt.append(window(torch_ops, max(repeats // 4, 1)))
    cells = sum(B * NA * ny * nx for ny, nx in SHAPES)
    no = 5 + NC
    med = statistics.median(ka)
    return {"shape": {"B": B, "maps": SHAPES, "na": NA, "nc": NC, "targets": NT, "matches_per_level": runner.counts.tolist()},
            "items": got.tolist(), "icaf_loss_ms": stats(ka), "icaf_loss_ms_again": stats(kb),
            "aa_spread_of_medians": round(abs(statistics.median(ka) - statistics.median(kb)) / statistics.median(ka), 4),
            "torch_ops_ms": stats(tt), "torch_ops_over_icaf_loss": round(statistics.median(tt) / med, 2),
            "objectness_bytes_needed": cells * 4, "objectness_bytes_touched": cells * no * 4, "tobj_bytes": cells * 4,
            "map_bytes_over_median_GBps": round(cells * no * 4 / (med * 1e-3) / 1e9, 1)}


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
        cl = val.loss_from_hyp(HYP, model, 1, 640)

        def once(with_loss):
            t0 = time.perf_counter()
            res = val.test(data, batch_size=8, imgsz=640, conf_thres=0.25, model=model, compute_loss=cl if with_loss else None)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res[0][4:]
        once(False), once(True)                                   # plans, runners, file cache
        plain_a, plain_b, loss_a, loss_b, items = [], [], [], [], None
        for _ in range(rounds):
            plain_a.append(once(False)[0])
            ms, items = once(True)
            loss_a.append(ms)
            plain_b.append(once(False)[0])
            loss_b.append(once(True)[0])
    return {"pairs": 16, "frame": [512, 640], "batch": 8, "batches": 2, "loss": list(items), "plain_ms": stats(plain_a), "plain_ms_again": stats(plain_b),
            "with_loss_ms": stats(loss_a), "with_loss_ms_again": stats(loss_b),
            "aa_spread_of_medians_ms": round(abs(statistics.median(plain_a) - statistics.median(plain_b)), 3),
            "with_minus_without_ms": round(statistics.median(loss_a + loss_b) - statistics.median(plain_a + plain_b), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "val_loss_bench.json"))
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    o = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("val_loss_bench measures on the MI355X only: no GPU found")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0),
              "what": "call: ms per call over %d groups of %d calls (torch formulation: %d), device events, kernel / kernel / torch interleaved; "
                      "loop: ms per test() call, host clock, %d alternating rounds" % (o.groups, o.repeats, max(o.repeats // 4, 1), o.rounds),
              "call": call_bench(dev, o.repeats, o.groups)}
    print(json.dumps(result["call"]))
    result["loop"] = loop_bench(dev, o.rounds)
    print(json.dumps(result["loop"]))
    os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
    with open(o.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", o.out)


if __name__ == "__main__":
    main()
