#!/usr/bin/env python3
"""Cost of a test-time-augmentation step (Model.forward(augment=True)) against the three plain forwards it is made of, resident on the GPU.

    python tools/tta_bench.py [--model s --batch 32 --size 640 --dtype bf16 --rounds 40 --out profiles/tta_bench.json]

Everything is timed with HIP event pairs around `--inner` back-to-back replays, the items interleaved round by round in a rotating order
(one process, one call: the numbers share the machine's state), medians reported:
  tta_step              stage -> the three plans' hipGraphs -> merge (engine.TtaPlan.run)
  forward_<H>x<W>       each plain plan alone
  tta_stage / tta_merge the two new kernels alone, with their algorithmic bytes (source read once, every output written once) over the time
  upsample_nearest      the yardstick, icaf_upsample_nearest: the head's own launch and one of the staging kernel's byte volume
The igemm configurations come from profiles/tune_cache.json; layers it does not cover (the scaled sizes) are tuned on the spot, and the
result records how many launches of each plan took their configuration from the committed cache."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch   # noqa: E402
import yaml    # noqa: E402

from icafusion_amd import ops                                     # noqa: E402
from icafusion_amd.models.yolo import Model                       # noqa: E402
from icafusion_amd.synth import synth_images, synth_state_dict    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="s"); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640); ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--rounds", type=int, default=40); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=3, help="replays inside one event pair")
    ap.add_argument("--no-autotune", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tta_bench.py measures on the GPU only"
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    cfg = yaml.safe_load(open(os.path.join(ROOT, "models", "transformer", f"yolov5{a.model}_Transfusion_kaist.yaml")))
    m = Model(cfg).eval()
    m.load_state_dict(synth_state_dict(m, 0))
    m = m.to(dev)
    m.compute_dtype, m.use_graph, m.autotune, m.static_outputs = dt, True, not a.no_autotune, True
    cache = os.path.join(ROOT, "profiles", "tune_cache.json")
    if m.autotune and os.path.exists(cache):
        ops.load_tune_cache(cache)
    committed = set(ops._TUNE_CACHE)
    B, H, W = a.batch, a.size, a.size
    tp = m.tta_plan_for(B, H, W, dev)
    rgb, ir = synth_images(B, H, W, 0)
    tp.inputs[0].copy_(rgb.to(dev)); tp.inputs[1].copy_(ir.to(dev))
    conv = ops.lib().icaf_conv2d
    configs = []
    for p, (s, f, hr, wr, hp, wp) in zip(tp.plans, tp.passes):
        convs = [l for l in p.launches if l.fn is conv]
        sigs = [ops._conv_signature(l.keep[0]) for l in convs]
        configs.append({"height": hp, "width": wp, "launches": len(p.launches), "conv_launches": len(convs),
                        "from_committed_tune_cache": sum(1 for s_ in sigs if s_ in committed),
                        "tuned_in_this_run": sum(1 for s_ in sigs if s_ not in committed) if m.autotune else 0,
                        "tiles": [[l.name, int(l.keep[0].tile)] for l in convs], "fused_paths": p.fusion_report()})
    # the yardstick: the head's largest nearest up-sampling of the full-size plan, and one moving about the staging kernel's bytes
    ups = [l for l in tp.plans[0].launches if l.fn is ops.lib().icaf_upsample_nearest]
    big_in = torch.randn((B, 160, 160, 64), device=dev).to(dt)
    big_out = torch.empty((B, 320, 320, 64), dtype=dt, device=dev)
    up_big = ops.upsample_nearest(big_in, big_out, 2)
    items = {"tta_step": tp.run, "tta_stage": tp.stage, "tta_merge": tp.merge, "upsample_nearest_large": up_big}
    for p, ps in zip(tp.plans, tp.passes):
        items[f"forward_{ps[4]}x{ps[5]}"] = p.run
    if ups:
        items["upsample_nearest_head"] = max(ups, key=lambda l: l.bytes)
    names = list(items)
    sp = ops.current_stream_ptr()
    e0, e1 = ops.Event(), ops.Event()
    times = {n: [] for n in names}
    for r in range(a.warmup + a.rounds):
        for k in range(len(names)):
            n = names[(k + r) % len(names)]
            e0.record(sp)
            for _ in range(a.inner):
                items[n](sp)
            e1.record(sp)
            ms = e0.elapsed_ms(e1) / a.inner
            if r >= a.warmup:
                times[n].append(ms)
    med = {n: sorted(v)[len(v) // 2] for n, v in times.items()}
    spread = {n: [min(v), max(v)] for n, v in times.items()}
    fwd = [n for n in names if n.startswith("forward_")]
    three = sum(med[n] for n in fwd)
    kern = {}
    for n in ("tta_stage", "tta_merge", "upsample_nearest_large", "upsample_nearest_head"):
        if n in items:
            kern[n] = {"ms": med[n], "algorithmic_bytes": int(items[n].bytes), "GB_per_s": items[n].bytes / (med[n] * 1e-3) / 1e9}
    yard = kern["upsample_nearest_large"]["GB_per_s"]
    res = {"model": f"yolov5{a.model}_Transfusion_kaist", "dtype": a.dtype, "batch": B, "height": H, "width": W,
           "device": ops.device_info(), "timing": f"HIP events around {a.inner} replays, median of {a.rounds} interleaved rounds after {a.warmup}",
           "ms": med, "ms_min_max": spread, "tta_step_ms": med["tta_step"], "three_forwards_ms": three,
           "overhead_ms": med["tta_step"] - three, "overhead_fraction_of_three_forwards": (med["tta_step"] - three) / three,
           "stage_plus_merge_ms": med["tta_stage"] + med["tta_merge"], "tta_step_over_plain_forward": med["tta_step"] / med[fwd[0]],
           "kernels": kern, "stage_over_yardstick": kern["tta_stage"]["GB_per_s"] / yard, "merge_over_yardstick": kern["tta_merge"]["GB_per_s"] / yard,
           "yardstick": "icaf_upsample_nearest, (B, 160, 160, 64) -> (B, 320, 320, 64) in the compute type", "autotune": bool(m.autotune),
           "plans": configs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("tta_step_ms", "three_forwards_ms", "overhead_ms", "overhead_fraction_of_three_forwards",
                                          "stage_over_yardstick", "merge_over_yardstick", "kernels", "ms")}))


if __name__ == "__main__":
    main()
