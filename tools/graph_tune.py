#!/usr/bin/env python3
"""Offline refinement of the igemm configuration choices against the only clock that matters: the replay time of the
whole captured forward graph.  The per-launch autotuner (ops.autotune_conv, in situ) cannot see how a kernel shares
the chip with the graph's parallel branches or with its neighbours' tails; this tool starts from its choices and, for
the layer signatures that cost most, re-captures the graph with every alternative configuration (including 128x64w8,
which the per-launch tuner is not offered) and keeps one only if the replay gets measurably faster.

    python tools/graph_tune.py [--model s --batch 32 --size 640 --dtype bf16 --top 24] --out profiles/tune_cache.json
    python tools/graph_tune.py --model l --dataset VEDAI --dtype f16 --batch 16 --size 1280 --seed-cache profiles/tune_cache_c5_l_vedai_f16_b16_1280.json --out ...
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch   # noqa: E402
import yaml    # noqa: E402

from icafusion_amd import ops                      # noqa: E402
from icafusion_amd.models.yolo import Model        # noqa: E402
from icafusion_amd.synth import synth_images, synth_state_dict   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="s"); ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--size", type=int, default=640); ap.add_argument("--dtype", default="bf16")
ap.add_argument("--top", type=int, default=24, help="number of layer signatures (by time) to refine")
ap.add_argument("--eps", type=float, default=0.004, help="relative improvement required to accept a change")
ap.add_argument("--height", type=int, default=0); ap.add_argument("--width", type=int, default=0)      # rectangular inputs (default: size x size)
ap.add_argument("--loops", type=int, default=1, help="DMFF iterations")
ap.add_argument("--dataset", default="kaist")
ap.add_argument("--seed-cache", default=None, help="start from these choices (default: profiles/tune_cache.json)")
ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "tune_graph.json"))
a = ap.parse_args()
dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
cfg = yaml.safe_load(open(os.path.join(ROOT, "models", "transformer", f"yolov5{a.model}_Transfusion_{a.dataset}.yaml")))
m = Model(cfg).eval(); m.load_state_dict(synth_state_dict(m, 0))
for i in (20, 21, 22):
    m.model[i].crosstransformer[0].loops = a.loops
m = m.to("cuda:0"); m.compute_dtype = dt
H, W = a.height or a.size, a.width or a.size
m.autotune = True
seed_cache = a.seed_cache or os.path.join(ROOT, "profiles", "tune_cache.json")
if os.path.exists(seed_cache):
    ops.load_tune_cache(seed_cache)          # start from the committed choices
plan = m.plan_for(a.batch, H, W, "cuda:0")
rgb, ir = synth_images(a.batch, H, W, 0)
plan.inputs[0].copy_(rgb.cuda()); plan.inputs[1].copy_(ir.cuda())
stream = torch.cuda.Stream(); sp = stream.cuda_stream


def replay_ms(reps=12):
    plan.capture()
    for _ in range(3):
        plan.run(sp)
    e0, e1 = ops.Event(), ops.Event()
    best = float("inf")
    for _ in range(3):                     # best of three timed bursts
        e0.record(sp)
        for _ in range(reps):
            plan.run(sp)
        e1.record(sp)
        best = min(best, e0.elapsed_ms(e1) / reps)
    return best


fn = ops.lib().icaf_conv2d
groups = {}
for l, (name, ms, fl, nb) in zip(plan.launches, plan.timed_run()):
    if l.fn is fn:
        g = groups.setdefault(ops._conv_signature(l.keep[0]), {"launches": [], "ms": 0.0})
        g["launches"].append(l); g["ms"] += ms
base = replay_ms()
print(f"start: {base:.4f} ms per replay ({a.batch / base * 1e3:.0f} pairs/s forward only)")
order = sorted(groups.items(), key=lambda kv: -kv[1]["ms"])[:a.top]
for sig, g in order:
    args0 = g["launches"][0].keep[0]
    cur = args0.tile
    cands = [c for c in ops.conv_candidates(args0) + ops.graph_tune_extras(args0) if c != cur]
    best_c, best_t = cur, base
    for c in cands:
        for l in g["launches"]:
            l.keep[0].tile = c
        if g["launches"][0].fn(*g["launches"][0].args, sp) != 0:       # configuration not applicable to this layer
            continue
        torch.cuda.synchronize()
        t = replay_ms()
        if t < best_t:
            best_c, best_t = c, t
    accept = best_t < base * (1 - a.eps)
    for l in g["launches"]:
        l.keep[0].tile = best_c if accept else cur
    if accept:
        ops._TUNE_CACHE[sig] = best_c
        print(f"  M={sig[0]:8d} N={sig[1]:4d} Cin={sig[2]:4d} k={sig[3]} x{len(g['launches'])}: {cur} -> {best_c}   {base:.4f} -> {best_t:.4f} ms")
        base = best_t
final = replay_ms()
print(f"final: {final:.4f} ms per replay ({a.batch / final * 1e3:.0f} pairs/s forward only)")
os.makedirs(os.path.dirname(a.out), exist_ok=True)
ops.save_tune_cache(a.out)
print("saved", a.out)
