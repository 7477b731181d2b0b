#!/usr/bin/env python3
"""The VGG16 two-stream backbone on the GPU: what a forward costs, where the time goes, and whether the fused image-fed stem earns its place.

    python tools/vgg_bench.py [--batch 32 --size 640 --dtype bf16 --rounds 12 --out profiles/vgg_bench.json]

One process, items interleaved round by round in a rotating order, medians reported (the method of tools/frames_bench.py):
  (a) yolov5_VGG16_Transfusion_kaist: the forward as one hipGraph replay (HIP events), forward + device NMS (wall clock around --steps
      steps + synchronize) as pairs/s, the launch count, per-kernel times (event pair around every launch of the eager plan, median over
      the rounds, summed by launch name) and the launch configuration id every VGG convolution ended up with
  (b) icaf_maxpool2d at the five levels (both streams, as the plan launches it) in GB/s of its algorithmic bytes, each next to
      icaf_upsample_nearest moving the same volume the other way (N / 4 in, N out against N in, N / 4 out) in the same loop
  (c) the first layer through icaf_vgg_stem against the generic route (icaf_preprocess_nchw to 8 channels + icaf_conv2d with K = 72,
      its configuration tuned), and a SECOND copy of the fused launch for the A/A spread of the loop.  The rule the default follows:
      fused stays on only if generic / fused - 1 exceeds that spread.
`python tools/vgg_bench.py --collect-parity results/parity_vgg16.jsonl` (no GPU) turns the records tests/test_gpu_vgg.py appended in the same call
into profiles/parity_vgg16.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch         # noqa: E402
import yaml          # noqa: E402

from icafusion_amd import ops                                     # noqa: E402
from icafusion_amd.models.common import VGGblock                  # noqa: E402
from icafusion_amd.models.yolo import Model                       # noqa: E402
from icafusion_amd.synth import synth_images, synth_state_dict    # noqa: E402
from icafusion_amd.utils.general import nms_device                # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def interleaved(items, rounds, warmup, inner, sp):
    """{name: [ms per launch]}: HIP events around `inner` calls of each item, the items in a rotating order round by round"""
    names = list(items)
    e0, e1 = ops.Event(), ops.Event()
    times = {n: [] for n in names}
    for r in range(warmup + rounds):
        for k in range(len(names)):
            n = names[(k + r) % len(names)]
            e0.record(sp)
            for _ in range(inner):
                items[n](sp)
            e1.record(sp)
            torch.cuda.synchronize()
            if r >= warmup:
                times[n].append(e0.elapsed_ms(e1) / inner)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="yolov5_VGG16_Transfusion_kaist.yaml")
    ap.add_argument("--batch", type=int, default=32); ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--rounds", type=int, default=12); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3, help="launches inside one event pair")
    ap.add_argument("--steps", type=int, default=4, help="forward + NMS steps inside one wall-clock interval")
    ap.add_argument("--no-autotune", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgg_bench.json"))
    ap.add_argument("--collect-parity", metavar="JSONL", help="no measurement: copy the records tests/test_gpu_vgg.py appended to JSONL (parity_vgg16.jsonl "
                                                                "in its results folder) into profiles/parity_vgg16.json and exit")
    a = ap.parse_args()
    if a.collect_parity:
        with open(a.collect_parity) as f:
            rows = [json.loads(l) for l in f if l.strip()]
        dst = os.path.join(ROOT, "profiles", "parity_vgg16.json")
        with open(dst, "w") as f:
            json.dump({"source": "tests/test_gpu_vgg.py, one run on one MI355X; collected by tools/vgg_bench.py --collect-parity", "records": rows}, f, indent=1)
        print(f"{len(rows)} records -> {dst}")
        return
    assert torch.cuda.is_available(), "vgg_bench.py measures on the GPU only"
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    B, S = a.batch, a.size
    sp = ops.current_stream_ptr()
    res = {"model": a.cfg[:-5], "dtype": a.dtype, "batch": B, "size": S, "device": ops.device_info(),
           "timing": f"HIP events around {a.inner} launches (forward: 1 graph replay), median of {a.rounds} interleaved rounds after {a.warmup}; "
                     f"pairs/s: wall clock around {a.steps} x (forward + NMS) + synchronize"}

    # ---- (c) first layer: fused stem against the generic route -----------------------------------------------------------------------
    cfg = yaml.safe_load(open(os.path.join(ROOT, "models", "transformer", a.cfg)))
    m = Model(cfg).eval()
    m.load_state_dict(synth_state_dict(m, 0))
    m = m.to(dev)
    m.compute_dtype, m.static_outputs = dt, True
    rgb, ir = synth_images(1, S, S, 0)
    imgs = torch.stack((rgb.expand(B, -1, -1, -1), ir.expand(B, -1, -1, -1))).contiguous().to(dev)

    class P:                                       # the two fields of a plan the packing helpers read
        dtype, device = dt, torch.device(dev)
    b0, b5 = m.model[0], m.model[5]
    y = torch.empty((2, B, S, S, 64), dtype=dt, device=dev)
    pre = torch.empty((2, B, S, S, 8), dtype=dt, device=dev)
    ws, _, bs = b0._packed(P, 0, b5, stem=True)
    wg, kpg, bg = b0._packed(P, 0, b5, cin_pad=8)
    fused = ops.vgg_stem(imgs, ws, bs, y)
    stage = ops.preprocess(imgs, pre, 0)
    conv = ops.conv2d(pre, wg, kpg, bg, y, 3, 3, 1, 1, 1, 1, 8, 64, ops.ACT_RELU)
    stage(sp); conv(sp); fused(sp)
    torch.cuda.synchronize()
    generic_tile = ops.autotune_conv(conv, sp, context=(stage,)) if not a.no_autotune else 0

    def generic(s):
        stage(s)
        conv(s)
    t = interleaved({"vgg_stem": fused, "generic_route": generic, "vgg_stem_again": fused}, a.rounds, a.warmup, a.inner, sp)
    med = {n: median(v) for n, v in t.items()}
    aa = abs(med["vgg_stem"] - med["vgg_stem_again"]) / med["vgg_stem"]
    gain = med["generic_route"] / med["vgg_stem"] - 1.0
    res["first_layer"] = {"ms": med, "ms_min_max": {n: [min(v), max(v)] for n, v in t.items()}, "aa_spread": aa, "generic_over_fused_minus_1": gain,
                          "fused_wins_by_more_than_the_spread": bool(gain > aa), "generic_conv_configuration": generic_tile,
                          "generic_conv_kernel": ops.conv_kernel_name(conv), "VGGblock.fuse_stem_default": bool(VGGblock.fuse_stem),
                          "default_follows_the_rule": bool(VGGblock.fuse_stem) == bool(gain > aa),
                          "fused_GB_per_s": fused.bytes / (med["vgg_stem"] * 1e-3) / 1e9,
                          "rule": "the fused stem is the default only if generic / fused - 1 > the A/A spread of this loop"}
    del y, pre, fused, stage, conv
    torch.cuda.empty_cache()

    # ---- (b) the pool at the five levels, next to the nearest resize at the same volume -------------------------------------------------
    pools = {}
    for lvl, (c, div) in enumerate(((64, 1), (128, 2), (256, 4), (512, 8), (512, 16)), 1):
        h = S // div
        big = torch.randn((2 * B, h, h, c), device=dev).to(dt)
        small = torch.empty((2 * B, h // 2, h // 2, c), dtype=dt, device=dev)
        big2 = torch.empty_like(big)
        mp, up = ops.maxpool2d(big, small), ops.upsample_nearest(small, big2, 2)
        tt = interleaved({"maxpool2d": mp, "upsample_nearest": up}, a.rounds, a.warmup, a.inner, sp)
        pools[f"level{lvl}"] = {"map": [2 * B, h, h, c], "algorithmic_bytes": int(mp.bytes),
                                **{n: {"ms": median(v), "GB_per_s": (mp.bytes if n == "maxpool2d" else up.bytes) / (median(v) * 1e-3) / 1e9}
                                   for n, v in tt.items()}}
        pools[f"level{lvl}"]["maxpool_over_upsample"] = pools[f"level{lvl}"]["maxpool2d"]["GB_per_s"] / pools[f"level{lvl}"]["upsample_nearest"]["GB_per_s"]
        del big, small, big2
        torch.cuda.empty_cache()
    res["maxpool"] = pools

    # ---- (a) the model -------------------------------------------------------------------------------------------------------------------
    m.autotune, m.use_graph = not a.no_autotune, True
    t0 = time.perf_counter()
    plan = m.plan_for(B, S, S, dev)
    res["plan_build_s"] = time.perf_counter() - t0
    plan.inputs[0].copy_(imgs[0]); plan.inputs[1].copy_(imgs[1])
    convs = [l for l in plan.launches if l.name == "vgg_conv3x3"]
    res["vgg_conv_configurations"] = [{"cin": l.keep[0].Cin, "cout": l.keep[0].Cout, "map": [l.keep[0].H, l.keep[0].W], "groups": l.keep[0].groups,
                                       "x_bytes_per_group": l.keep[0].B * l.keep[0].H * l.keep[0].W * l.keep[0].ldx * 2,
                                       "tile": l.keep[0].tile, "kernel": ops.conv_kernel_name(l),
                                       "candidates": ops.conv_candidates(l.keep[0]),
                                       "accepted": [c for c in ops.conv_candidates(l.keep[0]) if ops.config_valid(l, c)]} for l in convs]
    z = plan.outputs[0]

    def forward(s):
        plan.run(s)
    tf = interleaved({"forward": forward, "forward_again": forward}, a.rounds, a.warmup, 1, sp)
    fm = {n: median(v) for n, v in tf.items()}
    res["forward"] = {"ms": fm["forward"], "ms_min_max": [min(tf["forward"]), max(tf["forward"])], "pairs_per_s_forward_only": B / (fm["forward"] * 1e-3),
                      "aa_spread": abs(fm["forward"] - fm["forward_again"]) / fm["forward"], "launches": len(plan.launches),
                      "plan_bytes": int(plan.nbytes), "flops": float(sum(l.flops for l in plan.launches)),
                      "TFLOP_per_s": float(sum(l.flops for l in plan.launches)) / (fm["forward"] * 1e-3) / 1e12}
    rates = []
    for r in range(a.warmup + a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            plan.run(sp)
            nms_device(z, 0.25, 0.45, stream_ptr=sp)
        torch.cuda.synchronize()
        if r >= a.warmup:
            rates.append(a.steps * B / (time.perf_counter() - t0))
    res["forward_plus_nms"] = {"pairs_per_s": median(rates), "pairs_per_s_min_max": [min(rates), max(rates)]}
    per = {}
    for r in range(max(3, a.rounds // 3)):
        for i, (name, ms, flops, nbytes) in enumerate(plan.timed_run(sp)):
            per.setdefault((i, name), []).append(ms)
        torch.cuda.synchronize()
    by_name = {}
    for (i, name), v in per.items():
        e = by_name.setdefault(name, {"launches": 0, "ms": 0.0})
        e["launches"] += 1
        e["ms"] += median(v)
    res["kernels_eager_ms"] = dict(sorted(by_name.items(), key=lambda kv: -kv[1]["ms"]))
    res["kernels_eager_total_ms"] = sum(e["ms"] for e in by_name.values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
