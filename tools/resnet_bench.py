#!/usr/bin/env python3
"""The ResNet50 two-stream backbone on the GPU: what a forward costs, where the time goes, what the key-streaming attention kernel and the
residual-in-front-of-the-ReLU epilogue cost next to the forms they stand beside.

    python tools/resnet_bench.py [--batch 32 --size 640 --dtype bf16 --rounds 12 --out profiles/resnet_bench.json]

One process, items interleaved round by round in a rotating order, medians reported (the method of tools/vgg_bench.py):
  (a) yolov5_ResNet50_Transfusion_kaist: the forward as one hipGraph replay (HIP events), forward + device NMS (wall clock around --steps
      steps + synchronize) as pairs/s, the launch count, per-kernel times (event pair around every launch of the eager plan, median over
      the rounds, summed by launch name: the 7x7 stem, the blocks' 1x1 / 3x3 / shortcut / residual launches) and the launch configuration
      id every ResNet convolution ended up with
  (b) icaf_cross_attention in its streaming form at (B, N 100, C 2048), the P5 level of the model
  (c) the streaming form forced by the probe knob attn_stream against the resident form on a shape both accept: (B, N 100, C 1024)
  (d) a block's conv3 launch with the residual in front of the ReLU (res_mode = 1) against the same launch without a residual, at layer1's
      shape (64 -> 256 channels, both streams, 160 x 160 at 640 x 640), both on the configuration tuned for the residual launch
Everything here is recorded, nothing is gated: the resident attention kernel stays the default wherever it is built, whatever (c) says.
`python tools/resnet_bench.py --collect-parity results/parity_resnet50.jsonl` (no GPU) turns the records tests/test_gpu_resnet.py appended
into profiles/parity_resnet50.json."""
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
from icafusion_amd.models.yolo import Model                       # noqa: E402
from icafusion_amd.synth import synth_images, synth_state_dict    # noqa: E402
from icafusion_amd.utils.general import nms_device                # noqa: E402
from vgg_bench import interleaved, median                         # noqa: E402


def stats(v, extra=None):
    d = {"ms": median(v), "ms_min_max": [min(v), max(v)]}
    d.update(extra or {})
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="yolov5_ResNet50_Transfusion_kaist.yaml")
    ap.add_argument("--batch", type=int, default=32); ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--rounds", type=int, default=12); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=3, help="launches inside one event pair")
    ap.add_argument("--steps", type=int, default=4, help="forward + NMS steps inside one wall-clock interval")
    ap.add_argument("--no-autotune", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_bench.json"))
    ap.add_argument("--collect-parity", metavar="JSONL", help="no measurement: copy the records tests/test_gpu_resnet.py appended to JSONL "
                                                                "(parity_resnet50.jsonl in its results folder) into profiles/parity_resnet50.json and exit")
    a = ap.parse_args()
    if a.collect_parity:
        with open(a.collect_parity) as f:
            rows = [json.loads(l) for l in f if l.strip()]
        dst = os.path.join(ROOT, "profiles", "parity_resnet50.json")
        with open(dst, "w") as f:
            json.dump({"source": "tests/test_gpu_resnet.py, one run on one MI355X; collected by tools/resnet_bench.py --collect-parity", "records": rows},
                      f, indent=1)
        print(f"{len(rows)} records -> {dst}")
        return
    assert torch.cuda.is_available(), "resnet_bench.py measures on the GPU only"
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "f16": torch.float16}[a.dtype]
    B, S = a.batch, a.size
    sp = ops.current_stream_ptr()
    res = {"model": a.cfg[:-5], "dtype": a.dtype, "batch": B, "size": S, "device": ops.device_info(),
           "timing": f"HIP events around {a.inner} launches (forward: 1 graph replay), median of {a.rounds} interleaved rounds after {a.warmup}; "
                     f"pairs/s: wall clock around {a.steps} x (forward + NMS) + synchronize"}

    # ---- (b), (c) attention ------------------------------------------------------------------------------------------------------------
    heads, N = 8, 100
    att = {}
    for C in (2048, 1024):
        qkv = (torch.randn((2, B * N, 3 * C), device=dev) * 1.2).to(dt)
        out = torch.empty((2, B * N, C), dtype=dt, device=dev)
        launch = ops.cross_attention(qkv, out, B, N, heads)
        form = ops.cross_attention_form(dt, B, N, C, heads)
        cfgs = {"default": ops.cross_attention_config(dt, B, N, C, heads)}
        with ops.attn_stream():
            cfgs["attn_stream"] = ops.cross_attention_config(dt, B, N, C, heads)

        def forced(s, launch=launch):
            with ops.attn_stream():
                launch(s)
        items = {"default": launch, "default_again": launch}
        if form == 0:
            items["streaming_forced"] = forced
        for f in items.values():
            f(sp)
        torch.cuda.synchronize()
        t = interleaved(items, a.rounds, a.warmup, a.inner, sp)
        e = {"shape": [B, N, C], "heads": heads, "default_form": form, "config_dkp_qsplit_remap": cfgs, "flops": launch.flops,
             "algorithmic_bytes": int(launch.bytes)}
        for n, v in t.items():
            e[n] = stats(v, {"TFLOP_per_s": launch.flops / (median(v) * 1e-3) / 1e12, "GB_per_s": launch.bytes / (median(v) * 1e-3) / 1e9})
        e["aa_spread"] = abs(e["default"]["ms"] - e["default_again"]["ms"]) / e["default"]["ms"]
        if form == 0:
            e["streaming_over_resident"] = e["streaming_forced"]["ms"] / e["default"]["ms"]
        att[f"C{C}"] = e
        del qkv, out
        torch.cuda.empty_cache()
    res["cross_attention"] = att

    # ---- the model's weights ------------------------------------------------------------------------------------------------------------
    cfg = yaml.safe_load(open(os.path.join(ROOT, "models", "transformer", a.cfg)))
    m = Model(cfg).eval()
    m.load_state_dict(synth_state_dict(m, 0))
    m = m.to(dev)
    m.compute_dtype, m.static_outputs = dt, True
    rgb, ir = synth_images(1, S, S, 0)
    imgs = torch.stack((rgb.expand(B, -1, -1, -1), ir.expand(B, -1, -1, -1))).contiguous().to(dev)

    # ---- (d) conv3 of layer1 with and without the residual in front of the ReLU ---------------------------------------------------------
    # the time of a launch does not depend on the weights' values: two seeded streams of a 64 -> 256 1x1 layer, packed as a plan packs them
    gen = torch.Generator().manual_seed(0)
    wp, kp, bp = ops.pack_streams([(torch.randn((256, 64, 1, 1), generator=gen).to(dev) / 8, torch.randn((256,), generator=gen).to(dev))
                                   for _ in range(2)], dt)
    h = S // 4
    x = torch.randn((2, B, h, h, 64), device=dev).to(dt)
    r = torch.randn((2, B, h, h, 256), device=dev).to(dt)
    y = torch.empty((2, B, h, h, 256), dtype=dt, device=dev)
    with_res = ops.conv2d(x, wp, kp, bp, y, 1, 1, 1, 1, 0, 0, 64, 256, ops.ACT_RELU, res=r, res_pre_act=True)
    without = ops.conv2d(x, wp, kp, bp, y, 1, 1, 1, 1, 0, 0, 64, 256, ops.ACT_RELU)
    behind = ops.conv2d(x, wp, kp, bp, y, 1, 1, 1, 1, 0, 0, 64, 256, ops.ACT_RELU, res=r)
    tile = 0 if a.no_autotune else ops.autotune_conv(with_res, sp)
    without.keep[0].tile = behind.keep[0].tile = tile
    for f in (with_res, without, behind):
        f(sp)
    torch.cuda.synchronize()
    t = interleaved({"res_pre_act": with_res, "no_residual": without, "residual_behind_relu": behind, "res_pre_act_again": with_res},
                    a.rounds, a.warmup, a.inner, sp)
    e = {"shape": {"groups": 2, "pixels_per_group": B * h * h, "cin": 64, "cout": 256}, "configuration": tile, "kernel": ops.conv_kernel_name(with_res),
         "candidates": ops.conv_candidates(with_res.keep[0])}
    for n, v in t.items():
        lb = without.bytes if n == "no_residual" else with_res.bytes
        e[n] = stats(v, {"GB_per_s": lb / (median(v) * 1e-3) / 1e9, "algorithmic_bytes": int(lb)})
    e["aa_spread"] = abs(e["res_pre_act"]["ms"] - e["res_pre_act_again"]["ms"]) / e["res_pre_act"]["ms"]
    e["res_pre_act_over_no_residual"] = e["res_pre_act"]["ms"] / e["no_residual"]["ms"]
    e["res_pre_act_over_residual_behind"] = e["res_pre_act"]["ms"] / e["residual_behind_relu"]["ms"]
    res["conv3_layer1"] = e
    del x, r, y, with_res, without, behind
    torch.cuda.empty_cache()

    # ---- (a) the model -------------------------------------------------------------------------------------------------------------------
    m.autotune, m.use_graph = not a.no_autotune, True
    t0 = time.perf_counter()
    plan = m.plan_for(B, S, S, dev)
    res["plan_build_s"] = time.perf_counter() - t0
    plan.inputs[0].copy_(imgs[0]); plan.inputs[1].copy_(imgs[1])
    convs = [l for l in plan.launches if l.name.startswith("resnet_") and "pool" not in l.name]
    res["resnet_conv_configurations"] = [{"name": l.name, "cin": l.keep[0].Cin, "cout": l.keep[0].Cout, "map": [l.keep[0].H, l.keep[0].W],
                                          "k": l.keep[0].kh, "stride": l.keep[0].sh, "groups": l.keep[0].groups, "tile": l.keep[0].tile,
                                          "kernel": ops.conv_kernel_name(l)} for l in convs]
    res["attention_forms"] = [ops.cross_attention_form(dt, B, n, c, 8) for n, c in ((400, 512), (256, 1024), (100, 2048))]
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
    for r_ in range(a.warmup + a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            plan.run(sp)
            nms_device(z, 0.25, 0.45, stream_ptr=sp)
        torch.cuda.synchronize()
        if r_ >= a.warmup:
            rates.append(a.steps * B / (time.perf_counter() - t0))
    res["forward_plus_nms"] = {"pairs_per_s": median(rates), "pairs_per_s_min_max": [min(rates), max(rates)]}
    per = {}
    for r_ in range(max(3, a.rounds // 3)):
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
