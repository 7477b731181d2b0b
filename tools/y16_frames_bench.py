#!/usr/bin/env python3
"""Cost of serving 16-bit thermal frames (icaf_y16_window + icaf_letterbox_y16_frames; Model.forward_frames(formats=(None, "y16")) /
DetectionPipeline(frame_formats=(None, "y16"))).

    python tools/y16_frames_bench.py [--model s --batch 32 --size 640 --frame 512x640 --rounds 30 --out profiles/y16_frames_bench.json]

One process, items interleaved round by round in a rotating order, medians reported, every item with an `_again` twin on the same buffers
for the A/A spread (the method of tools/frames_bench.py).  --batch pairs, BGR visible + Y16 thermal:
  (1) icaf_y16_window alone (HIP event pairs around --inner launches) on two contents: uniform random counts, and a narrow scene (sigma 60
      counts around one level: every pixel in one or two high bytes, the contention case of an LDS histogram).
  (2) icaf_letterbox_y16_frames, default path and forced direct, and the whole device step (window + letterbox).
  Yardsticks, none of them the code under test:
  (3) icaf_letterbox_frames of the same pair with the thermal frame already 8-bit grey;
  (4) the same gain control written with torch ops on the device (sort, two ranks, the integer mapping) into the grey arena, then (3); the
      fused launches and this chain are checked to give the same planes before anything is timed;
  (5) utils.datasets.agc_window + agc_u16_to_u8 per frame on one CPU thread (wall clock);
  (6) the host-fed pipeline, depth --depth: submit_frames from pinned host memory with BGR + Y16 against BGR + 8-bit grey in one
      interleaved loop (wall clock around --steps submits + synchronize), pairs per second."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import yaml          # noqa: E402

from icafusion_amd import ops                                     # noqa: E402
from icafusion_amd.models.yolo import Model                       # noqa: E402
from icafusion_amd.pipeline import DetectionPipeline              # noqa: E402
from icafusion_amd.synth import synth_state_dict                  # noqa: E402
from icafusion_amd.utils import datasets as D                     # noqa: E402

CLIP = D.AGC_CLIP


def median(v):
    return sorted(v)[len(v) // 2]


def frames_of(kind, B, h0, w0, seed):
    g = np.random.default_rng(seed)
    if kind == "random":
        return g.integers(0, 65536, (B, h0, w0), dtype=np.uint16)
    return np.clip(np.rint(g.normal(30000, 60.0, (B, h0, w0))), 0, 65535).astype(np.uint16)


def agc_torch(raw, out):
    """The gain control a user writes with torch ops: raw (B, h0, w0) int32 counts -> out (B, h0, w0, 1) uint8, the rule of
    utils.datasets (the C-th smallest / largest value with C = clip * n // 10000 + 1, then the integer mapping)."""
    B, h0, w0 = raw.shape
    n = h0 * w0
    srt = torch.sort(raw.reshape(B, n), dim=1).values
    lo = srt[:, CLIP[0] * n // 10000].view(B, 1, 1)
    hi = srt[:, n - 1 - CLIP[1] * n // 10000].view(B, 1, 1)
    d = (hi - lo).clamp_(min=1)
    out.copy_((((torch.maximum(raw, lo) - lo) * 255 + (d >> 1)) // d).clamp_(max=255).unsqueeze(3))


def kernel_items(B, shape, size, dev):
    h0, w0 = shape
    geom1, _ = ops.frame_geometry([shape] * B, size)
    geom = np.concatenate((geom1, geom1))
    rows, end = ops.pack_y16_frames(geom, [3] * B + ["y16"] * B)
    grows = geom.copy()
    gend = ops.pack_frames(grows, [3] * B + [1] * B)
    bgr = np.random.default_rng(1).integers(0, 256, (B, h0, w0, 3), dtype=np.uint8)
    contents = {k: frames_of(k, B, h0, w0, 2 + i) for i, k in enumerate(("random", "narrow"))}
    arenas, raws = {}, {}
    for k, f in contents.items():
        host = np.zeros((end,), np.uint8)
        for b in range(B):
            o = int(rows[b]["g"]["offset"])
            host[o:o + bgr[b].size] = bgr[b].reshape(-1)
            o = int(rows[B + b]["g"]["offset"])
            host[o:o + 2 * h0 * w0] = f[b].reshape(-1).view(np.uint8)
        arenas[k] = torch.from_numpy(host).to(dev)
        raws[k] = torch.from_numpy(f.astype(np.int32)).to(dev)
    garena = torch.zeros((gend,), dtype=torch.uint8, device=dev)
    for b in range(B):
        o = int(grows[b]["offset"])
        garena[o:o + bgr[b].size].copy_(torch.from_numpy(bgr[b].reshape(-1)))
    go = int(grows[B]["offset"])
    assert int(grows[2 * B - 1]["offset"]) - go == (B - 1) * h0 * w0, "grey frames back to back: one view serves the torch chain"
    grey = garena[go:go + B * h0 * w0].view(B, h0, w0, 1)
    tab, gtab = ops.geom_tensor(rows, dev), ops.geom_tensor(grows, dev)
    wtab = {k: torch.zeros((2 * B, 2), dtype=torch.int32, device=dev) for k in contents}

    def planes():
        return torch.zeros((B, 6, size, size), dtype=torch.uint8, device=dev)
    sp = ops.current_stream_ptr()
    select = {k: [ops.y16_window(arenas[k], rows, tab, wtab[k], B, size, size) for _ in range(2)] for k in contents}
    py, pg = planes(), planes()
    lb = [ops.letterbox_y16_frames(arenas["narrow"], rows, tab, wtab["narrow"], p) for p in (py, planes())]
    plain = [ops.letterbox_frames(garena, grows, gtab, p) for p in (pg, planes())]
    facts = {}
    for k in contents:
        select[k][0](sp)
        torch.cuda.synchronize()
        facts[f"window_equals_host_rule_{k}"] = wtab[k][B:].cpu().tolist() == [list(D.agc_window(f, CLIP)) for f in contents[k]]
    lb[0](sp)
    agc_torch(raws["narrow"], grey)
    plain[0](sp)
    torch.cuda.synchronize()
    facts["fused_equals_torch_agc_then_letterbox"] = bool(torch.equal(py, pg))
    lo, hi = D.agc_window(contents["narrow"][0], CLIP)
    facts["torch_agc_equals_host_rule"] = bool(np.array_equal(grey[0, :, :, 0].cpu().numpy(), D.agc_u16_to_u8(contents["narrow"][0], lo, hi)))
    facts["y16_staged_by_budget_rule"] = bool(ops.y16_letterbox_staged(rows[B]))

    def direct(launch):
        def run(s):
            with ops.letterbox_direct(True):
                launch(s)
        return run

    def step(sel, launch):
        def run(s):
            sel(s)
            launch(s)
        return run

    def torch_chain(launch):
        def run(s):
            agc_torch(raws["narrow"], grey)
            launch(s)
        return run
    items = {}
    for name, pair in (("window_random", select["random"]), ("window_narrow", select["narrow"]), ("y16_letterbox_staged", lb),
                       ("y16_letterbox_direct", [direct(l) for l in lb]), ("y16_step_window_plus_letterbox", [step(s, l) for s, l in zip(select["narrow"], lb)]),
                       ("plain_letterbox_bgr_grey", plain), ("torch_agc_then_plain_letterbox", [torch_chain(l) for l in plain])):
        items[name], items[name + "_again"] = pair
    nbytes = {"window": select["narrow"][0].bytes, "y16_letterbox": lb[0].bytes, "plain_letterbox": plain[0].bytes}
    return items, nbytes, facts, contents


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="s"); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640); ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--frame", default="512x640")
    ap.add_argument("--rounds", type=int, default=30); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="launches inside one event pair")
    ap.add_argument("--steps", type=int, default=8, help="pipeline steps inside one wall-clock interval")
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--no-autotune", action="store_true"); ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "y16_frames_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "y16_frames_bench.py measures on the GPU only"
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    B, S = a.batch, a.size
    shape = tuple(int(v) for v in a.frame.split("x"))
    sp = ops.current_stream_ptr()

    # ---- (1) - (4): kernels alone ---------------------------------------------------------------------------------------------------
    items, nbytes, facts, contents = kernel_items(B, shape, S, dev)
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
    kern = {n: {"us": median(v) * 1e3, "us_min_max": [min(v) * 1e3, max(v) * 1e3]} for n, v in times.items()}
    us = {n: kern[n]["us"] for n in names if not n.endswith("_again")}
    ratios = {"window_narrow_over_random_time": us["window_narrow"] / us["window_random"],
              "y16_direct_over_staged_time": us["y16_letterbox_direct"] / us["y16_letterbox_staged"],
              "y16_letterbox_over_plain_letterbox_time": us["y16_letterbox_staged"] / us["plain_letterbox_bgr_grey"],
              "y16_step_over_plain_letterbox_time": us["y16_step_window_plus_letterbox"] / us["plain_letterbox_bgr_grey"],
              "window_share_of_the_device_step": us["window_narrow"] / us["y16_step_window_plus_letterbox"],
              "torch_chain_over_y16_step_time": us["torch_agc_then_plain_letterbox"] / us["y16_step_window_plus_letterbox"],
              "window_GB_per_s_narrow": nbytes["window"] / (us["window_narrow"] * 1e-6) / 1e9,
              "aa_spread": {n: abs(us[n] - kern[n + "_again"]["us"]) / us[n] for n in us}}

    # ---- (5): the host rule on one CPU thread ------------------------------------------------------------------------------------------
    torch.set_num_threads(1)
    host_ms = {}
    for k, f in contents.items():
        v = []
        for b in range(min(B, 8)):
            t0 = time.perf_counter()
            lo, hi = D.agc_window(f[b], CLIP)
            D.agc_u16_to_u8(f[b], lo, hi)
            v.append((time.perf_counter() - t0) * 1e3)
        host_ms[k] = {"ms_per_frame": median(v), "ms_per_batch": median(v) * B}
    res = {"batch": B, "size": S, "frame": list(shape), "clip_basis_points": list(CLIP), "device": ops.device_info(),
           "timing": f"kernels: HIP events around {a.inner} launches, median of {a.rounds} interleaved rounds after {a.warmup}; pipelines: wall clock "
                     f"around {a.steps} submits + synchronize, same rounds, interleaved; *_again: a second copy of the item (the A/A spread); "
                     "host: wall clock per frame, numpy on one thread",
           "kernels": kern, "algorithmic_bytes": {k: int(v) for k, v in nbytes.items()}, "ratios": ratios, "host_numpy": host_ms, "checks": facts}

    # ---- (6): host-fed pipelines ------------------------------------------------------------------------------------------------------
    if not a.no_pipeline:
        cfg = yaml.safe_load(open(os.path.join(ROOT, "models", "transformer", f"yolov5{a.model}_Transfusion_kaist.yaml")))
        cache = os.path.join(ROOT, "profiles", "tune_cache.json")
        if not a.no_autotune and os.path.exists(cache):
            ops.load_tune_cache(cache)

        def model():
            m = Model(cfg).eval()
            m.load_state_dict(synth_state_dict(m, 0))
            m = m.to(dev)
            m.compute_dtype, m.use_graph, m.autotune, m.static_outputs = dt, True, not a.no_autotune, True
            return m
        kw = dict(conf_thres=0.25, iou_thres=0.45, depth=a.depth, frames=shape)
        mk = {"y16": lambda: DetectionPipeline(model(), B, S, S, dev, frame_formats=(None, "y16"), **kw),
              "grey": lambda: DetectionPipeline(model(), B, S, S, dev, frame_channels=(3, 1), **kw)}
        pipes = {"bgr_y16": mk["y16"](), "bgr_grey": mk["grey"](), "bgr_y16_again": mk["y16"](), "bgr_grey_again": mk["grey"]()}
        h0, w0 = shape
        feeds = []                                                       # two sets of pinned buffers, only ever read
        for k in range(2):
            g = np.random.default_rng(10 + k)
            bgr = torch.from_numpy(g.integers(0, 256, (B, h0, w0, 3), dtype=np.uint8)).pin_memory()
            raw = frames_of("narrow", B, h0, w0, 20 + k)
            grey = np.stack([D.agc_u16_to_u8(f, *D.agc_window(f, CLIP)) for f in raw])[..., None]
            feeds.append({"y16": (bgr, torch.from_numpy(raw.view(np.int16)).pin_memory()), "grey": (bgr, torch.from_numpy(grey).pin_memory())})

        def run(name, k0):
            p = pipes[name]
            for k in range(a.steps):
                p.submit_frames(*feeds[(k0 + k) % 2][name.split("_")[1]])
            p.synchronize()
        pn = list(pipes)
        rates = {n: [] for n in pn}
        for r in range(a.warmup + a.rounds):
            for k in range(len(pn)):
                n = pn[(k + r) % len(pn)]
                t0 = time.perf_counter()
                run(n, r * a.steps)
                dtm = time.perf_counter() - t0
                if r >= a.warmup:
                    rates[n].append(a.steps * B / dtm)
        med = {n: median(v) for n, v in rates.items()}
        res["pipeline"] = {"frame": list(shape), "depth": a.depth, "nplans": pipes["bgr_grey"].nplans, "pairs_per_s": med,
                           "pairs_per_s_min_max": {n: [min(v), max(v)] for n, v in rates.items()},
                           "aa_spread": {n: abs(med[n] - med[n + "_again"]) / med[n] for n in ("bgr_y16", "bgr_grey")},
                           "y16_over_grey": med["bgr_y16"] / med["bgr_grey"],
                           "uploaded_bytes_per_step": {"bgr_y16": B * 5 * h0 * w0, "bgr_grey": B * 4 * h0 * w0}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
