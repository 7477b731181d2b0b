#!/usr/bin/env python3
"""Cost of serving calibrated RGB / IR pairs (icaf_letterbox_warp_frames; Model.forward_frames(align=...) / DetectionPipeline(frame_align=...)).

    python tools/warp_frames_bench.py [--model s --batch 32 --size 640 --rounds 30 --out profiles/warp_frames_bench.json]

One process, items interleaved round by round in a rotating order, medians reported, every item with an `_again` twin on the same buffers
for the A/A spread (the method of tools/frames_bench.py):
  (1) visible 512 x 640 BGR + thermal 512 x 640 grey, a 1 degree rotation and a few pixels of shift: the warped letterbox (default path
      and with the letterbox_direct knob) against the yardstick icaf_letterbox_frames of the same pair (HIP event pairs around --inner
      launches).  The warp reads up to 16 source bytes per output pixel where the plain letterbox reads 4: expect a ratio above 1.
  (2) visible 1080 x 1920 BGR + thermal 512 x 640 grey, `stretch` composed with a 1 degree rotation: the warped letterbox against what it
      replaces on the same GPU — F.grid_sample of the thermal batch to 1080 x 1920 (bilinear, zeros; the sampling grid built once), round,
      then icaf_letterbox_frames — and against utils.datasets.warp_perspective on one CPU thread per pair.
  (3) the host-fed pipeline at the sizes of (2), depth --depth: submit_frames(align=M) from pinned NATIVE frames against submit_frames of
      thermal frames pre-warped to 1080 x 1920, in one interleaved loop (wall clock around --steps submits + synchronize)."""
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


def median(v):
    return sorted(v)[len(v) // 2]


def rig(src_hw, aligned_hw, deg, shift):
    """aligned -> source: a rotation by `deg` about the aligned centre and a shift (aligned pixels), then the stretch between the sizes."""
    (h0, w0), c, s = aligned_hw, np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    cx, cy = (w0 - 1) / 2, (h0 - 1) / 2
    to, back = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]]), np.array([[1, 0, cx + shift[0]], [0, 1, cy + shift[1]], [0, 0, 1.0]])
    return (D.stretch_alignment(src_hw, aligned_hw).astype(np.float64) @ back @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ to).astype(np.float32)


def sampling_grid(M, src_hw, aligned_hw, dev):
    """The (1, h0, w0, 2) grid F.grid_sample(align_corners=True) takes for the aligned -> source matrix M (built once per rig)."""
    (hs, ws), (h0, w0) = src_hw, aligned_hw
    m = torch.from_numpy(M.astype(np.float64)).to(dev)
    y, x = torch.meshgrid(torch.arange(h0, dtype=torch.float64, device=dev), torch.arange(w0, dtype=torch.float64, device=dev), indexing="ij")
    Z = m[2, 0] * x + m[2, 1] * y + m[2, 2]
    u, v = (m[0, 0] * x + m[0, 1] * y + m[0, 2]) / Z, (m[1, 0] * x + m[1, 1] * y + m[1, 2]) / Z
    return torch.stack((2 * u / (ws - 1) - 1, 2 * v / (hs - 1) - 1), dim=2)[None].float()


def kernel_items(tag, B, vis_hw, src_hw, M, size, dev, seed, status_quo):
    """The launches for one pair of sizes on one arena of native frames (BGR visible + grey thermal source) and, for the yardstick and the
    status quo, one arena with a grey thermal frame of the visible size."""
    h0, w0 = vis_hw
    hs, ws = src_hw
    geom1, _ = ops.frame_geometry([vis_hw] * B, size)
    two = np.concatenate((geom1, geom1))
    wrows, wend = ops.pack_warp_frames(two, [3] * B + [(hs, ws, 1)] * B, [None] * B + [M] * B)
    prows = two.copy()
    pend = ops.pack_frames(prows, [3] * B + [1] * B)
    g = torch.Generator().manual_seed(seed)
    vis = torch.randint(0, 256, (B, h0, w0, 3), dtype=torch.uint8, generator=g).to(dev)
    src = torch.randint(0, 256, (B, hs, ws, 1), dtype=torch.uint8, generator=g).to(dev)
    warena, parena = torch.zeros((wend,), dtype=torch.uint8, device=dev), torch.zeros((pend,), dtype=torch.uint8, device=dev)
    for rows, arena, frames in ((wrows["g"], warena, list(vis) + list(src)), (prows[:B], parena, list(vis))):
        for r, f in zip(rows, frames):
            arena[int(r["offset"]):int(r["offset"]) + f.numel()].view(f.shape).copy_(f)
    first = int(prows[B]["offset"])
    assert (prows[B:]["offset"] == first + h0 * w0 * np.arange(B)).all(), "frame sizes whose buffers lie back to back in the arena"
    aligned = parena[first:first + B * h0 * w0].view(B, 1, h0, w0)
    grid = sampling_grid(M, src_hw, vis_hw, dev).expand(B, h0, w0, 2)
    srcf = src.permute(0, 3, 1, 2)

    def resample():
        out = torch.nn.functional.grid_sample(srcf.float(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        aligned.copy_(out.add_(0.5).floor_().clamp_(0, 255))
    resample()
    wtab, ptab = ops.geom_tensor(wrows, dev), ops.geom_tensor(prows, dev)

    def planes():
        return torch.zeros((B, 6, size, size), dtype=torch.uint8, device=dev)
    pw, pp = planes(), planes()
    warp = [ops.letterbox_warp_frames(warena, wrows, wtab, p) for p in (pw, planes())]
    plain = [ops.letterbox_frames(parena, prows, ptab, p) for p in (pp, planes())]
    sp = ops.current_stream_ptr()
    warp[0](sp), plain[0](sp)
    torch.cuda.synchronize()
    host = D.warp_perspective(src[0].cpu().numpy(), M, vis_hw)
    want = np.ascontiguousarray(D.letterbox(np.repeat(host, 3, axis=2), size)[0].transpose(2, 0, 1))
    diff = (pw[:, 3:].int() - pp[:, 3:].int()).abs()
    nby, nbx = -(-size // 32), -(-size // 64)
    staged = sum(ops.warp_letterbox_staged(wrows[B], (by, bx)) for by in range(nby) for bx in range(nbx))
    facts = {"kernel_equals_host_rule_frame_0": bool(np.array_equal(pw[0, 3:].cpu().numpy(), want)),
             "visible_planes_equal_plain_letterbox": bool(torch.equal(pw[:, :3], pp[:, :3])),
             "grid_sample_route_max_abs_difference": int(diff.max()), "grid_sample_route_differing_fraction": float((diff > 0).float().mean()),
             "thermal_tiles_staged_by_host_rule": f"{staged} of {nby * nbx}"}

    def direct(launch):
        def run(s):
            with ops.letterbox_direct(True):
                launch(s)
        return run

    def quo(launch):
        def run(s):
            resample()
            launch(s)
        return run
    items = {}
    for name, pair in (("warp", warp), ("warp_direct", [direct(l) for l in warp]), ("plain", plain)) + \
            ((("grid_sample_then_plain", [quo(l) for l in plain]),) if status_quo else ()):
        items[f"{name}_{tag}"], items[f"{name}_{tag}_again"] = pair
    return items, facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="s"); ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=640); ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--rounds", type=int, default=30); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5, help="launches inside one event pair")
    ap.add_argument("--steps", type=int, default=8, help="pipeline steps inside one wall-clock interval")
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--no-autotune", action="store_true"); ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_frames_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "warp_frames_bench.py measures on the GPU only"
    dev = "cuda:0"
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[a.dtype]
    B, S = a.batch, a.size
    thermal, hd = (512, 640), (1080, 1920)
    M1, M2 = rig(thermal, thermal, 1.0, (3.5, -2.25)), rig(thermal, hd, 1.0, (0.0, 0.0))
    sp = ops.current_stream_ptr()

    # ---- (1) + (2): kernels alone -----------------------------------------------------------------------------------------------------
    items, facts = {}, {}
    for tag, vis_hw, M, quo in (("512x640", thermal, M1, False), ("1080x1920", hd, M2, True)):
        it, facts[tag] = kernel_items(tag, B, vis_hw, thermal, M, S, dev, len(items) + 1, quo)
        items.update(it)
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

    def spread(n):
        return abs(kern[n]["us"] - kern[n + "_again"]["us"]) / kern[n]["us"]
    ratios = {}
    for tag in ("512x640", "1080x1920"):
        us = {n: kern[f"{n}_{tag}"]["us"] for n in ("warp", "warp_direct", "plain")}
        ratios[tag] = {"warp_over_plain_time": us["warp"] / us["plain"], "direct_over_staged_time": us["warp_direct"] / us["warp"],
                       "aa_spread": {n: spread(f"{n}_{tag}") for n in us}}
    quo = kern["grid_sample_then_plain_1080x1920"]["us"]
    ratios["1080x1920"]["grid_sample_route_over_warp_time"] = quo / kern["warp_1080x1920"]["us"]
    ratios["1080x1920"]["aa_spread"]["grid_sample_then_plain"] = spread("grid_sample_then_plain_1080x1920")
    torch.set_num_threads(1)
    frame = np.random.default_rng(9).integers(0, 256, thermal + (1,), dtype=np.uint8)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        D.warp_perspective(frame, M2, hd)
        host.append(time.perf_counter() - t0)
    res = {"batch": B, "size": S, "thermal": list(thermal), "device": ops.device_info(),
           "timing": f"kernels: HIP events around {a.inner} launches of the whole batch (both modalities), median of {a.rounds} interleaved rounds after "
                     f"{a.warmup}; pipelines: wall clock around {a.steps} submits + synchronize, same rounds, interleaved; *_again: a second copy of the "
                     f"item (the A/A spread); host: utils.datasets.warp_perspective of ONE 512 x 640 frame to 1080 x 1920 on one CPU thread, median of 3",
           "kernels": kern, "ratios": ratios, "checks": facts,
           "host_warp_perspective": {"ms_per_pair": median(host) * 1e3, "ms_per_batch": median(host) * 1e3 * B,
                                     "over_warp_kernel_time_per_batch": median(host) * B * 1e6 / kern["warp_1080x1920"]["us"]}}

    # ---- (3): host-fed pipelines ------------------------------------------------------------------------------------------------------
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
        kw = dict(conf_thres=0.25, iou_thres=0.45, depth=a.depth, frames=hd, frame_channels=(3, 1))
        al = dict(frame_align=(None, True), align_frames=thermal)
        pipes = {"native": DetectionPipeline(model(), B, S, S, dev, **kw, **al), "prewarped": DetectionPipeline(model(), B, S, S, dev, **kw),
                 "native_again": DetectionPipeline(model(), B, S, S, dev, **kw, **al), "prewarped_again": DetectionPipeline(model(), B, S, S, dev, **kw)}
        gen = torch.Generator().manual_seed(3)
        grid = sampling_grid(M2, thermal, hd, dev).expand(B, hd[0], hd[1], 2)
        feeds = []                                                       # two sets of pinned buffers, only ever read
        for _ in range(2):
            vis = torch.randint(0, 256, (B,) + hd + (3,), dtype=torch.uint8, generator=gen).pin_memory()
            src = torch.randint(0, 256, (B,) + thermal + (1,), dtype=torch.uint8, generator=gen)
            pre = torch.nn.functional.grid_sample(src.to(dev).permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            pre = pre.add_(0.5).floor_().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().pin_memory()
            feeds.append({"native": (vis, src.pin_memory()), "prewarped": (vis, pre)})

        def run(name, k0):
            p, kind = pipes[name], name.split("_")[0]
            for k in range(a.steps):
                p.submit_frames(*feeds[(k0 + k) % 2][kind], **({"align": M2} if kind == "native" else {}))
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
        up = {"native": B * (3 * hd[0] * hd[1] + thermal[0] * thermal[1]), "prewarped": B * 4 * hd[0] * hd[1]}
        res["pipeline"] = {"visible": list(hd), "thermal": list(thermal), "depth": a.depth, "nplans": pipes["native"].nplans, "pairs_per_s": med,
                           "pairs_per_s_min_max": {n: [min(v), max(v)] for n, v in rates.items()},
                           "aa_spread": {n: abs(med[n] - med[n + "_again"]) / med[n] for n in ("native", "prewarped")},
                           "native_over_prewarped": med["native"] / med["prewarped"], "uploaded_bytes_per_step": up,
                           "upload_GB_per_s": {n: up[n] * med[n] / B / 1e9 for n in up}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
