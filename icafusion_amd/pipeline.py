"""Two-stage detection pipeline: forward on one HIP stream, NMS (+ the detections all-gather) on a second one.

The reference runs `model(img, img2)` and `non_max_suppression` back to back for every batch with a device sync in
between (detect_twostream.py:83-88, test.py:126-141).  NMS is a latency-bound job that occupies one workgroup per
image (32 of 256 CUs at batch 32), so here batch i's NMS runs concurrently with batch i+1's forward:

    forward stream : graph(i) -> snapshot z(i) -> graph(i+1) -> snapshot z(i+1) -> ...
    nms stream     :              wait snapshot(i) -> candidates / sort / greedy (i) -> ...
    gather stream  :  (N > 1)                 wait the NMS of the group's last batch -> ONE all_gather of the group's detection blocks

With `depth` > 1 (bench default 2) that many batches are in flight: batch n replays plan n % nplans (own buffers, own hipGraph) on
forward stream n % depth, so the low-occupancy tail of one forward overlaps the full-width layers of the next (+13 % throughput on one
MI355X); NMS then reads each plan's own `z` and the plan is not replayed before its NMS has finished.  nplans = depth,
or a multiple of it when the pipeline is fed from host memory (u8=True): the host -> device copy of a batch then lands DIRECTLY in the
input buffer of a plan that no forward in flight is reading — one PCIe copy per batch and no device-to-device hop.

With depth 1, `z` is snapshotted into one of two staging buffers because the plan's output buffer is overwritten by the next
replay; events order snapshot -> NMS -> reuse.  Each of the two slots also owns its NMS runner (workspace + det / count /
keep output buffers) and its gathered block, so the tensors step n returned stay untouched until step n + 2 reuses the
slot — and two pipelines of the same shape never share buffers.  Results of step i are valid after `synchronize()`.
PyTorch streams / events are used as plumbing only; every kernel on both streams is ours (plus RCCL).
"""
import numpy as np
import torch

from . import dist as D
from . import ops
from .options import OPT
from .utils.datasets import agc_clip as agc_clip_checked
from .utils.general import nms_device


# further SETS of `depth` plans a host-fed pipeline owns: the copy of batch n waits for the END of the forward that used its target plan,
# depth * (1 + EXTRA_PLANS) steps earlier.  With chain graphs (see HOST_FED_BRANCHES) one extra set is enough — one process each, same box:
# 4 plans 14,745 / 14,983 pairs/s, 6 plans 14,605 (and 6 plans pin 11 GB for yolov5s batch 32); with branched graphs it took 6 plans to reach
# 13,400 (4 plans: 10,742)
# (Memory: a host-fed pipeline therefore holds depth * (1 + EXTRA_PLANS) COMPLETE plans — intermediates, hipGraph, NMS runner each: 2.0 GB per plan for
#  yolov5s batch 32 at 640 x 640, ~40 GB for yolov5l batch 16 at 1280 x 1280, i.e. 160 GB for the four plans of a depth-2 yolov5l VEDAI pipeline.  That
#  fits the 288 GB of an MI355X and nothing smaller; Model.plan_cache_bytes cannot evict plans a pipeline holds.)
EXTRA_PLANS = max(1, OPT.pipe_extra_plans)
COPY_STREAMS = max(1, OPT.pipe_copy_streams)      # a batch's host -> device copy in this many slices, one high-priority stream each
COPY_PRIO = OPT.pipe_copy_prio                    # the copy stream(s) on a high-priority queue: 15,600 / 15,501 pairs/s against 15,288 / 15,369 at normal priority
HOST_FED_BRANCHES = OPT.pipe_branches             # keep the hipGraph's parallel branches in host-fed pipelines (measured slower)
# (round 5's icaf_feed_copy — resident workgroups reading the pinned batch over PCIe instead of the DMA engine — measured 2 x slower inside the
#  serving loop and was removed in round 6)


class DetectionPipeline:
    def __init__(self, model, batch, height, width, device, conf_thres=0.25, iou_thres=0.45, classes=None,
                 agnostic=False, multi_label=False, max_det=300, world=1, overlap=True, force_gather=False, depth=1, u8=False, augment=False,
                 frames=None, frame_channels=(3, 3), frames_bgr=True, round_boxes=False, frame_formats=(None, None), yuv_matrix="bt601",
                 frame_align=(None, None), align_frames=None, align_border=0, agc_clip=(100, 100)):
        """frames=(max_h0, max_w0): the pipeline also takes NATIVE camera frames (`submit_frames`; implies u8): every plan owns a frame arena
        for `batch` pairs of up to that size (frame_channels: interleaved channels of the RGB / IR frames, 3 or 1) and a geometry table;
        the letterbox runs on the device in front of the plan and the boxes come back in native image space (round_boxes: torch.round
        applied, as detect_twostream.py:80).  frames_bgr: the frames are BGR (planes become RGB).
        frame_formats=(fmt_rgb, fmt_ir): a modality that arrives as YUV 4:2:0 names its layout ("nv12" | "nv21" | "i420" | "yv12"; None:
        interleaved frames of frame_channels) and is submitted as the decoder's contiguous buffer, (B, 3 * H0 // 2, W0) or a list of (3 * H0_i
        // 2, W0_i); its half of the arena holds 1.5 bytes per pixel and the conversion (yuv_matrix: "bt601" | "bt709" | "bt601-full") runs
        inside the letterbox, equal to utils.datasets.yuv420_to_bgr in front of the host letterbox byte for byte.
        frame_align=(None, True) (or (True, None)): a CALIBRATED rig — the marked modality is seen through a homography that
        `submit_frames(..., align=M)` takes per submit (Model.forward_frames' align=); its frames may have any size up to align_frames=
        (max_hs, max_ws), which sizes its half of every arena, while frames= stays the other, the aligned, modality's maximum.  Pixels
        the source does not cover are align_border.  Boxes come back in the un-warped modality's native space.
        frame_formats=(None, "y16") (either or both modalities): a 16-BIT THERMAL modality, raw counts submitted as a torch.uint16 /
        torch.int16 (B, H0, W0) tensor, its uint8 bytes (B, H0, 2 * W0) or a list of per-frame tensors; its half of the arena holds 2
        bytes per pixel.  Gain control runs on the device in front of the letterbox (Model.forward_frames' formats="y16"): agc_clip=
        (clip_lo, clip_hi) basis points per frame, or the window `submit_frames(..., agc_window=)` gives for a step; the windows a
        step used stay on the device in `pipe.frames["window"][plan index]`, int32 (2B, 2), rows modality * B + image.
        augment=True: every step is a test-time-augmentation step (Model.forward(augment=True), reference models/yolo_test.py:116-131:
        the plans are engine.TtaPlan objects) and NMS runs over the merged rows of the three passes (55,755 per image at 640 x 640).
        u8=True: the plans take the dataloader's uint8 (B, 6, H, W) RGB+IR batch (Model.forward_u8: `/255`, split and cast in the
        staging kernel, reference test.py:116-123) — `submit_u8` then feeds them from (pinned) host memory with the H2D copy on its own
        stream, overlapped with the forwards in flight."""
        # the kind of table the frames need (ops.KINDS): what cannot be combined is refused here, before anything is built
        kind = ops.frame_kind(frame_formats, tuple(a or None for a in frame_align) if any(frame_align) else None, who="", align_arg="frame_align",
                              formats_arg="frame_formats")
        if kind.window:
            agc_clip_checked(agc_clip)
        self.model, self.device, self.world = model, torch.device(device), world
        self.u8, self.augment = bool(u8) or frames is not None, bool(augment)
        self.gather = world > 1 or bool(force_gather)       # force_gather: run the all-gather even with one rank (hardware test of the RCCL path)
        self.nms_args = dict(conf_thres=conf_thres, iou_thres=iou_thres, classes=classes, agnostic=agnostic,
                             multi_label=multi_label, max_det=max_det)
        # (the pipeline replays the plans itself and reads plan.outputs: it does not touch Model.static_outputs — a later model(rgb, ir) of the
        #  same object still returns clones)
        # depth > 1: that many batches in flight, each with its own plan (buffers, hipGraph) and forward stream — the tails of one
        # forward (20x20 layers, DMFF, Detect: launches that leave CUs idle) overlap the full-width layers of the next
        self.depth = max(1, int(depth)) if overlap else 1         # overlap=False is the strictly sequential baseline: one batch, one stream
        # host-fed pipelines own ONE MORE plan than batches in flight: the copy of the next batch goes straight into the input of the plan that
        # is not in flight (round 4 copied into depth + 1 staging buffers and moved the batch into the plan's input device-to-device: 20 % of
        # the no-feed rate was lost to that hop and to the queue it shared)
        # (a MULTIPLE of depth: plan p then always replays on forward stream p % depth — a hipGraph keeps its stream — and the pipeline owns no more
        #  forward streams than forwards in flight: HIP deals a process's streams over a few hardware queues, and every extra stream is one more
        #  chance that two of them that should overlap share one)
        self.nplans = self.depth * (1 + EXTRA_PLANS) if (self.u8 and overlap) else self.depth
        # (host-fed: chain graphs.  A graph with parallel branches replays them on streams of its own, which share hardware queues with the copy
        #  and NMS streams: same box, one process each, 13,578 pairs/s with the branches, 15,153 without, 15,172 with no graph at all — and
        #  16,100-16,500 with the inputs resident, where the branches are worth 3 %)
        plan_for = model.tta_plan_for if self.augment else model.plan_for
        self.plans = [plan_for(batch, height, width, self.device, u8=self.u8, slot=s, branches=HOST_FED_BRANCHES or not (self.u8 and overlap))
                      for s in range(self.nplans)]
        # (a HIGH-PRIORITY stream: HIP maps the streams of a process onto a few hardware queues, and a copy stream that shares its queue with
        #  a forward stream waits behind that stream's graph — the copies then do not overlap the forwards at all; priority streams get
        #  queues of their own)
        self.copy_streams = [torch.cuda.Stream(device=self.device, priority=COPY_PRIO) for _ in range(COPY_STREAMS)] if self.u8 else []
        self.copy_stream = self.copy_streams[0] if self.u8 else None
        self.copied = [[torch.cuda.Event() for _ in self.copy_streams] for _ in self.plans]
        self.plan = self.plans[0]
        self.z = self._z(self.plan)
        # `depth` forward streams; plan p always replays on stream p % depth (alternating a graph between two streams cost the host-fed loop a
        # third of its rate), so at most `depth` forwards run at once by construction
        self.fwd_streams = [torch.cuda.Stream(device=self.device) for _ in range(self.depth)]
        self.fwd_stream = self.fwd_streams[0]
        self.fwd_done = [torch.cuda.Event() for _ in range(self.nplans)]
        self.nms_stream = torch.cuda.Stream(device=self.device) if overlap else self.fwd_stream
        self.overlap = overlap
        self.zbuf = [torch.empty_like(self.z) for _ in range(2)] if overlap else [self.z]
        self.snap_done = [torch.cuda.Event() for _ in range(2)]
        self.nms_done = [torch.cuda.Event() for _ in range(2)]
        nslots = 2 if overlap else 1
        rows, no = self.z.shape[1], self.z.shape[2]
        ml = bool(multi_label) and no - 5 > 1
        # The detection blocks of the slots lie SIDE BY SIDE in one allocation: with a process group the all-gather then runs once per GROUP of
        # steps (one per in-flight slot: `depth` batches with the bench's default pipeline) on a stream of its own behind the group's last NMS —
        # one latency-bound collective of group x 230 KB instead of `group` of them, and none of them on the NMS stream, where the RCCL kernel
        # sat between two batches' NMS launches (one GPU, --force-gather: -3.5 % with a gather per step on the NMS stream).
        blk = batch * max_det * 6 + batch
        self.group = self.nplans if self.nplans > 1 else 1          # steps per collective (the one-plan pipeline alternates two slots: one step each)
        nblocks = self.nplans if self.nplans > 1 else nslots
        self.group_block = torch.zeros((nblocks * blk,), dtype=torch.float32, device=self.device)
        slot_block = [self.group_block[k * blk:(k + 1) * blk] for k in range(nblocks)]
        self.runners = [ops.NmsRunner(batch, rows, no - 5, self.device, ml, max_det, want_keep=False, block=slot_block[k] if self.nplans == 1 else None)
                        for k in range(nslots)]
        if self.nplans > 1:
            self.deep_runners = [ops.NmsRunner(batch, rows, no - 5, self.device, ml, max_det, want_keep=False, block=slot_block[k]) for k in range(self.nplans)]
            self.nms_done_deep = [torch.cuda.Event() for _ in range(self.nplans)]
        # two generations of the gathered buffer: the tensors a step returned stay untouched until the gather AFTER the next one
        self.gathered = [torch.empty((world * self.group * blk,), dtype=torch.float32, device=self.device) for _ in range(2)] if self.gather else None
        self.gather_stream = torch.cuda.Stream(device=self.device) if (self.gather and overlap) else self.nms_stream
        self.gather_done = torch.cuda.Event()
        self.nms_group_done = torch.cuda.Event()
        self.gen, self.pending, self.gathers = 0, 0, 0               # generation the NEXT gather writes; steps since the last gather; gathers issued
        self.n = 0
        self.last = None
        self.frames = None
        if frames is None and any(f is not None for f in frame_formats):
            raise ValueError("frame_formats describes native frames: pass frames=(max_h0, max_w0) with it")
        if frames is None and (any(frame_align) or align_frames is not None):
            raise ValueError("frame_align / align_frames describe native frames: pass frames=(max_h0, max_w0) with them")
        if frames is not None:
            self._init_frames(kind, batch, height, width, frames, frame_channels, frames_bgr, round_boxes, frame_formats, yuv_matrix,
                              frame_align, align_frames, align_border, agc_clip)

    def _init_frames(self, kind, B, H, W, frames, chans, bgr, round_boxes, formats=(None, None), yuv_matrix="bt601", frame_align=(None, None),
                     align_frames=None, align_border=0, agc_clip=(100, 100)):
        """Per plan: a byte arena (RGB frames in its first half, IR frames in its second) and ONE table allocation — 2B descriptor rows
        of `kind` (ops.KINDS) for the letterbox, then B scale_coords rows for scale_detections — with a pinned host twin it is copied from."""
        max_h0, max_w0 = int(frames[0]), int(frames[1])
        chans = tuple(int(c) for c in chans)
        if max_h0 < 1 or max_w0 < 1 or len(chans) != 2 or any(c not in (1, 3) for c in chans):
            raise ValueError(f"frames=(max_h0, max_w0) with frame_channels of 1 or 3 each, got {frames} / {chans}")
        formats = tuple(formats)
        if len(formats) != 2 or any(f is not None and f != "y16" and f not in ops.YUV_LAYOUTS for f in formats):
            raise ValueError(f"frame_formats=(fmt_rgb, fmt_ir), each None, 'y16' or one of {', '.join(ops.YUV_LAYOUTS)}, got {formats!r}")
        warp = [bool(a) for a in frame_align].index(True) if any(frame_align) else None      # the aligned modality of a calibrated rig
        if (warp is None) != (align_frames is None):
            raise ValueError("frame_align marks the aligned modality and align_frames=(max_hs, max_ws) sizes its frames: pass both or neither")
        smax, border = (max_h0, max_w0), int(align_border)
        if warp is not None:
            smax = (int(align_frames[0]), int(align_frames[1]))
            if min(smax) < 1 or not 0 <= border <= 255:
                raise ValueError(f"align_frames=(max_hs, max_ws) and align_border in 0..255, got {align_frames} / {align_border}")
        A = ops.FRAME_ALIGN
        # what a pack function takes for a frame of each modality (ops.frame_specs) and the bytes it holds at the maximum size
        specs = [fmt if fmt is not None else (smax[0], smax[1], c) if m == warp else c for m, (c, fmt) in enumerate(zip(chans, formats))]
        cap = [B * (-(-ops.frame_bytes(s, max_h0, max_w0) // A) * A) for s in specs]
        opts = {"matrix": ops.yuv_matrix_code(yuv_matrix) if kind.name == "yuv" else 0, "clip": agc_clip, "border": border}
        probe1, _ = ops.frame_geometry([(max_h0, max_w0)] * B, (H, W))
        probe = np.concatenate([kind.pack(probe1.copy(), [specs[m]] * B, base=base, **opts)[0] for m, base in ((0, 0), (1, cap[0]))])
        gb = 2 * B * probe.dtype.itemsize
        self.frames = {"B": B, "H": H, "W": W, "max": (max_h0, max_w0), "chans": chans, "cap": cap, "geom_bytes": gb, "cache": {},
                       "arena": [], "tab_dev": [], "tab_host": [], "letterbox": [], "scale_rows": [], "scale_launch": {}, "pending": None,
                       "round": bool(round_boxes), "formats": formats, "kind": kind, "specs": specs, "opts": opts,
                       "warp": warp, "smax": smax, "window": []}
        f = self.frames
        for plan in self.plans:
            arena = torch.zeros((sum(cap),), dtype=torch.uint8, device=self.device)
            tab = torch.zeros((gb + B * 20,), dtype=torch.uint8, device=self.device)
            f["arena"].append(arena)
            f["tab_dev"].append(tab)
            f["tab_host"].append(torch.zeros((gb + B * 20,), dtype=torch.uint8).pin_memory())
            f["scale_rows"].append(tab[gb:].view(torch.float32).view(B, 5))
            f["window"].append(torch.zeros((2 * B, 2), dtype=torch.int32, device=self.device) if kind.window else None)
            f["letterbox"].append(kind.launches(arena, probe, tab, plan.inputs[0], bgr, B, window=f["window"][-1]))     # a step's launches, in order

    def _frame_table(self, shapes, contiguous, src_shapes=None):
        """(table bytes, descriptor rows) of one step's frames, cached per set of shapes: the geometry, the arena layout
        (ops.layout_modality: a uniform batch whose frames are whole 16-byte multiples keeps its layout, so ONE copy per modality moves it;
        other frames start on FRAME_ALIGN boundaries) and the validation against this pipeline's arena and output size.  The rows of an
        aligned modality lie around its SOURCE frames, with identity matrices, those of a 16-bit modality are in percentile mode:
        submit_frames writes a step's matrices and windows into the pinned table."""
        f = self.frames
        key = (tuple(shapes), contiguous) + ((tuple(src_shapes),) if src_shapes is not None else ())
        hit = f["cache"].get(key)
        if hit is None:
            B, cap, kind = f["B"], f["cap"], f["kind"]
            for h0, w0 in shapes:
                if h0 > f["max"][0] or w0 > f["max"][1]:
                    raise ValueError(f"a {h0}x{w0} frame exceeds the pipeline's frames={f['max']}")
            for hs, ws in src_shapes or ():
                if hs > f["smax"][0] or ws > f["smax"][1]:
                    raise ValueError(f"a {hs}x{ws} frame exceeds the pipeline's align_frames={f['smax']}")
            geom1, scale = ops.frame_geometry(shapes, (f["H"], f["W"]))
            halves = []
            for m, base in ((0, 0), (1, cap[0])):
                specs = [(hs, ws, f["chans"][m]) for hs, ws in src_shapes] if m == f["warp"] else [f["specs"][m]] * B
                rows, end = kind.pack(geom1.copy(), specs, base=base, **f["opts"])
                halves.append(ops.layout_modality(rows, end, base, cap[m], contiguous[m], m))
            geom = np.concatenate(halves)
            kind.validate(geom, sum(cap), f["H"], f["W"])
            table = np.concatenate((geom.view(np.uint8).reshape(-1), scale.view(np.uint8).reshape(-1)))
            if len(f["cache"]) >= 64:
                f["cache"].pop(next(iter(f["cache"])))
            hit = f["cache"][key] = (torch.from_numpy(table), geom)
        return hit

    def submit_frames(self, rgb, ir, align=None, agc_window=None):
        """One batch of NATIVE frames through the pipeline: rgb / ir are uint8 (B, H0, W0, ch) tensors or lists of (H0_i, W0_i, ch) tensors,
        in pinned host memory or on the device (a modality with a frame_formats layout: (B, 3 * H0 // 2, W0) or a list of (3 * H0_i // 2,
        W0_i) buffers, H0 and W0 even); a pair shares its size, sizes may change from step to step.  The frames and the step's
        geometry table are copied on the copy stream(s) under the events submit_u8 uses, the letterbox runs on the plan's forward stream in
        front of its graph, scale_detections on the NMS stream behind NMS: the (det, count) step() returns hold NATIVE-space boxes (rows >=
        count zeroed), and so does the gathered block of a process group.  Host buffers must stay untouched until their copy has run
        (`pipe.copied[n % pipe.nplans]`, as for submit_u8).
        align: for a pipeline built with frame_align, the step's alignment of the marked modality — a (3, 3) array, a (B, 3, 3) array or
        "stretch" (aligned -> source, Model.forward_frames' align=); it travels in the pinned geometry table with the rest of the rows.
        agc_window: for a pipeline with a "y16" modality, this step's gain-control window, (lo, hi) or a (B, 2) array, instead of the
        percentile window of each frame; it travels in the pinned table too."""
        f = self.frames
        if f is None:
            raise ValueError("DetectionPipeline(frames=(max_h0, max_w0)) takes native frames")
        B, chans, kind = f["B"], f["chans"], f["kind"]
        wins = None
        if agc_window is not None:
            if not kind.window:
                raise ValueError("submit_frames(agc_window=...) goes with DetectionPipeline(frame_formats=(..., 'y16'))")
            wins = ops._y16_windows(agc_window, B)
            for lo_, hi_ in wins:
                if not 0 <= lo_ <= hi_ <= 65535:
                    raise ValueError(f"agc_window ({lo_}, {hi_}) must satisfy 0 <= lo <= hi <= 65535")
        rgb, ir = (ops.y16_bytes(t) if fmt == "y16" else t for t, fmt in zip((rgb, ir), f["formats"]))
        if (align is None) != (f["warp"] is None):
            raise ValueError("submit_frames(align=...) goes with DetectionPipeline(frame_align=..., align_frames=...): both or neither")
        *lists, shapes, uniform, _, src_shapes, mats = kind.lists(rgb, ir, f["formats"], None if align is None else (align, None) if f["warp"] == 0 else (None, align))
        if len(shapes) != B:
            raise ValueError(f"submit_frames expects a batch of {B} pairs, got {len(shapes)}")
        mods, contiguous = [], []
        for m, (t, fr) in enumerate(zip((rgb, ir), lists)):
            if f["formats"][m] is None and any(x.shape[2] != chans[m] for x in fr):
                raise ValueError(f"modality {m}: frames must be uint8 (H0, W0, {chans[m]}) tensors")
            contiguous.append(bool(uniform[m] and t.is_contiguous() and (t[0].numel() % 16 == 0)))
            mods.append((t, fr))
        table, geom = self._frame_table(shapes, tuple(contiguous), src_shapes)        # raises before anything is enqueued
        pi = self.n % self.nplans
        fs = self.fwd_streams[pi % self.depth]
        arena, ncs = f["arena"][pi], len(self.copy_streams)
        on_device = any(x.is_cuda for _, fr in mods for x in fr)
        if self.n >= self.nplans:
            self.copied[pi][0].synchronize()                                # the last copy OUT of this plan's pinned table (nplans steps ago) has run
        f["tab_host"][pi].copy_(table)
        if kind.update is not None:                                         # this step's matrices / windows, into the pinned rows they belong to
            kind.update(f["tab_host"][pi].numpy()[:f["geom_bytes"]].view(kind.dtype), B, f["formats"], f["warp"], mats=mats, wins=wins)
        cur = torch.cuda.current_stream(self.device)
        for k, cs in enumerate(self.copy_streams):                          # the batch in `ncs` slices of images, one copy stream each
            lo, hi = B * k // ncs, B * (k + 1) // ncs
            if hi <= lo and k:
                continue
            if self.nplans == 1:                                            # sequential pipeline: behind everything the one plan has in flight
                cs.wait_stream(fs)
                cs.wait_stream(self.nms_stream)
            elif self.n >= self.nplans:
                cs.wait_event(self.fwd_done[pi])                            # this plan's previous forward has consumed its arena and table
                if k == 0:
                    cs.wait_event(self.nms_done_deep[pi])                   # ... and its scale_detections the scale rows
            if on_device:
                cs.wait_stream(cur)
            with torch.cuda.stream(cs):
                if k == 0:
                    f["tab_dev"][pi].copy_(f["tab_host"][pi], non_blocking=True)
                for m, (t, fr) in enumerate(mods):
                    rows = ops.frame_rows(geom[m * B:(m + 1) * B])
                    if contiguous[m]:
                        o, fb = int(rows[lo]["offset"]), t[0].numel()
                        arena[o:o + (hi - lo) * fb].view(t[lo:hi].shape).copy_(t[lo:hi], non_blocking=True)
                    else:
                        for b in range(lo, hi):
                            o = int(rows[b]["offset"])
                            arena[o:o + fr[b].numel()].view(fr[b].shape).copy_(fr[b], non_blocking=True)
            if on_device:
                for t, fr in mods:
                    for x in ([t] if torch.is_tensor(t) else fr):
                        if x.is_cuda:
                            x.record_stream(cs)
            self.copied[pi][k].record(cs)
            fs.wait_event(self.copied[pi][k])
        for launch in f["letterbox"][pi]:
            launch(fs.cuda_stream)
        f["pending"] = pi
        try:
            return self.step()
        finally:
            f["pending"] = None

    def _native_boxes(self, runner, stream_ptr):
        """Behind the NMS of a submit_frames step, on the NMS stream: the runner's block to native image space, in place."""
        f = self.frames
        if f is None or f["pending"] is None:
            return
        pi = f["pending"]
        key = (id(runner), pi)
        if key not in f["scale_launch"]:
            f["scale_launch"][key] = ops.scale_detections(runner.det, runner.count, f["scale_rows"][pi], round=f["round"])
        f["scale_launch"][key](stream_ptr)

    def _z(self, plan):
        """The decoded rows NMS reads: a TtaPlan's output IS the merged z, a plain plan's is (z, logits, raws)."""
        return plan.outputs if self.augment else plan.outputs[0]

    @property
    def inputs(self):
        """Static RGB / IR staging tensors (NCHW fp32) of the NEXT step's plan.  With depth > 1 every in-flight slot has its OWN
        staging tensors: they must be refilled before EVERY step (filling them once and stepping repeatedly would run every
        other batch on another slot's stale inputs), and the caller's copy must be ordered against the slot's forward stream —
        `submit()` does both."""
        return self.plans[self.n % self.nplans].inputs

    def submit(self, rgb, ir):
        """Copy one batch into the next step's staging tensors ON that step's forward stream, behind the plan's previous forward (the same
        stream when nplans == depth; an event otherwise) so a forward still reading them is never overwritten, then enqueue the step."""
        pi = self.n % self.nplans
        fs = self.fwd_streams[pi % self.depth]
        ins = self.plans[pi].inputs
        fs.wait_stream(torch.cuda.current_stream(self.device))     # rgb / ir may have been produced on the caller's stream
        with torch.cuda.stream(fs):                                # (the plan's own stream: behind its previous forward)
            ins[0].copy_(rgb, non_blocking=True)
            ins[1].copy_(ir, non_blocking=True)
        for t in (rgb, ir):                                        # the copies run on `fs`, possibly long after this call returns: tell the
            if t.is_cuda:                                          # caching allocator, or a temporary's memory is handed out (and overwritten
                t.record_stream(fs)                                # on the caller's stream) before the copy has read it
        return self.step()

    def submit_u8(self, img6):
        """One uint8 (B, 6, H, W) batch — pinned host memory (the reference's dataloader output, test.py:116) or a device tensor — through
        the pipeline.  The copy runs on the pipeline's COPY stream straight into the input buffer of plan n % nplans: the plan that ran
        nplans (= depth * (1 + EXTRA_PLANS)) steps ago, so the copy only waits for a forward that has long finished — NOT for one of the `depth` forwards in flight (a
        copy into the input of a plan that is still running could not start before that forward had ended: 9,960 pairs/s where the forward
        alone does 15,600; round 4's extra staging buffers + device-to-device hop: 13,059 of 16,238).  The host buffer must stay untouched
        until its copy has run (rotate >= nplans + 2 pinned buffers, or wait for the events in `pipe.copied[n % pipe.nplans]`, one per copy stream)."""
        assert self.u8, "DetectionPipeline(u8=True) takes uint8 batches"
        pi = self.n % self.nplans
        fs = self.fwd_streams[pi % self.depth]
        dst = self.plans[pi].inputs[0]
        B, ncs = img6.shape[0], len(self.copy_streams)
        for k, cs in enumerate(self.copy_streams):                # the batch in `ncs` slices of images, one copy stream (DMA queue) each
            lo, hi = B * k // ncs, B * (k + 1) // ncs
            if hi <= lo:
                continue
            if self.n >= self.nplans:
                cs.wait_event(self.fwd_done[pi])                  # this plan's previous forward (nplans steps ago) has consumed its input
            if img6.is_cuda:
                cs.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(cs):
                dst[lo:hi].copy_(img6[lo:hi], non_blocking=True)
            if img6.is_cuda:
                img6.record_stream(cs)
            self.copied[pi][k].record(cs)
            fs.wait_event(self.copied[pi][k])
        return self.step()

    def step(self):
        """Enqueue one batch: forward replay, then NMS (+ gather) on the second stream.  Returns (det, count) device tensors, valid once
        the nms stream has drained (see synchronize()) — ALWAYS rank-major: det (world, B, max_det, 6) fp32, count (world, B) int32, i.e.
        global batch order for contiguous shards (dist.flatten_gathered gives the (world * B, ...) form).  Without a gather (one rank)
        the leading axis has length 1 and the tensors are views of the slot's NMS output block."""
        if self.nplans > 1:
            return self._step_deep()
        i = (self.n & 1) if self.overlap else 0
        fs, ns = self.fwd_stream, self.nms_stream
        self.plan.run(fs.cuda_stream)
        if self.overlap:
            if self.n >= 2:
                fs.wait_event(self.nms_done[i])             # NMS of step n-2 has finished reading zbuf[i]
            with torch.cuda.stream(fs):
                self.zbuf[i].copy_(self.z, non_blocking=True)
            self.snap_done[i].record(fs)
            ns.wait_event(self.snap_done[i])
        if self.gather and self.gathers:
            ns.wait_event(self.gather_done)                 # the last gather has read this slot's block
        det, count, keep = nms_device(self.zbuf[i], stream_ptr=ns.cuda_stream, runner=self.runners[i], **self.nms_args)
        self._native_boxes(self.runners[i], ns.cuda_stream)
        out = (det[None], count[None])
        if self.gather:
            out = self._gather(self.runners[i].block, 0)
        if self.overlap:
            self.nms_done[i].record(ns)
        self.n += 1
        self.last = out
        return out

    def _gather(self, send, slot):
        """Step bookkeeping of the collective: returns the (det, count) views of this step inside the generation the NEXT gather writes, and
        issues that gather when the group is complete (or from synchronize(), for a group cut short).  `send` = what this rank contributes:
        one slot's block (one-plan pipeline) or the whole group_block."""
        B, max_det = self.runners[0].B, self.runners[0].max_det
        out = D.split_group_block(self.gathered[self.gen], self.world if self.world > 1 else 1, self.group, slot, B, max_det)
        self._send = send
        self.pending += 1
        if self.pending >= self.group:
            self._issue_gather()
        return out

    def _issue_gather(self):
        import torch.distributed as tdist
        ns, gs = self.nms_stream, self.gather_stream
        if gs is not ns:
            self.nms_group_done.record(ns)
            gs.wait_event(self.nms_group_done)              # behind the group's last NMS; the NMS stream itself goes on with the next batch
        with torch.cuda.stream(gs):
            tdist.all_gather_into_tensor(self.gathered[self.gen], self._send)
        self.gather_done.record(gs)
        self.gen ^= 1
        self.pending = 0
        self.gathers += 1

    def _step_deep(self):
        """Several plans: batch n runs plan n % nplans on forward stream n % depth (nplans is a multiple of depth: a plan keeps its stream); its NMS reads that plan's z directly (no snapshot: the
        plan is not replayed before its NMS has finished — which also orders the replay behind the plan's previous forward)."""
        pi = self.n % self.nplans
        fs, ns, plan = self.fwd_streams[pi % self.depth], self.nms_stream, self.plans[pi]
        if self.n >= self.nplans:
            fs.wait_event(self.nms_done_deep[pi])          # NMS of batch n - nplans has finished reading this plan's z
        plan.run(fs.cuda_stream)
        self.fwd_done[pi].record(fs)
        ns.wait_event(self.fwd_done[pi])
        if self.gather and self.gathers and self.pending == 0:
            ns.wait_event(self.gather_done)                # the last gather has read the blocks this group's NMS launches overwrite
        det, count, keep = nms_device(self._z(plan), stream_ptr=ns.cuda_stream, runner=self.deep_runners[pi], **self.nms_args)
        self._native_boxes(self.deep_runners[pi], ns.cuda_stream)
        out = (det[None], count[None])
        if self.gather:
            out = self._gather(self.group_block, pi)
        self.nms_done_deep[pi].record(ns)
        self.n += 1
        self.last = out
        return out

    def synchronize(self):
        """Everything enqueued so far has finished.  With a process group this also sends a group that is not full yet (every rank has taken
        the same number of steps, so every rank issues the same collectives)."""
        if self.gather and self.pending:
            self._issue_gather()
        for fs in self.fwd_streams:
            fs.synchronize()
        self.nms_stream.synchronize()
        if self.gather_stream is not self.nms_stream:
            self.gather_stream.synchronize()

    def __call__(self, rgb, ir):
        """Convenience: copy one batch in, run it, wait, return list of (n, 6) detections per image (all ranks' images, global order)."""
        det, count = self.submit(rgb, ir)
        self.synchronize()
        det, count = D.flatten_gathered(det, count)
        return [det[k, :n].clone() for k, n in enumerate(count.tolist())]
