"""Two-stream model assembly: `Model(cfg, ch=3, nc=None, anchors=None)` with the reference's construction API.

Semantics follow the reference's models/yolo_test.py (the file train.py / test.py actually import — the shipped
models/yolo.py is single-stream and broken): `forward(x, x2, augment=False, profile=False)` returns
`(z, logits, [raw x3])` in eval mode; layers carry `.i .f .type .np`; `from == -4` feeds the IR image; Detect
strides are fixed to [8, 16, 32] (models/yolo_test.py:104).

What differs is how a forward executes: the layer graph is compiled once per input shape into an `engine.Plan`
(flat list of HIP launches over NHWC buffers, Concat inputs written in place, optional hipGraph replay) instead of
being interpreted layer by layer in Python.
"""
import logging
import math
from copy import deepcopy
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..engine import ImageIn, Plan, TtaPlan
from .common import (C3, SPPF, Add, Bottleneck, Concat, Conv, Detect, HipModule, Lead, NiNfusion,  # noqa: F401
                     ResNetblock, ResNetlayer, TransformerFusionBlock, VGGblock, VirtualCat, emit_upsample)

logger = logging.getLogger(__name__)
_NAMESPACE = {"Conv": Conv, "C3": C3, "SPPF": SPPF, "Bottleneck": Bottleneck, "Concat": Concat, "Detect": Detect,
              "TransformerFusionBlock": TransformerFusionBlock, "NiNfusion": NiNfusion, "Add": Add, "VGGblock": VGGblock, "ResNetlayer": ResNetlayer, "nn": nn}


def make_divisible(x, divisor):
    return math.ceil(x / divisor) * divisor


# Test-time augmentation: the passes of the reference's Model.forward(augment=True) (models/yolo_test.py:118-119)
TTA_SCALES = (1, 0.83, 0.67)
TTA_FLIPS = (None, 3, None)            # 3 = left-right (x.flip(3)); the reference's set has no up-down flip


def tta_sizes(H, W, gs=32):
    """[(scale, flip, Hr, Wr, Hp, Wp)] of the passes for an H x W input: scale_img (utils/torch_utils.py:257-267) resizes to
    (int(H * s), int(W * s)) and pads to the next multiple of gs of H * s / W * s, all in Python double arithmetic; ratio 1 returns the
    input unchanged.  640 x 640: 531 -> 544 and 428 -> 448."""
    out = []
    for s, f in zip(TTA_SCALES, TTA_FLIPS):
        if s == 1.0:
            out.append((s, f, H, W, H, W))
        else:
            out.append((s, f, int(H * s), int(W * s), math.ceil(H * s / gs) * gs, math.ceil(W * s / gs) * gs))
    return out


def check_anchor_order(m):
    """Flip anchor order if it disagrees with stride order (reference utils/autoanchor.py:12-20)."""
    a = m.anchor_grid.prod(-1).view(-1)
    da, ds = a[-1] - a[0], m.stride[-1] - m.stride[0]
    if da.sign() != ds.sign():
        m.anchors[:] = m.anchors.flip(0)
        m.anchor_grid[:] = m.anchor_grid.flip(0)


def fuse_conv_and_bn(conv, bn):
    """Offline Conv+BN fold with the reference's signature (utils/torch_utils.py:182-202)."""
    fused = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                      groups=conv.groups, bias=True).requires_grad_(False).to(conv.weight.device, conv.weight.dtype)
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    fused.weight.copy_(conv.weight * scale[:, None, None, None])
    b = conv.bias if conv.bias is not None else torch.zeros_like(bn.running_mean)
    fused.bias.copy_((b - bn.running_mean) * scale + bn.bias)
    return fused


def parse_model(d, ch):
    """yaml dict -> (nn.Sequential, save list).  Row format and channel arithmetic as the reference's
    models/yolo_test.py:216-302, restricted to the module set of the *_Transfusion_* configs."""
    anchors, nc, gd, gw = d["anchors"], d["nc"], d["depth_multiple"], d["width_multiple"]
    na = (len(anchors[0]) // 2) if isinstance(anchors, list) else anchors
    no = na * (nc + 5)
    scope = dict(_NAMESPACE, nc=nc, anchors=anchors, **{"None": None})
    layers, save, c2 = [], [], ch[-1]
    for i, (f, n, m, args) in enumerate(d["backbone"] + d["head"]):
        if isinstance(m, str):
            try:
                m = eval(m, {"__builtins__": {}}, scope)
            except Exception as e:
                raise NotImplementedError(f"module '{m}' is not part of the MI355X hot path (SURVEY.md §2)") from e
        args = list(args)
        for j, a in enumerate(args):
            if isinstance(a, str):
                try:
                    args[j] = eval(a, {"__builtins__": {}}, scope)
                except Exception:
                    pass
        n = max(round(n * gd), 1) if n > 1 else n
        if m in (Conv, Bottleneck, SPPF, C3):
            first_layer = m is Conv and args[0] == 64       # both stream stems take the 3-channel image (:240)
            c1, c2 = (3 if first_layer else ch[f]), args[0]
            if c2 != no:
                c2 = make_divisible(c2 * gw, 8)
            args = [c1, c2, *args[1:]]
            if m is C3:
                args.insert(2, n)
                n = 1
        elif m is VGGblock:                                   # reference models/yolo_test.py:260-261: (num_convs, c1, c2) as written
            c2 = args[2]
        elif m is ResNetlayer:                                # reference models/yolo_test.py:255-259: (c1, c2, stride, is_first, num_blocks) as
            c2 = args[1] if args[3] is True else args[1] * 4  # written; the stem row keeps c2, every other row ends on expansion * c2
        elif m is Concat:
            c2 = sum(ch[x] for x in f)
        elif m is Detect:
            args.append([ch[x] for x in f])
            if isinstance(args[1], int):
                args[1] = [list(range(args[1] * 2))] * len(f)
        elif m is NiNfusion:                                  # reference models/yolo_test.py:280-283
            c1 = sum(ch[x] for x in f)
            c2 = c1 // 2
            args = [c1, c2, *args]
        elif m is Add:                                        # :266-268 — the yaml argument is REPLACED by the channel count,
            c2 = ch[f[0]]                                     # which therefore becomes Add's weight (kept as the reference does)
            args = [c2]
        elif m is TransformerFusionBlock:
            c2 = ch[f[0]]
            # positional arguments exactly as the reference passes them (models/yolo_test.py:284-286: args = [c2, *args[1:]],
            # i.e. vert_anchors, horz_anchors, h, block_exp, ...); the parameter-shared iteration count, which the reference
            # wires but never surfaces (models/common.py:691,744), is an optional trailing mapping: [1024, 10, 10, {loops_num: 3}]
            extra = dict(args.pop()) if args and isinstance(args[-1], dict) else {}
            if set(extra) - {"loops_num"}:
                raise ValueError(f"TransformerFusionBlock: unknown yaml keyword(s) {sorted(set(extra) - {'loops_num'})}")
            args = [c2, *args[1:]]
            m_ = m(*args, **extra)
        else:
            c2 = ch[f]
        if m is not TransformerFusionBlock:
            m_ = nn.Sequential(*[m(*args) for _ in range(n)]) if n > 1 else m(*args)
        t = str(m)[8:-2].replace("__main__.", "")
        np_ = sum(x.numel() for x in m_.parameters())
        m_.i, m_.f, m_.type, m_.np = i, f, t, np_
        logger.info("%3s%18s%3s%10.0f  %-40s%-30s" % (i, f, n, np_, t, args))
        save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
        layers.append(m_)
        if i == 0:
            ch = []
        ch.append(c2)
    return nn.Sequential(*layers), sorted(save)


def emit_any(m, plan, src, out=None, twin=None, lead=None):
    """Emit one yaml row: our HipModules, torch's nn.Upsample, or an nn.Sequential repeat of either.  `twin` is the
    same row of the other backbone stream when both run as one paired launch sequence."""
    if isinstance(m, nn.Upsample):
        return emit_upsample(m, plan, src, out=out)
    if isinstance(m, nn.Sequential):
        mods = list(m)
        for j, sub in enumerate(mods):
            src = emit_any(sub, plan, src, out if j == len(mods) - 1 else None, twin[j] if twin is not None else None)
        return src
    if not hasattr(m, "emit"):
        raise NotImplementedError(f"layer type {type(m).__name__} is outside the hot path")
    return m.emit(plan, src, **{k: v for k, v in (("out", out), ("twin", twin), ("lead", lead)) if v is not None})


def out_shape_any(m, src):
    """(C, H, W) one yaml row makes of its source shape(s): the row's own rule (`out_shape`), torch's nn.Upsample, an nn.Sequential repeat."""
    if isinstance(m, nn.Upsample):
        s = int(m.scale_factor)
        return src[0], src[1] * s, src[2] * s
    if isinstance(m, nn.Sequential):
        for sub in m:
            src = out_shape_any(sub, src)
        return src
    if not hasattr(m, "out_shape"):
        raise NotImplementedError(f"layer type {type(m).__name__} is outside the hot path")
    return m.out_shape(src)


def _same_structure(a, b):
    """May rows a and b run as one groups = 2 launch sequence?  Same type, and equal in everything the type says must match."""
    if type(a) is not type(b):
        return False
    if isinstance(a, nn.Sequential):
        return len(a) == len(b) and all(_same_structure(x, y) for x, y in zip(a, b))
    return hasattr(a, "pair_signature") and a.pair_signature() == b.pair_signature()


class Model(HipModule):
    # Execution switches of the MI355X implementation.  They are CLASS-level defaults on purpose: reference checkpoints are
    # whole pickled Model objects (train.py:424-435) whose __dict__ is restored without running this __init__, so every
    # attribute the reference does not know must resolve through the class (set it on an instance to override).
    compute_dtype = None     # None: the parameters' dtype (.half() / .bfloat16() as in the reference);
    #                          set to torch.bfloat16 / float16 to keep fp32 masters and only pack in 16 bit
    autotune = False         # device-time every igemm configuration once per plan and keep the fastest
    use_graph = False        # replay each plan as one hipGraph launch
    pair_streams = True      # run structurally identical RGB / IR backbone rows as one groups=2 launch
    branch_dmff = True       # capture the shallow DMFF blocks as parallel branches of the hipGraph
    # Upsample -> Concat -> C3: run the up-sampled half of the C3's 1x1 at low resolution (C3.emit, VirtualCat).  Built and
    # tested, OFF by default: the pre-term GEMMs only exist on the 4-wavefront tiles and the forward got 1.1 % slower
    # (2.573 vs 2.544 ms, same-box A/B) although two up-sampling launches and 40 % of those GEMMs' FLOPs disappear.
    fold_upsample = False
    static_outputs = False   # return views of plan-owned buffers instead of clones
    plan_cache_bytes = 64 << 30     # LRU cap on the plan-owned buffers of all cached (B, H, W, dtype) plans; None = unbounded

    def __init__(self, cfg="yolov5s.yaml", ch=3, nc=None, anchors=None):
        super().__init__()
        if isinstance(cfg, dict):
            self.yaml = cfg
        else:
            import yaml
            self.yaml_file = Path(cfg).name
            with open(cfg) as f:
                self.yaml = yaml.safe_load(f)
        ch = self.yaml["ch"] = self.yaml.get("ch", ch)
        if nc and nc != self.yaml["nc"]:
            logger.info(f"Overriding model.yaml nc={self.yaml['nc']} with nc={nc}")
            self.yaml["nc"] = nc
        if anchors:
            logger.info(f"Overriding model.yaml anchors with anchors={anchors}")
            self.yaml["anchors"] = round(anchors)
        self.model, self.save = parse_model(deepcopy(self.yaml), ch=[ch])
        self.names = [str(i) for i in range(self.yaml["nc"])]
        m = self.model[-1]
        if isinstance(m, Detect):
            m.stride = torch.Tensor([8.0, 16.0, 32.0])
            m.anchors /= m.stride.view(-1, 1, 1)
            check_anchor_order(m)
            self.stride = m.stride
        for mod in self.modules():                      # utils/torch_utils.py:144-154 (initialize_weights)
            if type(mod) is nn.BatchNorm2d:
                mod.eps, mod.momentum = 1e-3, 0.03

    # -- reference API ----------------------------------------------------------------------------------------
    def forward(self, x, x2, augment=False, profile=False):
        """augment=True: test-time augmentation, `(torch.cat(y, 1), None)` over the passes (scale, flip) = (1, -), (0.83, left-right),
        (0.67, -) of the reference's models/yolo_test.py:116-131: each pass runs scale_img (utils/torch_utils.py:257-267) of the
        (flipped) images through the plain forward, its boxes are divided by the scale and mirrored back, rows in pass order.  The
        reference's own loop is broken for the two-stream model (:122-123 scale only `x` and call forward_once(xi) without the second
        image: a TypeError); what it plainly means is built: the SAME flip and scale for both modalities.  Inputs whose 0.67 pass
        would hand a DMFF block a map smaller than its anchor grid raise ValueError (tta_min_size)."""
        if augment:
            return self._forward_augment(x, x2)
        return self.forward_once(x, x2, profile)

    def tta_min_size(self):
        """Smallest (H, W) forward(augment=True) accepts, derived from the model: the positional embedding of a
        TransformerFusionBlock has vert_anchors x horz_anchors rows (models/common.py:817-823), so the map it reads — the padded
        size of the SMALLEST pass over the stride of the rows feeding it — must not be smaller than that grid."""
        gs = int(self.stride.max())
        probe = 32 * gs
        shapes = self._layer_shapes(1, probe, probe)
        need_h = need_w = gs
        for m in self.model:
            if isinstance(m, TransformerFusionBlock) and not isinstance(m.f, int):
                _, h, w = shapes[m.f[0]]
                need_h, need_w = max(need_h, m.vert_anchors * (probe // h)), max(need_w, m.horz_anchors * (probe // w))

        def smallest(need):          # the smallest multiple of gs whose every pass is padded to at least `need`
            v = gs
            while min(p[4] for p in tta_sizes(v, v, gs)) < need:
                v += gs
            return v
        return smallest(need_h), smallest(need_w)

    def tta_plan_for(self, B, H, W, device="cuda", dtype=None, u8=False, slot=0, branches=True):
        """The engine.TtaPlan of forward(augment=True) / forward_u8(augment=True) for this shape: the full-size plan (u8: fed by the
        uint8 batch) and one ordinary fp32-input plan per scaled pass, all from plan_for — cached beside them under the same cap.
        They ARE the cached plans of those shapes and slots (a plain forward at 544 x 544 replays the plan a 640 x 640 TTA step uses for
        its 0.83 pass): as with plan_for, two users of one slot must not be in flight at the same time."""
        gs = int(self.stride.max())
        self._check_stride(H, W, gs)
        min_h, min_w = self.tta_min_size()
        if H < min_h or W < min_w:
            raise ValueError(f"test-time augmentation needs an input of at least {min_h}x{min_w}, got {H}x{W}: the "
                             f"{min(TTA_SCALES)} pass must not hand a DMFF block a map smaller than its anchor grid")
        dt, device, key = self._plan_key(B, H, W, device, dtype, u8, slot, branches, tta=True)
        plans = self.__dict__.setdefault("_plans", {})
        tp = plans.pop(key, None)
        if tp is None:
            passes = tta_sizes(H, W, gs)
            # passes padded to the SAME size (inputs of a stride or two: 32 x 32 pads every pass to 32 x 32) need plans of their own — one plan
            # cannot hold two passes' inputs: the k-th repeat of a size takes the plan of slot + 100 k
            seen, subs = {}, []
            for i, p in enumerate(passes):
                k = seen.get((p[4], p[5], u8 and i == 0), 0)
                seen[(p[4], p[5], u8 and i == 0)] = k + 1
                subs.append(self.plan_for(B, p[4], p[5], device, dt, u8=u8 and i == 0, slot=slot + 100 * k, branches=branches))
            full = subs[0]
            src = full.inputs[0] if u8 else full.input_pair
            stage = ops.tta_stage(src, [(sp.input_pair, p[2], p[3], p[1] == 3) for sp, p in zip(subs[1:], passes[1:])])
            zs = [sp.outputs[0] for sp in subs]
            merged = torch.zeros((B, sum(z.shape[1] for z in zs), zs[0].shape[2]), dtype=torch.float32, device=device)
            merge = ops.tta_merge(zs, [p[0] for p in passes], [p[1] == 3 for p in passes], merged, W)
            tp = TtaPlan(subs, stage, merge, merged, passes)
            plans = self.__dict__.setdefault("_plans", {})
        plans[key] = tp
        return tp

    def _forward_augment(self, x, x2=None):
        """x, x2: the fp image pair, or x alone: the uint8 (B, 6, H, W) batch."""
        return self._forward_images((x,) if x2 is None else (x, x2), u8=x2 is None, augment=True)

    def fuse(self):
        """Fold BatchNorm into the convs in place (reference models/yolo_test.py:182-190).  A VGGblock has none: nothing to fold.  A
        ResNetlayer keeps its BatchNorms, as in the reference (its fuse() only touches Conv): they are folded when the weights are packed."""
        for m in self.model.modules():
            if type(m) is Conv and hasattr(m, "bn"):
                with torch.no_grad():
                    m.conv = fuse_conv_and_bn(m.conv, m.bn)
                delattr(m, "bn")
        self.invalidate()
        return self

    def info(self, verbose=False, img_size=640):
        n_p = sum(p.numel() for p in self.parameters())
        logger.info(f"Model Summary: {len(list(self.modules()))} layers, {n_p} parameters")

    # -- plan construction ------------------------------------------------------------------------------------
    def _layer_shapes(self, B, H, W):
        """Static (C, H, W) of every layer output, needed to place Concat inputs before they are produced."""
        shapes = []
        for m in self.model:
            shapes.append(out_shape_any(m, self._source(m, (3, H, W), (3, H, W), shapes)))
        return shapes

    @staticmethod
    def _source(m, rgb, ir, outs):
        """What row m reads, by its `from`: the RGB / IR network input, the previous row's output, one earlier row's or a list of them."""
        if m.f == -4 or (m.f == -1 and m.i == 0):
            return ir if m.f == -4 else rgb
        prev = outs[-1] if outs else None
        return prev if m.f == -1 else outs[m.f] if isinstance(m.f, int) else [prev if j == -1 else outs[j] for j in m.f]

    def stream_twins(self):
        """{IR-stream row -> RGB-stream row} for the leading run of rows that are pure chains (from = -1) with
        identical structure in both backbones.  Those rows run as ONE launch sequence over pair acts
        (groups = 2: per-stream weights, gridDim.z = stream): half the launches, twice the workgroups each."""
        ir0 = next((m.i for m in self.model if m.f == -4), None)
        twins = {}
        if not self.pair_streams or ir0 is None or self.model[0].f != -1:
            return twins
        for k in range(min(ir0, len(self.model) - ir0)):
            a, b = self.model[k], self.model[ir0 + k]
            if a.f != -1 or b.f != (-4 if k == 0 else -1) or not _same_structure(a, b):
                break
            twins[ir0 + k] = k
        return twins

    def build_plan(self, B, H, W, device, dtype, u8=False):
        """u8=False: inputs are two fp32 NCHW images in [0, 1] (what the reference hands `model(img_rgb, img_ir)`);
        u8=True: ONE uint8 (B, 6, H, W) tensor, the dataloader's RGB+IR batch — `/255`, the channel split and the cast
        happen in the staging kernel (reference test.py:116-123).
        A sequence of passes; plan-owned buffers are allocated in this order: inputs, concat buffers, DMFF pair buffers (each in row
        order), then whatever emission allocates."""
        plan = Plan(device, dtype)
        images = self._plan_inputs(plan, B, H, W, u8)
        shapes = self._layer_shapes(B, H, W)
        virtual = self._upsample_folds()
        placement = self._place_concats(plan, B, shapes, virtual)
        dmff_pair = self._pair_dmff_inputs(plan, B, shapes, placement)
        twins = self._twin_run(placement)
        spans = self._emit_rows(plan, images, virtual, placement, dmff_pair, twins)
        if self.branch_dmff:
            self._assign_branches(plan, spans)
        return plan

    @staticmethod
    def _plan_inputs(plan, B, H, W, u8):
        """Allocates the staging buffer(s) and sets plan.inputs / plan.input_pair -> (both streams, RGB, IR) as ImageIn."""
        if u8:
            img6 = torch.zeros((B, 6, H, W), dtype=torch.uint8, device=plan.device)
            plan.inputs, plan.input_pair = [img6], None
            return ImageIn(img6, 0, pair=True), ImageIn(img6, 0), ImageIn(img6, 3)
        imgs = torch.zeros((2, B, 3, H, W), dtype=torch.float32, device=plan.device)   # RGB and IR staging, adjacent
        plan.inputs, plan.input_pair = [imgs[0], imgs[1]], imgs     # input_pair: both as one (2, B, 3, H, W) tensor
        return ImageIn(imgs), ImageIn(imgs[0]), ImageIn(imgs[1])

    def _row(self, i):
        return self.model[i] if i < len(self.model) else None

    def _upsample_folds(self):
        """Reads the yaml rows -> {Concat row: Upsample row} of every nn.Upsample -> Concat([-1, j]) -> C3 run (head rows 24-26, 28-30) when
        `fold_upsample` is set: the C3's first 1x1 commutes with the nearest up-sampling, so neither the up-sampled tensor nor the concat
        buffer is materialised (C3.emit, VirtualCat)."""
        virtual, used = {}, {}
        if not self.fold_upsample:
            return virtual
        for m in self.model:
            for j in ([m.f] if isinstance(m.f, int) else m.f):
                used.setdefault(m.i - 1 if j == -1 else j, []).append(m.i)
        for m in self.model:
            nxt, nx2 = self._row(m.i + 1), self._row(m.i + 2)
            if (isinstance(m, nn.Upsample) and m.f == -1 and m.i > 0 and m.mode == "nearest" and m.scale_factor is not None
                    and float(m.scale_factor) == int(m.scale_factor) and isinstance(nxt, Concat) and nxt.d == 1
                    and not isinstance(nxt.f, int) and len(nxt.f) == 2 and nxt.f[0] == -1 and isinstance(nxt.f[1], int)
                    and nxt.f[1] >= 0 and isinstance(nx2, C3) and nx2.f == -1 and used.get(m.i) == [nxt.i]
                    and used.get(nxt.i) == [nx2.i]):
                virtual[nxt.i] = m.i
        return virtual

    def _place_concats(self, plan, B, shapes, virtual):
        """Reads the Concat rows that are not folded away (`virtual`); allocates one buffer per Concat, in row order -> {producer row:
        (concat buffer, channel offset, channels)}: the producers write their slice of it."""
        placement = {}
        for m in self.model:
            if isinstance(m, Concat) and not isinstance(m.f, int) and m.i not in virtual:
                srcs = [m.i - 1 if j == -1 else j for j in m.f]
                if any(s in placement for s in srcs):
                    continue                       # a producer can live in only one concat buffer
                C, h, w = shapes[m.i]
                buf, off = plan.act(B, h, w, C), 0
                for s in srcs:
                    placement[s] = (buf, off, shapes[s][0])
                    off += shapes[s][0]
        return placement

    def _pair_dmff_inputs(self, plan, B, shapes, placement):
        """Reads the fusion rows and `placement`; allocates one (B, H, W, 2C) buffer per row whose two inputs are free, in row order -> {input row:
        (buffer, channel offset, C, the other input row)}: adjacent channel slices, so the 1x1 fuse conv reads cat(rgb, ir) in place (common.py)."""
        dmff_pair = {}
        for m in self.model:
            if (isinstance(m, NiNfusion) or (isinstance(m, TransformerFusionBlock) and m.fuse_tail)) \
                    and not isinstance(m.f, int) and len(m.f) == 2:
                i, j = m.f
                if i in placement or j in placement or i in dmff_pair or j in dmff_pair or shapes[i] != shapes[j]:
                    continue
                C, h, w = shapes[i]
                buf = plan.act(B, h, w, 2 * C)
                dmff_pair[i], dmff_pair[j] = (buf, 0, C, j), (buf, C, C, i)
        return dmff_pair

    def _twin_run(self, placement):
        """stream_twins() — a prefix run by construction — cut at the first row that a Concat placement pins to another buffer."""
        twins = self.stream_twins()
        ir0, run = min(twins, default=None), 0
        while ir0 is not None and (ir0 + run) in twins and run not in placement and (ir0 + run) not in placement:
            run += 1
        return {ir0 + k: k for k in range(run)}

    def _emit_rows(self, plan, images, virtual, placement, dmff_pair, twins):
        """Reads the maps of the passes above; appends every row's launches to `plan` in yaml order (a twin run's IR rows with their RGB
        rows) and sets plan.outputs -> {row: (its first launch, the end of its launches, emitted on its own)}."""
        in_pair, in_rgb, in_ir = images
        ir0, rgb_rows = min(twins, default=None), set(twins.values())
        y, spans, pair_out, lead = [], {}, {}, {}

        def done(x, *rows, own=False):              # every exit of the row loop: the row's output, and whose launches these were
            y.append(x)
            for r in rows:
                spans[r] = (n0, len(plan.launches), own)
        for m in self.model:
            n0 = len(plan.launches)
            if m.i in rgb_rows:                     # both streams in one paired launch sequence
                po = pair_out[m.i] = self._emit_twin_row(plan, m, in_pair if m.i == 0 else pair_out[m.i - 1], ir0, rgb_rows, lead, dmff_pair)
                done(None if po is None else po[0], m.i, ir0 + m.i)
            elif m.i in twins:                      # already emitted with its RGB twin
                po = pair_out[twins[m.i]]
                done(None if po is None else po[1])
            else:
                x = self._emit_own_row(plan, m, self._source(m, in_rgb, in_ir, y), virtual, placement, dmff_pair)
                done(x, m.i, own=m.i not in virtual and virtual.get(m.i + 1) != m.i)
        plan.outputs = y[-1]
        return spans

    @staticmethod
    def _defer(lead, row, convs, src):
        """This row launches nothing: `convs` (a Lead, with its input `src`) is emitted inside the launch of `row`, which pops it from `lead`."""
        lead[row] = (convs, src)

    def _emit_twin_row(self, plan, m, src, ir0, rgb_rows, lead, dmff_pair):
        """RGB row m and its IR twin as one launch sequence over the pair act / image pair `src` -> their pair act, or None when the row
        is deferred into a later row's launch (`lead`: {that row: (the Lead in front of it, its input)})."""
        i, twin, nxt, nx2 = m.i, self.model[ir0 + m.i], self._row(m.i + 1), self._row(m.i + 2)
        if (i == 0 and isinstance(m, Conv) and isinstance(nx2, C3) and {1, 2} <= rgb_rows and nxt.f == -1
                and nx2.f == -1 and not ({0, 1, ir0, ir0 + 1} & (set(self.save) | set(dmff_pair)))
                and m.stem2_ok(plan, src, nxt, nx2)):
            return self._defer(lead, 1, Lead(m, twin), src)          # rows 0-2a become one launch, emitted with the C3 row
        if i == 1 and 1 in lead:                                     # ... the 3x3 behind that stem
            stem, image = lead.pop(1)
            return self._defer(lead, 2, Lead(m, twin, stem.conv, stem.twin), image)
        if (isinstance(m, Conv) and i > 0 and isinstance(nxt, C3) and (i + 1) in rgb_rows and nxt.f == -1
                and i not in self.save and (ir0 + i) not in self.save and i not in dmff_pair
                and m.chain_ok(plan, nxt)):
            return self._defer(lead, i + 1, Lead(m, twin), src)      # a down-sampling Conv, emitted together with the C3 row
        convs, src = lead.pop(i, (None, src))
        pout = None
        if i in dmff_pair and dmff_pair[i][3] == ir0 + i:            # pair act = the two halves of the DMFF buffer
            buf, _, c, _ = dmff_pair[i]
            Bb, h, w, _ = buf.shape
            pout = buf.as_strided((2, Bb, h, w, c), (c, h * w * 2 * c, w * 2 * c, 2 * c, 1))
        return emit_any(m, plan, src, pout, twin=twin, lead=convs)

    @staticmethod
    def _emit_own_row(plan, m, src, virtual, placement, dmff_pair):
        """A row outside the twin run, from its source(s) `src` -> its output: written into its slice of a concat / DMFF pair buffer where
        one is placed; a folded Upsample / Concat row launches nothing and returns a description for the C3 behind it."""
        if virtual.get(m.i + 1) == m.i:                              # the Upsample row of a fold
            return src, int(m.scale_factor)
        if m.i in virtual:                                           # its Concat: a description of cat(up(low), other)
            (low, scale), other = src
            return VirtualCat(low, scale, other)
        buf, off, c = (placement.get(m.i) or dmff_pair.get(m.i) or (None, 0, 0))[:3]
        return emit_any(m, plan, src, None if buf is None else buf[..., off:off + c])

    def _assign_branches(self, plan, spans):
        """Reads the rows' launch ranges (`spans`, _emit_rows); tags launches with graph-branch ids and fills plan.branches.  DMFF blocks other
        than the last one become side branches of the captured graph: they depend only on their two backbone rows and nothing needs them before
        the head, so they overlap with the deeper backbone rows and are joined before the first head launch.  Detect levels fed by earlier head
        rows (P3, P4) only need that row: their 1x1 conv + decode run beside the remaining head rows and are joined at the end of the graph."""
        def branch(first, end, after, row):
            bid = len(plan.branches) + 1
            for l in plan.launches[first:end]:
                l.branch = bid
            plan.branches[bid] = {"after": after, "join_before": None, "row": row}
        dmff_rows = [m.i for m in self.model if isinstance(m, (TransformerFusionBlock, NiNfusion, Add))]
        for m in self.model:
            f, (n0, n1, own) = m.f, spans[m.i]
            if not own:
                continue
            if m.i in dmff_rows[:-1] and not isinstance(f, int) and n1 > n0:
                branch(n0, n1, max(spans[j][1] - 1 for j in f), m.i)
            elif dmff_rows and m.i == dmff_rows[-1] + 1:
                for b in plan.branches.values():
                    if b["join_before"] is None:
                        b["join_before"] = n0
            if isinstance(m, Detect) and not isinstance(f, int):
                per = (n1 - n0) // len(f)
                for lvl, j in enumerate(f[:-1]):
                    if per * len(f) == n1 - n0 and spans[j][1] < n0:
                        branch(n0 + lvl * per, n0 + (lvl + 1) * per, spans[j][1] - 1, m.i)

    def _check_eval(self):
        if self.training:
            raise NotImplementedError("icafusion_amd implements the eval-mode inference path only (call .eval())")

    @staticmethod
    def _check_images(*images):
        if not all(t.is_cuda for t in images):
            raise RuntimeError("icafusion_amd.Model runs on the MI355X only: move the model and inputs to cuda "
                               "(no CPU fallback exists; the CPU reference is oracle/icaf_oracle.py, test-only)")
        if len(images) == 2 and images[0].shape != images[1].shape:
            raise ValueError(f"RGB and IR batches must match, got {tuple(images[0].shape)} vs {tuple(images[1].shape)}")

    @staticmethod
    def _check_stride(H, W, gs=32):
        if H % gs or W % gs:
            raise ValueError(f"input size {H}x{W} must be a multiple of the max stride {gs}")

    @staticmethod
    def _feed(plan, *images):
        for dst, t in zip(plan.inputs, images):
            if t.data_ptr() != dst.data_ptr():
                dst.copy_(t)

    def _result(self, out):
        """plan.outputs — the (z, logits, raws) triple, or a TTA plan's merged tensor — as views if `static_outputs`, else as clones."""
        if self.static_outputs:
            return out
        return out.clone() if torch.is_tensor(out) else type(out)(self._result(t) for t in out)

    def _forward_images(self, images, u8=False, augment=False, profile=False):
        """The front end proper: check, find the plan (augment: the TTA plan, which checks the size itself), feed it, run it, hand out its outputs."""
        self._check_eval()
        self._check_images(*images)
        B, _, H, W = images[0].shape
        if not augment:
            self._check_stride(H, W)
        plan = (self.tta_plan_for if augment else self.plan_for)(B, H, W, images[0].device, u8=u8)
        self._feed(plan, *images)
        if profile and not augment:
            for name, ms, flops, nbytes in plan.timed_run():
                logger.info(f"{ms:10.3f} ms {flops / 1e9:10.2f} GFLOP  {name}")
        else:
            plan.run()
        out = self._result(plan.outputs)
        return (out, None) if augment else out

    def forward_once(self, x, x2, profile=False):
        return self._forward_images((x, x2), profile=profile)

    def forward_u8(self, img6, augment=False):
        """Forward from the dataloader's uint8 (B, 6, H, W) RGB+IR batch (reference test.py:116-128 does
        `.to(device).float() / 255`, splits `[:, :3]` / `[:, 3:]`, then `model(img_rgb, img_ir)`): same outputs as
        forward(), one quarter of the input bytes, no fp32 image ever materialised.  augment=True: as forward(augment=True),
        the scaled passes staged straight from the uint8 batch."""
        self._check_eval()
        if not img6.is_cuda or img6.dtype != torch.uint8 or img6.dim() != 4 or img6.shape[1] != 6:
            raise ValueError("forward_u8 expects a cuda uint8 tensor of shape (B, 6, H, W)")
        return self._forward_images((img6,), u8=True, augment=augment)

    def forward_frames(self, rgb, ir, img_size=640, bgr=True, augment=False, val_size=None, formats=None, yuv_matrix="bt601", align=None,
                       align_border=0, agc_clip=(100, 100), agc_window=None):
        """Forward from NATIVE camera frames: rgb / ir are cuda uint8 tensors (B, H0, W0, ch) in decoder layout (interleaved, ch = 3 or
        1) or lists of (H0_i, W0_i, ch) tensors for ragged sizes; a pair shares its size.  The letterbox to img_size (an int or (H, W);
        utils.datasets.letterbox, byte for byte) runs on the device straight into the uint8 plan's input, then the plan (or the TTA plan)
        replays: the result is bit-identical to forward_u8 of the host-letterboxed batch.  bgr=True: frames are BGR as imread_bgr / cv2
        deliver them (the planes become RGB, LoadImages' `[:, :, ::-1]`).  Returns (forward_u8's result, FrameGeometry): .scale is the
        cuda (B, 5) rows {gain, pad_x, pad_y, w0, h0} ops.scale_detections takes, .scale_host / .geom their host twins.  Frames are
        copied into an arena owned by the model; after the first call of a set of shapes nothing is allocated.
        val_size (an int): the VALIDATION loader's geometry instead (PairedValSet; ops.val_geometry(shapes, val_size, img_size)) — longest
        side to val_size (pixel-area average when shrinking, utils.datasets.resize_area_scalar byte for byte; bilinear when growing), then
        padded into img_size, the batch's letterbox shape; .scale then holds test.py's ratio_pad rows.
        formats=(fmt_rgb, fmt_ir): a modality that arrives as YUV 4:2:0 names its layout, "nv12" | "nv21" | "i420" | "yv12" (None: the
        interleaved frames above), and is handed over as the contiguous buffer a decoder returns — one uint8 (B, 3 * H0 // 2, W0) tensor
        or a list of (3 * H0_i // 2, W0_i) tensors, H0 and W0 even; the frame size comes from the other modality, or from the buffers when
        both are YUV.  yuv_matrix: "bt601" | "bt709" | "bt601-full" (or 0 / 1 / 2).  The colour conversion runs inside the letterbox
        (icaf_letterbox_yuv_frames); the result is bit-identical to forward_u8 of letterbox(utils.datasets.yuv420_to_bgr(...)).
        align=(A_rgb, A_ir): a CALIBRATED pair whose cameras differ in size and pose.  Exactly one entry is not None: a (3, 3) array (one
        rig, every pair), a (B, 3, 3) array (per pair) or "stretch" (same field of view, other resolution), mapping ALIGNED pixel
        coordinates to that modality's SOURCE pixel coordinates (utils.datasets.warp_perspective; cv2's WARP_INVERSE_MAP matrix).  That
        modality may have any size per frame; the OTHER modality's frame size is the aligned size and its letterbox the pair's, so boxes
        and FrameGeometry are in the un-warped modality's native space.  The homography is applied at the letterbox's taps
        (icaf_letterbox_warp_frames; pixels the source does not cover are align_border, 0..255): bit-identical to forward_u8 of
        letterbox(warp_perspective(frame, M, (h0, w0), align_border)) beside the plain letterbox of the other frame.  The matrices live in
        the device table and are rewritten per call: a rig that re-calibrates rebuilds nothing.
        formats=(None, "y16") (either or both modalities): a 16-BIT THERMAL modality, raw counts as a torch.uint16 / torch.int16 (B, H0,
        W0) tensor, its uint8 bytes (B, H0, 2 * W0), or a list of per-frame tensors.  Automatic gain control runs on the device:
        agc_clip=(clip_lo, clip_hi), basis points clipped at either end of each frame's histogram (utils.datasets.agc_window), or
        agc_window=(lo, hi) / a (B, 2) array, a window given by the caller; the counts are mapped to bytes at the letterbox's taps
        (utils.datasets.agc_u16_to_u8; icaf_y16_window + icaf_letterbox_y16_frames), bit-identical to forward_u8 of the host-mapped,
        host-letterboxed batch.  FrameGeometry.window holds, per modality, None or the cuda int32 (B, 2) windows this call used (a view
        of the model's table: the next call of the same shapes overwrites it), so that a caller can feed a damped copy back as agc_window."""
        self._check_eval()
        kind = ops.frame_kind(formats, align, val_size)                    # the table's kind (ops.KINDS); refuses what cannot be combined
        formats = (None, None) if formats is None else tuple(formats)
        matrix = ops.yuv_matrix_code(yuv_matrix) if kind.name == "yuv" else 0
        try:
            *fr, shapes, _, m, _, mats = kind.lists(rgb, ir, formats, align)
        except ValueError as e:
            raise ValueError(f"forward_frames expects cuda {kind.noun}: {e}") from None
        frames = fr[0] + fr[1]
        if not all(f.is_cuda for f in frames):
            raise ValueError(f"forward_frames expects cuda {kind.noun} (no CPU fallback exists)")
        B, device = len(fr[0]), frames[0].device
        H, W = (img_size, img_size) if isinstance(img_size, int) else img_size
        self._check_stride(H, W, int(self.stride.max()))
        st = self._frame_state(kind, H, W, shapes, ops.frame_specs(formats, fr, m), matrix, device, val_size)
        geom = st["geom"]
        if kind.update is not None:      # this call's matrices / border / clip / windows: written into the rows, validated, copied in stream order below
            kind.update(geom, B, formats, m, mats=mats, border=align_border, clip=agc_clip, wins=None if agc_window is None else ops._y16_windows(agc_window, B))
            kind.validate(geom, st["arena"].numel(), H, W)
        plan = (self.tta_plan_for if augment else self.plan_for)(B, H, W, device, u8=True)
        dst = plan.inputs[0]
        if st["dst"] is not dst:                          # the plan was rebuilt (evicted from the cache): bind the launches to its new input
            st["launches"] = kind.launches(st["arena"], geom, st["geom_dev"], dst, bgr, B, window=st["window"], mode=st["mode"], mode_dev=st["mode_dev"])
            st["dst"] = dst
        if kind.update is not None:
            st["geom_dev"].copy_(ops.geom_tensor(geom))
        for o, f in zip(ops.frame_rows(geom)["offset"], frames):          # tight rows (a YUV buffer: luma rows, then its chroma): a frame is one run of bytes
            st["arena"][int(o):int(o) + f.numel()].view(f.shape).copy_(f)
        last = st["launches"][-1]
        last.args = last.args[:-1] + (int(bool(bgr)),)
        for launch in st["launches"]:
            launch(ops.current_stream_ptr())
        plan.run()
        out = self._result(plan.outputs)
        return ((out, None) if augment else out), st["info"]

    def _frame_state(self, kind, H, W, shapes, specs, matrix, device, val_size):
        """forward_frames' table, arena and launches for one kind of table and one set of frame shapes: found, or made and kept (least
        recently used out).  specs (ops.frame_specs) holds each frame's format, channels or source size."""
        key = (kind.name, H, W, tuple(shapes), specs, matrix, device, val_size)
        states = self.__dict__.setdefault("_frame_states", {})
        st = states.pop(key, None)
        if st is None:
            mode = window = None
            if val_size is None:
                geom1, scale = ops.frame_geometry(shapes, (H, W))
            else:                                         # (ops.frame_kind: the plain kind alone has the validation geometry)
                geom1, mode1, scale = ops.val_geometry(shapes, val_size, (H, W))
                mode = np.concatenate((mode1, mode1))
            geom, nbytes = kind.pack(np.concatenate((geom1, geom1)), specs, matrix=matrix)
            B = len(shapes)
            if kind.window:                               # rows modality * B + image; FrameGeometry.window: the views of the 16-bit modalities
                window = torch.zeros((2 * B, 2), dtype=torch.int32, device=device)
            st = {"geom": geom, "geom_dev": ops.geom_tensor(geom, device), "arena": torch.zeros((nbytes,), dtype=torch.uint8, device=device),
                  "mode": mode, "mode_dev": None if mode is None else torch.from_numpy(mode).to(device), "window": window,
                  "info": ops.FrameGeometry(geom, scale, torch.from_numpy(scale).to(device),
                                            None if window is None else tuple(window[m * B:(m + 1) * B] if s == "y16" else None for m, s in enumerate(specs[::B]))),
                  "dst": None, "launches": None}
            while len(states) >= 8:                       # a few sets of shapes stay resident (arena + table each)
                states.pop(next(iter(states)))
        states[key] = st
        return st

    def plan_for(self, B, H, W, device="cuda", dtype=None, u8=False, slot=0, branches=True):
        """Pre-build (and return) the execution plan; its .inputs are the static RGB / IR staging buffers (u8: the one
        uint8 6-channel staging buffer).  Plans live in a least-recently-used cache capped at `plan_cache_bytes` of plan-owned
        buffers: a validation run with rectangular batches and a ragged last batch (test.py) meets a new (B, H, W) every few
        batches, and each plan pins all of its intermediates (yolov5l 1280x1280 b16: ~40 GB).  Evicted plans are freed as
        soon as nobody else (a DetectionPipeline, a caller) holds them; the newest plan is always kept.
        branches=False: the plan's hipGraph is one chain (no parallel DMFF / Detect branches, whatever `branch_dmff` says) — what a
        host-fed pipeline wants: a graph with branches runs them on streams of its own, and those share hardware queues with the
        pipeline's copy and NMS streams."""
        dt, device, key = self._plan_key(B, H, W, device, dtype, u8, slot, branches)
        plans = self.__dict__.setdefault("_plans", {})
        plan = plans.pop(key, None)
        if plan is None:
            cap = self.plan_cache_bytes
            if cap is not None:                     # make room BEFORE allocating the new plan's buffers
                hint = self._plan_bytes_hint(plans, B, H, W, dt)
                while plans and sum(p.nbytes for p in plans.values()) > max(cap - hint, 0):
                    plans.pop(next(iter(plans)))
            plan = self.build_plan(B, H, W, device, dt, u8=u8)
            if not branches and plan.branches:
                for l in plan.launches:
                    l.branch = 0
                plan.branches = {}
            if device.type == "cuda":
                if self.autotune:
                    plan.autotune()
                if self.use_graph:
                    plan.capture()
            if cap is not None:
                while plans and sum(p.nbytes for p in plans.values()) + plan.nbytes > cap:
                    plans.pop(next(iter(plans)))
        plans[key] = plan                           # (re-)insert as most recently used
        return plan

    def _plan_key(self, B, H, W, device, dtype, u8, slot, branches, tta=False):
        """-> (dtype, device, cache key) of a plan: the defaults resolved (the parameters' dtype, the current cuda device), then what
        else tells plans apart — slot: further plans of the same shape (own buffers) for batches in flight side by side."""
        dt = dtype or self.compute_dtype or next(self.parameters()).dtype
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        tags = (("tta",) if tta else ()) + (("u8",) if u8 else ()) + (("slot", slot) if slot else ()) + (() if branches else ("chain",))
        return dt, device, (B, H, W, dt, device) + tags

    @staticmethod
    def _plan_bytes_hint(plans, B, H, W, dt):
        """Expected size of the plan about to be built: plan-owned buffers scale with B * H * W * element size, so the densest
        cached plan's bytes per input element, times the new shape (a tiny plan next to a cached 40 GB one no longer evicts it).
        Plans that somebody else still holds (a DetectionPipeline, a caller of plan_for) stay allocated after eviction: the cap
        bounds what the CACHE pins, not the process."""
        es = torch.empty((), dtype=dt).element_size()
        per = 0.0
        for key, p in plans.items():
            pb, ph, pw, pdt = key[:4]
            per = max(per, p.nbytes / float(pb * ph * pw * torch.empty((), dtype=pdt).element_size()))
        return int(per * B * H * W * es)
