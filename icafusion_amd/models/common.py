"""Module library of the two-stream detector, MI355X edition.

Same class names, constructor signatures, attribute names and state_dict keys as the reference's
models/common.py (so `parse_model`'s name lookup, pickled checkpoints and `load_state_dict(strict=True)` keep
working — SURVEY.md §8b), but the modules do no arithmetic themselves: each one *emits* HIP kernel launches into
an `engine.Plan` over NHWC buffers.  `forward(x)` on a single module builds and runs a one-module plan, so the
classes still duck-type as nn.Modules taking/returning NCHW-shaped tensors.

There is deliberately no PyTorch / CPU fallback: calling a module with CPU tensors, in training mode, or without
libicaf.so raises.
"""
import collections
import math

import torch
import torch.nn as nn

from .. import ops
from ..options import OPT
from ..engine import ImageIn, Plan, concat_view, from_act, to_act

BN_EPS_DEFAULT = 1e-5


def autopad(k, p=None):
    """'same' padding for odd kernels (reference models/common.py:36-40)."""
    if p is None:
        p = k // 2 if isinstance(k, int) else [v // 2 for v in k]
    return p


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def conv_out(n, k, s, p):
    """Output extent of a k / stride s / padding p window over n positions (floor, as Conv2d and MaxPool2d)."""
    return (n + 2 * p - k) // s + 1


def conv2d_shape(k, H, W):
    """(C, H', W') an nn.Conv2d makes of an H x W map."""
    (kh, kw), (sh, sw), (ph, pw) = k.kernel_size, k.stride, _pair(k.padding)
    return k.out_channels, conv_out(H, kh, sh, ph), conv_out(W, kw, sw, pw)


def pool_window(pool):
    """(kernel, stride, padding) of a square nn.MaxPool2d."""
    return tuple(v if isinstance(v, int) else v[0] for v in (pool.kernel_size, pool.stride, pool.padding))


def fold_bn(conv, bn=None):
    """fp32 (weight, bias) of an nn.Conv2d, the eval-mode BatchNorm2d behind it folded in."""
    w = conv.weight.detach().float()
    b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
    if bn is not None:
        scale = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + bn.eps)
        w = w * scale[:, None, None, None]
        b = (b - bn.running_mean.detach().float()) * scale + bn.bias.detach().float()
    return w, b


def stage_image(plan, x, c1, s2d=False):
    """Network image (ImageIn x, c1 channels) in, NHWC act out — s2d: in 2 x 2 space-to-depth form, 4 * c1 channels at half the size — the
    channels padded to whole 16-byte vectors.  Allocates the act and appends the staging launch -> (act, its channel count)."""
    B, _, H, W = x.shape
    vec = ops.VEC[plan.dtype]
    cpad = -(-(4 * c1 if s2d else c1) // vec) * vec
    pre = plan.act(B, H // 2 if s2d else H, W // 2 if s2d else W, cpad, pair=x.pair)
    tag = "s2d" if s2d else "pad"
    plan.add(ops.preprocess_u8(x.t, pre, int(s2d), x.c0, name=f"preprocess_u8_{tag}") if x.u8
             else ops.preprocess(x.t, pre, int(s2d), name=f"preprocess_{tag}"))
    return pre, cpad


def emit_maxpool(plan, x, pool, out, name):
    """nn.MaxPool2d `pool` of the act / pair act x into `out` (allocated when None): one launch, or one per stream when the pair's halves
    are channel slices of a fusion buffer."""
    k, s, p = pool_window(pool)
    B, H, W, C = x.shape[-4:]
    if out is None:
        out = plan.act(B, conv_out(H, k, s, p), conv_out(W, k, s, p), C, pair=x.dim() == 5)
    if x.dim() == 5 and out.stride(0) != B * out.stride(1):
        for g in range(2):
            plan.add(ops.maxpool2d(x[g], out[g], k, s, p, name=name))
    else:
        plan.add(ops.maxpool2d(x, out, k, s, p, name=name))
    return out


def pair_signature(self):
    """What must match for two rows to run as one groups = 2 launch sequence: state_dict keys and shapes, Conv2d geometries, Conv activations."""
    return ([(k, tuple(v.shape)) for k, v in self.state_dict().items()],
            [(c.kernel_size, c.stride, c.padding, c.groups) for c in self.modules() if isinstance(c, nn.Conv2d)],
            [type(c.act) for c in self.modules() if isinstance(c, Conv)])


def _module_dtype(m, fallback=torch.float32):
    forced = getattr(m, "compute_dtype", None)
    if forced is not None:
        return forced
    for p in m.parameters():
        return p.dtype
    return fallback


class HipModule(nn.Module):
    """Base: stand-alone execution of `emit` + packed-weight cache."""

    def invalidate(self):
        for m in self.modules():
            if hasattr(m, "_cache"):
                m._cache = {}
            if hasattr(m, "_plans"):
                m._plans = {}

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self.__dict__["_cache"] = {}
        self.__dict__["_plans"] = {}

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self.__dict__["_cache"] = {}
        self.__dict__["_plans"] = {}
        return r

    def _cached(self, key, make):
        c = self.__dict__.setdefault("_cache", {})
        if key not in c:
            c[key] = make()
        return c[key]

    def packed_convs(self, plan, streams, swap_halves=False, cin_slice=None, transform=None, cin_pad=None, pack=None):
        """-> (wp, kp, bp), the launch form of convolution weights.  streams: per stream the (Conv2d, BatchNorm2d or None) pairs whose outputs
        are concatenated along Cout; BatchNorm is folded, the K halves swapped / the K columns cin_slice kept, `transform` applied, then
        pack(rows, dtype, cin_pad) — ops.pack_streams unless given — pads Cin, casts and stacks the streams.  Cached on self under a key derived
        from exactly these arguments: whoever asks for the same packing gets the same tensor, and nobody spells a key."""
        key = ("pack", plan.dtype, plan.device, tuple(tuple((id(c), id(b)) for c, b in s) for s in streams), bool(swap_halves),
               None if cin_slice is None else tuple(cin_slice), transform, cin_pad, pack)

        def make():
            rows = []
            for s in streams:
                w, b = (torch.cat(t) for t in zip(*(fold_bn(conv, bn) for conv, bn in s)))
                if swap_halves:
                    h = w.shape[1] // 2
                    w = torch.cat((w[:, h:], w[:, :h]), 1)
                if cin_slice is not None:
                    w = w[:, cin_slice[0]:cin_slice[1]]
                rows.append((w if transform is None else transform(w), b))
            return (pack or ops.pack_streams)(rows, plan.dtype, cin_pad)
        return self._cached(key, make)

    # stand-alone call: NCHW tensor(s) in, NCHW-shaped tensor(s) out
    def forward(self, x):
        xs = x if isinstance(x, (list, tuple)) else [x]
        if self.training:
            raise NotImplementedError("icafusion_amd implements the eval-mode inference path only (call .eval())")
        for t in xs:
            if not t.is_cuda:
                raise RuntimeError("icafusion_amd modules run on the MI355X only: move inputs to cuda "
                                   "(there is no CPU fallback; the CPU reference lives in oracle/)")
        dt = _module_dtype(self, xs[0].dtype)
        key = (tuple(tuple(t.shape) for t in xs), dt, xs[0].device)
        plans = self.__dict__.setdefault("_plans", {})
        if key not in plans:
            plan = Plan(xs[0].device, dt)
            ins = []
            for t in xs:
                if t.shape[1] % ops.VEC[dt] != 0:
                    buf = torch.zeros(t.shape, dtype=torch.float32, device=t.device)
                    ins.append(ImageIn(buf))
                else:
                    ins.append(plan.act(t.shape[0], t.shape[2], t.shape[3], t.shape[1]))
            plan.inputs = ins
            plan.outputs = self.emit(plan, ins if isinstance(x, (list, tuple)) else ins[0])
            plans[key] = plan
        plan = plans[key]
        for src, dst in zip(xs, plan.inputs):
            if isinstance(dst, ImageIn):
                dst.t.copy_(src)
            else:
                dst.copy_(src.permute(0, 2, 3, 1))
        plan.run()
        out = plan.outputs
        if isinstance(out, torch.Tensor) and out.dim() == 4:
            return from_act(out).clone(memory_format=torch.preserve_format)
        return out


# ----------------------------------------------------------------------------------------------------------
# convolution family
# ----------------------------------------------------------------------------------------------------------
def act_code(act):
    """ops.ACT_* of the torch activation module behind a convolution."""
    for kind, code in ((nn.SiLU, ops.ACT_SILU), (nn.Identity, ops.ACT_NONE), (nn.GELU, ops.ACT_GELU)):
        if isinstance(act, kind):
            return code
    raise NotImplementedError(f"activation {type(act).__name__} is outside the hot path")


def is_conv(k, kernel, stride=None, padding=None):
    """Is the nn.Conv2d k a plain (groups 1, undilated) kernel x kernel window — of this stride, this padding, where given?"""
    return (k.kernel_size == (kernel, kernel) and k.groups == 1 and k.dilation == (1, 1) and (stride is None or k.stride == (stride, stride))
            and (padding is None or _pair(k.padding) == (padding, padding)))


def silu16(plan, *convs):
    """The condition every fused form shares: a 16-bit plan, and these Convs end in SiLU."""
    return plan.dtype in (torch.bfloat16, torch.float16) and all(isinstance(c.act, nn.SiLU) for c in convs)


class Chained(collections.namedtuple("Chained", "convs twins y keep x2", defaults=(None, None, False, None))):
    """1x1 SiLU Convs riding on another launch's output tile, from C3.emit down to ops.conv2d / ops.bottleneck.  convs: the Convs, their outputs
    concatenated (a C3's cv1 | cv2); twins: their counterparts of the other stream; y: what they write.  keep: the carrying layer's own output
    (residual included) is written too and the 1x1 consumes it as stored (a Bottleneck's 3x3 followed by the next Bottleneck's 1x1) — otherwise
    only y is written.  x2: the chained Conv reads cat(the carrying layer's output, x2) (a C3's last Bottleneck carrying cv3, x2 = cv2's output)."""
    __slots__ = ()

    def launch_form(self, plan, paired, swap_halves=False):
        """-> ops.Chain: the same record with the Convs replaced by their packed weights."""
        tw = self.twins if paired else None
        w, kp, b = self.convs[0].packed(plan, tw[0] if tw else None, self.convs[1:], tw[1:] if tw else (), swap_halves=swap_halves)
        return ops.Chain(w, kp, b, self.y, sum(c.conv.out_channels for c in self.convs), self.keep, self.x2)


class Lead(collections.namedtuple("Lead", "conv twin stem stem_twin", defaults=(None, None, None))):
    """A deferred row of the plan builder: the down-sampling Conv (and its twin) whose launch the C3 behind it emits, cv1 | cv2 chained on its
    output tile; with `stem` the image-fed 6x6 / s2 Conv in front of it as well (icaf_stem2: rows 0-2a as one launch)."""
    __slots__ = ()

    @property
    def from_image(self):
        return self.stem is not None


def check_conv(plan, k, who, c1=None, got=None):
    """What a convolution launch refuses, stated once: groups and dilation, and — for an act of `got` channels where the launch reads c1 —
    another channel count (ValueError) or a width that is no whole number of 16-byte vectors.  emit_conv runs it before it allocates or
    appends anything; an emitter of several launches runs it up front for the widths inside, so that it refuses before its first launch."""
    if k.groups != 1 or k.dilation != (1, 1):
        raise NotImplementedError("grouped / dilated convolutions are outside the hot path")
    if got is not None and got != c1:
        raise ValueError(f"{who} expects {c1} input channels, got {got}")
    if got is not None and c1 % ops.VEC[plan.dtype]:
        raise NotImplementedError(f"channel count {c1} must be a multiple of {ops.VEC[plan.dtype]} for dtype {plan.dtype}")


def emit_conv(plan, owner, x, streams, act, name, out=None, res=None, res_pre_act=False, pre_term=None, pre_nearest=False, swap_halves=False,
              cin_slice=None, chain=None, s2d=False):
    """Append ONE convolution launch (icaf_conv2d): nn.Conv2d [+ BatchNorm2d] + activation `act` over the act / pair act / ImageIn x.
    name: the launch's name; {kh} {kw} {sh} are filled in from the window launched.
    streams: per stream the (Conv2d, BatchNorm2d or None) pairs whose outputs are concatenated along Cout (HipModule.packed_convs); two
          streams: x / out / res are pair acts and the launch has groups = 2.  owner: the module whose cache holds the packed weights.
    An ImageIn is staged first (stage_image: NHWC, channels padded to whole vectors; s2d: in space-to-depth form, its 6x6 / s2 / p2 window
          then running as 3x3 / s1 / p1 over four times the channels).
    out: allocated when None.  res / res_pre_act: residual behind / in front of the activation (ops.conv2d).  pre_term: fp32 coarse map
          (B, h, w, Cout) added, bilinearly resized (pre_nearest: nearest), before bias + activation (icaf.h).
    cin_slice: (k0, k1) — use only these input-channel columns of the weights (x then has k1 - k0 channels): the full-resolution half of
          a 1x1 conv over cat(up(a), b), whose other half arrives as the nearest pre_term.
    swap_halves: x holds the two halves of the layer's input channels in swapped order (C3 after an odd number of fused Bottlenecks):
          the weight columns are swapped to match when they are packed.
    chain: Chained — its 1x1s run on this launch's output tile; -> chain.y, or `out` when chain.keep."""
    k = streams[0][0][0]
    (kh, kw), (sh, sw), (ph, pw), c1 = k.kernel_size, k.stride, _pair(k.padding), k.in_channels
    assert all((e.kernel_size, e.stride, _pair(e.padding), e.in_channels) == ((kh, kw), (sh, sw), (ph, pw), c1) for s in streams for e, _ in s), \
        "fused convs must share geometry"
    c2 = sum(e.out_channels for e, _ in streams[0])
    paired = len(streams) == 2
    who = f"{type(owner).__name__} ({name})"
    transform = cin_pad = None
    if isinstance(x, ImageIn):
        assert x.pair == paired and cin_slice is None
        check_conv(plan, k, who)
        x, c1 = stage_image(plan, x, c1, s2d)
        cin_pad = c1
        if s2d:                           # 6x6/s2/p2 over the image == 3x3/s1/p1 over space-to-depth(image)
            transform, (kh, kw, sh, sw, ph, pw) = ops.s2d_conv_weight, (3, 3, 1, 1, 1, 1)
    else:
        assert (x.dim() == 5) == paired and not s2d
        if cin_slice is not None:
            assert (kh, kw) == (1, 1) and not swap_halves and 0 <= cin_slice[0] < cin_slice[1] <= c1
            c1 = cin_slice[1] - cin_slice[0]
        check_conv(plan, k, who, c1, x.shape[-1])
    wp, kp, bp = owner.packed_convs(plan, streams, swap_halves, cin_slice, transform, cin_pad)
    B, H, W = x.shape[-4:-1]
    Ho, Wo = conv_out(H, kh, sh, ph), conv_out(W, kw, sw, pw)
    if out is None:                       # (also in front of a chain that writes only chain.y: the order plans number their buffers in)
        out = plan.act(B, Ho, Wo, c2, pair=paired)
    ch = None if chain is None else chain.launch_form(plan, paired)
    if ch is not None and not ch.keep:
        out = ch.y[..., :c2] if ch.y.shape[-1] >= c2 else plan.act(B, Ho, Wo, c2, pair=paired)   # (y is ignored by the kernel)
    plan.add(ops.conv2d(x, wp, kp, bp, out, kh, kw, sh, sw, ph, pw, c1, c2, act, res=res, res_pre_act=res_pre_act, pre=pre_term,
                        pre_nearest=pre_nearest, chain=ch, name=name.format(kh=kh, kw=kw, sh=sh)))
    return out if ch is None or ch.keep else ch.y


class Conv(HipModule):
    """Conv2d(bias=False) + BatchNorm2d + SiLU (reference models/common.py:48-60).  On the device this is one
    implicit-GEMM launch with BN folded into the packed weights (as utils/torch_utils.py:182-202 does offline) and
    bias + SiLU in the epilogue; `fuse()`d modules (no .bn) are handled identically."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        super().__init__()
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False)
        self.bn = nn.BatchNorm2d(c2)
        self.act = nn.SiLU() if act is True else (act if isinstance(act, nn.Module) else nn.Identity())

    fuse_stem = True     # image-fed 6x6/s2 layers: staging + convolution as one persistent kernel (16-bit types)

    def fuseforward(self, x):           # kept for API parity with Model.fuse(); same device path
        return self.forward(x)

    def folded(self):
        """fp32 (weight, bias) with BatchNorm folded in."""
        return fold_bn(self.conv, getattr(self, "bn", None))

    pair_signature = pair_signature

    def out_shape(self, src):
        return conv2d_shape(self.conv, src[1], src[2])

    def _streams(self, twin=None, also=(), twin_also=()):
        """packed_convs' / emit_conv's per-stream lists: this layer, `also` appended along Cout; with `twin` the other stream's as well."""
        assert len(twin_also) == (len(also) if twin is not None else 0)
        streams = [(self,) + tuple(also)] + ([(twin,) + tuple(twin_also)] if twin is not None else [])
        return [[(c.conv, getattr(c, "bn", None)) for c in convs] for convs in streams]

    def packed(self, plan, twin=None, also=(), twin_also=(), swap_halves=False, cin_slice=None, transform=None, cin_pad=None):
        """-> (wp, kp, bp), the launch form of this layer's weights: BN folded, `also` appended along Cout, the K halves swapped /
        the K columns cin_slice kept, `transform` (ops.s2d_conv_weight) applied, Cin padded to cin_pad, cast to plan.dtype; with
        `twin` the two streams stacked.  Packed once per distinct set of arguments (HipModule.packed_convs, cached on self)."""
        return self.packed_convs(plan, self._streams(twin, also, twin_also), swap_halves, cin_slice, transform, cin_pad)

    def emit(self, plan, x, out=None, res=None, twin=None, also=(), twin_also=(), pre_term=None, swap_halves=False,
             chain=None, pre_nearest=False, cin_slice=None):
        """Append this layer's launch (emit_conv).

        twin: the structurally identical Conv of the other backbone stream — x / out / res are then pair acts
              (2, B, H, W, C) and both streams run as ONE groups=2 launch with per-stream weights.
        also: further Convs with the same geometry and activation reading the same input (C3's cv1 and cv2): their
              output channels are appended to this layer's, one GEMM with N = sum of the widths (twin_also: the
              twin stream's counterparts).
        pre_term / pre_nearest / cin_slice / swap_halves: as emit_conv.
        chain: Chained — 1x1 SiLU Convs (the cv1 | cv2 of the C3 behind a down-sampling Conv, the next Bottleneck's cv1, a C3's cv3)
              applied to this layer's output tile inside the same launch."""
        act = act_code(self.act)
        assert all(act_code(e.act) == act for e in also), "fused convs must share an activation"
        paired = twin is not None
        s2d = False
        if isinstance(x, ImageIn):
            B, _, H, W = x.shape
            s2d = is_conv(self.conv, 6, 2, 2) and H % 2 == 0 and W % 2 == 0
            c1, c2 = self.conv.in_channels, self.conv.out_channels
            if (s2d and self.fuse_stem and plan.dtype in (torch.bfloat16, torch.float16) and c1 == 3 and c2 in (32, 64)
                    and not also and res is None and (not x.u8 or (paired and x.c0 == 0))):
                # staging + convolution in one persistent kernel reading the NCHW image itself (stem.hip)
                assert x.pair == paired
                wp, kp, bp = self.packed(plan, twin, swap_halves=swap_halves, transform=ops.s2d_conv_weight, cin_pad=16)
                if out is None:
                    out = plan.act(B, H // 2, W // 2, c2, pair=paired)
                plan.add(ops.stem(x.t, wp, kp, bp, out, c2))
                return out
        name = "conv{kh}x{kw}s{sh}" + ("" if chain is None else "+cv3" if chain.x2 is not None else "+1x1")
        return emit_conv(plan, self, x, self._streams(twin, also, twin_also), act, name, out=out, res=res, pre_term=pre_term,
                         pre_nearest=pre_nearest, swap_halves=swap_halves, cin_slice=cin_slice, chain=chain, s2d=s2d)

    fuse_stem2 = True    # stem + the 3x3/s2 Conv behind it + that Conv's chained cv1 | cv2 as ONE persistent kernel

    def stem2_ok(self, plan, x, nxt, c3):
        """self = image-fed 6x6/s2 stem, nxt = the Conv behind it, c3 = the C3 behind that: can icaf_stem2 run all three?
        (mirrors its argument checks: 16-bit, 3 -> 32 -> 64 -> 2 x 32 channels, i.e. the yolov5s width)"""
        if not (self.fuse_stem2 and self.fuse_stem and isinstance(x, ImageIn) and x.pair and isinstance(nxt, Conv)
                and silu16(plan, self) and (not x.u8 or x.c0 == 0)):
            return False
        k0, k1 = self.conv, nxt.conv
        _, _, H, W = x.shape
        return (is_conv(k0, 6, 2, 2) and (k0.in_channels, k0.out_channels) == (3, 32) and H % 2 == 0 and W % 2 == 0
                and is_conv(k1, 3, 2, 1) and (k1.in_channels, k1.out_channels) == (32, 64)
                and nxt.chain_ok(plan, c3) and 2 * c3.cv1.conv.out_channels == 64)

    def emit_stem2(self, plan, x, lead, chain):
        """Rows 0-2a of both streams as one launch: self = lead.stem, chain = the C3's cv1 | cv2 and the pair act they write."""
        w0, kp0, b0 = self.packed(plan, lead.stem_twin, transform=ops.s2d_conv_weight, cin_pad=16)
        w1, kp1, b1 = lead.conv.packed(plan, lead.twin)
        c = chain.launch_form(plan, True)
        plan.add(ops.stem2(x.t, w0, kp0, b0, w1, kp1, b1, c.w, c.kp, c.bias, c.y, self.conv.out_channels, lead.conv.conv.out_channels, c.cout))
        return c.y

    chain_fuse = True    # let a C3 behind this Conv run its cv1 | cv2 GEMM on this layer's output tile (one launch)

    def chain_ok(self, plan, c3):
        """Can the fused cv1 | cv2 GEMM of `c3` ride on this conv's output tile?  (mirrors the checks of icaf_conv2d)"""
        k, cv = self.conv, c3.cv1.conv
        n1, n2 = k.out_channels, 2 * cv.out_channels
        return (self.chain_fuse and silu16(plan, self, c3.cv1) and is_conv(k, 3) and k.in_channels % 32 == 0
                and is_conv(cv, 1, 1) and cv.in_channels == n1 and c3.cv2.conv.out_channels == cv.out_channels
                and max(n1, n2) <= self.chain_max_width)

    chain_max_width = 128

    def chain_ok_1x1(self, plan, nxt):
        """Can the 1x1 SiLU Conv `nxt` (the next Bottleneck's cv1) ride on this 3x3 layer's output tile, this layer's output
        (shortcut included) being written as well?  (icaf_conv2d: chain_keep)"""
        k, kn = self.conv, nxt.conv
        return (self.chain_fuse and silu16(plan, self, nxt) and is_conv(k, 3) and k.in_channels % 64 == 0
                and is_conv(kn, 1, 1) and kn.in_channels == k.out_channels and max(k.out_channels, kn.out_channels) <= self.chain_max_width)

    chain_tail = OPT.c3_tail      # A/B switch: a C3's cv3 rides on its last Bottleneck's 3x3 (a class default, as fuse_decode)

    def chain_ok_tail(self, plan, cv3):
        """Can the C3's cv3 (1x1 SiLU over cat(m, cv2)) ride on this 3x3 layer — the block's last Bottleneck.cv2 — so that neither m nor
        the concatenation reach HBM?  (icaf_conv2d: x2; built in cwide.hip for 128 -> 128 layers with 256 output channels of cv3)"""
        k, k3 = self.conv, cv3.conv
        return (self.chain_tail and OPT.cwide and silu16(plan, self, cv3) and is_conv(k, 3, 1, 1) and (k.in_channels, k.out_channels) == (128, 128)
                and is_conv(k3, 1, 1, 0) and k3.in_channels == 2 * k.out_channels and k3.out_channels == 256)


class VGGblock(HipModule):
    """num_convs x (Conv2d(3x3, padding 1, bias) + ReLU), then MaxPool2d(2, 2) (reference models/common.py:109-128; the reference's
    `blk` list is not registered, so `vggblock` is the whole state_dict surface).  No BatchNorm: nothing to fold.  On the device: one
    ReLU implicit-GEMM launch per conv (icaf_conv2d, ACT_RELU) and one icaf_maxpool2d; the block that reads the image runs its first
    conv through icaf_vgg_stem in the 16-bit types, straight from the NCHW image."""

    def __init__(self, num_convs, c1, c2):
        super().__init__()
        blk = [nn.Sequential(nn.Conv2d(in_channels=c1 if j == 0 else c2, out_channels=c2, kernel_size=3, padding=1), nn.ReLU())
               for j in range(num_convs)]
        blk.append(nn.MaxPool2d(kernel_size=2, stride=2))
        self.vggblock = nn.Sequential(*blk)

    # image-fed first conv as ONE kernel (icaf_vgg_stem, 16-bit types) instead of preprocess_pad + an igemm with K = 72.  Built and tested, OFF by
    # default: measured on MI355X (tools/vgg_bench.py, profiles/vgg_bench.json: bf16, both streams, batch 32, 640 x 640, interleaved in one loop) the
    # fused kernel takes 2.62 ms against 1.50 ms for the two generic launches (A/A spread 0.3 %) — 160 registers leave two waves per SIMD to hide
    # 16 scalar image loads per lane and round; the generic route writes and re-reads only 16 bytes per pixel.
    fuse_stem = False

    def convs(self):
        return [s[0] for s in self.vggblock if isinstance(s, nn.Sequential)]

    def pair_signature(self):
        """... and the plain torch modules behind the convolutions: the same activations, the same pool window."""
        return pair_signature(self) + ([(type(c), getattr(c, "kernel_size", None), getattr(c, "stride", None), getattr(c, "padding", None))
                                        for s in self.vggblock for c in (s if isinstance(s, nn.Sequential) else [s]) if not isinstance(c, nn.Conv2d)],)

    def out_shape(self, src):                   # 3x3 / s1 / p1 convs keep the size, the closing pool halves it (floor)
        k, s, p = pool_window(self.vggblock[-1])
        return self.convs()[-1].out_channels, conv_out(src[1], k, s, p), conv_out(src[2], k, s, p)

    @staticmethod
    def _pack_stem(rows, dt, cin_pad):
        """icaf_vgg_stem's form of the image-fed conv: w [64][32] per stream, bias fp32 [64]."""
        ws, bs = [ops.vgg_stem_weight(w, dt) for w, _ in rows], [b.contiguous() for _, b in rows]
        return (ws[0], 32, bs[0]) if len(rows) == 1 else (torch.stack(ws).contiguous(), 32, torch.stack(bs).contiguous())

    def _streams(self, j, twin):
        return [[(b.convs()[j], None)] for b in ((self,) if twin is None else (self, twin))]

    def _packed(self, plan, j, twin, cin_pad=None, stem=False):
        """(wp, kp, bp) of conv j in its launch form, or with stem=True in icaf_vgg_stem's; with `twin` the two streams stacked."""
        return self.packed_convs(plan, self._streams(j, twin), cin_pad=cin_pad, pack=VGGblock._pack_stem if stem else None)

    def emit(self, plan, x, out=None, twin=None):
        paired = twin is not None
        pool = self.vggblock[-1]
        if not isinstance(pool, nn.MaxPool2d) or pool.dilation not in (1, (1, 1)) or pool.ceil_mode:
            raise NotImplementedError("VGGblock ends with a plain nn.MaxPool2d")
        for s in list(self.vggblock)[:-1]:
            if not (isinstance(s, nn.Sequential) and len(s) == 2 and isinstance(s[0], nn.Conv2d) and isinstance(s[1], nn.ReLU)):
                raise NotImplementedError("VGGblock rows are Sequential(Conv2d, ReLU): another activation is outside the hot path")
        convs = self.convs()
        if not all(is_conv(k, 3, 1, 1) and k.bias is not None for k in convs):
            raise NotImplementedError("VGGblock convolutions are 3x3 / stride 1 / padding 1 with bias")
        for j in range(1, len(convs)):          # the widths inside the block are refused before its first launch
            check_conv(plan, convs[j], f"VGGblock conv {j}", convs[j].in_channels, convs[j - 1].out_channels)
        for j, k in enumerate(convs):
            y = None
            if isinstance(x, ImageIn):
                B, _, H, W = x.shape
                y = plan.act(B, H, W, k.out_channels, pair=paired)      # in FRONT of the staging buffer: the order plans number their buffers in
                if self.fuse_stem and plan.dtype in (torch.bfloat16, torch.float16) and (k.in_channels, k.out_channels) == (3, 64):
                    assert x.pair == paired
                    wp, _, bp = self._packed(plan, 0, twin, stem=True)
                    plan.add(ops.vgg_stem(x.t, wp, bp, y, c0=x.c0 if x.u8 else 0))
                    x = y
                    continue
            x = emit_conv(plan, self, x, self._streams(j, twin), ops.ACT_RELU, "vgg_conv3x3", out=y)
        return emit_maxpool(plan, x, pool, out, "vgg_maxpool")


class ResNetblock(HipModule):
    """ResNet bottleneck (reference models/common.py:131-156): relu(bn1(conv1 1x1)) -> relu(bn2(conv2 3x3 / stride)) -> bn3(conv3 1x1) +
    shortcut(x) -> relu, the shortcut a 1x1 / stride convolution + BatchNorm where the shape changes and the identity otherwise.  On the
    device: three ReLU implicit-GEMM launches (four with a shortcut convolution, which has no activation), BatchNorm folded when the
    weights are packed, and the add + ReLU in conv3's epilogue with the residual IN FRONT of the activation (icaf.h: res_mode = 1)."""
    expansion = 4

    def __init__(self, c1, c2, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_channels=c1, out_channels=c2, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(c2)
        self.conv2 = nn.Conv2d(in_channels=c2, out_channels=c2, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(c2)
        self.conv3 = nn.Conv2d(in_channels=c2, out_channels=self.expansion * c2, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(self.expansion * c2)
        self.shortcut = nn.Sequential()
        if stride != 1 or c1 != self.expansion * c2:
            self.shortcut = nn.Sequential(nn.Conv2d(in_channels=c1, out_channels=self.expansion * c2, kernel_size=1, stride=stride, bias=False),
                                          nn.BatchNorm2d(self.expansion * c2))

    def _check(self):
        k1, k2, k3 = self.conv1, self.conv2, self.conv3
        ok = ((k1.kernel_size, k1.stride, _pair(k1.padding)) == ((1, 1), (1, 1), (0, 0)) and k2.kernel_size == (3, 3) and _pair(k2.padding) == (1, 1)
              and k2.stride[0] == k2.stride[1] and (k3.kernel_size, k3.stride, _pair(k3.padding)) == ((1, 1), (1, 1), (0, 0))
              and all(k.groups == 1 and k.dilation == (1, 1) for k in (k1, k2, k3))
              and k1.out_channels == k2.in_channels and k2.out_channels == k3.in_channels)
        sc = list(self.shortcut)
        if sc:
            ok = ok and (len(sc) == 2 and isinstance(sc[0], nn.Conv2d) and isinstance(sc[1], nn.BatchNorm2d) and sc[0].kernel_size == (1, 1)
                         and _pair(sc[0].padding) == (0, 0) and sc[0].stride == k2.stride and sc[0].groups == 1
                         and sc[0].in_channels == k1.in_channels and sc[0].out_channels == k3.out_channels)
        else:
            ok = ok and k2.stride == (1, 1) and k1.in_channels == k3.out_channels
        if not ok:
            raise NotImplementedError("ResNetblock: 1x1 -> 3x3 / stride -> 1x1 with a 1x1 / stride shortcut convolution or the identity")

    def emit(self, plan, x, out=None, twin=None):
        self._check()
        check_conv(plan, self.conv2, "ResNetblock conv2", self.conv2.in_channels, self.conv1.out_channels)     # the width inside, before the first launch
        blocks = (self,) if twin is None else (self, twin)

        def conv(k, bn, x, name, act=ops.ACT_RELU, **kw):
            # BatchNorm is folded HERE, when the weights are packed: the modules keep theirs, as the reference's fuse() leaves them (it only touches Conv)
            return emit_conv(plan, self, x, [[(b.get_submodule(k), b.get_submodule(bn))] for b in blocks], act, name, **kw)
        t = conv("conv2", "bn2", conv("conv1", "bn1", x, "resnet_conv1x1"), "resnet_conv3x3s{sh}")
        res = conv("shortcut.0", "shortcut.1", x, "resnet_shortcut1x1s{sh}", ops.ACT_NONE) if len(self.shortcut) else x
        return conv("conv3", "bn3", t, "resnet_conv1x1+res", out=out, res=res, res_pre_act=True)


class ResNetlayer(HipModule):
    """One yaml row of a ResNet50 stream (reference models/common.py:159-181; the reference's `blk` list is not registered, `layer` is the
    whole state_dict surface).  is_first: Conv2d(7x7 / s2 / p3) + BatchNorm + ReLU + MaxPool2d(3, 2, 1) — on the device the staging kernel
    (image -> NHWC, channels padded to one 16-byte vector), one ReLU implicit-GEMM launch walking the 49 taps (K = 49 x the padded
    channels) and icaf_maxpool2d.  Otherwise num_blocks ResNetblocks, the first with `stride`."""
    expansion = 4

    def __init__(self, c1, c2, stride=1, is_first=False, num_blocks=1):
        super().__init__()
        self.is_first = is_first
        if self.is_first:
            self.layer = nn.Sequential(nn.Conv2d(in_channels=c1, out_channels=c2, kernel_size=7, stride=2, padding=3, bias=False),
                                       nn.BatchNorm2d(c2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
        else:
            blk = [ResNetblock(c1, c2, stride)] + [ResNetblock(self.expansion * c2, c2, 1) for _ in range(num_blocks - 1)]
            self.layer = nn.Sequential(*blk)

    def pair_signature(self):
        """... the same kind of row, and behind a stem's convolution the same plain torch modules (BatchNorm eps, ReLU, pool window)."""
        return pair_signature(self) + (self.is_first, [(type(c), getattr(c, "eps", None), getattr(c, "kernel_size", None), getattr(c, "stride", None),
                                                        getattr(c, "padding", None)) for c in self.layer if self.is_first and not isinstance(c, nn.Conv2d)])

    def out_shape(self, src):                   # 7x7 / s2 / p3 + 3 / 2 / 1 pool for the stem row, the blocks' 3x3 strides otherwise (floor)
        _, H, W = src
        if self.is_first:
            C, H, W = conv2d_shape(self.layer[0], H, W)
            k, s, p = pool_window(self.layer[3])
            return C, conv_out(H, k, s, p), conv_out(W, k, s, p)
        for b in self.layer:
            H, W = conv_out(H, 3, b.conv2.stride[0], 1), conv_out(W, 3, b.conv2.stride[0], 1)
        return self.layer[-1].conv3.out_channels, H, W

    def emit(self, plan, x, out=None, twin=None):
        paired = twin is not None
        if not self.is_first:
            blocks = list(self.layer)
            for j, b in enumerate(blocks):
                if not isinstance(b, ResNetblock):
                    raise NotImplementedError("ResNetlayer rows are ResNetblocks")
                x = b.emit(plan, x, out=out if j == len(blocks) - 1 else None, twin=twin.layer[j] if paired else None)
            return x
        mods = list(self.layer)
        if not (len(mods) == 4 and isinstance(mods[0], nn.Conv2d) and isinstance(mods[1], nn.BatchNorm2d) and isinstance(mods[2], nn.ReLU)
                and isinstance(mods[3], nn.MaxPool2d) and mods[3].dilation in (1, (1, 1)) and not mods[3].ceil_mode):
            raise NotImplementedError("the first ResNetlayer is Conv2d + BatchNorm2d + ReLU + a plain MaxPool2d")
        layers = (self,) if twin is None else (self, twin)
        y = emit_conv(plan, self, x, [[(l.layer[0], l.layer[1])] for l in layers], ops.ACT_RELU, "resnet_stem{kh}x{kw}s{sh}")
        return emit_maxpool(plan, y, mods[3], out, "resnet_maxpool")


class Bottleneck(HipModule):
    """1x1 -> 3x3 with optional identity shortcut (reference models/common.py:184-194); the shortcut add is the
    residual term of the second conv's epilogue (which may write in place over its own residual: every output
    element is read and written by the same thread, and the GEMM's input is the 1x1's separate output)."""

    def __init__(self, c1, c2, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_, c2, 3, 1, g=g)
        self.add = shortcut and c1 == c2

    def emit(self, plan, x, out=None, twin=None):
        t = self.cv1.emit(plan, x, twin=twin.cv1 if twin is not None else None)
        return self.cv2.emit(plan, t, out=out, res=x if self.add else None,
                             twin=twin.cv2 if twin is not None else None)

    fuse = True      # use the one-launch kernel (icaf_bottleneck) where it is built and measured faster
    fuse_widths = (32,)

    def fusable(self, plan, x):
        """One-launch form: built for c_ in {32, 64} (16-bit types, 1x1 then 3x3 / s1 / p1, SiLU); USED for c_ = 32 on wide
        maps only: measured on MI355X (both streams, batch 32) 174 us against 73 + 112 us at 160x160 / c_ = 32, but
        155 us against 30 + 62 us at 80x80 / c_ = 64, where two LDS patches leave room for one workgroup per CU."""
        a, b = self.cv1.conv, self.cv2.conv
        c = a.in_channels
        return (self.fuse and silu16(plan, self.cv1, self.cv2) and c in self.fuse_widths
                and a.out_channels == c and b.in_channels == c and b.out_channels == c and is_conv(a, 1, 1, 0) and is_conv(b, 3, 1, 1)
                and x.shape[-2] >= 64)

    def emit_fused(self, plan, x, out, twin=None, cv3=None):
        """y = [x +] SiLU(conv3x3(SiLU(conv1x1(x)))) as ONE launch; `out` must be a different buffer (slice) than x.
        cv3: Chained with x2 — the C3's cv3 rides on the launch: x2 is the cv2 half of its input, y its output; the Bottleneck's own
        output is then never written (`out` is ignored)."""
        c = self.cv1.conv.in_channels
        paired = twin is not None
        tail = None if cv3 is None else cv3.launch_form(plan, paired, swap_halves=True)          # K columns in the order [cv2 | m]
        w1, kp1, b1 = self.cv1.packed(plan, twin.cv1 if paired else None)
        w2, kp2, b2 = self.cv2.packed(plan, twin.cv2 if paired else None)
        plan.add(ops.bottleneck(x, w1, kp1, b1, w2, kp2, b2, None if tail else out, c, self.add, 1 if c == 32 else 2, cv3=tail))
        return tail.y if tail else out


class C3(HipModule):
    """CSP bottleneck with three convs (reference models/common.py:216-227).  cv1 and cv2 read the same input, so they
    run as ONE GEMM writing both halves of the buffer cv3 reads (the torch.cat is never materialised); the
    bottleneck chain then updates the first half in place."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5):
        super().__init__()
        c_ = int(c2 * e)
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c1, c_, 1, 1)
        self.cv3 = Conv(2 * c_, c2, 1)
        self.m = nn.Sequential(*[Bottleneck(c_, c_, shortcut, g, e=1.0) for _ in range(n)])

    pair_signature = pair_signature

    def out_shape(self, src):
        return self.cv3.conv.out_channels, src[1], src[2]

    fuse_cv3 = True      # n = 1, c_ = 32: Bottleneck + cv3 as one launch (icaf_bottleneck with a chained cv3)
    chain_bottlenecks = True     # n > 1: a Bottleneck's 3x3 (+ shortcut) and the next Bottleneck's 1x1 as one launch

    def emit(self, plan, x, out=None, twin=None, lead=None):
        """lead: Lead — the down-sampling Conv in front of this block whose output only this block reads; `x` is then THAT
        conv's input (with lead.stem the image pair itself) and cv1 | cv2 run chained on its output tile (the tensor between
        the two yaml rows is never written)."""
        vcat = x if isinstance(x, VirtualCat) else None
        if vcat is not None:
            assert lead is None and twin is None
            x = vcat.other
        if lead is not None and lead.from_image:
            B, _, H, W = x.shape
            H, W = conv_out(H // 2, 3, 2, 1), conv_out(W // 2, 3, 2, 1)          # behind the 6x6 / s2 stem, then the 3x3 / s2 Conv
        elif lead is not None:
            B = x.shape[-4]
            _, H, W = conv2d_shape(lead.conv.conv, *x.shape[-3:-1])
        else:
            B, H, W = x.shape[-4:-1]
        c_ = self.cv1.conv.out_channels
        paired = twin is not None
        fused = [blk.fusable(plan, x if lead is None else torch.empty((B, H, W, 1), device="meta")) for blk in self.m]
        # Buffer of three c_-wide slots [a | b | a']: cv1|cv2 write [a | b]; a fused Bottleneck cannot run in place (its
        # neighbours' patches read x), so the chain ping-pongs between slot 0 and slot 2; cv3 then reads [a | b] or
        # [b | a'] — in the second case with its weight columns swapped to match.
        k3 = self.cv3.conv
        tail3 = (self.fuse_cv3 and len(self.m) == 1 and fused[0] and silu16(plan, self.cv3) and c_ == 32 and k3.out_channels == 64
                 and is_conv(k3, 1, 1) and k3.in_channels == 2 * c_)
        cat = plan.act(B, H, W, (3 if any(fused) and not tail3 else 2) * c_, pair=paired)
        if lead is not None:
            both = Chained((self.cv1, self.cv2), (twin.cv1, twin.cv2) if paired else None, cat[..., :2 * c_])
            if lead.from_image:
                lead.stem.emit_stem2(plan, x, lead, both)
            else:
                lead.conv.emit(plan, x, twin=lead.twin, chain=both)
        elif vcat is not None:
            # cv(cat(up(a), b)) = SiLU(up(Wa . a) + Wb . b + bias): the 1x1 commutes with the nearest up-sampling, so the
            # a-half of cv1 | cv2 runs at LOW resolution (fp32 out, a quarter of the pixels) and enters the GEMM over b as its
            # nearest-resized pre-activation term; nn.Upsample's output and the Concat buffer are never written or read.
            ca, cb = vcat.low.shape[-1], vcat.other.shape[-1]
            wa, kpa, _ = self.cv1.packed(plan, also=(self.cv2,), cin_slice=(0, ca))           # (the bias stays in the GEMM over b)
            Bl, hl, wl, _ = vcat.low.shape
            P = plan.empty((Bl, hl, wl, 2 * c_), torch.float32)
            plan.add(ops.conv2d(vcat.low, wa, kpa, None, P, 1, 1, 1, 1, 0, 0, ca, 2 * c_, ops.ACT_NONE, name="c3_up_term"))
            self.cv1.emit(plan, x, out=cat[..., :2 * c_], also=(self.cv2,), pre_term=P, pre_nearest=True, cin_slice=(ca, ca + cb))
        else:
            self.cv1.emit(plan, x, out=cat[..., :2 * c_], twin=twin.cv1 if paired else None, also=(self.cv2,),
                          twin_also=(twin.cv2,) if paired else ())
        if tail3:         # the single fused Bottleneck carries cv3 as well: cat(m, cv2) and m never reach HBM
            if out is None:
                out = plan.act(B, H, W, k3.out_channels, pair=paired)
            return self.m[0].emit_fused(plan, cat[..., :c_], None, twin=twin.m[0] if paired else None,
                                        cv3=Chained((self.cv3,), (twin.cv3,) if paired else None, out, x2=cat[..., c_:2 * c_]))
        cur = 0
        t_next = None                       # the next Bottleneck's 1x1 output, when the previous 3x3 launch produced it
        for j, blk in enumerate(self.m):
            a = cat[..., cur * c_:(cur + 1) * c_]
            tw = twin.m[j] if paired else None
            if fused[j]:
                cur = 2 - cur
                blk.emit_fused(plan, a, cat[..., cur * c_:(cur + 1) * c_], twin=tw)
                continue
            nxt = self.m[j + 1] if j + 1 < len(self.m) and not fused[j + 1] else None
            t = t_next if t_next is not None else blk.cv1.emit(plan, a, twin=tw.cv1 if paired else None)
            t_next, ch = None, None
            if nxt is not None and self.chain_bottlenecks and blk.cv2.chain_ok_1x1(plan, nxt.cv1):
                t_next = plan.act(B, H, W, nxt.cv1.conv.out_channels, pair=paired)
                ch = Chained((nxt.cv1,), (twin.m[j + 1].cv1,) if paired else None, t_next, keep=True)
            if j == len(self.m) - 1 and cur == 0 and blk.cv2.chain_ok_tail(plan, self.cv3):
                # the block's tail as ONE launch: m = [a +] SiLU(conv3x3(t)) stays in the kernel's staging tile, cv3 reads [m | b] from there
                # and from cv2's half of the buffer (icaf.h: icaf_conv_args.x2) — m is never written, cat(m, b) never read
                if out is None:
                    out = plan.act(B, H, W, k3.out_channels, pair=paired)
                return blk.cv2.emit(plan, t, out=a, res=a if blk.add else None, twin=tw.cv2 if paired else None,
                                    chain=Chained((self.cv3,), (twin.cv3,) if paired else None, out, x2=cat[..., c_:2 * c_]))
            blk.cv2.emit(plan, t, out=a, res=a if blk.add else None, twin=tw.cv2 if paired else None, chain=ch)
        src = cat[..., :2 * c_] if cur == 0 else cat[..., c_:3 * c_]
        return self.cv3.emit(plan, src, out=out, twin=twin.cv3 if paired else None, swap_halves=cur != 0)


class SPPF(HipModule):
    """Spatial pyramid pooling - fast (reference models/common.py:252-267): the three chained max pools run as
    one kernel writing the three extra channel groups of the buffer cv2 reads."""

    def __init__(self, c1, c2, k=5):
        super().__init__()
        c_ = c1 // 2
        self.cv1 = Conv(c1, c_, 1, 1)
        self.cv2 = Conv(c_ * 4, c2, 1, 1)
        self.m = nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2)

    pair_signature = pair_signature

    def out_shape(self, src):
        return self.cv2.conv.out_channels, src[1], src[2]

    def emit(self, plan, x, out=None, twin=None):
        B, H, W = x.shape[-4:-1]
        c_ = self.cv1.conv.out_channels
        k = pool_window(self.m)[0]
        paired = twin is not None
        cat = plan.act(B, H, W, 4 * c_, pair=paired)
        self.cv1.emit(plan, x, out=cat[..., :c_], twin=twin.cv1 if paired else None)
        plan.add(ops.sppf_pool(cat[..., :c_], cat[..., c_:2 * c_], cat[..., 2 * c_:3 * c_], cat[..., 3 * c_:], k))
        return self.cv2.emit(plan, cat, out=out, twin=twin.cv2 if paired else None)


class VirtualCat:
    """cat(nearest_up(low, scale), other) that is never materialised: a C3 consumes it (C3.emit)."""

    def __init__(self, low, scale, other):
        self.low, self.scale, self.other = low, scale, other
        B, h, w, _ = low.shape
        assert other.shape[:3] == (B, h * scale, w * scale)
        self.shape = (B, h * scale, w * scale, low.shape[3] + other.shape[3])


class Concat(HipModule):
    """Channel concatenation (reference models/common.py:313-321).  When the producers already wrote adjacent
    slices of one buffer (the normal case inside Model) this is free."""

    def __init__(self, dimension=1):
        super().__init__()
        self.d = dimension

    def out_shape(self, srcs):
        return sum(t[0] for t in srcs), srcs[0][1], srcs[0][2]

    def emit(self, plan, xs, out=None):
        if self.d != 1:
            raise NotImplementedError("only channel concatenation is on the hot path")
        v = concat_view(xs)
        if v is not None and out is None:
            return v
        B, H, W, _ = xs[0].shape
        if out is None:
            out = plan.act(B, H, W, sum(t.shape[3] for t in xs))
        c0 = 0
        for t in xs:
            plan.add(ops.copy_channels(t, out[..., c0:c0 + t.shape[3]]))
            c0 += t.shape[3]
        return out


class Add(HipModule):
    """Weighted sum of the two streams (reference models/common.py:324-331): x[0]*w + x[1]*(1-w)."""

    def __init__(self, weight=0.5):
        super().__init__()
        self.w = weight

    def out_shape(self, srcs):
        return srcs[0]

    def emit(self, plan, xs, out=None):
        a, b = xs
        if out is None:
            out = plan.act(*a.shape)
        plan.add(ops.axpby(a, b, out, self.w, 1 - self.w))
        return out


class NiNfusion(HipModule):
    """Concat + k x k convolution (no BN, no bias) + SiLU (reference models/common.py:348-360): one GEMM over the two
    streams' features, which Model.build_plan places as adjacent channel slices so the concat is free."""

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1):
        super().__init__()
        self.concat = Concat(dimension=1)
        self.conv = nn.Conv2d(c1, c2, k, s, autopad(k, p), groups=g, bias=False)
        self.act = nn.SiLU()

    def out_shape(self, srcs):
        return conv2d_shape(self.conv, srcs[0][1], srcs[0][2])

    def emit(self, plan, xs, out=None):
        x = self.concat.emit(plan, list(xs))
        return emit_conv(plan, self, x, [[(self.conv, None)]], act_code(self.act), "conv{kh}x{kw}s{sh}", out=out)


def emit_upsample(m, plan, x, out=None):
    """nn.Upsample(None, 2, 'nearest') rows of the head (yaml rows 24 / 28)."""
    if m.mode != "nearest" or m.scale_factor is None or float(m.scale_factor) != int(m.scale_factor):
        raise NotImplementedError("only integer-factor nearest upsampling is on the hot path")
    s = int(m.scale_factor)
    B, H, W, C = x.shape
    if out is None:
        out = plan.act(B, H * s, W * s, C)
    plan.add(ops.upsample_nearest(x, out, s))
    return out


# ----------------------------------------------------------------------------------------------------------
# DMFF
# ----------------------------------------------------------------------------------------------------------
class LearnableCoefficient(nn.Module):
    """Scalar gain, init 1 (reference models/common.py:569-576); folded into GEMM epilogue alphas."""

    def __init__(self):
        super().__init__()
        self.bias = nn.Parameter(torch.FloatTensor([1.0]), requires_grad=True)


class LearnableWeights(nn.Module):
    """Two scalar mixing weights, init 0.5 (reference models/common.py:579-587)."""

    def __init__(self):
        super().__init__()
        self.w1 = nn.Parameter(torch.tensor([0.5]), requires_grad=True)
        self.w2 = nn.Parameter(torch.tensor([0.5]), requires_grad=True)


class AdaptivePool2d(nn.Module):
    """Fixed-output pooling with stride = in // out, kernel = in - (out-1)*stride (reference
    models/common.py:868-891).  Holds geometry only; the arithmetic is in icaf_dmff_pool_tokens."""

    def __init__(self, output_h, output_w, pool_type="avg"):
        super().__init__()
        self.output_h, self.output_w, self.pool_type = output_h, output_w, pool_type

    def window(self, h, w):
        """-> (out_h, out_w, kh, kw, sh, sw)"""
        if h > self.output_h or w > self.output_w:
            sh, sw = h // self.output_h, w // self.output_w
            if sh == 0 or sw == 0:
                raise ValueError(f"feature map {h}x{w} too small for {self.output_h}x{self.output_w} anchors")
            return (self.output_h, self.output_w, h - (self.output_h - 1) * sh, w - (self.output_w - 1) * sw, sh, sw)
        return h, w, 1, 1, 1, 1


class CrossAttention(HipModule):
    """Bidirectional cross-modal attention parameters (reference models/common.py:590-687)."""

    def __init__(self, d_model, d_k, d_v, h, attn_pdrop=.1, resid_pdrop=.1):
        super().__init__()
        assert d_k % h == 0
        self.d_model, self.h = d_model, h
        self.d_k = self.d_v = d_model // h
        for mod in ("vis", "ir"):
            setattr(self, f"que_proj_{mod}", nn.Linear(d_model, h * self.d_k))
            setattr(self, f"key_proj_{mod}", nn.Linear(d_model, h * self.d_k))
            setattr(self, f"val_proj_{mod}", nn.Linear(d_model, h * self.d_v))
        # registration order of the reference: 6 projections, then the two output projections
        self.out_proj_vis = nn.Linear(h * self.d_v, d_model)
        self.out_proj_ir = nn.Linear(h * self.d_v, d_model)
        self.attn_drop = nn.Dropout(attn_pdrop)
        self.resid_drop = nn.Dropout(resid_pdrop)
        self.LN1 = nn.LayerNorm(d_model)
        self.LN2 = nn.LayerNorm(d_model)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=0.001)
                nn.init.constant_(m.bias, 0)


def _mlp(d_model, block_exp, resid_pdrop):
    return nn.Sequential(nn.Linear(d_model, block_exp * d_model), nn.GELU(),
                         nn.Linear(block_exp * d_model, d_model), nn.Dropout(resid_pdrop))


class CrossTransformerBlock(HipModule):
    """One parameter-shared iterative cross-attention block (reference models/common.py:690-759).  `ln_input`,
    `ln_output`, `mlp` and the block-level `LN1` exist only so that reference checkpoints load strictly; the
    reference never uses them in forward."""

    def __init__(self, d_model, d_k, d_v, h, block_exp, attn_pdrop, resid_pdrop, loops_num=1):
        super().__init__()
        self.loops = loops_num
        self.ln_input = nn.LayerNorm(d_model)
        self.ln_output = nn.LayerNorm(d_model)
        self.crossatt = CrossAttention(d_model, d_k, d_v, h, attn_pdrop, resid_pdrop)
        self.mlp_vis = _mlp(d_model, block_exp, resid_pdrop)
        self.mlp_ir = _mlp(d_model, block_exp, resid_pdrop)
        self.mlp = _mlp(d_model, block_exp, resid_pdrop)
        self.LN1 = nn.LayerNorm(d_model)
        self.LN2 = nn.LayerNorm(d_model)
        for i in range(1, 9):
            setattr(self, f"coefficient{i}", LearnableCoefficient())

    # packed parameters: per-modality weight stacks [2][Np][Kp]
    def _packed(self, plan):
        def make():
            ca = self.crossatt
            dt, f = plan.dtype, (lambda t: t.detach().float())

            def lin(vis, ir):          # one nn.Linear (or several, concatenated along the outputs) per modality
                return ops.pack_streams([(torch.cat([f(l.weight) for l in ls]), torch.cat([f(l.bias) for l in ls])) for ls in (vis, ir)], dt)
            qkv = lin(*([getattr(ca, f"{n}_proj_{m}") for n in ("que", "key", "val")] for m in ("vis", "ir")))
            outp = lin([ca.out_proj_vis], [ca.out_proj_ir])
            fc1 = lin([self.mlp_vis[0]], [self.mlp_ir[0]])
            fc2 = lin([self.mlp_vis[2]], [self.mlp_ir[2]])
            ln = {k: f(v).contiguous() for k, v in (("a1w", ca.LN1.weight), ("a1b", ca.LN1.bias),
                                                    ("a2w", ca.LN2.weight), ("a2b", ca.LN2.bias),
                                                    ("mw", self.LN2.weight), ("mb", self.LN2.bias))}
            co = [float(getattr(self, f"coefficient{i}").bias.detach().float().cpu()) for i in range(1, 9)]
            return dict(qkv=qkv, out=outp, fc1=fc1, fc2=fc2, ln=ln, co=co,
                        eps=(ca.LN1.eps, ca.LN2.eps, self.LN2.eps))
        return self._cached(("blk", plan.dtype, plan.device), make)

    @staticmethod
    def _gemm(plan, x, packed, y, cin, cout, act, res=None, alpha_acc=1.0, alpha_res=1.0, name="linear"):
        wp, kp, bp = packed
        rows = x.shape[1]
        gs = dict(x=x.stride(0), w=wp.stride(0), bias=bp.stride(0), y=y.stride(0),
                  res=res.stride(0) if res is not None else 0)

        def rows_act(t, c):       # group 0 of a (2, rows, C) token tensor (row stride t.stride(1)) as a (rows, 1, 1, c) act
            ld = t.stride(1)
            return t[0].as_strided((rows, 1, 1, c), (ld, ld, ld, 1))
        plan.add(ops.conv2d(rows_act(x, cin), wp, kp, bp, rows_act(y, cout), 1, 1, 1, 1, 0, 0,
                            cin, cout, act, res=rows_act(res, cout) if res is not None else None,
                            alpha_acc=alpha_acc, alpha_res=alpha_res, groups=2, group_strides=gs, name=name))

    # 16-bit types: one iteration = icaf_dmff_ln_qkv + icaf_dmff_attn_mlp (2 launches) instead of 7 (ICAF_DMFF_FUSE=0: A/B switch)
    fuse_block = OPT.dmff_fuse
    # The two-launch kernels (dmff_fused.hip: LN + QKV, then attention + out-projection + LN + MLP in ONE workgroup) are built for C <= 512 and
    # USED up to this width.  Round 2 measured them ahead at C <= 128 only (111 vs 145 us for the seven per-layer launches at P3; at C = 256 /
    # 512 one workgroup per CU cannot hide its own latencies: 166 vs 141, 430 vs 153 us); round 3 moved C = 256 / 512 to the three-launch form
    # (dmff_wide.hip); round 4 built that form for C = 128 too (four wavefronts, weights streamed per wave into registers: no barrier in a
    # GEMM pass) and the stand-alone attention kernel got the rewritten inner loop: P3 block 88 us (two launches) vs 78 us (three), whole
    # bench 15,003 / 15,061 vs 15,181 pairs/s on one box — so the default is 64 and every yolov5s level runs three launches.
    # ICAF_DMFF_FUSE_MAX_C=128 restores the two-launch form at P3 (A/B, tests).
    fuse_max_c = OPT.dmff_fuse_max_c
    # fp32 plans keep the per-layer launches (the goldens then cover them); True runs the fp32 INSTANTIATION of the fused kernels where
    # it exists: the same templates the 16-bit path runs, held to the reference's fp32 goldens (tests/test_gpu_dmff_fused.py) — the two-launch
    # form at C <= fuse_max_c <= 128, and (round 5) the THREE-launch form every yolov5s level runs by default, at C = 128 (dmff_wide.hip)
    fuse_fp32 = OPT.dmff_fuse_fp32

    # wide levels, 16-bit types: three launches per iteration (ICAF_DMFF_WIDE=0: the seven per-layer launches, A/B switch)
    fuse_wide = OPT.dmff_wide
    res32 = OPT.dmff_res32        # loops > 1: the token stream between iterations in fp32 (A/B switch)
    wide_max_c = OPT.dmff_wide_max_c

    BlockForm = collections.namedtuple("BlockForm", "form ksplit stream32")     # form: "two-launch" / "three-launch" / "per-layer"

    def block_form(self, plan, C, N):
        """THE decision how an iteration of this block runs at a level: the class switches above say what is wanted, ops.dmff_wide_ksplit which
        hidden split is preferred, and the library (ops.dmff_block_forms, on every device) what is built.  A preferred or forced split that is
        not built falls back to none; the fp32 token stream (loops > 1) is dropped where it is not built for the split."""
        hid, h, dt = self.mlp_vis[0].out_features, self.crossatt.h, plan.dtype
        per_layer = self.BlockForm("per-layer", 1, False)
        # (fp32 plans keep the per-layer launches unless the parity instantiations are asked for)
        if not self.fuse_block or self.mlp_vis[2].in_features != hid or (dt == torch.float32 and not self.fuse_fp32):
            return per_layer
        if C <= self.fuse_max_c:
            return self.BlockForm("two-launch", 1, False) if ops.dmff_block_forms(dt, C, N, h, hid)[0] else per_layer
        if self.fuse_wide and C <= self.wide_max_c:
            ks = ops.dmff_wide_ksplit(N, C)                # few tokens per image, weights beyond an XCD's L2: hidden columns split over ks workgroups
            s32 = bool(self.res32 and int(self.loops) > 1 and dt != torch.float32)
            for form in dict.fromkeys(((ks, s32), (ks, False), (1, s32), (1, False))):
                if ops.dmff_block_forms(dt, C, N, h, hid, *form)[1]:
                    return self.BlockForm("three-launch", *form)
        return per_layer

    def emit_tokens(self, plan, tok, B, N, final_out=None):
        """tok: (2, B*N, C) [0]=RGB [1]=IR -> same shape after `loops` shared-weight iterations.  final_out: optional
        (2, B*N, C) view (any row / group strides) that the last iteration writes instead of a fresh buffer."""
        p = self._packed(plan)
        C = tok.shape[2]
        rows = tok.shape[1]
        co, ln = p["co"], p["ln"]
        hid, heads = self.mlp_vis[0].out_features, self.crossatt.h
        nloops = int(self.loops)
        form, ks, r32 = self.block_form(plan, C, N)
        coef = dict(co=co, hidden=hid)
        if nloops > 1 and (plan.dtype != torch.float32 or form == "three-launch"):
            plan.notes.setdefault("dmff_fp32_token_stream", {})[f"C={C}"] = r32

        def out(it):
            return final_out if (final_out is not None and it == nloops - 1) else plan.tokens(2, rows, C)
        # the buffers a fused form keeps across its iterations; x_att, the normalised tile and the hidden activations never reach HBM in either
        if form != "per-layer":
            qkv = plan.tokens(2, rows, 3 * C)
        if form == "three-launch":
            att = plan.tokens(2, rows, C)
            part = plan.empty((ks, 2, rows, C), torch.float32) if ks > 1 else None
            # several iterations: the residual chain x -> x_att -> x' is carried in FP32 from one iteration to the next (two ping-pong buffers); the
            # 16-bit tokens are still written (LayerNorm + QKV read them).  Rounding the stream to 16 bits twice per iteration had used up the parity
            # margin of the 3-iteration configuration (0.91 x the reference's own bf16 error)
            t32 = [plan.empty((2, rows, C), torch.float32) for _ in range(2)] if r32 else None
        for it in range(nloops):
            if form == "two-launch":         # dmff_fused.hip: LayerNorm + QKV, then attention + out-projection + LayerNorm + MLP
                plan.add(ops.dmff_ln_qkv(tok, qkv, p, ln, coef, p["eps"], B, N, heads))
                nxt = out(it)
                plan.add(ops.dmff_attn_mlp(tok, qkv, nxt, p, ln, coef, p["eps"], B, N, heads))
            elif form == "three-launch":     # dmff_wide.hip: LayerNorm + QKV, attention, out-projection + LayerNorm + MLP (+ the reduce of a hidden split)
                plan.add(ops.dmff_wide_ln_qkv(tok, qkv, p, ln, coef, p["eps"], B, N, heads))
                plan.add(ops.cross_attention(qkv, att, B, N, heads))
                nxt = out(it)
                # (the LAST iteration writes y32 too although nothing reads it — 2 * rows * C * 4 bytes, 3 % of the launch's traffic at P3: the kernels' R32
                #  instantiation writes both token streams or neither, and a third instantiation for one launch in `loops` was not worth its compile time)
                for l in ops.dmff_launches(True, True, tok, None, att, nxt, p, ln, coef, p["eps"], B, N, heads, "dmff_proj_mlp", part, ks,
                                           x32=(t32[(it - 1) & 1] if (r32 and it > 0) else None), y32=(t32[it & 1] if r32 else None)):
                    plan.add(l)
            else:
                n1 = plan.tokens(2, rows, C)
                plan.add(ops.layernorm(tok, n1, ln["a1w"], ln["a1b"], ln["a2w"], ln["a2b"], p["eps"][0], name="ln_attn"))
                qkv = plan.tokens(2, rows, 3 * C)
                self._gemm(plan, n1, p["qkv"], qkv, C, 3 * C, ops.ACT_NONE, name="qkv_proj")
                att = plan.tokens(2, rows, C)
                plan.add(ops.cross_attention(qkv, att, B, N, heads))
                xatt = plan.tokens(2, rows, C)
                self._gemm(plan, att, p["out"], xatt, C, C, ops.ACT_NONE, res=tok, alpha_res=(co[0], co[2]),
                           alpha_acc=(co[1], co[3]), name="out_proj")
                n2 = plan.tokens(2, rows, C)
                plan.add(ops.layernorm(xatt, n2, ln["mw"], ln["mb"], ln["mw"], ln["mb"], p["eps"][2], name="ln_mlp"))
                h = plan.tokens(2, rows, hid)
                self._gemm(plan, n2, p["fc1"], h, C, hid, ops.ACT_GELU, name="mlp_fc1")
                nxt = out(it)
                self._gemm(plan, h, p["fc2"], nxt, hid, C, ops.ACT_NONE, res=xatt, alpha_res=(co[4], co[6]),
                           alpha_acc=(co[5], co[7]), name="mlp_fc2")
            tok = nxt
        return tok


class TransformerFusionBlock(HipModule):
    """DMFF: Dual-Modality Feature Fusion (reference models/common.py:762-865).

    The reference's positional signature is kept; the extra keyword `loops_num` (yaml: a trailing `{loops_num: n}` mapping,
    see models/yolo.py) exposes the iterative parameter-shared loop the reference wires but never surfaces
    (models/common.py:691,744)."""

    # class-level (not set in __init__): instances un-pickled from reference checkpoints never ran this __init__
    fuse_tail = True         # run interpolate + residual + cat + conv1x1_out as one GEMM when the layout allows
    out_shape = Add.out_shape

    def __init__(self, d_model, vert_anchors=16, horz_anchors=16, h=8, block_exp=4, n_layer=1, embd_pdrop=0.1,
                 attn_pdrop=0.1, resid_pdrop=0.1, loops_num=1):
        super().__init__()
        self.n_embd, self.vert_anchors, self.horz_anchors = d_model, vert_anchors, horz_anchors
        self.pos_emb_vis = nn.Parameter(torch.zeros(1, vert_anchors * horz_anchors, d_model))
        self.pos_emb_ir = nn.Parameter(torch.zeros(1, vert_anchors * horz_anchors, d_model))
        self.avgpool = AdaptivePool2d(vert_anchors, horz_anchors, "avg")
        self.maxpool = AdaptivePool2d(vert_anchors, horz_anchors, "max")
        self.vis_coefficient = LearnableWeights()
        self.ir_coefficient = LearnableWeights()
        self.crosstransformer = nn.Sequential(*[
            CrossTransformerBlock(d_model, d_model, d_model, h, block_exp, attn_pdrop, resid_pdrop, loops_num)
            for _ in range(n_layer)])
        self.concat = Concat(dimension=1)
        self.conv1x1_out = Conv(c1=d_model * 2, c2=d_model, k=1, s=1, p=0, g=1, act=True)

    def emit(self, plan, xs, out=None):
        rgb, ir = xs
        B, H, W, C = rgb.shape
        assert ir.shape == rgb.shape and C == self.n_embd
        th, tw, kh, kw, sh, sw = self.avgpool.window(H, W)
        N = th * tw
        if N != self.pos_emb_vis.shape[1]:
            raise ValueError(f"DMFF: {th}x{tw} tokens do not match the {self.pos_emb_vis.shape[1]} positional "
                             "embeddings (input feature map smaller than the anchor grid)")

        def make():
            f = lambda t: t.detach().float().reshape(-1).contiguous()          # noqa: E731
            wv, wi = self.vis_coefficient, self.ir_coefficient
            return (f(self.pos_emb_vis), f(self.pos_emb_ir),
                    (float(wv.w1.detach().float().cpu()), float(wv.w2.detach().float().cpu())),
                    (float(wi.w1.detach().float().cpu()), float(wi.w2.detach().float().cpu())))
        pos_v, pos_i, w_v, w_i = self._cached(("dmff", plan.device), make)
        tok = plan.tokens(2, B * N, C)
        plan.add(ops.dmff_pool_tokens(rgb, ir, pos_v, pos_i, tok, th, tw, kh, kw, sh, sw, w_v, w_i))
        feat2c = concat_view([rgb, ir]) if self.fuse_tail else None
        if (2 * C * rgb.element_size()) % 128:        # the pre-term GEMM instantiations walk K in whole 128-byte slices
            feat2c = None
        blocks = list(self.crosstransformer)
        if feat2c is None or not blocks or int(blocks[-1].loops) < 1:
            # general path: materialise cat(rgb + up(tok_rgb), ir + up(tok_ir)), then the 1x1 fuse conv
            for blk in blocks:
                tok = blk.emit_tokens(plan, tok, B, N)
            merged = plan.act(B, H, W, 2 * C)
            plan.add(ops.dmff_upsample_merge(tok, rgb, ir, merged, th, tw))
            return self.conv1x1_out.emit(plan, merged, out=out)
        # Fused tail (both streams' features are adjacent channel slices of one buffer, as Model.build_plan places them):
        # the 1x1 convolution commutes with the bilinear resize and with the residual add (all linear), so
        #   conv(cat(rgb + up(t_rgb), ir + up(t_ir))) = conv(cat(rgb, ir)) + up(conv(cat(t_rgb, t_ir)))
        # The token-resolution product P is a tiny GEMM (fp32 out); the full-resolution GEMM reads the untouched
        # features and adds bilinear(P) before bias + SiLU in its epilogue.  The (B, H, W, 2C) merged tensor of
        # models/common.py:827-840 is never written or read.
        tokcat = plan.empty((B * N, 2 * C), plan.dtype)                      # [t_rgb | t_ir] per token
        final = tokcat.as_strided((2, B * N, C), (C, 2 * C, 1))
        for j, blk in enumerate(blocks):
            tok = blk.emit_tokens(plan, tok, B, N, final_out=final if j == len(blocks) - 1 else None)
        conv = self.conv1x1_out
        wp, kp, _ = conv.packed(plan)                                         # BN scale folded in; bias stays in the main GEMM
        P = plan.empty((B, th, tw, C), torch.float32)
        plan.add(ops.conv2d(tokcat.view(B * N, 1, 1, 2 * C), wp, kp, None, P.view(B * N, 1, 1, C), 1, 1, 1, 1, 0, 0,
                            2 * C, C, ops.ACT_NONE, name="dmff_tail_tokens"))
        return conv.emit(plan, feat2c, out=out, pre_term=P)


# ----------------------------------------------------------------------------------------------------------
# Detect
# ----------------------------------------------------------------------------------------------------------
class Detect(HipModule):
    """Detection head (reference models/yolo_test.py:26-71).  Per level: 1x1 conv (fp32 output) + one decode
    kernel that writes z / logits / the permuted raw map directly in their final layouts."""
    stride = None
    export = False
    # 16-bit plans: a level's 1x1 conv and its decode run as ONE launch (icaf_detect_conv; ICAF_DETECT_FUSE=0: A/B switch).  A class
    # default: un-pickled reference checkpoints never run this constructor.
    fuse_decode = OPT.detect_fuse

    def out_shape(self, srcs):       # (z, logits, raws): nothing downstream reads a shape
        return None

    def __init__(self, nc=80, anchors=(), ch=()):
        super().__init__()
        self.nc, self.no = nc, nc + 5
        self.nl, self.na = len(anchors), len(anchors[0]) // 2
        self.grid = [torch.zeros(1)] * self.nl
        a = torch.tensor(anchors).float().view(self.nl, -1, 2)
        self.register_buffer("anchors", a)
        self.register_buffer("anchor_grid", a.clone().view(self.nl, 1, -1, 1, 1, 2))
        self.m = nn.ModuleList(nn.Conv2d(c, self.no * self.na, 1) for c in ch)

    def _apply(self, fn, *a, **k):
        """Anchors stay fp32 whatever the model is cast to: pixel sizes such as 373 are not representable in bf16
        and the decode runs in fp32 anyway."""
        keep = {n: getattr(self, n).detach().float().clone() for n in ("anchors", "anchor_grid")}
        r = super()._apply(fn, *a, **k)
        for n, v in keep.items():
            cur = getattr(self, n)
            if cur.dtype != torch.float32:
                setattr(self, n, v.to(cur.device))
        return r

    def emit(self, plan, xs):
        B = xs[0].shape[0]
        rows = sum(self.na * t.shape[1] * t.shape[2] for t in xs)
        z = plan.empty((B, rows, self.no), torch.float32)
        logits = plan.empty((B, rows, self.nc), torch.float32)
        raws, off = [], 0
        ag = self.anchor_grid.detach().float().cpu().view(self.nl, self.na * 2)
        strides = [float(s) for s in self.stride]
        for l, x in enumerate(xs):
            _, ny, nx, c = x.shape
            conv = self.m[l]
            nout = self.na * self.no
            wp, kp, bp = self._cached(("det", l, plan.dtype, plan.device), lambda: ops.pack_streams(
                [(conv.weight.detach().float(), conv.bias.detach().float())], plan.dtype))
            raw = plan.empty((B, self.na, ny, nx, self.no), torch.float32)
            if self.fuse_decode and ops.detect_conv_ok(x, self.na, self.no, c):
                # 16-bit maps: conv + decode in ONE launch (icaf_detect_conv) - the fp32 conv map never reaches HBM
                plan.add(ops.detect_conv(x, wp, kp, bp, z, logits, raw, self.na, self.no, off, strides[l], ag[l].tolist(), c))
                raws.append(raw)
                off += self.na * ny * nx
                continue
            # pixel stride padded to a 16-byte multiple (18 -> 20 floats): the conv epilogue then leaves 16-byte stores instead of scalar ones
            p = plan.act(B, ny, nx, (nout + 3) // 4 * 4, dtype=torch.float32)[..., :nout]
            plan.add(ops.conv2d(x, wp, kp, bp, p, 1, 1, 1, 1, 0, 0, c, nout, ops.ACT_NONE, name="detect_conv"))
            plan.add(ops.detect_decode(p, z, logits, raw, self.na, self.no, off, strides[l], ag[l].tolist()))
            raws.append(raw)
            off += self.na * ny * nx
        return z, logits, raws

    def forward(self, xs):
        if self.training:
            raise NotImplementedError("Detect: training branch is outside the inference hot path")
        dt = _module_dtype(self)
        plan = Plan(xs[0].device, dt)
        acts = [to_act(t, dt) for t in xs]
        z, logits, raws = self.emit(plan, acts)
        plan.run()
        return z, logits, raws


__all__ = ["autopad", "Conv", "Bottleneck", "C3", "SPPF", "Concat", "Add", "NiNfusion", "LearnableCoefficient", "LearnableWeights",
           "AdaptivePool2d", "CrossAttention", "CrossTransformerBlock", "TransformerFusionBlock", "Detect",
           "emit_upsample", "HipModule", "math"]
