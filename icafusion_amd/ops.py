"""Thin torch-tensor front end over the C ABI (include/icaf.h).

Activation tensors ("acts") are torch views of shape (B, H, W, C) whose last dim is contiguous and whose pixel
stride ld = t.stride(2) may exceed C (channel slice of a wider NHWC buffer).  Every function here either launches
one kernel on a stream or returns a `Launch` record that does so later (used by the static execution plan).
PyTorch only provides device memory and streams here — none of its operators run on the hot path.
"""
import collections
import contextlib
import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib
from .options import OPT
from ._lib import BneckArgs, ConvArgs, DmffArgs, FrameGeom, Stem2Args, WarpGeom, Y16Geom, YuvGeom, check, lib, F32, BF16, F16, ACT_NONE, ACT_SILU, ACT_GELU, ACT_RELU  # noqa: F401
from ._lib import CONFLUENCE_MAX_CAND, LOSS_MAX_LEVELS, LOSS_MAX_ANCHORS, LOSS_MAX_TARGETS, LOSS_SLOT_INTS  # noqa: F401

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}     # elements per 16-byte vector
N_ALIGN = 128     # packed-weight rows are padded to this (largest BN tile)
K_ALIGN_BYTES = 128


def dtype_code(dt):
    try:
        return _DT[dt]
    except KeyError:
        raise _lib.IcafError(f"unsupported dtype {dt}; supported: float32, bfloat16, float16") from None


def k_align(dt):
    return K_ALIGN_BYTES // torch.empty((), dtype=dt).element_size()


def current_stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def _act_geom(t):
    """(B, H, W, C, ld) of an act; a 5-D (2, B, H, W, C) *pair* (the two streams of the backbone at a constant
    element stride, t.stride(0)) reports the geometry of one member."""
    if t.dim() == 5:
        assert t.shape[0] == 2, f"pair acts hold exactly two streams, got {t.shape}"
        t = t[0]
    assert t.dim() == 4 and t.stride(3) == 1, f"act must be NHWC-contiguous in C, got {t.shape} {t.stride()}"
    B, H, W, Cc = t.shape
    ld = t.stride(2)
    assert t.stride(1) == W * ld and (B == 1 or t.stride(0) == H * W * ld), f"bad act strides {t.stride()}"
    return B, H, W, Cc, ld


def flat_pair(t):
    """View a pair act (2, B, H, W, C) as one act of batch 2B (weight-less kernels treat the streams as more batch)."""
    if t.dim() == 4:
        return t
    G, B, H, W, Cc = t.shape
    assert t.stride(0) == B * t.stride(1), "pair members must be adjacent in memory"
    return t.as_strided((G * B, H, W, Cc), t.stride()[1:])


class Launch:
    """One recorded kernel launch: fn(*args, stream)."""
    __slots__ = ("fn", "args", "keep", "name", "flops", "bytes", "branch")

    def __init__(self, fn, args, keep=(), name="", flops=0, nbytes=0):
        self.fn, self.args, self.keep, self.name, self.flops, self.bytes = fn, args, keep, name, flops, nbytes
        self.branch = 0          # 0 = main chain; > 0 = a side branch of the captured graph (engine.Plan.branches)

    def __call__(self, stream_ptr):
        st = self.fn(*self.args, stream_ptr)
        if st != 0:
            check(st, self.name)


# ------------------------------------------------------------------------------------------------------------
# weight packing (one-time, at plan build; not on the hot path)
# ------------------------------------------------------------------------------------------------------------
def pack_matrix(w2d, dt):
    """[Cout][K] fp32 -> zero-padded [Np][Kp] in dtype dt (K-major rows)."""
    n, k = w2d.shape
    ka = k_align(dt)
    np_, kp = -(-n // N_ALIGN) * N_ALIGN, -(-k // ka) * ka
    out = torch.zeros((np_, kp), dtype=dt, device=w2d.device)
    out[:n, :k] = w2d.to(dt)
    return out, kp


def pack_bias(b, n):
    np_ = -(-n // N_ALIGN) * N_ALIGN
    out = torch.zeros((np_,), dtype=torch.float32, device=b.device)
    out[:n] = b.float()
    return out


def pack_conv_weight(w4d, dt, cin_pad=None):
    """[Cout][Cin][kh][kw] -> [Np][Kp] with k = (kh, kw, cin) and cin padded to cin_pad."""
    co, ci, kh, kw = w4d.shape
    w = w4d.permute(0, 2, 3, 1)
    if cin_pad is not None and cin_pad != ci:
        w = torch.nn.functional.pad(w, (0, cin_pad - ci))
    return pack_matrix(w.reshape(co, -1).contiguous(), dt)


def pack_streams(rows, dt, cin_pad=None):
    """rows: one fp32 (weight [Cout][K] or [Cout][Cin][kh][kw], bias [Cout] or None) per stream -> (wp, kp, bp): the plain [Np][Kp] /
    [Np] packs for one row, the contiguous stacks [2][Np][Kp] / [2][Np] for two (bp is None where the biases are)."""
    packs = []
    for w, b in rows:
        wp, kp = pack_matrix(w, dt) if w.dim() == 2 else pack_conv_weight(w, dt, cin_pad)
        packs.append((wp, None if b is None else pack_bias(b, w.shape[0])))
    if len(packs) == 1:
        return packs[0][0], kp, packs[0][1]
    wps, bps = zip(*packs)
    return torch.stack(wps).contiguous(), kp, None if bps[0] is None else torch.stack(bps).contiguous()


_FRAG_CACHE = {}              # id(packed tensor) -> (weakref to it, fragment-major copy); entries die with the packed tensor
# (execution switches — which kernels the tuner may offer a layer, retune requests — live in options.PlanOptions; read as OPT.<field>)


def frag_weights(w_packed):
    """Second copy of packed 16-bit weights ([Np][Kp] or stacked [G][Np][Kp]) in FRAGMENT-MAJOR order for the kernels that feed
    the weight operand from registers (igemm_wreg.hip; icaf.h: icaf_conv_args.wf): [G][Np / 32][Kp / 16][64][8], lane (hi * 32 + r) of
    block (nb, ks) = w[nb * 32 + r][ks * 16 + hi * 8 : + 8].  Built once per packed tensor (plan-build time), cached by storage."""
    key = id(w_packed)
    hit = _FRAG_CACHE.get(key)
    if hit is not None and hit[0]() is w_packed:
        return hit[1]
    w = w_packed if w_packed.dim() == 3 else w_packed[None]
    G, np_, kp = w.shape
    ve = 16 // w.element_size()                     # elements per 16-byte fragment: 8 (16-bit types), 4 (fp32: the parity instantiation of dmff_wide.hip)
    assert np_ % 32 == 0 and kp % (2 * ve) == 0 and w.element_size() in (2, 4)
    f = w.reshape(G, np_ // 32, 32, kp // (2 * ve), 2, ve).permute(0, 1, 3, 4, 2, 5).contiguous()      # g, nb, ks, hi, r, e
    f = f.reshape(G, np_ // 32, kp // (2 * ve), 64, ve)
    if w_packed.dim() == 2:
        f = f[0]
    # The copy lives exactly as long as the packed tensor it mirrors: HipModule.invalidate() / .to() / load_state_dict drop the module's
    # packed tensors, and the finaliser then drops the copy (a strong reference here pinned every old pack in device memory forever).
    _FRAG_CACHE[key] = (weakref.ref(w_packed), f)
    weakref.finalize(w_packed, _FRAG_CACHE.pop, key, None)
    return f


def s2d_conv_weight(w4d):
    """6x6/s2/p2 kernel over C channels -> equivalent 3x3/s1/p1 kernel over the 4C space-to-depth channels
    ordered (dy, dx, c):  W3[co][(dy*2+dx)*C + c][ty][tx] = W[co][c][2ty+dy][2tx+dx]."""
    co, ci, kh, kw = w4d.shape
    assert kh == 6 and kw == 6
    w = w4d.reshape(co, ci, 3, 2, 3, 2)                  # co, c, ty, dy, tx, dx
    return w.permute(0, 3, 5, 1, 2, 4).reshape(co, 4 * ci, 3, 3).contiguous()


# ------------------------------------------------------------------------------------------------------------
# launches
# ------------------------------------------------------------------------------------------------------------
# A 1x1 + SiLU layer riding on another launch's output tile (conv2d's chain=, bottleneck's cv3=): w / kp / bias its packed weights (stacked per
# stream for pair acts), y its output, cout its width.  keep: the carrying layer's own output is written too and the 1x1 consumes it as stored.
# x2: the 1x1 reads K = [the carrying layer's tile | x2] (a C3's cv3 over cat(m, cv2)).
class Chain(collections.namedtuple("Chain", "w kp bias y cout keep x2", defaults=(False, None))):
    __slots__ = ()

    @classmethod
    def of(cls, v):                       # a chain= / cv3= argument: None, a Chain, or a mapping with its field names (the kernel tests' spelling)
        return v if v is None or isinstance(v, cls) else cls(**v)

    def __getitem__(self, k):             # a field by its name too: Launch.keep holds the record, and its readers ask chain["y"]
        return getattr(self, k) if isinstance(k, str) else tuple.__getitem__(self, k)


def conv2d(x, w_packed, kp, bias, y, kh, kw, sh, sw, ph, pw, cin, cout, act, res=None, alpha_acc=1.0,
           alpha_res=1.0, groups=1, group_strides=None, tile=0, name="conv2d", pre=None, chain=None, pre_nearest=False, res_pre_act=False):
    """Record an implicit-GEMM conv / linear.  x, y, res are acts; for groups=2 they are the group-0 views and
    group_strides = dict(x=, w=, bias=, y=, res=) gives element strides to group 1.
    res_pre_act: the residual is added IN FRONT of the activation, y = relu(conv(x) + bias + res) rounded once (icaf.h: res_mode = 1; a
    ResNet bottleneck's conv3): ReLU layers with a residual, unit alphas, no pre term and no chained layer only — the library refuses the rest."""
    chain = Chain.of(chain)
    B, H, W, cx, ldx = _act_geom(x)
    By, Ho, Wo, cy, ldy = _act_geom(y)
    assert cx >= cin and cy >= cout and By == B
    assert Ho == (H + 2 * ph - kh) // sh + 1 and Wo == (W + 2 * pw - kw) // sw + 1, "conv geometry mismatch"
    if x.dim() == 5:                  # pair act: both backbone streams in one launch, per-stream weights
        assert group_strides is None and y.dim() == 5 and w_packed.dim() == 3 and (res is None or res.dim() == 5)
        groups = 2
        group_strides = dict(x=x.stride(0), w=w_packed.stride(0), bias=bias.stride(0) if bias is not None else 0,
                             y=y.stride(0), res=res.stride(0) if res is not None else 0)
    a = ConvArgs()
    a.x, a.w, a.y = x.data_ptr(), w_packed.data_ptr(), y.data_ptr()
    a.bias = bias.data_ptr() if bias is not None else None
    a.res = res.data_ptr() if res is not None else None
    gs = group_strides or {}
    a.x_gs, a.w_gs, a.bias_gs = gs.get("x", 0), gs.get("w", 0), gs.get("bias", 0)
    a.y_gs, a.res_gs = gs.get("y", 0), gs.get("res", 0)
    a.groups = groups
    a.B, a.H, a.W, a.Cin, a.ldx = B, H, W, cin, ldx
    a.Ho, a.Wo, a.Cout, a.ldy = Ho, Wo, cout, ldy
    a.kh, a.kw, a.sh, a.sw, a.ph, a.pw = kh, kw, sh, sw, ph, pw
    a.ldr = _act_geom(res)[4] if res is not None else 0
    a.Kp, a.act = kp, act
    a.dtype, a.out_dtype = dtype_code(x.dtype), dtype_code(y.dtype)
    assert w_packed.dtype == x.dtype and (res is None or res.dtype == x.dtype)
    aa = alpha_acc if isinstance(alpha_acc, (tuple, list)) else (alpha_acc, alpha_acc)
    ar = alpha_res if isinstance(alpha_res, (tuple, list)) else (alpha_res, alpha_res)
    a.alpha_acc[0], a.alpha_acc[1] = float(aa[0]), float(aa[1])
    a.alpha_res[0], a.alpha_res[1] = float(ar[0]), float(ar[1])
    a.tile = tile
    a.res_mode = int(bool(res_pre_act))
    if pre is not None:               # fp32 coarse map (B, h, w, >= cout) added, bilinearly resized, before the activation
        Bp, hp, wp_, cp, ldp = _act_geom(pre)
        assert pre.dtype == torch.float32 and Bp == B and cp >= cout and groups == 1
        a.pre, a.pre_h, a.pre_w, a.ldpre = pre.data_ptr(), hp, wp_, ldp
        a.pre_mode = int(bool(pre_nearest))     # nearest: the map is the low-resolution half of a 1x1 conv over cat(up(a), b)
    if chain is not None:             # chained 1x1 + SiLU on the output tile (icaf.h)
        y2 = chain.y
        B2, H2, W2, c2y, ldy2 = _act_geom(y2)
        assert (B2, H2, W2) == (B, Ho, Wo) and c2y >= chain.cout and y2.dtype == x.dtype and (y2.dim() == 5) == (x.dim() == 5)
        a.w2, a.y2 = chain.w.data_ptr(), y2.data_ptr()
        a.bias2 = chain.bias.data_ptr() if chain.bias is not None else None
        a.Kp2, a.Cout2, a.ldy2 = chain.kp, chain.cout, ldy2
        a.chain_keep = int(bool(chain.keep))
        if x.dim() == 5:
            a.w2_gs, a.y2_gs = chain.w.stride(0), y2.stride(0)
            a.bias2_gs = chain.bias.stride(0) if chain.bias is not None else 0
        x2 = chain.x2
        if x2 is not None:            # C3 tail: the chained layer reads K = [this layer's tile | x2] (icaf.h: icaf_conv_args.x2)
            Bx, Hx, Wx, cx2, ldx2 = _act_geom(x2)
            assert (Bx, Hx, Wx) == (B, Ho, Wo) and cx2 >= cout and x2.dtype == x.dtype and (x2.dim() == 5) == (x.dim() == 5)
            a.x2, a.ldx2, a.x2_gs = x2.data_ptr(), ldx2, (x2.stride(0) if x.dim() == 5 else 0)
    wf = None
    if wants_wf(a):                   # a kernel that feeds the weight operand from registers (igemm_wreg.hip, cwide.hip) is built for this layer
        wf = frag_weights(w_packed)
        a.wf, a.wf_gs = wf.data_ptr(), (wf.stride(0) if w_packed.dim() == 3 else 0)
    m = B * Ho * Wo
    flops = 2.0 * m * cout * kh * kw * cin * groups
    es, eo = x.element_size(), y.element_size()
    nbytes = groups * (B * H * W * cin * es + cout * kh * kw * cin * es + m * cout * eo
                       + (m * cout * es if res is not None else 0))
    if chain is not None:
        k2 = cout * (2 if chain.x2 is not None else 1)
        flops += 2.0 * m * k2 * chain.cout * groups
        nbytes += groups * (m * chain.cout - (0 if chain.keep else m * cout)) * eo      # y2 is written instead of / besides y
        if chain.x2 is not None:
            nbytes += groups * (m * cout + k2 * chain.cout) * es       # the x2 half of the chained layer's input, its weights
    return Launch(lib().icaf_conv2d, (C.byref(a),), keep=(a, x, w_packed, bias, y, res, pre, chain, wf), name=name, flops=flops,
                  nbytes=nbytes)


def bottleneck(x, w1_packed, kp1, bias1, w2_packed, kp2, bias2, y, c, add, shape, name="bottleneck", cv3=None):
    """Whole Bottleneck (1x1 -> 3x3 [+ x]) in one launch (icaf_bottleneck).  x, y: acts or pair acts of c channels in
    DIFFERENT buffers; w1 / w2: packed 1x1 / 3x3 weights (stacked per stream for pair acts).
    cv3: Chain with x2 — the C3's cv3 rides on the block: x2 is the cv2 half of its input, w its packed weights with K columns ordered
    [cv2 | m]; only cv3's output (cv3.y) is written and `y` may be None."""
    cv3 = Chain.of(cv3)
    if cv3 is not None and y is None:
        y = cv3.y[..., :c]                       # (ignored by the kernel; satisfies the argument checks)
    inner = conv2d(x, w2_packed, kp2, bias2, y, 3, 3, 1, 1, 1, 1, c, c, ACT_SILU, res=x if add else None, name=name,
                   chain=None if cv3 is None else cv3._replace(x2=None))
    b = BneckArgs()
    C.memmove(C.byref(b.conv), C.byref(inner.keep[0]), C.sizeof(ConvArgs))
    b.w1, b.bias1 = w1_packed.data_ptr(), bias1.data_ptr()
    paired = x.dim() == 5
    b.w1_gs, b.bias1_gs = (w1_packed.stride(0), bias1.stride(0)) if paired else (0, 0)
    b.Kp1, b.shape = kp1, shape
    B, H, W, _, _ = _act_geom(x)
    g = 2 if paired else 1
    flops = inner.flops + 2.0 * g * B * H * W * c * c
    es = x.element_size()
    nbytes = g * (B * H * W * c * es * (3 if add else 2) + (9 * c * c + c * c) * es)
    if cv3 is not None:
        x2 = cv3.x2
        B2, H2, W2, c2, ldx2 = _act_geom(x2)
        assert (B2, H2, W2) == (B, H, W) and c2 >= c and x2.dtype == x.dtype and (x2.dim() == 5) == paired
        b.x2, b.ldx2, b.x2_gs = x2.data_ptr(), ldx2, x2.stride(0) if paired else 0
        nbytes = g * (B * H * W * es * (2 * c + cv3.cout) + (10 * c * c + 2 * c * cv3.cout) * es)
        flops += 2.0 * g * B * H * W * c * cv3.cout          # (conv2d counted K = c for the chained layer; cv3 has K = 2c)
    return Launch(lib().icaf_bottleneck, (C.byref(b),), keep=(b, inner.keep, w1_packed, bias1, cv3), name=name + ("+cv3" if cv3 else ""),
                  flops=flops, nbytes=nbytes)


_TUNE_CACHE = {}
_RETUNED = set()
BUILT_NOT_OFFERED = (29, 31, 32, 33, 34)      # 128x64 with 8 wavefronts (graph_tune.py tries it), LDS-DMA 128 B x3 (pipeline 3: never won)
# cwide.hip (80 + shape): (stride, Cin) -> ids, for Cout in multiples of 128 (stride 1: 128 -> 128 only); 8 x 16 / 8 x 8 output pixels per workgroup
_CWIDE = {(1, 128): (81, 82), (2, 64): (83, 85), (2, 128): (84,)}
_CTILE = {41: (32, 1), 42: (64, 1), 43: (64, 1), 44: (64, 2), 45: (128, 1)}     # ctile.hip (40 + shape): id -> (BN, stride)


def _cwide_ids(s3, cin, cout):
    return [] if (cout % 128 or (s3 == 1 and cout != 128)) else list(_CWIDE.get((s3, cin), ()))


def cwide_shapes(kh, kw, sh, sw, ph, pw, cin, cout):
    """Tile ids (80 + shape) of cwide.hip that are built for this 3x3 layer: resident halo patch, weights streamed into registers."""
    return _cwide_ids(sh if ((kh, kw, ph, pw) == (3, 3, 1, 1) and sh == sw) else 0, cin, cout)


def _conv_signature(a):
    return (a.B * a.Ho * a.Wo, a.Cout, a.Cin, a.kh, a.kw, a.sh, a.sw, a.H, a.W, a.ldx, a.ldy, a.groups, a.dtype,
            a.out_dtype, a.act, bool(a.res) + getattr(a, "res_mode", 0), bool(a.pre) + a.pre_mode, a.Cout2 if a.w2 else 0, 2 if a.x2 else bool(a.chain_keep))


class _Layer:
    """What the candidate rules ask of one conv (any object with ConvArgs' field names), derived once."""
    def __init__(self, a):
        self.same16 = a.dtype != F32 and a.out_dtype == a.dtype            # 16-bit in and out
        self.pre, self.chain, self.tail, self.plain = bool(a.pre), bool(a.w2) and not a.x2, bool(a.w2) and bool(a.x2), not a.pre and not a.w2
        self.taps128 = (a.Cin * 2) % 128 == 0                              # whole 128-byte K slices per filter tap (16-bit types)
        self.s3 = a.sh if ((a.kh, a.kw, a.ph, a.pw) == (3, 3, 1, 1) and a.sh == a.sw) else 0      # 3x3 / pad 1 with stride s3 (0: another filter)
        self.one = (a.kh, a.kw, a.sh, a.sw, a.ph, a.pw) == (1, 1, 1, 1, 0, 0)                     # plain 1x1
        self.silu, self.pix = a.act == ACT_SILU, a.B * a.Ho * a.Wo
        # the two families that read the fragment-major weight copy (icaf_conv_args.wf): offered once it exists, and it is built for them
        self.wreg = self.same16 and self.taps128 and self.plain and a.Cout > 64 and OPT.wreg_gemm
        self.cwide = _cwide_ids(self.s3, a.Cin, a.Cout) if (self.same16 and self.silu and not self.pre and OPT.cwide) else []


def wants_wf(a):
    """Does the layer get the fragment-major weight copy — is an igemm_wreg.hip or cwide.hip kernel built for it?"""
    L = _Layer(a)
    return bool(L.wreg or L.cwide)


def conv_candidates(a):
    """Launch-configuration ids worth timing for one conv (ConvArgs `a`), each id's rule stated once, by kernel family; chained / pre-term
    launches only have the configurations that are built for them.  Ids the library builds and no rule offers: BUILT_NOT_OFFERED.
    Activations: igemm.hip, igemm_stream.hip and igemm_wreg.hip dispatch on all four codes (128 x 512 of igemm_wreg not on GELU); cstream.hip,
    cwide.hip, ctile.hip and every chained / pre-term launch are SiLU-only — `L.silu` below is the library's own check, so a ReLU layer
    (VGGblock) is never offered an id of theirs.  res_mode = 1 (the residual in front of the ReLU, ResNetblock's conv3) exists on the
    families that run ReLU, as a plain same-type ReLU layer with a residual; any other request has no configuration at all."""
    L = _Layer(a)
    if getattr(a, "res_mode", 0) and not (a.res_mode == 1 and a.res and a.act == ACT_RELU and L.plain and a.out_dtype == a.dtype):
        return []
    big1 = a.out_dtype != F32 and a.Cout > 64                              # the 128x128 tile: no fp32-output build, and 128x64 serves Cout <= 64
    if L.tail:                         # C3 tail (the chained cv3 reads [tile | x2]): cwide.hip's 8 x 16 / 8 x 8 forms only
        # Below ~200 k pixels per stream (the 40 x 40 maps of yolov5s at batch 32 / 64: one round of 8 x 16 tiles for the chip) only the 8 x 8
        # form is offered: isolated timings prefer 8 x 16 there (2 workgroups of 252 registers and 70 KB per CU), but with a second forward in
        # flight that form starves the co-running kernels — same-box A/B of the whole bench: 15,858 with 8 x 16 against 16,082 without the tail and
        # 16,091 with 8 x 8 (3 workgroups of 168 registers and 35 KB).  The 80 x 80 / 160 x 160 maps of yolov5l have 4 - 16 x the tiles: tuned.
        return ([82] if L.pix < OPT.tail_8x16_minpix else [81, 82]) if OPT.cwide else []
    cands = []
    # ---- igemm.hip: tile + 10 * pipeline (0: LDS-DMA 64 B x3, 1: register-staged, 2: LDS-DMA 128 B x2; 3 = 128 B x3 never won) ----
    if L.chain:                        # chained 1x1: one N tile covering both layers, LDS-DMA pipelines 0 / 2
        cands += [2, 22] if max(a.Cout, a.Cout2) <= 64 else [1, 21]
    elif L.pre:                        # pre-activation term: built for tiles 128x128 / 128x64 on the LDS-DMA pipelines 0 / 2
        cands += [t + 10 * pipe for pipe in (0, 2) for t in (1, 2) if t == 2 or big1]
        if L.same16 and a.Cout >= 128 and L.taps128:
            cands.append(28)                 # the 8-wavefront 128x128 tile carries the pre term as well
    else:
        cands += [t + 10 * pipe for pipe in (0, 1, 2) for t in (1, 2, 3, 4) if (t != 1 or big1) and (t != 3 or a.Cout <= 32)]
        if L.same16 and a.Cout >= 128:       # 8-wavefront tiles (128-byte LDS-DMA pipeline only)
            cands += [25, 28] + ([26] if a.Cout >= 256 else [])
    # ---- igemm_stream.hip: persistent streaming GEMM, 128 x 64 (52) and 128 x 128 (51), also with the pre term of 1x1 SiLU layers; a launch
    #      the device's CU count rules out returns an error and is skipped ----
    if (L.same16 and L.taps128 and a.Cout % 8 == 0 and OPT.stream_gemm
            and (L.plain or (L.pre and L.silu and L.one and a.groups == 1))):
        cands += [52] + ([51] if a.Cout > 64 else [])
    # ---- cstream.hip: persistent 3x3 with the filter (and a chained 1x1) resident in LDS, 64 -> (<= 64) channels ----
    if (L.s3 == 1 and a.Cin == 64 and a.Cout <= 64 and a.Cout % 8 == 0 and L.same16 and L.silu and not L.pre and OPT.cstream
            and (not L.chain or (a.Cout == 64 and a.Cout2 <= 64))):
        cands.append(71)
    # ---- cwide.hip: resident halo patch, weights (and the chained 1x1's) streamed into registers ----
    if a.wf and (not L.chain or (a.Cout == 128 and a.Cout2 <= 128 and a.Cout2 % 32 == 0)):
        cands += L.cwide
    # ---- igemm_wreg.hip: weights fed from registers ----
    if a.wf and L.wreg:
        cands.append(61)                     # 128 x 128 ...
        if a.Cout > 128 and -(-a.Cout // 256) * 256 <= -(-a.Cout // 128) * 128:
            cands.append(62)                 # ... and 128 x 256 (its last channel tile must stay inside the packed Np = Cout rounded up to 128: wreg_check)
        # round 4: a wave owns 64 channels — the pixel feed per MAC halves
        if a.Cout > 128 and a.Cout % 256 == 0:
            cands.append(64)                 # 128 x 256 with four waves: two workgroups per CU
        if a.Cout > 256 and a.Cout % 512 == 0 and a.act != ACT_GELU:
            cands.append(63)                 # 128 x 512 with eight waves
        if L.pix * a.groups <= OPT.wreg64_maxpix:  # few pixels (the 20 x 20 / 40 x 40 rows at batch 32): 64-pixel tiles double the workgroups
            cands.append(66)                 # 64 x 128, four waves x 32 channels
            if a.Cout > 128 and a.Cout % 256 == 0:
                cands.append(65)             # 64 x 256, four waves x 64 channels
    # ---- ctile.hip: 3x3 direct convolution from an LDS halo patch ----
    if L.s3 and L.silu and a.out_dtype == a.dtype and L.plain:
        cands += [i for i, (bn, stride) in _CTILE.items() if L.s3 == stride and a.Cout <= bn and (bn < 64 or a.Cout > bn // 2)]
    return cands


def graph_tune_extras(a):
    """Built ids that only tools/graph_tune.py tries (against the whole graph's replay time): 29, for plain 16-bit layers wider than the 256x32 tile."""
    L = _Layer(a)
    return [29] if (L.same16 and L.plain and a.Cout > 32) else []


def autotune_conv(launch, stream_ptr, reps=3, context=()):
    """Time every (tile, pipeline) configuration of one recorded conv launch on the device and keep the fastest.
    All configurations walk K in the same order, so the result is bit-identical whichever is picked.
    context: the launches that precede this one in its plan — replayed (untimed) before every timed launch so that L2 /
    MALL hold what they hold in the real forward (the layer's input freshly written by its producers, not the layer's
    own previous run); timing a layer against itself back to back ranks the candidates wrongly at the margin."""
    a = launch.keep[0]
    sig = _conv_signature(a)
    cands = conv_candidates(a)
    keep = None
    if sig in _TUNE_CACHE:
        # A cached id is only as good as the state it was tuned under: the signature does not encode whether the fragment-major
        # weights exist (ICAF_WREG_GEMM / ICAF_CWIDE), which A/B switches are set, or the device's CU count (the persistent
        # streaming GEMM needs its channel tiles to divide an XCD's workgroups).  The entry is applied only if it is still a candidate
        # for THIS launch and the library's own check for that configuration accepts it; otherwise it is dropped and the launch re-tuned.
        if tile_valid(launch, _TUNE_CACHE[sig], cands):
            cached = _TUNE_CACHE[sig]
            fresh = [c for c in cands if (c in OPT.retune_tiles or (OPT.retune_pre and a.pre)) and c != cached]
            if not fresh or sig in _RETUNED:
                a.tile = cached
                return a.tile
            # ICAF_RETUNE_TILES: configurations added after the cache was written get their chance against the cached choice (and only
            # against it), and must beat it by 3 % — the per-launch timing mis-ranks by a few per cent from run to run
            _RETUNED.add(sig)
            keep, cands = cached, [cached] + fresh
        else:
            del _TUNE_CACHE[sig]
    best, best_ms = 0, float("inf")
    e0, e1 = Event(), Event()
    for c in cands:
        a.tile = c
        st = launch.fn(*launch.args, stream_ptr)
        if st != 0:
            continue
        if context:
            ms = 0.0
            for _ in range(reps):
                for l in context:
                    l(stream_ptr)
                e0.record(stream_ptr)
                launch.fn(*launch.args, stream_ptr)
                e1.record(stream_ptr)
                ms += e0.elapsed_ms(e1)
        else:
            e0.record(stream_ptr)
            for _ in range(reps):
                launch.fn(*launch.args, stream_ptr)
            e1.record(stream_ptr)
            ms = e0.elapsed_ms(e1)
        if keep is not None and c != keep:
            ms *= 1.03                          # a newcomer must win clearly
        if ms < best_ms:
            best, best_ms = c, ms
    a.tile = best
    _TUNE_CACHE[sig] = best
    return best


def config_valid(launch, tile):
    """The library's verdict alone: does launch configuration `tile` run this recorded conv launch?  icaf_conv2d_kernel_name resolves a
    launch exactly as icaf_conv2d does (same table row, same check) and launches nothing."""
    a = launch.keep[0]
    saved, a.tile = a.tile, tile
    try:
        return lib().icaf_conv2d_kernel_name(launch.args[0], C.create_string_buffer(256), 256) == 0
    finally:
        a.tile = saved


def tile_valid(launch, tile, cands=None):
    """Is launch configuration `tile` usable for this recorded conv launch — a candidate for its arguments AND accepted by the library?"""
    return tile in (conv_candidates(launch.keep[0]) if cands is None else cands) and config_valid(launch, tile)


def save_tune_cache(path):
    import json
    with open(path, "w") as f:
        json.dump([[list(k), v] for k, v in _TUNE_CACHE.items()], f)


def load_tune_cache(path):
    import json
    with open(path) as f:
        for k, v in json.load(f):
            _TUNE_CACHE[tuple(k)] = v


def conv_kernel_name(launch):
    buf = C.create_string_buffer(256)
    check(lib().icaf_conv2d_kernel_name(launch.args[0], buf, 256), "icaf_conv2d_kernel_name")
    return buf.value.decode()


def preprocess(img, out, mode, name="preprocess"):
    """img: (B, C, H, W) fp32 NCHW contiguous; out: act (B, H', W', Cpad)."""
    assert img.dtype == torch.float32 and img.is_contiguous()
    if img.dim() == 5:                # both streams' images stacked (2, B, C, H, W): one launch over 2B images
        img, out = img.view(-1, *img.shape[2:]), flat_pair(out)
    B, Cc, H, W = img.shape
    Bo, Ho, Wo, cpad, ldo = _act_geom(out)
    assert ldo == cpad and Bo == B
    assert (Ho, Wo) == ((H // 2, W // 2) if mode == 1 else (H, W))
    nb = img.numel() * 4 + out.numel() * out.element_size()
    return Launch(lib().icaf_preprocess_nchw, (img.data_ptr(), out.data_ptr(), dtype_code(out.dtype), B, Cc, H, W,
                                               cpad, mode), keep=(img, out), name=name, nbytes=nb)


def preprocess_u8(img, out, mode, c0=0, name="preprocess_u8"):
    """img: (B, Ctot, H, W) uint8 NCHW contiguous (the dataloader's RGB+IR batch); out: act (B, H', W', Cpad) fed from
    channels [c0, c0+3), or a pair act (2, B, H', W', Cpad) fed from [c0, c0+3) and [c0+3, c0+6)."""
    assert img.dtype == torch.uint8 and img.is_contiguous() and img.dim() == 4
    nstreams = 2 if out.dim() == 5 else 1
    B, Ctot, H, W = img.shape
    o = flat_pair(out)
    Bo, Ho, Wo, cpad, ldo = _act_geom(o)
    assert ldo == cpad and Bo == nstreams * B and c0 + 3 * nstreams <= Ctot
    assert (Ho, Wo) == ((H // 2, W // 2) if mode == 1 else (H, W))
    nb = nstreams * B * 3 * H * W + o.numel() * o.element_size()
    return Launch(lib().icaf_preprocess_u8, (img.data_ptr(), o.data_ptr(), dtype_code(o.dtype), B, Ctot, c0, 3, nstreams,
                                             H, W, cpad, mode), keep=(img, out), name=name, nbytes=nb)


def _image_arg(img, paired):
    """(u8, ctot, B, H, W) of the network image an image-fed kernel reads: fp32 (B, 3, H, W) / (2, B, 3, H, W) [both streams], or the dataloader's
    uint8 (B, ctot, H, W) batch, whose channels hold the streams side by side."""
    u8 = img.dtype == torch.uint8
    assert img.is_contiguous() and (u8 or img.dtype == torch.float32)
    if u8:
        assert img.dim() == 4
        B, ctot, H, W = img.shape
    else:
        assert img.dim() == (5 if paired else 4)
        B, _, H, W = img.shape[-4:]
        ctot = 3
    return u8, ctot, B, H, W


def stem(img, w_packed, kp, bias, y, cout, name="stem"):
    """Staging + 6x6/s2/p2 stem conv in one persistent kernel (icaf_stem).  img: fp32 (B, 3, H, W) / (2, B, 3, H, W)
    [both streams], or uint8 (B, 6, H, W) [both streams]; y: act or pair act of cout channels at half resolution."""
    paired = y.dim() == 5
    u8, ctot, B, H, W = _image_arg(img, paired)
    assert not u8 or (paired and ctot >= 6)
    By, Ho, Wo, cy, ldy = _act_geom(y)
    assert (By, Ho, Wo) == (B, H // 2, W // 2) and cy >= cout and w_packed.dtype == y.dtype
    g = 2 if paired else 1
    nb = g * B * 3 * H * W * (1 if u8 else 4) + g * B * Ho * Wo * cout * y.element_size()
    flops = 2.0 * g * B * Ho * Wo * cout * 144
    return Launch(lib().icaf_stem, (img.data_ptr(), int(u8), ctot, w_packed.data_ptr(), bias.data_ptr(), y.data_ptr(), ldy,
                                    dtype_code(y.dtype), g, B, H, W, cout, kp,
                                    w_packed.stride(0) if paired else 0, bias.stride(0) if paired else 0,
                                    y.stride(0) if paired else 0),
                  keep=(img, w_packed, bias, y), name=name, flops=flops, nbytes=nb)


def stem2(img, w0, kp0, b0, w1, kp1, b1, w2, kp2, b2, y, c0, c1, c2, name="stem+conv3x3s2+1x1"):
    """Stem, the 3x3/s2 conv behind it and a chained 1x1 in one persistent kernel (icaf_stem2): img as `stem`; w0 / w1 /
    w2: the packed weights of the three layers (stacked per stream for a pair act y); y: (B, H/4, W/4, >= c2) act."""
    paired = y.dim() == 5
    u8, ctot, B, H, W = _image_arg(img, paired)
    assert not u8 or (paired and ctot >= 6)
    By, Ho, Wo, cy, ldy = _act_geom(y)
    assert (By, Ho, Wo) == (B, (H // 2 - 1) // 2 + 1, (W // 2 - 1) // 2 + 1) and cy >= c2
    assert w0.dtype == w1.dtype == w2.dtype == y.dtype
    a = Stem2Args()
    a.img, a.img_u8, a.ctot = img.data_ptr(), int(u8), ctot
    a.dtype, a.nstreams, a.B, a.H, a.W = dtype_code(y.dtype), 2 if paired else 1, B, H, W
    for k, (w, b, kp, c) in enumerate(((w0, b0, kp0, c0), (w1, b1, kp1, c1), (w2, b2, kp2, c2))):
        setattr(a, f"w{k}", w.data_ptr()); setattr(a, f"bias{k}", b.data_ptr())
        setattr(a, f"w{k}_gs", w.stride(0) if paired else 0); setattr(a, f"bias{k}_gs", b.stride(0) if paired else 0)
        setattr(a, f"Kp{k}", kp); setattr(a, f"C{k}", c)
    a.y, a.y_gs, a.ldy = y.data_ptr(), y.stride(0) if paired else 0, ldy
    g = a.nstreams
    hs, ws = H // 2, W // 2
    flops = 2.0 * g * B * (hs * ws * c0 * 144 + Ho * Wo * (c1 * 9 * c0 + c2 * c1))
    nb = g * B * (3 * H * W * (1 if u8 else 4) + Ho * Wo * c2 * y.element_size())
    return Launch(lib().icaf_stem2, (C.byref(a),), keep=(a, img, w0, b0, w1, b1, w2, b2, y), name=name, flops=flops, nbytes=nb)


def vgg_stem_weight(w4d, dt):
    """[64][3][3][3] fp32 -> [64][32] in dtype dt: K = 27 in the order (ky, kx, c), zero-padded to 32 (icaf_vgg_stem)."""
    co, ci, kh, kw = w4d.shape
    assert (co, ci, kh, kw) == (64, 3, 3, 3)
    out = torch.zeros((co, 32), dtype=dt, device=w4d.device)
    out[:, :27] = w4d.permute(0, 2, 3, 1).reshape(co, 27).to(dt)
    return out


def vgg_stem(img, w, bias, y, c0=0, name="vgg_stem"):
    """Image-fed 3x3 / s1 / p1 conv 3 -> 64 + bias + ReLU in one launch (icaf_vgg_stem).  img: fp32 (B, 3, H, W) / (2, B, 3, H, W) [both
    streams], or uint8 (B, Ctot, H, W) read from channel c0 on (both streams: [c0, c0 + 6)); w: vgg_stem_weight packs ([64][32], stacked per
    stream for a pair act y), bias fp32 [64] / [2][64]; y: act or pair act of 64 channels at the image's resolution."""
    paired = y.dim() == 5
    g = 2 if paired else 1
    u8, ctot, B, H, W = _image_arg(img, paired)
    assert c0 + 3 * g <= ctot if u8 else (img.shape[-3] == 3 and c0 == 0)
    By, Ho, Wo, cy, ldy = _act_geom(y)
    assert (By, Ho, Wo) == (B, H, W) and cy >= 64 and w.dtype == y.dtype and w.shape[-2:] == (64, 32) and w.dim() == (3 if paired else 2)
    assert bias.dtype == torch.float32 and bias.shape[-1] >= 64 and w.is_contiguous() and bias.stride(-1) == 1
    nb = g * B * 3 * H * W * (1 if u8 else 4) + g * B * H * W * 64 * y.element_size()
    flops = 2.0 * g * B * H * W * 64 * 27
    return Launch(lib().icaf_vgg_stem, (img.data_ptr() + c0 * H * W, int(u8), ctot, w.data_ptr(), bias.data_ptr(), y.data_ptr(), ldy,
                                        dtype_code(y.dtype), g, B, H, W, 64, 32,
                                        w.stride(0) if paired else 0, bias.stride(0) if paired else 0, y.stride(0) if paired else 0),
                  keep=(img, w, bias, y), name=name, flops=flops, nbytes=nb)


def maxpool2d(x, y, k=2, s=2, p=0, name="maxpool2d"):
    """nn.MaxPool2d(k, s, p) over an act or a pair act (2B images): (k, s, p) = (2, 2, 0) or (3, 2, 1), floor output size."""
    x, y = flat_pair(x), flat_pair(y)
    B, H, W, Cc, ldx = _act_geom(x)
    By, Ho, Wo, Cy, ldy = _act_geom(y)
    assert (By, Cy) == (B, Cc) and (Ho, Wo) == ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1) and y.dtype == x.dtype
    nb = (B * H * W + B * Ho * Wo) * Cc * x.element_size()
    return Launch(lib().icaf_maxpool2d, (x.data_ptr(), ldx, y.data_ptr(), ldy, dtype_code(x.dtype), B, H, W, Cc, k, s, p),
                  keep=(x, y), name=name, nbytes=nb)


def sppf_pool(x, y1, y2, y3, k, name="sppf_pool"):
    x, y1, y2, y3 = flat_pair(x), flat_pair(y1), flat_pair(y2), flat_pair(y3)
    B, H, W, Cc, ldx = _act_geom(x)
    ldy = _act_geom(y1)[4]
    assert _act_geom(y2)[4] == ldy and _act_geom(y3)[4] == ldy
    nb = 4 * x.numel() * x.element_size()
    return Launch(lib().icaf_sppf_pool, (x.data_ptr(), ldx, y1.data_ptr(), y2.data_ptr(), y3.data_ptr(), ldy,
                                         dtype_code(x.dtype), B, H, W, Cc, k), keep=(x, y1, y2, y3), name=name,
                  nbytes=nb)


def sppf_config(dtype, H, W, Cc):
    """Channel vectors per workgroup icaf_sppf_pool picks for this geometry (0 = the global-memory kernel), the probe knob included."""
    v = C.c_int(-1)
    check(lib().icaf_sppf_config(dtype_code(dtype), H, W, Cc, C.byref(v)), "icaf_sppf_config")
    return v.value


def upsample_nearest(x, y, scale, name="upsample_nearest"):
    B, H, W, Cc, ldx = _act_geom(x)
    By, Hy, Wy, Cy, ldy = _act_geom(y)
    assert (Hy, Wy, Cy) == (H * scale, W * scale, Cc)
    nb = (x.numel() + y.numel()) * x.element_size()
    return Launch(lib().icaf_upsample_nearest, (x.data_ptr(), ldx, y.data_ptr(), ldy, dtype_code(x.dtype), B, H, W,
                                                Cc, scale), keep=(x, y), name=name, nbytes=nb)


def copy_channels(x, y, name="copy_channels"):
    B, H, W, Cc, ldx = _act_geom(x)
    ldy = _act_geom(y)[4]
    assert y.shape == x.shape
    nb = 2 * x.numel() * x.element_size()
    return Launch(lib().icaf_copy_channels, (x.data_ptr(), ldx, y.data_ptr(), ldy, dtype_code(x.dtype),
                                             B * H * W, Cc), keep=(x, y), name=name, nbytes=nb)


def axpby(x0, x1, y, a, b, name="add_fusion"):
    """y = a*x0 + b*x1 over acts of equal shape."""
    B, H, W, Cc, ld0 = _act_geom(x0)
    ld1, ldy = _act_geom(x1)[4], _act_geom(y)[4]
    assert x1.shape == x0.shape and y.shape == x0.shape
    nb = 3 * x0.numel() * x0.element_size()
    return Launch(lib().icaf_axpby, (x0.data_ptr(), ld0, x1.data_ptr(), ld1, y.data_ptr(), ldy, dtype_code(x0.dtype),
                                     B * H * W, Cc, float(a), float(b)), keep=(x0, x1, y), name=name, nbytes=nb)


def dmff_pool_tokens(fea_rgb, fea_ir, pos_rgb, pos_ir, tokens, th, tw, kh, kw, sh, sw, w_rgb, w_ir,
                     name="dmff_pool_tokens"):
    B, H, W, Cc, ld0 = _act_geom(fea_rgb)
    ld1 = _act_geom(fea_ir)[4]
    assert tokens.shape == (2, B * th * tw, Cc) and tokens.is_contiguous()
    assert pos_rgb.dtype == torch.float32 and pos_rgb.numel() == th * tw * Cc
    nb = 2 * fea_rgb.numel() * fea_rgb.element_size() + tokens.numel() * tokens.element_size()
    return Launch(lib().icaf_dmff_pool_tokens,
                  (fea_rgb.data_ptr(), ld0, fea_ir.data_ptr(), ld1, pos_rgb.data_ptr(), pos_ir.data_ptr(),
                   tokens.data_ptr(), dtype_code(tokens.dtype), B, H, W, Cc, th, tw, kh, kw, sh, sw,
                   float(w_rgb[0]), float(w_rgb[1]), float(w_ir[0]), float(w_ir[1])),
                  keep=(fea_rgb, fea_ir, pos_rgb, pos_ir, tokens), name=name, nbytes=nb)


def dmff_pool_config(dtype, B, H, W, Cc, th, tw, kh, kw, sh, sw):
    """dict(kernel 0 = element / 1 = rows, R rows in flight, TR token rows per workgroup, index64) icaf_dmff_pool_tokens picks for this geometry,
    the probe knob index64 included."""
    v = [C.c_int(-1) for _ in range(4)]
    check(lib().icaf_dmff_pool_config(dtype_code(dtype), B, H, W, Cc, th, tw, kh, kw, sh, sw, *(C.byref(x) for x in v)), "icaf_dmff_pool_config")
    return dict(zip(("kernel", "R", "TR", "index64"), (x.value for x in v)))


def layernorm(x, y, g0, b0, g1, b1, eps=1e-5, name="layernorm"):
    """x, y: (G, rows, C) contiguous; group g normalised with (g_g, b_g) fp32 vectors."""
    G, rows, Cc = x.shape
    assert x.is_contiguous() and y.is_contiguous() and y.shape == x.shape
    nb = 2 * x.numel() * x.element_size()
    return Launch(lib().icaf_layernorm, (x.data_ptr(), y.data_ptr(), g0.data_ptr(), b0.data_ptr(), g1.data_ptr(),
                                         b1.data_ptr(), dtype_code(x.dtype), rows, Cc, G, float(eps)),
                  keep=(x, y, g0, b0, g1, b1), name=name, nbytes=nb)


def cross_attention(qkv, out, B, N, heads, name="cross_attention"):
    """qkv: (2, B*N, 3C); out: (2, B*N, C)."""
    G, rows, c3 = qkv.shape
    Cc = c3 // 3
    assert G == 2 and rows == B * N and out.shape == (2, rows, Cc) and qkv.is_contiguous() and out.is_contiguous()
    flops = 2 * B * heads * 4.0 * N * N * (Cc // heads)
    nb = (qkv.numel() + out.numel()) * qkv.element_size()
    return Launch(lib().icaf_cross_attention, (qkv.data_ptr(), out.data_ptr(), dtype_code(qkv.dtype), B, N, Cc,
                                               heads), keep=(qkv, out), name=name, flops=flops, nbytes=nb)


def cross_attention_config(dtype, B, N, Cc, heads):
    """(padded head dimension, query splits per head, XCD remap 0 / 1) icaf_cross_attention picks for this shape, the probe knob included."""
    dkp, qs, rm = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    check(lib().icaf_cross_attention_config(dtype_code(dtype), B, N, Cc, heads, C.byref(dkp), C.byref(qs), C.byref(rm)),
          "icaf_cross_attention_config")
    return dkp.value, qs.value, rm.value


def cross_attention_form(dtype, B, N, Cc, heads):
    """0: icaf_cross_attention runs the resident kernel for this shape, 1: the key-streaming one (icaf.h), the probe knob included."""
    form = C.c_int(-1)
    check(lib().icaf_cross_attention_form(dtype_code(dtype), B, N, Cc, heads, C.byref(form)), "icaf_cross_attention_form")
    return form.value


@contextlib.contextmanager
def _caller_knob(name, on):
    """A library knob that a caller sets, not the options object (icaf.h: icaf_set_option): `on` inside the `with`, back to 0 behind it."""
    check(lib().icaf_set_option(name.encode(), int(bool(on))), f"icaf_set_option({name})")
    try:
        yield
    finally:
        check(lib().icaf_set_option(name.encode(), 0), f"icaf_set_option({name})")


def attn_stream(on=True):
    """Force icaf_cross_attention onto its key-streaming form inside a `with` (icaf.h: icaf_cross_attention_form): an A/B knob of the
    library for timings and tests.  Like letterbox_direct it is set by a caller, not by the options object."""
    return _caller_knob("attn_stream", on)


def dmff_block_forms(dt, C_, N, heads, hidden, ksplit=1, stream32=False):
    """(two-launch form built, three-launch form built at this ksplit with / without the fp32 token stream) for one block shape: the verdict of
    the library's own resolve and table lookup (icaf.h: icaf_dmff_block_forms — host code, asked on every device)."""
    if dt not in (torch.bfloat16, torch.float16, torch.float32):
        return False, False
    two, three = C.c_int(0), C.c_int(0)
    check(lib().icaf_dmff_block_forms(dtype_code(dt), int(C_), int(N), int(heads), int(hidden), int(ksplit), int(bool(stream32)),
                                      C.byref(two), C.byref(three)), "dmff_block_forms")
    return bool(two.value), bool(three.value)


def _dmff_args(x, qkv, y, packs, ln, coef, eps, B, N, heads):
    """icaf_dmff_args for one block iteration.  x: (2, B*N, C) contiguous tokens; qkv: (2, B*N, 3C); y: (2, B*N, C) view with
    any group / row stride; packs = dict(qkv=, out=, fc1=, fc2=) of (weights [2][Np][Kp], Kp, bias [2][Np]) stacks."""
    G, rows, Cc = x.shape
    assert G == 2 and rows == B * N and x.is_contiguous() and (qkv is None or (qkv.shape == (2, rows, 3 * Cc) and qkv.is_contiguous()))
    a = DmffArgs()
    a.x, a.qkv = x.data_ptr(), (qkv.data_ptr() if qkv is not None else None)
    a.x_gs = x.stride(0)
    if y is not None:
        assert y.shape == (2, rows, Cc) and y.stride(2) == 1 and y.dtype == x.dtype
        a.y, a.y_gs, a.ldy = y.data_ptr(), y.stride(0), y.stride(1)
    for name, key in (("wqkv", "qkv"), ("wo", "out"), ("w1", "fc1"), ("w2", "fc2")):
        w, kp, b = packs[key]
        assert w.dtype == x.dtype and w.dim() in (3, 5) and b.dim() == 2          # ([2][Np][Kp], or its fragment-major copy)
        setattr(a, name, w.data_ptr()); setattr(a, "b" + name[1:], b.data_ptr())
        setattr(a, name + "_gs", w.stride(0)); setattr(a, "b" + name[1:] + "_gs", b.stride(0))
    a.Kp, a.Kp4 = packs["qkv"][1], packs["fc2"][1]
    assert packs["out"][1] == a.Kp and packs["fc1"][1] == a.Kp
    a.hidden = coef["hidden"]
    a.ln_attn_gamma[0], a.ln_attn_gamma[1] = ln["a1w"].data_ptr(), ln["a2w"].data_ptr()
    a.ln_attn_beta[0], a.ln_attn_beta[1] = ln["a1b"].data_ptr(), ln["a2b"].data_ptr()
    a.ln_mlp_gamma, a.ln_mlp_beta = ln["mw"].data_ptr(), ln["mb"].data_ptr()
    a.dtype, a.B, a.N, a.C, a.heads = dtype_code(x.dtype), B, N, Cc, heads
    a.eps_attn, a.eps_mlp = float(eps[0]), float(eps[2])
    co = coef["co"]
    a.coef_res_attn[0], a.coef_res_attn[1] = co[0], co[2]
    a.coef_acc_attn[0], a.coef_acc_attn[1] = co[1], co[3]
    a.coef_res_mlp[0], a.coef_res_mlp[1] = co[4], co[6]
    a.coef_acc_mlp[0], a.coef_acc_mlp[1] = co[5], co[7]
    return a


def _wide_packs(packs):
    """packs with fragment-major weight copies (frag_weights: cached per packed tensor) — what the dmff_wide kernels read"""
    return {k: ((frag_weights(v[0]), v[1], v[2]) if k in ("qkv", "out", "fc1", "fc2") else v) for k, v in packs.items()}


def dmff_launches(mlp, wide, x, qkv, att, y, packs, ln, coef, eps, B, N, heads, name, partial=None, ksplit=1, x32=None, y32=None):
    """The launches of one half of a block iteration, as a list — mlp False: LayerNorm + the six Linear(C, C) projections; True: out-projection +
    LayerNorm + MLP (two-launch form: with the crossed attention in front, in the same launch).  wide: the three-launch kernels, which read
    fragment-major weights; ksplit > 1 splits the hidden columns over ksplit workgroups per tile (partial: fp32 (ksplit, 2, rows, C) scratch)
    and a second small launch reduces the partial sums.  x32 / y32: the fp32 token stream across iterations (icaf.h: icaf_dmff_args)."""
    L = lib()
    rows, Cc = x.shape[1], x.shape[2]
    es, hid = x.element_size(), coef["hidden"]
    wp = _wide_packs(packs) if wide else packs
    a = _dmff_args(x, qkv, y, wp, ln, coef, eps, B, N, heads)
    keep = (a, x, qkv, att, y, wp, packs, ln, partial, x32, y32)
    if not mlp:
        if wide:
            a.reserved = OPT.dmff_qkv_npass                  # output-channel passes per workgroup: 0 = automatic (icaf.h)
        return [Launch(L.icaf_dmff_wide_ln_qkv if wide else L.icaf_dmff_ln_qkv, (C.byref(a),), keep=keep, name=name, flops=2.0 * 2 * rows * Cc * 3 * Cc,
                       nbytes=2 * (rows * Cc * es + 3 * Cc * Cc * es + rows * 3 * Cc * es))]
    flops = 2.0 * 2 * rows * (Cc * Cc + 2 * Cc * hid)
    wbytes = (Cc * Cc + 2 * Cc * hid) * es
    if not wide:
        return [Launch(L.icaf_dmff_attn_mlp, (C.byref(a),), keep=keep, name=name, flops=2.0 * (B * heads * 4.0 * N * N * (Cc // heads)) + flops,
                       nbytes=2 * (rows * 3 * Cc * es + 2 * rows * Cc * es + wbytes))]
    assert att.shape == (2, rows, Cc) and att.is_contiguous() and att.dtype == x.dtype
    nbytes = 2 * (3 * rows * Cc * es + wbytes)
    for t in (x32, y32):
        assert t is None or (y32 is not None and t.dtype == torch.float32 and t.shape == (2, rows, Cc) and t.is_contiguous())
    if y32 is not None:
        a.y32 = y32.data_ptr()
        a.x32 = x32.data_ptr() if x32 is not None else None
        nbytes += (2 if x32 is not None else 1) * 2 * rows * Cc * 4
    if ksplit == 1:
        return [Launch(L.icaf_dmff_wide_proj_mlp, (C.byref(a), att.data_ptr()), keep=keep, name=name, flops=flops, nbytes=nbytes)]
    assert partial is not None and partial.dtype == torch.float32 and partial.is_contiguous() and partial.shape == (ksplit, 2, rows, Cc)
    return [Launch(L.icaf_dmff_wide_proj_mlp_split, (C.byref(a), att.data_ptr(), partial.data_ptr(), int(ksplit)), keep=keep, name=name,
                   flops=flops + 2.0 * 2 * rows * Cc * Cc * (ksplit - 1),                         # the repeated out-projection
                   nbytes=nbytes + partial.numel() * 4),
            Launch(L.icaf_dmff_wide_reduce, (C.byref(a), partial.data_ptr(), int(ksplit)), keep=keep, name=name + "_reduce",
                   nbytes=partial.numel() * 4 + 2 * 2 * rows * Cc * es)]


def dmff_ln_qkv(x, qkv, packs, ln, coef, eps, B, N, heads, name="dmff_ln_qkv"):
    """LayerNorm + the six Linear(C, C) projections of CrossAttention as one launch (icaf_dmff_ln_qkv)."""
    return dmff_launches(False, False, x, qkv, None, None, packs, ln, coef, eps, B, N, heads, name)[0]


def dmff_attn_mlp(x, qkv, y, packs, ln, coef, eps, B, N, heads, name="dmff_attn_mlp"):
    """Crossed attention + out-projection + LayerNorm + MLP of one block iteration as one launch (icaf_dmff_attn_mlp)."""
    return dmff_launches(True, False, x, qkv, None, y, packs, ln, coef, eps, B, N, heads, name)[0]


def dmff_wide_ln_qkv(x, qkv, packs, ln, coef, eps, B, N, heads, name="dmff_ln_qkv"):
    """LayerNorm + the six Linear(C, C) projections, three-launch form (icaf_dmff_wide_ln_qkv)."""
    return dmff_launches(False, True, x, qkv, None, None, packs, ln, coef, eps, B, N, heads, name)[0]


def dmff_wide_proj_mlp(x, att, y, packs, ln, coef, eps, B, N, heads, name="dmff_proj_mlp", partial=None, ksplit=1, x32=None, y32=None):
    """Out-projection + LayerNorm + MLP of one block iteration behind cross_attention: one launch (icaf_dmff_wide_proj_mlp), or with ksplit > 1
    the LIST [icaf_dmff_wide_proj_mlp_split, icaf_dmff_wide_reduce] — the shape the kernel tests call it by; plans take dmff_launches' list."""
    ls = dmff_launches(True, True, x, None, att, y, packs, ln, coef, eps, B, N, heads, name, partial, ksplit, x32, y32)
    return ls if ksplit > 1 else ls[0]


def dmff_wide_ksplit(N, C_):
    """The hidden-column split PREFERRED for a level (what is built is the library's business: CrossTransformerBlock.block_form asks it): 2 where
    a modality's weights (9 C^2 16-bit elements) overflow an XCD's 4 MB L2 AND the level has few tokens per image (N <= 128: P5 of yolov5s — 100
    tokens, i.e. 100 tiles of 64 rows for 256 CUs at batch 32, 4.7 MB of weights per modality), else 1.  Deliberately a function of the LEVEL
    (N, C), never of the batch size: the split changes the fp32 association of the fc2 sum, and a shard of a batch must reproduce the same rows
    of the full batch bit for bit (tests/test_gpu_fullsize.py; yolov5l's P4 — C = 512, N = 256, one tile per CU at batch 32 — measured slower
    with the split anyway).  ICAF_OPTIONS=dmff_ksplit=n forces n."""
    return OPT.dmff_ksplit or (2 if (9 * C_ * C_ * 2 > 3 * 2 ** 20 and N <= 128) else 1)


def dmff_upsample_merge(tokens, fea_rgb, fea_ir, out, th, tw, name="dmff_upsample_merge"):
    B, H, W, Cc, ld0 = _act_geom(fea_rgb)
    ld1 = _act_geom(fea_ir)[4]
    Bo, Ho, Wo, Co, ldo = _act_geom(out)
    assert (Bo, Ho, Wo, Co) == (B, H, W, 2 * Cc) and tokens.shape == (2, B * th * tw, Cc)
    nb = (2 * fea_rgb.numel() + out.numel()) * out.element_size()
    return Launch(lib().icaf_dmff_upsample_merge,
                  (tokens.data_ptr(), fea_rgb.data_ptr(), ld0, fea_ir.data_ptr(), ld1, out.data_ptr(), ldo,
                   dtype_code(out.dtype), B, H, W, Cc, th, tw), keep=(tokens, fea_rgb, fea_ir, out), name=name,
                  nbytes=nb)


def detect_decode(p, z, logits, raw, na, no, row_offset, stride, anchors_px, name="detect_decode"):
    """p: fp32 act (B, ny, nx, >=na*no); z: (B, rows_total, no); raw: (B, na, ny, nx, no)."""
    B, ny, nx, cp, ldp = _act_geom(p)
    assert p.dtype == torch.float32 and z.dtype == torch.float32 and z.is_contiguous()
    arr = (C.c_float * (2 * na))(*[float(v) for v in anchors_px])
    nb = p.numel() * 4 + 3 * B * na * ny * nx * no * 4
    return Launch(lib().icaf_detect_decode,
                  (p.data_ptr(), ldp, z.data_ptr(), logits.data_ptr() if logits is not None else None,
                   raw.data_ptr() if raw is not None else None, B, ny, nx, na, no, z.shape[1], row_offset,
                   float(stride), arr), keep=(p, z, logits, raw, arr), name=name, nbytes=nb)


def detect_decode_kernel(p, z, raw, na, no):
    """Kernel icaf_detect_decode launches for these tensors: 0 = one thread per pixel, 1 = one thread per element (alignment counts)."""
    B, ny, nx, cp, ldp = _act_geom(p)
    k = C.c_int(-1)
    check(lib().icaf_detect_decode_kernel(p.data_ptr(), ldp, z.data_ptr(), raw.data_ptr() if raw is not None else None, B, ny, nx, na, no,
                                          C.byref(k)), "icaf_detect_decode_kernel")
    return k.value


def detect_conv_ok(x, na, no, cin):
    """Can icaf_detect_conv (Detect level in one launch) take this level?  16-bit maps, 3 anchors, no in {6, 8, 14}, Cin * 2 % 128 == 0."""
    return x.dtype in (torch.bfloat16, torch.float16) and na == 3 and no in (6, 8, 14) and (cin * 2) % 128 == 0 and x.dim() == 4


def detect_conv(x, w_packed, kp, bias, z, logits, raw, na, no, row_offset, stride, anchors_px, cin, name="detect_conv+decode"):
    """One Detect level in ONE launch (icaf_detect_conv): x (B, ny, nx, >= cin) 16-bit act -> z (B, rows_total, no), logits, raw; the
    1x1 output conv (packed weights / bias as for conv2d) runs as the persistent streaming GEMM with the decode as its epilogue."""
    B, ny, nx, cx, ldx = _act_geom(x)
    assert cx >= cin and z.dtype == torch.float32 and z.is_contiguous() and w_packed.dtype == x.dtype
    a = ConvArgs()
    a.x, a.w, a.bias = x.data_ptr(), w_packed.data_ptr(), bias.data_ptr() if bias is not None else None
    a.y = z.data_ptr()                                   # (never written: icaf_conv_args wants a non-null y)
    a.groups = 1
    a.B, a.H, a.W, a.Cin, a.ldx = B, ny, nx, cin, ldx
    a.Ho, a.Wo, a.Cout, a.ldy = ny, nx, na * no, na * no
    a.kh = a.kw = a.sh = a.sw = 1
    a.Kp, a.act = kp, ACT_NONE
    a.dtype, a.out_dtype = dtype_code(x.dtype), F32
    a.alpha_acc[0] = a.alpha_acc[1] = 1.0
    arr = (C.c_float * (2 * na))(*[float(v) for v in anchors_px])
    m = B * ny * nx
    nb = m * cin * x.element_size() + 3 * m * na * no * 4
    return Launch(lib().icaf_detect_conv,
                  (C.byref(a), z.data_ptr(), logits.data_ptr() if logits is not None else None, raw.data_ptr() if raw is not None else None,
                   na, no, z.shape[1], row_offset, float(stride), arr), keep=(a, x, w_packed, bias, z, logits, raw, arr), name=name,
                  flops=2.0 * m * na * no * cin, nbytes=nb)


def tta_stage(src, passes, name="tta_stage"):
    """scale_img of both modalities for every scaled pass of test-time augmentation in one launch (icaf_tta_stage).  src: the
    full-size fp32 (2, B, 3, H, W) staging pair or the uint8 (B, 6, H, W) batch; passes: [(dst, Hr, Wr, flip)] with dst the fp32
    (2, B, 3, Hp, Wp) staging pair of the pass's plan."""
    u8 = src.dtype == torch.uint8
    assert src.is_contiguous() and (src.dim() == 4 and src.shape[1] >= 6 if u8 else src.dtype == torch.float32 and src.dim() == 5 and src.shape[0] == 2)
    B, _, H, W = src.shape[-4:]
    arr = (_lib.TtaPass * len(passes))()
    nb = 2 * B * 3 * H * W * (1 if u8 else 4)                  # algorithmic bytes: the source once, every output once
    for p, (dst, hr, wr, flip) in zip(arr, passes):
        assert dst.dtype == torch.float32 and dst.is_contiguous() and dst.dim() == 5 and dst.shape[:3] == (2, B, 3)
        p.dst, p.Hr, p.Wr, p.Hp, p.Wp, p.flip = dst.data_ptr(), hr, wr, dst.shape[3], dst.shape[4], int(bool(flip))
        nb += dst.numel() * 4
    return Launch(lib().icaf_tta_stage, (src.data_ptr(), int(u8), src.shape[1] if u8 else 3, B, H, W, arr, len(passes)),
                  keep=(src, arr, [p[0] for p in passes]), name=name, nbytes=nb)


def tta_merge(zs, scales, flips, out, width, name="tta_merge"):
    """De-scale, de-flip and concatenate the passes' decoded rows (icaf_tta_merge): zs[i] (B, N_i, no) fp32 -> out (B, sum N_i, no)."""
    B, _, no = out.shape
    n = len(zs)
    assert out.dtype == torch.float32 and out.is_contiguous() and sum(z.shape[1] for z in zs) == out.shape[1]
    assert all(z.dtype == torch.float32 and z.is_contiguous() and z.shape[0] == B and z.shape[2] == no for z in zs)
    ptrs = (C.c_void_p * n)(*[z.data_ptr() for z in zs])
    rows = (C.c_longlong * n)(*[z.shape[1] for z in zs])
    sc = (C.c_float * n)(*[float(s) for s in scales])
    fl = (C.c_int * n)(*[int(bool(f)) for f in flips])
    return Launch(lib().icaf_tta_merge, (ptrs, rows, sc, fl, n, out.data_ptr(), B, no, float(width)),
                  keep=(zs, out, ptrs, rows, sc, fl), name=name, nbytes=2 * out.numel() * 4)


class NmsRunner:
    """Pre-allocated NMS launch for a fixed (B, rows, nc) — graph-capturable; results stay on the device."""

    def __init__(self, B, rows, nc, device, multi_label=False, max_det=300, want_keep=True, block=None, max_labels=0, merge=False):
        """want_keep=False skips the kept-index output (torchvision's return value; one more small launch) — the serving
        pipeline only needs the detection rows.  `block`: a flat fp32 tensor of B * max_det * 6 + B elements to use as the detection block
        (the pipeline lays the blocks of consecutive steps side by side so that ONE collective moves all of them).
        max_labels: room for that many apriori label rows per image behind the prediction rows (launch(labels=...), icaf_nms_ex); merge: the
        reference's merge-NMS (utils/general.py:594-600) follows the walk.  With both at their defaults the runner calls icaf_nms as ever."""
        self.B, self.rows, self.nc, self.max_det = B, rows, nc, max_det
        self.multi_label = bool(multi_label) and nc > 1
        self.max_labels, self.merge = int(max_labels), bool(merge)
        if self.max_labels < 0:
            raise ValueError("NmsRunner: max_labels must not be negative")
        sz = C.c_size_t(0)
        if self.max_labels:
            a = _lib.NmsArgs()
            a.B, a.rows, a.nc, a.multi_label, a.max_labels = B, rows, nc, int(self.multi_label), self.max_labels
            check(lib().icaf_nms_ex_workspace_bytes(C.byref(a), C.byref(sz)), "nms_workspace")
        else:
            check(lib().icaf_nms_workspace_bytes(B, rows, nc, int(self.multi_label), C.byref(sz)), "nms_workspace")
        self.ws = torch.empty((max(sz.value, 16),), dtype=torch.uint8, device=device)
        from .dist import detection_block            # det + count in ONE allocation: the block the all-gather sends as it is
        if block is None:
            self.block, self.det, self.count = detection_block(B, max_det, device)
        else:
            n = B * max_det * 6
            assert block.dtype == torch.float32 and block.is_contiguous() and block.numel() == n + B and block.device == torch.device(device)
            self.block, self.det, self.count = block, block[:n].view(B, max_det, 6), block[n:].view(torch.int32)
        self.keep = torch.zeros((B, max_det), dtype=torch.int32, device=device) if want_keep else None

    def launch(self, pred, conf_thres, iou_thres, agnostic=False, classes=None, max_nms=30000, max_wh=4096.0,
               stream_ptr=None, labels=None, label_off=None, redundant=True):
        """labels (L, 5) fp32 [cls, cx, cy, w, h] in pixels and label_off (B + 1,) int32 on the device (nms_label_table builds and checks them):
        image b's apriori labels are rows label_off[b] .. label_off[b + 1], at most the runner's max_labels."""
        assert pred.dtype == torch.float32 and pred.is_contiguous() and pred.shape == (self.B, self.rows, 5 + self.nc)
        cls_arr, ncls = None, 0
        if classes is not None:
            ncls = len(classes)
            cls_arr = (C.c_int * max(ncls, 1))(*[int(c) for c in classes])
        stream = stream_ptr if stream_ptr is not None else current_stream_ptr()
        keep_ptr = self.keep.data_ptr() if self.keep is not None else None
        if labels is None and not self.merge:
            st = lib().icaf_nms(pred.data_ptr(), self.B, self.rows, self.nc, float(conf_thres), float(iou_thres),
                                int(self.multi_label), int(bool(agnostic)), cls_arr, ncls, self.max_det, int(max_nms),
                                float(max_wh), self.det.data_ptr(), self.count.data_ptr(), keep_ptr,
                                self.ws.data_ptr(), self.ws.numel(), stream)
            check(st, "icaf_nms")
            return self.det, self.count, self.keep
        if self.merge and int(max_nms) < _lib.NMS_MERGE_LIMIT:
            raise ValueError(f"merge-NMS needs max_nms >= {_lib.NMS_MERGE_LIMIT}: the reference would merge over a truncated candidate list")
        a = _lib.NmsArgs()
        a.pred, a.B, a.rows, a.nc = pred.data_ptr(), self.B, self.rows, self.nc
        a.conf_thres, a.iou_thres, a.multi_label, a.agnostic = float(conf_thres), float(iou_thres), int(self.multi_label), int(bool(agnostic))
        a.classes, a.n_classes = (C.addressof(cls_arr) if cls_arr is not None else None), ncls
        a.max_det, a.max_nms, a.max_wh = self.max_det, int(max_nms), float(max_wh)
        a.det, a.count, a.keep_idx = self.det.data_ptr(), self.count.data_ptr(), keep_ptr
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        a.merge, a.redundant = int(self.merge), int(bool(redundant))
        if labels is not None:
            if label_off is None:
                raise ValueError("NmsRunner.launch: labels need label_off")
            if not self.max_labels:
                raise ValueError("NmsRunner.launch: the runner was built with max_labels=0")
            assert labels.dtype == torch.float32 and labels.is_contiguous() and labels.dim() == 2 and labels.shape[1] == 5 and labels.device == pred.device
            assert label_off.dtype == torch.int32 and label_off.is_contiguous() and label_off.shape == (self.B + 1,) and label_off.device == pred.device
            if labels.shape[0]:                                     # an empty table: no label anywhere, the plain candidate stage
                a.labels, a.label_off, a.max_labels = labels.data_ptr(), label_off.data_ptr(), self.max_labels
        check(lib().icaf_nms_ex(C.byref(a), stream), "icaf_nms_ex")
        return self.det, self.count, self.keep


def nms_label_table(labels, B, nc, max_labels=None, device=None):
    """The per-image apriori label lists of non_max_suppression(labels=...) -> (table (L, 5) fp32, label_off (B + 1,) int32, longest list), built
    and CHECKED on the host from the small tensors: every class an id in [0, nc), at most max_labels rows per image (when given).  `labels`: a
    sequence of B (n_i, 5) tensors / arrays [cls, cx, cy, w, h] in pixels, empty entries allowed.  The tensors go to `device` when it is given."""
    if len(labels) != B:
        raise ValueError(f"apriori labels for {len(labels)} images, the batch holds {B}")
    rows, off = [], [0]
    for i, l in enumerate(labels):
        l = torch.as_tensor(l, dtype=torch.float32).detach().cpu().reshape(-1, 5) if len(l) else torch.zeros((0, 5))
        if len(l):
            c = l[:, 0]
            if not bool(((c >= 0) & (c < nc)).all()):
                raise ValueError(f"apriori labels of image {i}: class ids must be in [0, {nc})")
        if max_labels is not None and len(l) > max_labels:
            raise ValueError(f"apriori labels of image {i}: {len(l)} rows, max_labels is {max_labels}")
        rows.append(l)
        off.append(off[-1] + len(l))
    table, off_t = torch.cat(rows).contiguous(), torch.tensor(off, dtype=torch.int32)
    if device is not None:
        table, off_t = table.to(device), off_t.to(device)
    return table, off_t, max(b - a for a, b in zip(off, off[1:]))


def confluence_select(cand, n, nc, p_thres, det=None, count=None, keep_idx=None, want_keep=True, stream_ptr=None):
    """Confluence (reference utils/confluence.py:109-193) on candidate lists that already live on the device (icaf_confluence_select): cand
    (B, max_cand, 6) fp32 [x1, y1, x2, y2, conf, cls], n (B,) int32.  Returns (det (B, max_cand, 6), count (B,) int32, keep_idx (B, max_cand)
    int32 or None): the kept rows in ascending candidate index, zeros behind them.  conf > 2e-4 is the caller's to guarantee.  No host sync."""
    assert cand.is_cuda and cand.dtype == torch.float32 and cand.is_contiguous() and cand.dim() == 3 and cand.shape[2] == 6
    B, max_cand, _ = cand.shape
    assert n.dtype == torch.int32 and n.is_contiguous() and n.shape == (B,) and n.device == cand.device
    if det is None:
        det = torch.zeros((B, max_cand, 6), dtype=torch.float32, device=cand.device)
    if count is None:
        count = torch.zeros((B,), dtype=torch.int32, device=cand.device)
    if keep_idx is None and want_keep:
        keep_idx = torch.zeros((B, max_cand), dtype=torch.int32, device=cand.device)
    assert det.dtype == torch.float32 and det.is_contiguous() and det.shape == (B, max_cand, 6) and count.dtype == torch.int32 and count.shape == (B,)
    assert keep_idx is None or (keep_idx.dtype == torch.int32 and keep_idx.is_contiguous() and keep_idx.shape == (B, max_cand))
    st = lib().icaf_confluence_select(cand.data_ptr(), n.data_ptr(), B, max_cand, int(nc), float(p_thres), det.data_ptr(), count.data_ptr(),
                                      keep_idx.data_ptr() if keep_idx is not None else None,
                                      stream_ptr if stream_ptr is not None else current_stream_ptr())
    check(st, "icaf_confluence_select")
    return det, count, keep_idx


class ConfluenceRunner:
    """Pre-allocated confluence launch (icaf_confluence: candidate stage + select) for a fixed (B, rows, nc) — graph-capturable; results stay
    on the device.  Owns the det / count / keep block and the workspace.  count[b] < 0: image b had -count[b] > max_cand candidates and was
    refused (its rows are zero)."""

    def __init__(self, B, rows, nc, device, max_cand=CONFLUENCE_MAX_CAND, want_keep=True):
        self.B, self.rows, self.nc, self.max_cand = B, rows, nc, int(max_cand)
        sz = C.c_size_t(0)
        check(lib().icaf_confluence_workspace_bytes(B, rows, nc, self.max_cand, C.byref(sz)), "confluence_workspace")
        self.ws = torch.empty((max(sz.value, 16),), dtype=torch.uint8, device=device)
        from .dist import detection_block
        self.block, self.det, self.count = detection_block(B, self.max_cand, device)
        self.keep = torch.zeros((B, self.max_cand), dtype=torch.int32, device=device) if want_keep else None

    def launch(self, pred, conf_thres, p_thres, stream_ptr=None):
        assert pred.dtype == torch.float32 and pred.is_contiguous() and pred.shape == (self.B, self.rows, 5 + self.nc)
        st = lib().icaf_confluence(pred.data_ptr(), self.B, self.rows, self.nc, float(conf_thres), float(p_thres), self.max_cand,
                                   self.det.data_ptr(), self.count.data_ptr(), self.keep.data_ptr() if self.keep is not None else None,
                                   self.ws.data_ptr(), self.ws.numel(), stream_ptr if stream_ptr is not None else current_stream_ptr())
        check(st, "icaf_confluence")
        return self.det, self.count, self.keep


def loss_workspace(shapes, B, na, nt):
    """icaf_loss_workspace_bytes for `nt` targets: (bytes, tobj_off [nl], slots_off [nl]) — byte offsets from the workspace's start; tobj_off
    does not depend on nt."""
    nl = len(shapes)
    ny, nx = (C.c_int * max(nl, 1))(*[int(s[0]) for s in shapes]), (C.c_int * max(nl, 1))(*[int(s[1]) for s in shapes])
    sz, toff, soff = C.c_size_t(0), (C.c_size_t * max(nl, 1))(), (C.c_size_t * max(nl, 1))()
    check(lib().icaf_loss_workspace_bytes(nl, ny, nx, int(B), int(na), int(nt), C.byref(sz), toff, soff), "loss_workspace")
    return sz.value, list(toff)[:nl], list(soff)[:nl]


def loss_params_block(prm):
    """dict (utils.loss.loss_params) -> icaf_loss_params"""
    blk = _lib.LossParams(*[float(prm[k]) for k in ("box", "obj", "cls", "cls_pw", "obj_pw", "anchor_t", "gr", "cp", "cn")])
    for i, b in enumerate(prm["balance"][:5]):
        blk.balance[i] = float(b)
    return blk


def loss_launch(maps, shapes, B, na, nc, anchors, targets, prm, out, counts, ws, nl=None, ws_bytes=None, stream_ptr=None):
    """The raw icaf_loss call, status returned unchecked (the refusal tests read it): maps a list of data pointers, anchors a host fp32
    array (nl, na, 2), targets a device (nt, 6) fp32 tensor, out (4,) fp32 / counts (nl,) int32 / ws uint8 device tensors."""
    nl = len(shapes) if nl is None else nl
    ptrs = (C.c_void_p * 8)(*([int(m) if m else None for m in maps] + [None] * (8 - len(maps))))
    ny, nx = (C.c_int * 8)(*([int(s[0]) for s in shapes] + [0] * (8 - len(shapes)))), (C.c_int * 8)(*([int(s[1]) for s in shapes] + [0] * (8 - len(shapes))))
    anc = np.ascontiguousarray(anchors, np.float32)
    blk = loss_params_block(prm)
    return lib().icaf_loss(ptrs, ny, nx, int(nl), int(B), int(na), int(nc), anc.ctypes.data_as(C.POINTER(C.c_float)), targets.data_ptr(),
                           int(targets.shape[0]), C.byref(blk), out.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                           ws.numel() if ws_bytes is None else int(ws_bytes), stream_ptr if stream_ptr is not None else current_stream_ptr())


class LossRunner:
    """Pre-allocated validation-loss launch (icaf_loss: the forward value of the reference's ComputeLoss, no gradients) for a fixed
    (B, level shapes, na, nc): owns the workspace (sized for LOSS_MAX_TARGETS, so any batch's target table fits), the four output values and
    the per-level match counts; results stay on the device, no host sync.  loss_workspace() says where the tobj maps and the slot tables
    of the last launch lie in `ws`."""

    def __init__(self, B, shapes, na, nc, anchors, device, max_targets=LOSS_MAX_TARGETS):
        self.B, self.shapes, self.na, self.nc = int(B), [tuple(int(v) for v in s) for s in shapes], int(na), int(nc)
        self.anchors = np.ascontiguousarray(anchors.numpy() if torch.is_tensor(anchors) else anchors, np.float32).reshape(len(self.shapes), self.na, 2)
        self.max_targets = int(max_targets)
        nbytes, self.tobj_off, _ = loss_workspace(self.shapes, self.B, self.na, self.max_targets)
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
        self.out = torch.zeros((4,), dtype=torch.float32, device=device)
        self.counts = torch.zeros((len(self.shapes),), dtype=torch.int32, device=device)

    def launch(self, maps, targets, prm, stream_ptr=None):
        assert len(maps) == len(self.shapes) and targets.dtype == torch.float32 and targets.is_contiguous() and targets.dim() == 2 and targets.shape[1] == 6
        for m, (ny, nx) in zip(maps, self.shapes):
            assert m.dtype == torch.float32 and m.is_contiguous() and m.shape == (self.B, self.na, ny, nx, 5 + self.nc)
        if targets.shape[0] > self.max_targets:
            raise ValueError(f"LossRunner: {targets.shape[0]} targets, the workspace was sized for {self.max_targets}")
        st = loss_launch([m.data_ptr() for m in maps], self.shapes, self.B, self.na, self.nc, self.anchors, targets, prm, self.out, self.counts,
                         self.ws, stream_ptr=stream_ptr)
        check(st, "icaf_loss")
        return self.out, self.counts


# ------------------------------------------------------------------------------------------------------------
# native camera frames: device letterbox in, native-space boxes out
# ------------------------------------------------------------------------------------------------------------
# one row per (modality, image): the layout of icaf_frame_geom (include/icaf.h)
GEOM_DTYPE = np.dtype(FrameGeom)
assert GEOM_DTYPE.itemsize == C.sizeof(FrameGeom) == 48
FRAME_ALIGN = 256          # frames start on this boundary inside an arena (the kernel needs 16)
# what a forward from frames hands back beside its result: the descriptor rows, the scale_coords rows, and those on the device
# (window: per modality None or, for a 16-bit thermal modality, the cuda int32 (B, 2) gain-control windows the step used)
FrameGeometry = collections.namedtuple("FrameGeometry", "geom scale_host scale window", defaults=(None,))


def _geom_row(g, i, shape, fit, how):
    """Fill descriptor row `g` for frame i of native `shape`: h0, w0, nh, nw, top, left and the fp32 tap scales sx = w0 / nw, sy = h0 / nh
    (offset / pitch / ch stay 0 for pack_frames); returns (h0, w0).  fit(h0, w0) -> (nh, nw, place) is the caller's resize rule, `how` its
    name in the refusal; place() -> (top, left) runs only once the resized block is known to hold a pixel."""
    h0, w0 = (int(v) for v in shape)
    if h0 < 1 or w0 < 1:
        raise ValueError(f"frame {i}: empty shape {h0}x{w0}")
    nh, nw, place = fit(h0, w0)
    if nw < 1 or nh < 1:
        raise ValueError(f"frame {i}: {h0}x{w0} {how} leaves no pixel ({nh}x{nw})")
    top, left = place()
    g["h0"], g["w0"], g["nh"], g["nw"], g["top"], g["left"] = h0, w0, nh, nw, top, left
    g["sx"], g["sy"] = np.float32(w0 / nw), np.float32(h0 / nh)
    return h0, w0


def frame_geometry(shapes, new_shape, scaleup=True):
    """The letterbox of native (h0, w0) frames to `new_shape` as numbers (utils.datasets.letterbox_geometry is the one definition of r,
    new_unpad, dw / dh and the round(d -+ 0.1) split): returns (geom, scale).  geom: GEOM_DTYPE rows, one per shape — h0, w0, nh, nw,
    top, left and the fp32 tap scales sx = w0 / nw, sy = h0 / nh; offset / pitch / ch are left 0 for pack_frames.  scale: float32
    (n, 5) rows {gain, pad_x, pad_y, w0, h0} of scale_coords(new_shape, ., (h0, w0)) with ratio_pad=None (utils/general.py:82-93) — what
    scale_detections and match_predictions take."""
    from .utils.datasets import letterbox_geometry
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    H, W = int(new_shape[0]), int(new_shape[1])
    geom = np.zeros((len(shapes),), GEOM_DTYPE)
    scale = np.zeros((len(shapes), 5), np.float32)

    def fit(h0, w0):
        _, (nw, nh), _, (top, _, left, _) = letterbox_geometry((h0, w0), (H, W), scaleup)
        return nh, nw, lambda: (top, left)
    for i, shape in enumerate(shapes):
        h0, w0 = _geom_row(geom[i], i, shape, fit, f"letterboxed to {H}x{W}")
        gain = min(H / h0, W / w0)
        scale[i] = (gain, (W - w0 * gain) / 2, (H - h0 * gain) / 2, w0, h0)
    return geom, scale


def pack_frames(geom, channels, pitch=None, base=0):
    """Lay frames out back to back in a byte arena: fills offset / pitch / ch of the rows (pitch: bytes per row, default w0 * ch; frames
    start on FRAME_ALIGN boundaries from `base` on) and returns the first free byte behind them."""
    off = int(base)
    for g, ch, p in zip(geom, _per_row(channels, len(geom)), _per_row(pitch, len(geom))):
        off = _place(g, off, ch, int(g["w0"]) * int(ch) if p is None else p)
    return off


def _per_row(v, n, single=lambda v: False):
    """An argument of a pack function as a list of n: one value for all rows (None, an int, a string, or what `single` takes for one), or
    one value per row."""
    return [v] * n if v is None or isinstance(v, (int, str)) or single(v) else list(v)


def _place(g, off, ch, pitch, nrows=None):
    """The frame of descriptor row `g` at the first FRAME_ALIGN boundary from `off` on: sets offset / ch / pitch and returns the first byte
    behind its `nrows` (default h0) rows."""
    off = -(-int(off) // FRAME_ALIGN) * FRAME_ALIGN
    g["offset"], g["ch"], g["pitch"] = off, int(ch), int(pitch)
    return off + (int(g["h0"]) if nrows is None else int(nrows)) * int(pitch)


def _table_rows(geom, dtype):
    """Zeroed rows of a table kind around `geom`: frame_geometry's GEOM_DTYPE rows, or rows of the kind whose "g" is filled."""
    rows = np.zeros((len(geom),), dtype)
    rows["g"] = frame_rows(geom)
    return rows


def frame_rows(rows):
    """The icaf_frame_geom rows of a table of any kind: GEOM_DTYPE rows themselves, or field "g" of the rows that embed them."""
    return rows if rows.dtype == GEOM_DTYPE else rows["g"]


def _tap_caps(g):
    """The caps of the staging rules (include/icaf.h): the (rows, columns) a 32 x 64 tile of descriptor row `g` can tap at most, or None for
    a tap scale of 1024 and more (such frames are never staged)."""
    sx, sy = np.float32(g["sx"]), np.float32(g["sy"])
    if not (sx < 1024 and sy < 1024):
        return None
    return min(int(g["h0"]), int(np.float32(32) * sy) + 4), min(int(g["w0"]), int(np.float32(64) * sx) + 4)


def _rect_staged(g, ch, budget):
    """One rectangle of `ch` bytes a pixel under `budget`: rows of whole 16-byte vectors, up to 15 bytes of alignment phase each."""
    caps = _tap_caps(g)
    return caps is not None and caps[0] * ((caps[1] * ch + 30) >> 4) * 16 <= budget


def letterbox_staged(g):
    """The budget rule of icaf_letterbox_frames for one descriptor row (include/icaf.h): True = its tiles stage their source rectangle
    in LDS, False = they tap global memory (frames scaled down so far that a 32 x 64 tile's rectangle exceeds the budget)."""
    return _rect_staged(g, int(g["ch"]), _lib.LETTERBOX_LDS_BYTES)


def _validate_row(i, g, arena_bytes, H, W, src=None):
    """validate_frames' checks of descriptor row i.  src = (hs, ws): the frame in the arena is that SOURCE (a calibrated pair's warped
    modality) and h0 x w0 the aligned frame seen through it."""
    off, h0, w0, pitch, ch, nh, nw, top, left = (int(g[k]) for k in ("offset", "h0", "w0", "pitch", "ch", "nh", "nw", "top", "left"))
    hs, ws = (h0, w0) if src is None else src
    if ch not in (1, 3):
        raise ValueError(f"frame {i}: {ch} interleaved channels (1 or 3)")
    if hs < 1 or ws < 1:
        raise ValueError(f"frame {i}: empty source frame ({hs}x{ws})" if src else f"frame {i}: empty frame or resized block ({h0}x{w0} -> {nh}x{nw})")
    if h0 < 1 or w0 < 1 or nh < 1 or nw < 1:
        raise ValueError(f"frame {i}: empty {'aligned ' if src else ''}frame or resized block ({h0}x{w0} -> {nh}x{nw})")
    if pitch < ws * ch:
        raise ValueError(f"frame {i}: pitch {pitch} is less than a {'source ' if src else ''}row of {ws} pixels x {ch} channels")
    if off < 0 or off % 16:
        raise ValueError(f"frame {i}: offset {off} must be a non-negative multiple of 16")
    if off + hs * pitch > arena_bytes:
        raise ValueError(f"frame {i}: bytes [{off}, {off + hs * pitch}) leave the arena of {arena_bytes} bytes")
    if top < 0 or left < 0 or top + nh > H or left + nw > W:
        raise ValueError(f"frame {i}: resized block {nh}x{nw} at ({top}, {left}) leaves the {H}x{W} output")
    if not (g["sx"] > 0 and g["sy"] > 0):
        raise ValueError(f"frame {i}: tap scales must be positive")


def validate_frames(geom, arena_bytes, H, W):
    """Host check of descriptor rows against an arena of `arena_bytes` and an H x W output: raises ValueError with the reason.  The
    kernel trusts the table — nothing reaches the device before this has passed."""
    for i, g in enumerate(geom):
        _validate_row(i, g, arena_bytes, H, W)


def geom_tensor(geom, device=None, pin=False):
    """Descriptor rows as the flat uint8 tensor the device table is copied from / lives in."""
    t = torch.from_numpy(np.ascontiguousarray(geom).view(np.uint8).reshape(-1).copy())
    if device is not None:
        return t.to(device)
    return t.pin_memory() if pin else t


def frame_lists(rgb, ir):
    """Native frames as callers hand them over — per modality one uint8 (B, H0, W0, ch) tensor or a list of (H0_i, W0_i, ch) tensors, ch = 3
    or 1, a pair sharing its size — as (frames_rgb, frames_ir, shapes, uniform): the two lists of B frames, their (h0, w0), and per modality
    whether it came as one 4-D tensor.  Anything else raises ValueError; device, batch size and channel counts are the caller's to check."""
    fr, uniform = _pair_lists((rgb, ir), (4, 4))
    for f in fr[0] + fr[1]:
        if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] not in (1, 3):
            raise ValueError("frames must be uint8 tensors of shape (H0, W0, ch), ch = 3 or 1")
    shapes = [tuple(f.shape[:2]) for f in fr[0]]
    if shapes != [tuple(f.shape[:2]) for f in fr[1]]:
        raise ValueError("the RGB and IR frame of a pair must have the same size (a calibrated pair of unequal sizes: pass align=)")
    return fr[0], fr[1], shapes, uniform


def _pair_lists(mods, dims, what="(B, H0, W0, ch) tensors or two equally long lists of (H0, W0, ch) tensors"):
    """The two modalities as handed over -> ([frames of modality 0, of modality 1], uniform): a tensor of dims[m] dimensions is a uniform
    batch and split along its first axis, a list or tuple is taken frame by frame; both hold the same number of frames, one at least."""
    uniform = tuple(torch.is_tensor(t) and t.dim() == d for t, d in zip(mods, dims))
    fr = [[t[i] for i in range(t.shape[0])] if u else list(t) if isinstance(t, (list, tuple)) else None for t, u in zip(mods, uniform)]
    if fr[0] is None or fr[1] is None or not fr[0] or len(fr[0]) != len(fr[1]):
        raise ValueError(f"native frames come as two {what}")
    return fr, uniform


def _frames_checked(kind, arena, geom, geom_dev, dst, B=None, HW=None, window=None, mode=None, mode_dev=None):
    """What every frame launch of a table `kind` asks before any device call, for its host rows `geom`: the tensors' layout, the tables'
    sizes (window: the int32 window table of a 16-bit kind; mode / mode_dev: icaf_resize_frames' host rows and device table), the kind's
    validator against the arena and the H x W output, the mode rows, and last that all live on the device.  The output is dst's
    (B, ctot, H, W), or — for a launch without one — B and HW = (H, W).  Returns (n, B, ctot, H, W)."""
    n = len(geom)
    if kind.dtype != GEOM_DTYPE and geom.dtype != kind.dtype:
        raise ValueError(f"the descriptor rows must be {kind.rows}_GEOM_DTYPE rows (pack_{kind.rows.lower()}_frames)")
    if window is not None and (window.dtype != torch.int32 or not window.is_contiguous() or window.numel() < 2 * n):
        raise ValueError(f"the window table must be a contiguous int32 tensor of {n} (lo, hi) rows")
    if arena.dtype != torch.uint8 or not arena.is_contiguous() or arena.dim() != 1:
        raise ValueError("the arena must be a flat contiguous uint8 tensor")
    ctot = None
    if dst is not None:
        if dst.dtype != torch.uint8 or not dst.is_contiguous() or dst.dim() != 4:
            raise ValueError("dst must be a contiguous uint8 (B, ctot, H, W) tensor")
        B, ctot, H, W = dst.shape
        if W % 16:
            raise ValueError(f"output width {W} must be a multiple of 16")
    else:
        H, W = HW
    if n % B or n == 0 or (ctot is not None and 3 * (n // B) > ctot):
        raise ValueError(f"{n} descriptors for a batch of {B} images" + (f" with {ctot} channels" if ctot is not None else ""))
    if geom_dev.numel() * geom_dev.element_size() < n * kind.dtype.itemsize:
        raise ValueError("the device table is smaller than the descriptor rows")
    if (mode is None) != (mode_dev is None):
        raise ValueError("the mode table needs its host rows and its device copy, or neither (all rows mode 0)")
    if mode is not None:
        if len(mode) != n or mode_dev.dtype != torch.int32 or not mode_dev.is_contiguous() or mode_dev.numel() < n:
            raise ValueError(f"the mode table must hold one int32 per descriptor ({n}), host and device")
    kind.validate(geom, arena.numel(), H, W)
    for i in range(n if mode is not None else 0):
        md, g = int(mode[i]), geom[i]
        if md not in (0, 1):
            raise ValueError(f"frame {i}: mode {md} (0 = bilinear, 1 = area)")
        if md == 1 and (int(g["nh"]) > int(g["h0"]) or int(g["nw"]) > int(g["w0"])):
            raise ValueError(f"frame {i}: the area mode only shrinks ({int(g['h0'])}x{int(g['w0'])} -> {int(g['nh'])}x{int(g['nw'])})")
    if not all(t.is_cuda for t in (arena, dst, geom_dev, window, mode_dev) if t is not None):
        raise ValueError("arena, tables and dst must be cuda tensors (no CPU fallback exists)")
    return n, B, ctot, H, W


def _frames_launch(fn, kind, arena, geom, geom_dev, dst, swap_rb, name, extra=(), **tables):
    """The Launch of a frame kernel, everything checked before any device call (_frames_checked).  fn: the entry point's name; kind: the
    record of its table; extra: the device table the entry point takes behind the descriptors — icaf_resize_frames' modes (None: all rows
    mode 0), icaf_letterbox_y16_frames' windows; tables: the same as _frames_checked's window= or mode= / mode_dev=."""
    n, B, ctot, H, W = _frames_checked(kind, arena, geom, geom_dev, dst, **tables)
    nb = sum(kind.read(q) for q in geom) + n * 3 * H * W         # frames read once (at most, for a warped source), planes written once
    tables = (geom_dev.data_ptr(),) + tuple(t.data_ptr() if t is not None else None for t in extra)
    return Launch(getattr(lib(), fn), (arena.data_ptr(),) + tables + (n // B, B, dst.data_ptr(), ctot, H, W, int(bool(swap_rb))),
                  keep=(arena, geom_dev, dst) + tuple(extra), name=name, nbytes=nb)


def letterbox_frames(arena, geom, geom_dev, dst, swap_rb=True, c0=0, name="letterbox_frames"):
    """Letterbox the frames of a byte arena into the uint8 (B, ctot, H, W) plan input (icaf_letterbox_frames).  arena: flat cuda uint8;
    geom: the HOST descriptor rows (nstreams * B, entry modality * B + image) the device table `geom_dev` holds — or will hold by the
    time the launch runs, for a table refreshed per step (validate_frames each refresh) — validated here, before any device call;
    modality m fills channels [3m, 3m + 3)."""
    return _frames_launch("icaf_letterbox_frames", KINDS["plain"], arena, geom, geom_dev, dst, swap_rb, name)


# native YUV 4:2:0 frames: one row per (modality, image) in the layout of icaf_yuv_geom (include/icaf.h) — field "g" is a GEOM_DTYPE row
YUV_GEOM_DTYPE = np.dtype(YuvGeom)
assert YUV_GEOM_DTYPE.itemsize == C.sizeof(YuvGeom) == 80 and YUV_GEOM_DTYPE["g"] == GEOM_DTYPE
YUV_LAYOUTS = {"nv12": (2, 0), "nv21": (2, 1), "i420": (1, 0), "yv12": (1, 1)}      # layout -> (c_step, Cr stored first)
YUV_MATRICES = {"bt601": 0, "bt709": 1, "bt601-full": 2}


def yuv_matrix_code(matrix):
    """0 / 1 / 2 of icaf_yuv_geom.matrix from the value itself or its name (bt601, bt709, bt601-full); ValueError for anything else."""
    code = YUV_MATRICES.get(matrix, matrix) if isinstance(matrix, str) else matrix
    if code not in (0, 1, 2) or isinstance(code, bool):
        raise ValueError(f"unknown YUV matrix {matrix!r} (0 / 'bt601', 1 / 'bt709', 2 / 'bt601-full')")
    return int(code)


def pack_yuv_frames(geom, layouts, pitch=None, c_pitch=None, matrix=0, base=0):
    """pack_frames for tables that hold YUV 4:2:0 surfaces: returns (rows, end) — YUV_GEOM_DTYPE rows around `geom` (frame_geometry's
    GEOM_DTYPE rows, or YUV rows whose "g" is filled) and the first free byte behind the frames.  layouts: per row, or one for all,
    "nv12" | "nv21" | "i420" | "yv12" (a kind-1 row) or 3 / 1 (a kind-0 row, laid out exactly as pack_frames lays it out).  A YUV frame
    is laid out as a decoder hands it over: h0 luma rows of `pitch` bytes (default w0), directly behind them ceil(h0 / 2) chroma rows of
    `c_pitch` bytes (default: ceil(w0 / 2) samples, tight) — one plane of CbCr / CrCb pairs, or the Cb and the Cr plane (i420) / Cr and
    Cb (yv12) one behind the other.  Frames start on FRAME_ALIGN boundaries from `base` on."""
    n = len(geom)
    rows = _table_rows(geom, YUV_GEOM_DTYPE)
    code = yuv_matrix_code(matrix)
    off = int(base)
    for i, (q, lay, p, cp) in enumerate(zip(rows, _per_row(layouts, n), _per_row(pitch, n), _per_row(c_pitch, n))):
        g = q["g"]
        h0, w0 = int(g["h0"]), int(g["w0"])
        if lay in (1, 3):
            off = _place(g, off, lay, w0 * lay if p is None else p)
            continue
        if lay not in YUV_LAYOUTS:
            raise ValueError(f"frame {i}: unknown layout {lay!r} (3, 1 or one of {', '.join(YUV_LAYOUTS)})")
        step, cr_first = YUV_LAYOUTS[lay]
        chh, cw = (h0 + 1) // 2, (w0 + 1) // 2
        first = _place(g, off, 1, w0 if p is None else p)
        q["kind"], q["matrix"], q["c_step"], q["c_pitch"] = 1, code, step, cw * step if cp is None else int(cp)
        second = first + 1 if step == 2 else first + chh * int(q["c_pitch"])
        q["cb_offset"], q["cr_offset"] = (second, first) if cr_first else (first, second)
        off = first + (1 if step == 2 else 2) * chh * int(q["c_pitch"])
    return rows, off


def yuv_letterbox_staged(q):
    """The budget rule of icaf_letterbox_yuv_frames for one table row (include/icaf.h): True = its tiles stage the luma rectangle and the
    chroma samples under it in LDS, False = they tap global memory.  A kind-0 row follows letterbox_staged."""
    g = q["g"]
    if int(q["kind"]) == 0:
        return letterbox_staged(g)
    caps = _tap_caps(g)
    if caps is None:
        return False
    (rows, cols), h0, w0, step = caps, int(g["h0"]), int(g["w0"]), int(q["c_step"])
    crows, ccols = min((h0 + 1) // 2, rows // 2 + 1), min((w0 + 1) // 2, cols // 2 + 1)
    vectors = rows * ((cols + 30) >> 4) + (1 if step == 2 else 2) * crows * ((ccols * step + 30) >> 4)
    return vectors * 16 <= _lib.YUV_LDS_BYTES


def validate_yuv_frames(geom, arena_bytes, H, W):
    """validate_frames for YUV_GEOM_DTYPE rows: raises ValueError with the row and the reason — everything validate_frames refuses of
    "g", an unknown kind, and for kind-1 rows a ch that is not 1, a c_step that is not 1 or 2, an unknown matrix, a c_pitch too small for
    ceil(w0 / 2) samples, interleaved chroma whose offsets are not one byte apart, chroma planes that leave the arena.  The kernel trusts
    the table — nothing reaches the device before this has passed."""
    for i, q in enumerate(geom):
        if int(q["kind"]) not in (0, 1):
            raise ValueError(f"frame {i}: kind {int(q['kind'])} (0 = interleaved row, 1 = YUV 4:2:0)")
    validate_frames(geom["g"], arena_bytes, H, W)
    for i, q in enumerate(geom):
        if int(q["kind"]) == 0:
            continue
        g = q["g"]
        cb, cr, cp, step, matrix = (int(q[k]) for k in ("cb_offset", "cr_offset", "c_pitch", "c_step", "matrix"))
        chh, cw = (int(g["h0"]) + 1) // 2, (int(g["w0"]) + 1) // 2
        if int(g["ch"]) != 1:
            raise ValueError(f"frame {i}: a YUV 4:2:0 row describes its Y plane with ch 1, got {int(g['ch'])}")
        if step not in (1, 2):
            raise ValueError(f"frame {i}: c_step {step} (2 = interleaved chroma, 1 = planar)")
        if matrix not in (0, 1, 2):
            raise ValueError(f"frame {i}: matrix {matrix} (0 = BT.601, 1 = BT.709, 2 = BT.601 full range)")
        if cp < cw * step:
            raise ValueError(f"frame {i}: c_pitch {cp} is less than a chroma row of {cw} samples x {step} bytes")
        if step == 2 and abs(cb - cr) != 1:
            raise ValueError(f"frame {i}: interleaved chroma needs cb_offset and cr_offset one byte apart, got {cb} / {cr}")
        for name, o in (("Cb", cb), ("Cr", cr)):
            end = o + (chh - 1) * cp + (cw - 1) * step + 1
            if o < 0 or end > arena_bytes:
                raise ValueError(f"frame {i}: {name} bytes [{o}, {end}) leave the arena of {arena_bytes} bytes")


def letterbox_yuv_frames(arena, geom, geom_dev, dst, swap_rb=True, name="letterbox_yuv_frames"):
    """letterbox_frames for tables with YUV 4:2:0 rows (icaf_letterbox_yuv_frames): kind-1 rows are converted at the bilinear taps and
    equal letterbox(yuv420_to_bgr(...)) byte for byte (planes R, G, B; swap_rb is not read for them), kind-0 rows are letterbox_frames'
    own.  geom: the HOST YUV_GEOM_DTYPE rows the device table `geom_dev` holds, validated here, before any device call."""
    return _frames_launch("icaf_letterbox_yuv_frames", KINDS["yuv"], arena, geom, geom_dev, dst, swap_rb, name)


def yuv_frame_lists(rgb, ir, formats):
    """frame_lists for modalities that may arrive as YUV 4:2:0: formats = (fmt_rgb, fmt_ir), each None (an interleaved modality, as
    frame_lists takes it) or "nv12" | "nv21" | "i420" | "yv12" — then one uint8 (B, 3 * H0 // 2, W0) tensor or a list of (3 * H0_i // 2,
    W0_i) tensors, the contiguous buffer a decoder binding returns, H0 and W0 even.  The frame sizes come from the interleaved modality,
    or from the buffers themselves when both are YUV.  Returns (frames_rgb, frames_ir, shapes, uniform) like frame_lists."""
    formats = tuple(formats)
    if len(formats) != 2 or any(f is not None and f not in YUV_LAYOUTS for f in formats):
        raise ValueError(f"formats=(fmt_rgb, fmt_ir), each None or one of {', '.join(YUV_LAYOUTS)}, got {formats!r}")
    nd = [3 if f else 4 for f in formats]
    fr, uniform = _pair_lists((rgb, ir), nd, "batch tensors or two equally long lists of frames")
    shapes = [None, None]
    for m, fmt in enumerate(formats):
        for f in fr[m]:
            if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != nd[m] - 1 or (fmt is None and f.shape[2] not in (1, 3)):
                raise ValueError("frames must be uint8 tensors of shape (H0, W0, ch), ch = 3 or 1" if fmt is None else
                                 f"{fmt} frames must be uint8 tensors of shape (3 * H0 // 2, W0)")
        if fmt is None:
            shapes[m] = [tuple(f.shape[:2]) for f in fr[m]]
    if shapes[0] is None and shapes[1] is None:                  # both YUV: the buffers state their own size
        for f in fr[0]:
            if f.shape[0] % 3:
                raise ValueError(f"a YUV 4:2:0 buffer has 3 * H0 // 2 rows, got {f.shape[0]}")
        shapes[0] = [(2 * f.shape[0] // 3, f.shape[1]) for f in fr[0]]
    size = shapes[0] if shapes[0] is not None else shapes[1]
    for h0, w0 in size if any(formats) else ():
        if h0 % 2 or w0 % 2:
            raise ValueError(f"a YUV 4:2:0 buffer needs even H0 and W0, got {h0}x{w0} (odd sizes: ops.pack_yuv_frames)")
    for m, fmt in enumerate(formats):
        if fmt is not None and [tuple(f.shape) for f in fr[m]] != [(3 * h0 // 2, w0) for h0, w0 in size]:
            raise ValueError(f"a {fmt} buffer of a frame of H0 x W0 has shape (3 * H0 // 2, W0): expected {[(3 * h0 // 2, w0) for h0, w0 in size]}, "
                             f"got {[tuple(f.shape) for f in fr[m]]}")
    if shapes[0] is not None and shapes[1] is not None and shapes[0] != shapes[1]:
        raise ValueError("the RGB and IR frame of a pair must have the same size")
    return fr[0], fr[1], [tuple(int(v) for v in s) for s in size], uniform


# calibrated RGB / IR pairs: one row per (modality, image) in the layout of icaf_warp_geom (include/icaf.h) — field "g" is a GEOM_DTYPE row
WARP_GEOM_DTYPE = np.dtype(WarpGeom)
assert WARP_GEOM_DTYPE.itemsize == C.sizeof(WarpGeom) == 104 and WARP_GEOM_DTYPE["g"] == GEOM_DTYPE


def alignment_matrices(align, src_shapes, shapes):
    """One modality's alignment as float32 (B, 3, 3) ALIGNED -> SOURCE matrices (utils.datasets.warp_perspective's convention): `align`
    is a (3, 3) array (one rig, every pair), a (B, 3, 3) array (per pair) or "stretch" (utils.datasets.stretch_alignment of each pair's
    source and aligned size).  ValueError for any other shape and for a non-finite entry."""
    from .utils.datasets import stretch_alignment
    B = len(shapes)
    if isinstance(align, str):
        if align != "stretch":
            raise ValueError(f"an alignment is a (3, 3) or ({B}, 3, 3) matrix or 'stretch', got {align!r}")
        return np.stack([stretch_alignment(s, a) for s, a in zip(src_shapes, shapes)])
    a = align.detach().cpu().numpy() if torch.is_tensor(align) else np.asarray(align)
    if a.dtype.kind not in "fiu" or a.shape not in ((3, 3), (B, 3, 3)):
        raise ValueError(f"an alignment is a (3, 3) or ({B}, 3, 3) matrix or 'stretch', got shape {a.shape} of {a.dtype}")
    a = np.ascontiguousarray(np.broadcast_to(a.astype(np.float64).astype(np.float32), (B, 3, 3)))
    if not np.isfinite(a).all():
        raise ValueError("an alignment matrix has a non-finite entry")
    return a


def pack_warp_frames(geom, sources, matrices=None, borders=0, pitch=None, base=0):
    """pack_frames for tables of calibrated pairs: returns (rows, end) — WARP_GEOM_DTYPE rows around `geom` (frame_geometry's GEOM_DTYPE
    rows, or WARP rows whose "g" is filled) and the first free byte behind the frames.  sources: a list with one entry per row, or one
    entry (an int or a tuple) for all rows — 3 / 1 (a
    kind-0 row: the frame has its row's h0 x w0 and that many channels, laid out exactly as pack_frames lays it out) or (hs, ws, ch) (a
    kind-1 row: h0 x w0 is the ALIGNED size, the frame in the arena is the hs x ws source).  matrices: per row (or one for all) the 3 x 3
    aligned -> source matrix of a kind-1 row, None for kind 0; borders: 0..255 per row or one for all; pitch: bytes per source row (default
    tight).  Frames start on FRAME_ALIGN boundaries from `base` on."""
    n = len(geom)
    rows = _table_rows(geom, WARP_GEOM_DTYPE)
    srcs = _per_row(sources, n, lambda s: isinstance(s, tuple) and len(s) == 3 and isinstance(s[0], int))
    mats, bords, pitches = _per_row(matrices, n, lambda m: getattr(m, "shape", None) == (3, 3)), _per_row(borders, n), _per_row(pitch, n)
    if not (len(srcs) == len(mats) == len(bords) == len(pitches) == n):
        raise ValueError(f"{n} rows need {n} sources, matrices, borders and pitches (or one for all)")
    off = int(base)
    for i, (q, src, mat, bd, p) in enumerate(zip(rows, srcs, mats, bords, pitches)):
        g = q["g"]
        if isinstance(src, (int, np.integer)):
            if mat is not None:
                raise ValueError(f"frame {i}: a matrix needs a (hs, ws, ch) source; {src} alone describes an unwarped frame")
            off = _place(g, off, src, int(g["w0"]) * int(src) if p is None else p)
            continue
        if len(src) != 3:
            raise ValueError(f"frame {i}: a source is 3, 1 or (hs, ws, ch), got {src!r}")
        hs, ws, ch = (int(v) for v in src)
        if mat is None:
            raise ValueError(f"frame {i}: a (hs, ws, ch) source needs its 3 x 3 matrix")
        m = np.asarray(mat, np.float64).astype(np.float32)
        if m.shape != (3, 3):
            raise ValueError(f"frame {i}: an alignment matrix is 3 x 3, got shape {m.shape}")
        q["kind"], q["hs"], q["ws"], q["border"], q["m"] = 1, hs, ws, int(bd), m.reshape(9)
        off = _place(g, off, ch, ws * ch if p is None else p, nrows=hs)
    return rows, off


def validate_warp_frames(geom, arena_bytes, H, W):
    """validate_frames for WARP_GEOM_DTYPE rows: raises ValueError with the row and the reason — an unknown kind, for kind-0 rows
    everything validate_frames refuses, for kind-1 rows the same of the SOURCE frame (hs x ws x ch at offset / pitch) and of the aligned
    block, a border outside 0..255 and a non-finite matrix entry.  The kernel trusts the table — nothing reaches the device before this
    has passed."""
    for i, q in enumerate(geom):
        kind = int(q["kind"])
        if kind not in (0, 1):
            raise ValueError(f"frame {i}: kind {kind} (0 = plain row, 1 = warped)")
        if kind == 0:
            _validate_row(i, q["g"], arena_bytes, H, W)
            continue
        _validate_row(i, q["g"], arena_bytes, H, W, src=(int(q["hs"]), int(q["ws"])))
        border = int(q["border"])
        if not 0 <= border <= 255:
            raise ValueError(f"frame {i}: border {border} outside 0..255")
        if not np.isfinite(q["m"]).all():
            raise ValueError(f"frame {i}: the alignment matrix has a non-finite entry")


def warp_letterbox_staged(q, tile):
    """The stage rule of icaf_letterbox_warp_frames for one table row and one 32 x 64 output tile (include/icaf.h), tile = (tile row, tile
    column): True = the tile copies a box of the source frame into LDS and taps it, False = it taps global memory (a tile of padding
    only, a corner behind the horizon or with non-finite coordinates, a box outside the frame or beyond the budget).  The device's own
    fp32 operations, one by one.  A kind-0 row follows letterbox_staged."""
    g = q["g"]
    if int(q["kind"]) == 0:
        return letterbox_staged(g)
    f32 = np.float32
    by, bx = (int(v) for v in tile)
    top, left, nh, nw = (int(g[k]) for k in ("top", "left", "nh", "nw"))
    ra, rb = max(by * 32, top) - top, min(by * 32 + 32, top + nh) - 1 - top
    ca, cb = max(bx * 64, left) - left, min(bx * 64 + 64, left + nw) - 1 - left
    if ra > rb or ca > cb:
        return False

    def tap(j, scale, n):
        s = (f32(j) + f32(0.5)) * f32(scale)
        i = int(np.floor(s - f32(0.5)))
        return min(max(i, 0), n - 1), min(max(i + 1, 0), n - 1)
    (ylo, _), (_, yhi) = tap(ra, g["sy"], int(g["h0"])), tap(rb, g["sy"], int(g["h0"]))
    (xlo, _), (_, xhi) = tap(ca, g["sx"], int(g["w0"])), tap(cb, g["sx"], int(g["w0"]))
    m = np.asarray(q["m"], f32)
    x, y = np.array([xlo, xhi, xlo, xhi], f32), np.array([ylo, ylo, yhi, yhi], f32)
    with np.errstate(all="ignore"):
        Z = (m[6] * x + m[7] * y) + m[8]
        u, v = ((m[0] * x + m[1] * y) + m[2]) / Z, ((m[3] * x + m[4] * y) + m[5]) / Z
    if not ((Z > 0).all() and np.isfinite(u).all() and np.isfinite(v).all()):
        return False
    ilo, ihi = max(np.floor(u.min()) - f32(1), f32(0)), min(np.floor(u.max()) + f32(2), f32(int(q["ws"]) - 1))
    jlo, jhi = max(np.floor(v.min()) - f32(1), f32(0)), min(np.floor(v.max()) + f32(2), f32(int(q["hs"]) - 1))
    if not (ilo <= ihi and jlo <= jhi):
        return False
    ncols, nrows = int(ihi) - int(ilo) + 1, int(jhi) - int(jlo) + 1
    return nrows * ((ncols * int(g["ch"]) + 30) >> 4) * 16 <= _lib.WARP_LDS_BYTES


def letterbox_warp_frames(arena, geom, geom_dev, dst, swap_rb=True, name="letterbox_warp_frames"):
    """letterbox_frames for tables of calibrated pairs (icaf_letterbox_warp_frames): kind-1 rows are seen through their homography at the
    bilinear taps and equal letterbox(utils.datasets.warp_perspective(...)) byte for byte, kind-0 rows are letterbox_frames' own.  geom:
    the HOST WARP_GEOM_DTYPE rows the device table `geom_dev` holds — or will hold by the time the launch runs, for a table refreshed per
    step (validate_warp_frames each refresh) — validated here, before any device call."""
    return _frames_launch("icaf_letterbox_warp_frames", KINDS["align"], arena, geom, geom_dev, dst, swap_rb, name)


def _aligned_modality(align):
    """align=(A_rgb, A_ir) -> (index of the one modality that carries an alignment, that alignment); ValueError for any other form."""
    try:
        a_rgb, a_ir = align
    except (TypeError, ValueError):
        raise ValueError("align=(A_rgb, A_ir): one entry per modality, None for the modality that is not warped") from None
    if a_rgb is not None and a_ir is not None:
        raise ValueError("align=(A_rgb, A_ir): both modalities carry an alignment; one of them defines the aligned space and stays None")
    if a_rgb is None and a_ir is None:
        raise ValueError("align=(A_rgb, A_ir): neither modality carries an alignment (plain pairs: leave align=None)")
    return (0, a_rgb) if a_rgb is not None else (1, a_ir)


def warp_frame_lists(rgb, ir, align):
    """frame_lists for a calibrated pair: align = (A_rgb, A_ir), exactly one of them not None — that modality is seen through its
    alignment (alignment_matrices: a (3, 3) or (B, 3, 3) aligned -> source matrix, or "stretch") and may have any size per frame; the
    OTHER modality's frame sizes are the aligned sizes.  Returns (frames_rgb, frames_ir, shapes, uniform, m, src_shapes, matrices): the two
    lists of B frames, the aligned (h0, w0), per modality whether it came as one 4-D tensor, the aligned modality's index, its frames'
    (hs, ws) and the float32 (B, 3, 3) matrices.  Anything else raises ValueError."""
    m, a = _aligned_modality(align)
    fr, uniform = _pair_lists((rgb, ir), (4, 4))
    for f in fr[0] + fr[1]:
        if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] not in (1, 3) or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError("frames must be uint8 tensors of shape (H0, W0, ch), ch = 3 or 1")
    shapes = [tuple(int(v) for v in f.shape[:2]) for f in fr[1 - m]]
    src_shapes = [tuple(int(v) for v in f.shape[:2]) for f in fr[m]]
    return fr[0], fr[1], shapes, uniform, m, src_shapes, alignment_matrices(a, src_shapes, shapes)


# 16-bit thermal frames: one row per (modality, image) in the layout of icaf_y16_geom (include/icaf.h) — field "g" is a GEOM_DTYPE row
Y16_GEOM_DTYPE = np.dtype(Y16Geom)
assert Y16_GEOM_DTYPE.itemsize == C.sizeof(Y16Geom) == 72 and Y16_GEOM_DTYPE["g"] == GEOM_DTYPE
Y16_DTYPES = tuple(getattr(torch, n) for n in ("uint16", "int16") if hasattr(torch, n))      # the same bits either way


def _y16_windows(window, n):
    """pack_y16_frames' `window` as a list of n entries, each None (mode 1) or an (lo, hi) pair of ints (mode 0)."""
    if window is None:
        return [None] * n
    if torch.is_tensor(window):
        window = window.detach().cpu().numpy()
    if not isinstance(window, np.ndarray) and any(w is None for w in window):
        rows = list(window)
    else:
        w = np.asarray(window)
        if w.shape == (2,):
            rows = [w] * n
        elif w.ndim == 2 and w.shape[1] == 2:
            rows = list(w)
        else:
            raise ValueError(f"a gain-control window is (lo, hi) or one (lo, hi) row per frame, got shape {w.shape}")
    if len(rows) != n:
        raise ValueError(f"{len(rows)} gain-control windows for {n} frames")
    out = []
    for w in rows:
        if w is not None and any(int(v) != v for v in w):
            raise ValueError(f"a gain-control window holds integers, got {tuple(w)!r}")
        out.append(None if w is None else (int(w[0]), int(w[1])))
    return out


def pack_y16_frames(geom, layouts, pitch=None, clip=None, window=None, base=0):
    """pack_frames for tables that hold 16-bit thermal frames: returns (rows, end) — Y16_GEOM_DTYPE rows around `geom` (frame_geometry's
    GEOM_DTYPE rows, or Y16 rows whose "g" is filled) and the first free byte behind the frames.  layouts: per row, or one for all, "y16"
    (a kind-1 row: h0 rows of little-endian uint16, `pitch` BYTES each, default 2 * w0) or 3 / 1 (a kind-0 row, laid out exactly as
    pack_frames lays it out).  clip: (clip_lo, clip_hi) in basis points for the percentile window (mode 1; default
    utils.datasets.AGC_CLIP); window: None, or (lo, hi) for every Y16 row, or one entry per row of the table, None or (lo, hi) — a row
    with a window is a mode-0 row.  Frames start on FRAME_ALIGN boundaries from `base` on."""
    from .utils.datasets import AGC_CLIP, agc_clip
    n = len(geom)
    rows = _table_rows(geom, Y16_GEOM_DTYPE)
    clip_lo, clip_hi = agc_clip(AGC_CLIP if clip is None else clip)
    off = int(base)
    for i, (q, lay, p, win) in enumerate(zip(rows, _per_row(layouts, n), _per_row(pitch, n), _y16_windows(window, n))):
        g = q["g"]
        w0 = int(g["w0"])
        if lay in (1, 3):
            off = _place(g, off, lay, w0 * lay if p is None else p)
        elif lay == "y16":
            off = _place(g, off, 1, 2 * w0 if p is None else p)
            q["kind"], q["mode"], q["clip_lo"], q["clip_hi"] = 1, 1 if win is None else 0, clip_lo, clip_hi
            if win is not None:
                q["lo"], q["hi"] = win
        else:
            raise ValueError(f"frame {i}: unknown layout {lay!r} (3, 1 or 'y16')")
    return rows, off


def y16_letterbox_staged(q):
    """The budget rule of icaf_letterbox_y16_frames for one table row (include/icaf.h): True = its tiles stage the MAPPED bytes of their
    source rectangle in LDS, False = they tap global memory.  A kind-0 row follows letterbox_staged; a kind-1 row the same rule for one
    byte per pixel under ICAF_Y16_LDS_BYTES."""
    g = q["g"]
    if int(q["kind"]) == 0:
        return letterbox_staged(g)
    return _rect_staged(g, 1, _lib.Y16_LDS_BYTES)


def validate_y16_frames(geom, arena_bytes, H, W):
    """validate_frames for Y16_GEOM_DTYPE rows: raises ValueError with the row and the reason — everything validate_frames refuses of
    "g" (the 16-byte alignment, the frame inside the arena, the block inside the output), an unknown kind, and for kind-1 rows a ch that
    is not 1, an odd pitch or one below 2 * w0 bytes, an unknown mode, a clip outside 0..4999 basis points, a window that is not 0 <= lo
    <= hi <= 65535.  The kernels trust the table — nothing reaches the device before this has passed."""
    for i, q in enumerate(geom):
        if int(q["kind"]) not in (0, 1):
            raise ValueError(f"frame {i}: kind {int(q['kind'])} (0 = interleaved row, 1 = 16-bit thermal)")
    validate_frames(geom["g"], arena_bytes, H, W)
    for i, q in enumerate(geom):
        if int(q["kind"]) == 0:
            continue
        g = q["g"]
        pitch, w0, mode, lo, hi, clip_lo, clip_hi = (int(v) for v in (g["pitch"], g["w0"], q["mode"], q["lo"], q["hi"], q["clip_lo"], q["clip_hi"]))
        if int(g["ch"]) != 1:
            raise ValueError(f"frame {i}: a 16-bit thermal row has ch 1, got {int(g['ch'])}")
        if pitch % 2 or pitch < 2 * w0:
            raise ValueError(f"frame {i}: pitch {pitch} must be an even number of bytes, at least 2 * w0 = {2 * w0}")
        if mode not in (0, 1):
            raise ValueError(f"frame {i}: mode {mode} (0 = window given, 1 = percentile)")
        if not (0 <= clip_lo <= 4999 and 0 <= clip_hi <= 4999):
            raise ValueError(f"frame {i}: clip ({clip_lo}, {clip_hi}) must lie in 0..4999 basis points each")
        if mode == 0 and not 0 <= lo <= hi <= 65535:
            raise ValueError(f"frame {i}: window ({lo}, {hi}) must satisfy 0 <= lo <= hi <= 65535")


def y16_window(arena, geom, geom_dev, window_dev, B, H, W, name="y16_window"):
    """The gain-control windows of a table's 16-bit thermal rows (icaf_y16_window): window_dev, int32 (n, 2) on the device, takes (lo, hi)
    of every kind-1 row — utils.datasets.agc_window of the frame for a mode-1 row, the row's own pair for a mode-0 row; rows of kind 0
    keep what they hold.  geom: the HOST rows the device table `geom_dev` holds, validated here (against an H x W output) before any
    device call; B: images per modality.  Nothing is read back."""
    n = _frames_checked(KINDS["y16"], arena, geom, geom_dev, None, B=B, HW=(H, W), window=window_dev)[0]
    nb = sum(2 * 2 * int(q["g"]["h0"]) * int(q["g"]["w0"]) for q in geom if int(q["kind"]) and int(q["mode"]))       # two passes over a frame
    return Launch(lib().icaf_y16_window, (arena.data_ptr(), geom_dev.data_ptr(), n // B, B, window_dev.data_ptr()),
                  keep=(arena, geom_dev, window_dev), name=name, nbytes=nb)


def letterbox_y16_frames(arena, geom, geom_dev, window_dev, dst, swap_rb=True, name="letterbox_y16_frames"):
    """letterbox_frames for tables with 16-bit thermal rows (icaf_letterbox_y16_frames): kind-1 rows are mapped to bytes at the bilinear
    taps with their row of `window_dev` (y16_window fills it; it runs first) and equal letterbox(agc_u16_to_u8(frame, lo, hi)) byte for
    byte in all three planes, kind-0 rows are letterbox_frames' own.  geom: the HOST Y16_GEOM_DTYPE rows the device table `geom_dev`
    holds, validated here, before any device call."""
    return _frames_launch("icaf_letterbox_y16_frames", KINDS["y16"], arena, geom, geom_dev, dst, swap_rb, name, extra=(window_dev,), window=window_dev)


def y16_bytes(t):
    """A 16-bit thermal modality as bytes: a torch.uint16 / torch.int16 tensor (..., H0, W0) becomes its uint8 view (..., H0, 2 * W0)
    (little-endian, as the kernels read it), a uint8 tensor is taken as that view already, a list or tuple is converted frame by frame."""
    if isinstance(t, (list, tuple)):
        return [y16_bytes(f) for f in t]
    if torch.is_tensor(t) and t.dtype in Y16_DTYPES and t.dim() >= 2:
        return (t if t.stride(-1) == 1 else t.contiguous()).view(torch.uint8)
    return t


def y16_frame_lists(rgb, ir, formats):
    """frame_lists for modalities that may arrive as 16-bit thermal frames: formats = (fmt_rgb, fmt_ir), each None (an interleaved
    modality, as frame_lists takes it) or "y16" — then a torch.uint16 / torch.int16 (B, H0, W0) tensor, or its uint8 byte buffer (B, H0,
    2 * W0), or a list of per-frame (H0_i, W0_i) / (H0_i, 2 * W0_i) tensors.  Returns (frames_rgb, frames_ir, shapes, uniform) like
    frame_lists; the frames of a Y16 modality come back as uint8 (H0, 2 * W0) views."""
    formats = tuple(formats)
    if len(formats) != 2 or any(f not in (None, "y16") for f in formats):
        raise ValueError(f"formats=(fmt_rgb, fmt_ir), each None or 'y16', got {formats!r}")
    mods = [y16_bytes(t) if f else t for t, f in zip((rgb, ir), formats)]
    nd = [3 if f else 4 for f in formats]
    fr, uniform = _pair_lists(mods, nd, "batch tensors or two equally long lists of frames")
    shapes = []
    for m, fmt in enumerate(formats):
        for f in fr[m]:
            if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != nd[m] - 1 or (fmt is None and f.shape[2] not in (1, 3)) or \
                    (fmt is not None and (f.shape[1] % 2 or f.shape[1] < 2 or f.shape[0] < 1)):
                raise ValueError("frames must be uint8 tensors of shape (H0, W0, ch), ch = 3 or 1" if fmt is None else
                                 "y16 frames must be 16-bit tensors of shape (H0, W0) or their uint8 bytes (H0, 2 * W0)")
        shapes.append([(int(f.shape[0]), int(f.shape[1]) // 2 if fmt else int(f.shape[1])) for f in fr[m]])
    if shapes[0] != shapes[1]:
        raise ValueError("the RGB and IR frame of a pair must have the same size")
    return fr[0], fr[1], shapes[0], uniform


def val_geometry(shapes, img_size, batch_shape):
    """The validation loader's two steps for native (h0, w0) frames as numbers (PairedValSet.__getitem__; reference utils/datasets.py:
    1116-1122 + letterbox): returns (geom, mode, scale).  Step 1, the loader's own numbers: r = img_size / max(h0, w0), (nw, nh) =
    (int(w0 r), int(h0 r)) unless r == 1; mode 1 (pixel-area average) for r < 1, mode 0 for r > 1 (bilinear up-scale) and r == 1 (copy).
    Step 2, letterbox_geometry((nh, nw), batch_shape, scaleup=False), must be pure padding — what the loader's rectangular batch shapes
    and a square img_size batch give; a frame it would resize a second time raises ValueError.  geom: GEOM_DTYPE rows as frame_geometry's
    (offset / pitch / ch left for pack_frames); mode: int32 per row; scale: float32 (n, 5) rows {nh / h0, dw, dh, w0, h0} — scale_coords'
    ratio_pad form, the rows test.py builds from the loader's `shapes`."""
    from .utils.datasets import letterbox_geometry
    if isinstance(batch_shape, int):
        batch_shape = (batch_shape, batch_shape)
    H, W = int(batch_shape[0]), int(batch_shape[1])
    n = len(shapes)
    geom, mode, scale = np.zeros((n,), GEOM_DTYPE), np.zeros((n,), np.int32), np.zeros((n, 5), np.float32)
    for i, shape in enumerate(shapes):
        def fit(h0, w0):
            r = img_size / max(h0, w0)
            nh, nw = (int(h0 * r), int(w0 * r)) if r != 1 else (h0, w0)

            def place():
                _, new_unpad, (dw, dh), (top, _, left, _) = letterbox_geometry((nh, nw), (H, W), scaleup=False)
                if new_unpad != (nw, nh):
                    raise ValueError(f"frame {i}: {h0}x{w0} -> {nh}x{nw} does not fit the {H}x{W} batch by padding alone (letterbox would "
                                     f"resize it to {new_unpad[1]}x{new_unpad[0]})")
                mode[i] = 1 if r < 1 else 0
                scale[i] = (nh / h0, dw, dh, w0, h0)
                return top, left
            return nh, nw, place
        _geom_row(geom[i], i, shape, fit, f"with its longest side at {img_size}")
    return geom, mode, scale


def area_staged(g):
    """The budget rule of icaf_resize_frames for one mode-1 descriptor row (include/icaf.h): True = its tiles tabulate their weights and keep
    the fp32 rows of the vertical pass in LDS, at least two output rows at a time; False = direct path (a shrink of 7 x and more on an axis, or
    source spans too wide for two rows)."""
    h0, w0, nh, nw, ch = (int(g[k]) for k in ("h0", "w0", "nh", "nw", "ch"))
    sy, sx = h0 / nh, w0 / nw
    if int(sy) + 2 > _lib.RESIZE_MAX_TAPS or int(sx) + 2 > _lib.RESIZE_MAX_TAPS:
        return False
    floats = ((min(w0, int(64.0 * sx) + 2) * ch + 3) & ~3) + 4
    return min(32, _lib.RESIZE_LDS_BYTES // (4 * floats)) >= 2


def resize_frames(arena, geom, mode_dev, geom_dev, dst, swap_rb=True, mode=None, name="resize_frames"):
    """letterbox_frames with a resize mode per descriptor (icaf_resize_frames): mode 0 rows are letterbox_frames' bilinear resize, mode 1
    rows the pixel-area average of utils.datasets.resize_area_scalar, byte for byte.  mode: the HOST int rows the device table `mode_dev`
    (int32) holds; both None = every row mode 0.  Validated here, before any device call: validate_frames, and nh <= h0, nw <= w0 for mode 1."""
    return _frames_launch("icaf_resize_frames", KINDS["plain"], arena, geom, geom_dev, dst, swap_rb, name, extra=(mode_dev,), mode=mode, mode_dev=mode_dev)


# One record per kind of table — what Model.forward_frames and DetectionPipeline ask of it:
#   name      "plain" | "yuv" | "align" | "y16" (part of forward_frames' state key)
#   rows      the kind's prefix of its *_GEOM_DTYPE / pack_*_frames names ("" for plain), noun: what its frames are called in a refusal
#   dtype     the row dtype (frame_rows gives the embedded icaf_frame_geom rows of any of them)
#   lists     (rgb, ir, formats, align) -> (frames_rgb, frames_ir, shapes, uniform, aligned modality, its source shapes, its matrices)
#   pack      (geom, specs, base, matrix=, clip=, border=) -> (rows, end); specs: one entry per row, see frame_specs
#   validate  (rows, arena_bytes, H, W)
#   read      row -> bytes of its frame (frame_bytes states the same for a maximum size, before any row exists)
#   window    True: the kind's step writes an int32 (n, 2) window table that its letterbox reads
#   launches  (arena, rows, rows_dev, dst, swap_rb, B, window=, mode=, mode_dev=) -> the Launches of a step, in order; swap_rb is the
#             last argument of the last
#   update    None, or (rows, B, formats, aligned modality, mats=, border=, clip=, wins=): the row fields rewritten per call / per submit
FrameKind = collections.namedtuple("FrameKind", "name rows noun dtype lists pack validate read window launches update")


def _update_warp(rows, B, formats, m, mats=None, border=None, **_):
    """This call's matrices (float32 (B, 3, 3)) and border into the aligned modality's rows; None leaves the field."""
    if mats is not None:
        rows["m"][m * B:(m + 1) * B] = mats.reshape(B, 9)
    if border is not None:
        rows["border"][m * B:(m + 1) * B] = int(border)


def _update_y16(rows, B, formats, m, clip=None, wins=None, **_):
    """This call's gain control into the rows of the Y16 modalities: wins, None or B entries (_y16_windows), gives a frame its window
    (mode 0) or None (mode 1, the percentile window of clip_lo / clip_hi); clip=None leaves the clip."""
    from .utils.datasets import agc_clip
    for mod, fmt in enumerate(formats):
        if fmt != "y16":
            continue
        sl = slice(mod * B, (mod + 1) * B)
        if clip is not None:
            rows["clip_lo"][sl], rows["clip_hi"][sl] = agc_clip(clip)
        win = [None] * B if wins is None else wins
        rows["mode"][sl] = [w is None for w in win]
        rows["lo"][sl], rows["hi"][sl] = [0 if w is None else w[0] for w in win], [0 if w is None else w[1] for w in win]


def _y16_launches(arena, rows, rows_dev, dst, swap_rb, B, window=None, **_):
    H, W = dst.shape[2:]
    return [y16_window(arena, rows, rows_dev, window, B, H, W), letterbox_y16_frames(arena, rows, rows_dev, window, dst, swap_rb)]


def _yuv_read(q):
    h0, w0 = int(q["g"]["h0"]), int(q["g"]["w0"])
    return h0 * w0 + 2 * ((h0 + 1) // 2) * ((w0 + 1) // 2) if int(q["kind"]) else h0 * w0 * int(q["g"]["ch"])


KINDS = {k.name: k for k in (
    FrameKind("plain", "", "uint8 frames", GEOM_DTYPE, lambda rgb, ir, formats, align: frame_lists(rgb, ir) + (None, None, None),
              lambda geom, specs, base=0, **_: (geom, pack_frames(geom, specs, base=base)), validate_frames,
              lambda g: int(g["h0"]) * int(g["w0"]) * int(g["ch"]), False,
              lambda arena, rows, rows_dev, dst, swap_rb, B, mode=None, mode_dev=None, **_:
              [letterbox_frames(arena, rows, rows_dev, dst, swap_rb) if mode is None else resize_frames(arena, rows, mode_dev, rows_dev, dst, swap_rb, mode)], None),
    FrameKind("yuv", "YUV", "uint8 frames", YUV_GEOM_DTYPE, lambda rgb, ir, formats, align: yuv_frame_lists(rgb, ir, formats) + (None, None, None),
              lambda geom, specs, base=0, matrix=0, **_: pack_yuv_frames(geom, specs, matrix=matrix, base=base), validate_yuv_frames, _yuv_read, False,
              lambda arena, rows, rows_dev, dst, swap_rb, B, **_: [letterbox_yuv_frames(arena, rows, rows_dev, dst, swap_rb)], None),
    FrameKind("align", "WARP", "uint8 frames", WARP_GEOM_DTYPE, lambda rgb, ir, formats, align: warp_frame_lists(rgb, ir, align),
              lambda geom, specs, base=0, border=0, **_:
              pack_warp_frames(geom, list(specs), [np.eye(3, dtype=np.float32) if isinstance(s, tuple) else None for s in specs], border, base=base),
              validate_warp_frames, lambda q: (int(q["hs"]) * int(q["ws"]) if int(q["kind"]) else int(q["g"]["h0"]) * int(q["g"]["w0"])) * int(q["g"]["ch"]),
              False, lambda arena, rows, rows_dev, dst, swap_rb, B, **_: [letterbox_warp_frames(arena, rows, rows_dev, dst, swap_rb)], _update_warp),
    FrameKind("y16", "Y16", "frames", Y16_GEOM_DTYPE, lambda rgb, ir, formats, align: y16_frame_lists(rgb, ir, formats) + (None, None, None),
              lambda geom, specs, base=0, clip=None, **_: pack_y16_frames(geom, specs, clip=clip, base=base), validate_y16_frames,
              lambda q: int(q["g"]["h0"]) * int(q["g"]["w0"]) * (2 if int(q["kind"]) else int(q["g"]["ch"])), True, _y16_launches, _update_y16))}


def frame_kind(formats, align, val_size=None, who="forward_frames: ", align_arg="align=", formats_arg="formats"):
    """The record of the table kind that serves formats=(fmt_rgb, fmt_ir) (None, or each None, "y16" or a YUV 4:2:0 layout) and align
    (None, or (A_rgb, A_ir) with exactly one entry not None).  The ONE place that refuses what cannot be combined yet: a table holds
    one kind of row, and only plain tables have the validation geometry (val_size).  who / align_arg / formats_arg: how the caller's
    arguments are called in the refusal."""
    formats = tuple(formats) if formats is not None else (None, None)
    y16, yuv = "y16" in formats, any(f is not None and f != "y16" for f in formats)
    if y16 and yuv:
        raise ValueError("a 16-bit thermal modality ('y16') beside a YUV 4:2:0 modality is not supported yet: one table holds one kind of row")
    if y16 and val_size is not None:
        raise ValueError(f"{who}16-bit thermal frames ('y16') have no validation geometry (val_size); the validation sets are 8-bit")
    if y16 and align is not None:
        raise ValueError(f"{who}{align_arg} takes interleaved 8-bit frames; a 16-bit thermal modality ('y16') cannot be combined with it yet")
    if align is not None and val_size is not None:
        raise ValueError(f"{who}{align_arg} has no validation geometry (val_size); validation sets are registered offline")
    if align is not None and yuv:
        raise ValueError(f"{who}{align_arg} takes interleaved frames; a YUV 4:2:0 modality ({formats_arg}) cannot be combined with it yet")
    if align is not None:
        _aligned_modality(align)
    if yuv and val_size is not None:
        raise ValueError(f"{who}YUV 4:2:0 frames have no validation geometry (val_size); the area down-scale reads interleaved frames")
    return KINDS["y16" if y16 else "align" if align is not None else "yuv" if yuv else "plain"]


def frame_specs(formats, frames, aligned=None):
    """What a pack function takes per row, for the frame lists of the two modalities: the format's name ("y16", "nv12", ...), the source's
    (hs, ws, ch) for a frame of the aligned modality, else the interleaved channels."""
    return tuple(fmt if fmt is not None else tuple(int(v) for v in f.shape) if m == aligned else int(f.shape[2])
                 for m, (fmt, fs) in enumerate(zip(formats, frames)) for f in fs)


def frame_bytes(spec, h0, w0):
    """Bytes of the arena one frame of `spec` (frame_specs) occupies when it is h0 x w0 (an aligned modality's source: its own hs x ws):
    2 a pixel for "y16", 1.5 for YUV 4:2:0 (luma + the chroma of sizes rounded up), else the interleaved channels."""
    if isinstance(spec, tuple):
        return spec[0] * spec[1] * spec[2]
    if spec == "y16":
        return 2 * h0 * w0
    if spec in YUV_LAYOUTS:
        return h0 * w0 + 2 * ((h0 + 1) // 2) * ((w0 + 1) // 2)
    return h0 * w0 * int(spec)


def layout_modality(rows, end, base, cap, contiguous, m=0):
    """The arena layout of ONE modality's rows as a pack function laid them out from `base` on (`end`: the first free byte behind them), in
    place: a uniform batch that arrives as one contiguous tensor (`contiguous`) keeps its layout — frame b at base + b frame sizes, so
    ONE copy moves the batch — the chroma offsets of YUV rows moving with their frame; other frames stay on their FRAME_ALIGN starts and
    must fit the modality's `cap` bytes (ValueError).  Returns rows."""
    g, B = frame_rows(rows), len(rows)
    if contiguous:
        at = base + (end - int(g[B - 1]["offset"])) * np.arange(B)           # (end - last offset: the bytes of one frame, chroma included)
        for k in ("cb_offset", "cr_offset") if "cb_offset" in (rows.dtype.names or ()) else ():
            rows[k] += (rows["kind"] != 0) * (at - g["offset"])
        g["offset"] = at
    elif end - base > cap:
        raise ValueError(f"the frames of modality {m} need {end - base} bytes of the arena's {cap}")
    return rows


def scale_detections(det, count, scale, out=None, round=False, name="scale_detections"):
    """scale_coords + clip_coords (+ torch.round) of an NMS output block on the device (icaf_scale_detections): det (B, max_det, 6) /
    count (B,) int32, scale (B, 5) fp32 device rows {gain, pad_x, pad_y, w0, h0}; out defaults to det (in place).  Rows >= count[b]
    come out as zeros."""
    out = det if out is None else out
    if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or not det.is_contiguous() or not det.is_cuda:
        raise ValueError("det must be a contiguous cuda float32 (B, max_det, 6) tensor")
    if out.shape != det.shape or out.dtype != det.dtype or not out.is_contiguous() or out.device != det.device:
        raise ValueError("out must match det")
    B, max_det, _ = det.shape
    if count.dtype != torch.int32 or count.numel() != B or not count.is_contiguous() or count.device != det.device:
        raise ValueError("count must be a cuda int32 (B,) tensor")
    if scale.dtype != torch.float32 or tuple(scale.shape) != (B, 5) or not scale.is_contiguous() or scale.device != det.device:
        raise ValueError("scale must be a cuda float32 (B, 5) tensor of {gain, pad_x, pad_y, w0, h0} rows")
    return Launch(lib().icaf_scale_detections, (det.data_ptr(), count.data_ptr(), B, max_det, scale.data_ptr(), int(bool(round)), out.data_ptr()),
                  keep=(det, count, scale, out), name=name, nbytes=2 * det.numel() * 4)


class MissrateTable:
    """The label table of a KAIST annotation file on the device (utils.missrate.load_annotations -> missrate_table)."""
    __slots__ = ("box", "height", "occlusion", "ignore", "off", "images", "labels", "max_labels")


def missrate_table(table, device="cuda"):
    """Label table of utils.missrate.load_annotations -> device tensors for missrate_match.  ValueError, before anything is uploaded, when
    an image holds more than 256 labels (one workgroup keeps an image's labels in the registers of a wave) or the arrays disagree."""
    off = np.asarray(table["off"], dtype=np.int64)
    G = len(table["id"])
    if off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != G or (np.diff(off) < 0).any():
        raise ValueError("off must be ascending offsets from 0 to the number of labels, one image at least")
    if np.asarray(table["box"]).shape != (G, 4) or any(len(table[k]) != G for k in ("height", "occlusion", "ignore")):
        raise ValueError("box (G, 4), height, occlusion and ignore (G,) must describe the same labels")
    most = int(np.diff(off).max())
    if most > _lib.MISSRATE_MAX_LABELS:
        raise ValueError(f"image {int(np.diff(off).argmax())} holds {most} labels; icaf_missrate_match takes at most {_lib.MISSRATE_MAX_LABELS}")
    if torch.device(device).type != "cuda":
        raise ValueError("the label table lives on a cuda device (no CPU fallback exists)")
    t = MissrateTable()
    t.box = torch.from_numpy(np.array(table["box"], dtype=np.float64)).to(device)
    t.height = torch.from_numpy(np.array(table["height"], dtype=np.float64)).to(device)
    t.occlusion = torch.from_numpy(np.array(table["occlusion"], dtype=np.int32)).to(device)
    t.ignore = torch.from_numpy(np.array(table["ignore"], dtype=np.int32)).to(device)
    t.off = torch.from_numpy(off.astype(np.int32)).to(device)
    t.images, t.labels, t.max_labels = len(off) - 1, G, most
    return t


def _missrate_store(dt, dt_count):
    if dt.dim() != 3 or dt.shape[2] != 5 or dt.dtype != torch.float64 or not dt.is_contiguous() or not dt.is_cuda:
        raise ValueError("dt must be a contiguous cuda float64 (I, cap, 5) tensor")
    I, cap, _ = dt.shape
    if I < 1 or cap < 1 or cap > _lib.MISSRATE_MAX_DET:
        raise ValueError(f"the detection store holds {I} images x {cap} rows; cap must be in [1, {_lib.MISSRATE_MAX_DET}]")
    if dt_count.dtype != torch.int32 or dt_count.numel() != I or not dt_count.is_contiguous() or dt_count.device != dt.device:
        raise ValueError("dt_count must be a cuda int32 (I,) tensor")
    return I, cap


def missrate_stage(predn, det, count, image_index, image_index_dev, dt, dt_count, name="missrate_stage"):
    """One validation batch into the detection store of the KAIST miss-rate evaluation (icaf_missrate_stage): predn (B, max_det, 4)
    native-space xyxy and det (B, max_det, 6) / count (B,) int32 as match_predictions leaves them; image_index: the HOST ints (store row
    of every image of the batch, distinct, inside the store) that the device int32 tensor `image_index_dev` holds.  Rows
    [0, min(count, cap)) of dt[image_index[b]] become {x1, y1, x2 - x1, y2 - y1 (fp32), score} in fp64, dt_count[image_index[b]] that
    bound.  Validated here, before any device call."""
    if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or not det.is_contiguous() or not det.is_cuda:
        raise ValueError("det must be a contiguous cuda float32 (B, max_det, 6) tensor")
    B, max_det, _ = det.shape
    if tuple(predn.shape) != (B, max_det, 4) or predn.dtype != torch.float32 or not predn.is_contiguous() or predn.device != det.device:
        raise ValueError("predn must be a contiguous cuda float32 (B, max_det, 4) tensor beside det")
    if count.dtype != torch.int32 or count.numel() != B or not count.is_contiguous() or count.device != det.device:
        raise ValueError("count must be a cuda int32 (B,) tensor")
    I, cap = _missrate_store(dt, dt_count)
    if dt.device != det.device:
        raise ValueError("the detection store and the batch must share a device")
    idx = [int(v) for v in image_index]
    if len(idx) != B or len(set(idx)) != B or min(idx) < 0 or max(idx) >= I:
        raise ValueError(f"image_index must name {B} distinct rows of the {I}-image store")
    if image_index_dev.dtype != torch.int32 or not image_index_dev.is_contiguous() or image_index_dev.numel() < B or image_index_dev.device != det.device:
        raise ValueError("image_index_dev must be a cuda int32 tensor of at least B entries")
    return Launch(lib().icaf_missrate_stage, (predn.data_ptr(), det.data_ptr(), count.data_ptr(), image_index_dev.data_ptr(), B, max_det,
                                             dt.data_ptr(), dt_count.data_ptr(), I, cap),
                  keep=(predn, det, count, image_index_dev, dt, dt_count), name=name, nbytes=B * max_det * (20 + 40))


def missrate_outputs(tab, cap, device):
    """Output tensors of missrate_match: order (I, cap) int32, dt_gt (I, cap, 7) int32, dt_ignore (I, cap) uint8, gt_ignore (G,) uint8."""
    return (torch.zeros((tab.images, cap), dtype=torch.int32, device=device),
            torch.full((tab.images, cap, _lib.MISSRATE_SETUPS), -1, dtype=torch.int32, device=device),
            torch.zeros((tab.images, cap), dtype=torch.uint8, device=device), torch.zeros((max(tab.labels, 1),), dtype=torch.uint8, device=device))


def missrate_match(tab, dt, dt_count, order, dt_gt, dt_ignore, gt_ignore, name="missrate_match"):
    """Score sort + ignore-aware greedy matching of every image under the seven KAIST set-ups in one launch (icaf_missrate_match;
    reference evaluation_script.py:46-294).  tab: missrate_table; dt (I, cap, 5) fp64 / dt_count (I,) int32: the detection store; the
    outputs as missrate_outputs allocates them.  Rows at or beyond dt_count[i] (and positions >= 1000) keep what they held."""
    if not isinstance(tab, MissrateTable):
        raise ValueError("tab must come from missrate_table")
    I, cap = _missrate_store(dt, dt_count)
    if I != tab.images:
        raise ValueError(f"the store holds {I} images, the label table {tab.images}")
    for t, shape, dtype, what in ((order, (I, cap), torch.int32, "order"), (dt_gt, (I, cap, _lib.MISSRATE_SETUPS), torch.int32, "dt_gt"),
                                  (dt_ignore, (I, cap), torch.uint8, "dt_ignore")):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dt.device:
            raise ValueError(f"{what} must be a contiguous {dtype} tensor of shape {shape} beside dt")
    if gt_ignore.dtype != torch.uint8 or gt_ignore.numel() < tab.labels or not gt_ignore.is_contiguous() or gt_ignore.device != dt.device:
        raise ValueError("gt_ignore must be a cuda uint8 tensor with one entry per label")
    if tab.off.device != dt.device:
        raise ValueError("the label table and the detection store must share a device")
    return Launch(lib().icaf_missrate_match, (tab.box.data_ptr() or None, tab.height.data_ptr() or None, tab.occlusion.data_ptr() or None,
                                             tab.ignore.data_ptr() or None, tab.off.data_ptr(), I, tab.max_labels, dt.data_ptr(),
                                             dt_count.data_ptr(), cap, order.data_ptr(), dt_gt.data_ptr(), dt_ignore.data_ptr(),
                                             gt_ignore.data_ptr()),
                  keep=(tab, dt, dt_count, order, dt_gt, dt_ignore, gt_ignore), name=name, nbytes=dt.numel() * 8 + I * cap * 33)


def missrate_evaluate(table, dt, dt_count, device="cuda"):
    """Host arrays in, host arrays out: upload the label table and the packed store (utils.missrate.pack_detections), one missrate_match
    launch, download.  Returns a dict of numpy arrays order / dt_gt / dt_ignore / gt_ignore."""
    dt, dt_count = np.array(dt, dtype=np.float64), np.array(dt_count, dtype=np.int32)            # copies: torch wants writable arrays
    if dt.ndim != 3 or dt.shape[2] != 5 or dt_count.shape != (dt.shape[0],) or dt_count.min(initial=0) < 0 or dt_count.max(initial=0) > dt.shape[1]:
        raise ValueError("dt must be (I, cap, 5) and dt_count (I,) with 0 <= dt_count <= cap")
    if not np.isfinite(dt[:, :, 4][np.arange(dt.shape[1])[None, :] < dt_count[:, None]]).all():
        raise ValueError("non-finite detection score")
    tab = missrate_table(table, device)
    dt_d, cnt_d = torch.from_numpy(dt).to(device), torch.from_numpy(dt_count).to(device)
    outs = missrate_outputs(tab, dt.shape[1], dt_d.device)
    missrate_match(tab, dt_d, cnt_d, *outs)(current_stream_ptr())
    order, dt_gt, dt_ignore, gt_ignore = (o.cpu().numpy() for o in outs)
    return {"order": order, "dt_gt": dt_gt, "dt_ignore": dt_ignore, "gt_ignore": gt_ignore[:tab.labels]}


class StatsStore:
    """Data-set-wide store of validation statistics on the device (icaf_stats_stage): one row per detection of the pass, in the order in
    which test.py's host loop concatenates its per-image `stats` (image order, then row order).  mask (capacity,) int16 holds the TP flags
    (bit t = threshold t), conf (capacity,) fp32, cls (capacity,) int32; the cursor and the any_tp flag live on the device, so staging a
    batch reads nothing back.  `capacity` is the host's upper bound of the rows (images x max_det): the store cannot overflow."""

    def __init__(self, capacity, T, device="cuda"):
        capacity, T = int(capacity), int(T)
        if T < 1 or T > _lib.STATS_MAX_T:                 # the library's own limits (it refuses them too), before anything is allocated
            raise _lib.IcafError(f"icaf_stats_stage: T must be in [1, {_lib.STATS_MAX_T}] ({T})")
        if capacity < 1 or capacity > _lib.STATS_MAX_ROWS:
            raise _lib.IcafError(f"icaf_stats_stage: the store's capacity must be in [1, {_lib.STATS_MAX_ROWS}] rows ({capacity})")
        if torch.device(device).type != "cuda":
            raise ValueError("the statistics store lives on a cuda device (no CPU fallback exists)")
        self.capacity, self.T = capacity, T
        self.mask = torch.zeros((capacity,), dtype=torch.int16, device=device)
        self.conf = torch.zeros((capacity,), dtype=torch.float32, device=device)
        self.cls = torch.zeros((capacity,), dtype=torch.int32, device=device)
        self.state = torch.zeros((2,), dtype=torch.int32, device=device)           # cursor, any_tp
        self._rows = None

    def stage(self, correct, det, count, stream_ptr=None):
        """Append one batch: correct (B, max_det, T) uint8, det (B, max_det, 6) fp32, count (B,) int32.  One launch, nothing is read back."""
        stats_stage(correct, det, count, self.mask, self.conf, self.cls, self.state[0:1], self.state[1:2])(
            stream_ptr if stream_ptr is not None else current_stream_ptr())
        self._rows = None

    def rows(self):
        """The number of rows staged so far (reads the cursor: one synchronisation); raises if a batch did not fit."""
        if self._rows is None:
            self._rows = int(self.state[0].item())
        if self._rows > self.capacity:
            raise _lib.IcafError(f"the statistics store holds {self.capacity} rows, {self._rows} were staged")
        return self._rows

    def any_tp(self):
        return bool(self.state[1].item())

    def to_host(self):
        """(correct (n, T) bool, conf (n,) fp32, cls (n,) int32) as numpy: what the host loop's concatenated `stats` hold."""
        n = self.rows()
        mask = self.mask[:n].cpu().numpy().view(np.uint16)
        return ((mask[:, None] >> np.arange(self.T, dtype=np.uint16)[None, :]) & 1).astype(bool), self.conf[:n].cpu().numpy(), self.cls[:n].cpu().numpy()


def stats_stage(correct, det, count, store_mask, store_conf, store_cls, cursor, any_tp, name="stats_stage"):
    """One validation batch into the statistics store (icaf_stats_stage).  Shapes and dtypes are validated here; T and the capacity are
    refused by the library, before any launch."""
    if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or not det.is_contiguous() or not det.is_cuda:
        raise ValueError("det must be a contiguous cuda float32 (B, max_det, 6) tensor")
    B, max_det, _ = det.shape
    if correct.dim() != 3 or tuple(correct.shape[:2]) != (B, max_det) or correct.dtype != torch.uint8 or not correct.is_contiguous() or correct.device != det.device:
        raise ValueError("correct must be a contiguous cuda uint8 (B, max_det, T) tensor beside det")
    if count.dtype != torch.int32 or count.numel() != B or not count.is_contiguous() or count.device != det.device:
        raise ValueError("count must be a cuda int32 (B,) tensor")
    cap = store_mask.numel()
    for t, dtype, what in ((store_mask, torch.int16, "store_mask"), (store_conf, torch.float32, "store_conf"), (store_cls, torch.int32, "store_cls")):
        if t.dim() != 1 or t.numel() != cap or t.dtype != dtype or not t.is_contiguous() or t.device != det.device:
            raise ValueError(f"{what} must be a contiguous {dtype} (capacity,) tensor beside det")
    for t, what in ((cursor, "cursor"), (any_tp, "any_tp")):
        if t.numel() != 1 or t.dtype != torch.int32 or t.device != det.device:
            raise ValueError(f"{what} must be one cuda int32 beside det")
    return Launch(lib().icaf_stats_stage, (correct.data_ptr(), det.data_ptr(), count.data_ptr(), B, max_det, correct.shape[2], store_mask.data_ptr(),
                                          store_conf.data_ptr(), store_cls.data_ptr(), cap, cursor.data_ptr(), any_tp.data_ptr()),
                  keep=(correct, det, count, store_mask, store_conf, store_cls, cursor, any_tp), name=name,
                  nbytes=B * max_det * (correct.shape[2] + 24 + 10))


def ap_workspace(n, T, device):
    """(workspace uint8 tensor, byte offset of the tpc table int32 [T][n]) for ap_per_class_device (icaf_ap_workspace_bytes)."""
    nbytes, tpc_off = C.c_size_t(0), C.c_size_t(0)
    check(lib().icaf_ap_workspace_bytes(int(n), int(T), C.byref(nbytes), C.byref(tpc_off)), "icaf_ap_workspace_bytes")
    return torch.empty((nbytes.value + 256,), dtype=torch.uint8, device=device), tpc_off.value


def ap_per_class_device(stats, unique_classes, n_l, T=None, want_perm=False, want_tpc=False, stream_ptr=None):
    """ap_per_class on the device (icaf_ap_per_class; reference utils/metrics.py:18-82) with a DEFINED order: class ascending, confidence
    descending, equal confidences in arrival order.  stats: a StatsStore, or (mask int16 (>= n,), conf fp32, cls int32, n) device tensors
    with T given; unique_classes / n_l: the sorted classes of the labels and their label counts (host sequences or numpy).
    Returns a dict of numpy arrays: ap (nc, T), p / r / f1 (nc, 1000) fp64, best (the argmax index), tp / fp / fn (nc,), and on request
    perm (n,) (sorted position -> arrival index) and tpc (T, n) (inclusive TP count inside the class, by sorted position)."""
    if isinstance(stats, StatsStore):
        mask, conf, cls, n, T = stats.mask, stats.conf, stats.cls, stats.rows(), stats.T
    else:
        mask, conf, cls, n = stats
        n = int(n)
        if T is None:
            raise ValueError("T (the number of IoU thresholds) must be given with plain tensors")
    if mask.dtype != torch.int16 or conf.dtype != torch.float32 or cls.dtype != torch.int32 or not mask.is_cuda:
        raise ValueError("mask / conf / cls must be cuda int16 / float32 / int32 tensors")
    if n < 0 or min(mask.numel(), conf.numel(), cls.numel()) < n or not (mask.is_contiguous() and conf.is_contiguous() and cls.is_contiguous()):
        raise ValueError(f"mask / conf / cls must be contiguous and hold the {n} rows")
    dev = mask.device
    uc = np.ascontiguousarray(np.asarray(unique_classes).astype(np.int32))
    nl = np.ascontiguousarray(np.asarray(n_l).astype(np.int32))
    nc = int(uc.shape[0])
    if uc.ndim != 1 or nl.shape != uc.shape or (nc > 1 and (np.diff(uc) <= 0).any()):
        raise ValueError("unique_classes must be ascending and distinct, n_l their label counts")
    uc_d, nl_d = torch.from_numpy(uc).to(dev), torch.from_numpy(nl).to(dev)
    T = int(T)
    ws, tpc_off = ap_workspace(n, T, dev) if 1 <= T <= _lib.STATS_MAX_T and 0 <= n <= _lib.STATS_MAX_ROWS else (torch.empty((512,), dtype=torch.uint8, device=dev), 0)
    shift = (-ws.data_ptr()) % 256
    ap = torch.zeros((max(nc, 1), max(T, 1)), dtype=torch.float64, device=dev)
    p, r, f1 = (torch.zeros((max(nc, 1), _lib.AP_CURVE_POINTS), dtype=torch.float64, device=dev) for _ in range(3))
    best = torch.zeros((1,), dtype=torch.int32, device=dev)
    report = torch.zeros((max(nc, 1), 3), dtype=torch.float64, device=dev)
    perm = torch.zeros((max(n, 1),), dtype=torch.int32, device=dev) if want_perm else None
    check(lib().icaf_ap_per_class(mask.data_ptr() or None, conf.data_ptr() or None, cls.data_ptr() or None, n, T, uc_d.data_ptr() or None,
                                 nl_d.data_ptr() or None, nc, ap.data_ptr(), p.data_ptr(), r.data_ptr(), f1.data_ptr(), best.data_ptr(),
                                 report.data_ptr(), perm.data_ptr() if perm is not None else None, ws.data_ptr() + shift, ws.numel() - shift,
                                 stream_ptr if stream_ptr is not None else current_stream_ptr()), "icaf_ap_per_class")
    rep = report[:nc].cpu().numpy()
    out = {"ap": ap[:nc, :T].cpu().numpy(), "p": p[:nc].cpu().numpy(), "r": r[:nc].cpu().numpy(), "f1": f1[:nc].cpu().numpy(),
           "best": int(best.item()), "tp": rep[:, 0].copy(), "fp": rep[:, 1].copy(), "fn": rep[:, 2].copy()}
    if want_perm:
        out["perm"] = perm[:n].cpu().numpy()
    if want_tpc:
        out["tpc"] = ws[shift + tpc_off:shift + tpc_off + 4 * T * max(n, 1)].view(torch.int32).view(T, max(n, 1))[:, :n].cpu().numpy()
    return out


def confusion_matrix(predn, det, count, labels, label_off, matrix, conf=0.25, iou_thres=0.45, name="confusion_matrix"):
    """One batch into the confusion matrix (icaf_confusion_matrix; reference utils/metrics.py:121-159): predn (B, max_det, 4) native-space
    boxes as match_predictions writes them, det (B, max_det, 6), count (B,) int32, labels (L, 5) fp32 [cls, x1, y1, x2, y2] sorted by image,
    label_off (B + 1,) int32, matrix (nc + 1, nc + 1) int32 on the device (accumulated).  IoU ties: lowest label, then lowest detection."""
    if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or not det.is_contiguous() or not det.is_cuda:
        raise ValueError("det must be a contiguous cuda float32 (B, max_det, 6) tensor")
    B, max_det, _ = det.shape
    if tuple(predn.shape) != (B, max_det, 4) or predn.dtype != torch.float32 or not predn.is_contiguous() or predn.device != det.device:
        raise ValueError("predn must be a contiguous cuda float32 (B, max_det, 4) tensor beside det")
    if count.dtype != torch.int32 or count.numel() != B or not count.is_contiguous() or count.device != det.device:
        raise ValueError("count must be a cuda int32 (B,) tensor")
    if label_off.dtype != torch.int32 or label_off.numel() != B + 1 or not label_off.is_contiguous() or label_off.device != det.device:
        raise ValueError("label_off must be a cuda int32 (B + 1,) tensor")
    if labels.dtype != torch.float32 or not labels.is_contiguous() or (labels.numel() and (labels.dim() != 2 or labels.shape[1] != 5 or labels.device != det.device)):
        raise ValueError("labels must be a contiguous cuda float32 (L, 5) tensor")
    if matrix.dim() != 2 or matrix.shape[0] != matrix.shape[1] or matrix.shape[0] < 2 or matrix.dtype != torch.int32 or not matrix.is_contiguous() or matrix.device != det.device:
        raise ValueError("matrix must be a contiguous cuda int32 (nc + 1, nc + 1) tensor")
    return Launch(lib().icaf_confusion_matrix, (predn.data_ptr(), det.data_ptr(), count.data_ptr(), B, max_det, labels.data_ptr() if labels.numel() else None,
                                               label_off.data_ptr(), matrix.shape[0] - 1, float(conf), float(iou_thres), matrix.data_ptr()),
                  keep=(predn, det, count, labels, label_off, matrix), name=name, nbytes=B * max_det * 40)


def letterbox_direct(on=True):
    """Force icaf_letterbox_frames (and its YUV, warp and Y16 siblings) onto its direct path (no LDS staging) inside a `with`: an A/B knob of the library, it changes no result."""
    return _caller_knob("letterbox_direct", on)


def area_direct(on=True):
    """Force the area rows of icaf_resize_frames onto their direct path (no LDS) inside a `with`: an A/B knob of the library, it changes no result."""
    return _caller_knob("area_direct", on)


# ------------------------------------------------------------------------------------------------------------
# graph capture + events
# ------------------------------------------------------------------------------------------------------------
def match_predictions(det, count, labels, label_off, iouv, scale=None, predn=None, stream_ptr=None, max_labels=None):
    """TP flags of every detection at every IoU threshold on the device (icaf_match_predictions; reference
    test.py:196-230).  det (B, max_det, 6) / count (B,) int32: the NMS output block; labels (L, 5) fp32 [cls, x1, y1,
    x2, y2] in native image space sorted by image, label_off (B + 1,) int32; scale (B, 5) fp32 [gain, pad_x, pad_y, w0,
    h0] or None; iouv (T,) fp32.  Returns uint8 (B, max_det, T); rows >= count[b] are unspecified.  max_labels: the host's
    maximum of labels per image (it built label_off); when given, label_off is not read back."""
    B, max_det, six = det.shape
    assert six == 6 and det.dtype == torch.float32 and det.is_contiguous() and count.dtype == torch.int32
    assert label_off.dtype == torch.int32 and label_off.numel() == B + 1 and iouv.dtype == torch.float32
    assert labels.dtype == torch.float32 and labels.is_contiguous() and (labels.numel() == 0 or labels.shape[1] == 5)
    T = iouv.numel()
    correct = torch.empty((B, max_det, T), dtype=torch.uint8, device=det.device)
    if max_labels is None:
        off = label_off.cpu()
        max_l = int((off[1:] - off[:-1]).max()) if B else 0
    else:
        max_l = int(max_labels)
    st = lib().icaf_match_predictions(det.data_ptr(), count.data_ptr(), B, max_det, labels.data_ptr() if labels.numel() else None,
                                      label_off.data_ptr(), max_l, scale.data_ptr() if scale is not None else None, iouv.data_ptr(), T,
                                      correct.data_ptr(), predn.data_ptr() if predn is not None else None,
                                      stream_ptr if stream_ptr is not None else current_stream_ptr())
    check(st, "icaf_match_predictions")
    return correct


class Graph:
    def __init__(self):
        self.exec = C.c_void_p(None)

    def capture(self, stream_ptr, fn):
        check(lib().icaf_graph_begin(stream_ptr), "graph_begin")
        try:
            fn()
        finally:
            st = lib().icaf_graph_end(stream_ptr, C.byref(self.exec))
        check(st, "graph_end")

    def launch(self, stream_ptr):
        check(lib().icaf_graph_launch(self.exec, stream_ptr), "graph_launch")

    def __del__(self):
        try:
            if self.exec:
                lib().icaf_graph_destroy(self.exec)
        except Exception:
            pass


class Event:
    def __init__(self):
        self.ev = C.c_void_p(None)
        check(lib().icaf_event_create(C.byref(self.ev)), "event_create")

    def record(self, stream_ptr):
        check(lib().icaf_event_record(self.ev, stream_ptr), "event_record")

    def wait(self, stream_ptr):
        """Make `stream_ptr` wait for this event (inside a capture: adds a dependency edge / joins the capture)."""
        check(lib().icaf_stream_wait_event(stream_ptr, self.ev), "stream_wait_event")

    def elapsed_ms(self, stop):
        ms = C.c_float(0)
        check(lib().icaf_event_elapsed_ms(self.ev, stop.ev, C.byref(ms)), "event_elapsed")
        return ms.value

    def __del__(self):
        try:
            lib().icaf_event_destroy(self.ev)
        except Exception:
            pass


def device_info():
    cu, lds = C.c_int(0), C.c_int(0)
    buf = C.create_string_buffer(64)
    check(lib().icaf_device_info(C.byref(cu), C.byref(lds), buf, 64), "device_info")
    return {"cu_count": cu.value, "lds_bytes": lds.value, "arch": buf.value.decode()}
