"""Boundary and untouched-memory tests of the Detect head (detect.hip): the per-pixel kernels detect_pixel_kernel<3, {6, 8, 14}> (path P), the
general detect_decode_kernel<true> (path E, forced with the knob detect_elementwise and confirmed through ops.detect_decode_kernel) and the
DetectEpi epilogue of detect_conv_kernel (path F, ops.detect_conv).

Reference: tests/detect_nms_ref.py decode64, a float64 statement of the reference's eval decode; z within rtol 1e-6 / atol 1e-5 of it, in
bits where the fp32 value follows exactly (logit >= 17, logit <= -104); raw and logits are copies of the input, bit for bit.  P and E must
give the same bits wherever P accepts the case, F the bits of icaf_conv2d followed by P.

Every output lives in a numerics.PoisonedFlat: z and logits hold three levels' rows of which ONE is launched (first, middle or last), raw is
its own buffer; after the launch every element outside the level's rows and every guard holds the sentinel (NaN, then a finite pattern),
every element inside does not.  The input map is a channel slice of a wider buffer with NaN in all padding; path F reads a 16-bit map with
NaN behind cin and pixel counts that are no multiple of the 128-pixel tile.  Both decode kernels take a second trip through their
grid-stride loop in one case each.  A closing test fails if a kernel choice of detect_select was never seen.

Left out: detect_decode_kernel<false> (64-bit index arithmetic) needs 2^31 output elements — 8 GB of z alone."""
import contextlib
import math
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detect_nms_ref as R                              # noqa: E402
import numerics as nm                                   # noqa: E402
from numerics import BF16, F16, F32                     # noqa: E402
from helpers import lib_option                          # noqa: E402
from icafusion_amd import ops                           # noqa: E402
from icafusion_amd._lib import IcafError                # noqa: E402

DEV = "cuda:0"
NA = 3
PADS = {"P": ((2, 0), (2, 4)), "E": ((1, 0), (0, 3))}   # (floats before, floats behind) the pixel's na * no values: ldp - na * no = 2, 6 / 1, 3
REACH = {}                                              # reason -> kernel ops.detect_decode_kernel reported (0 per pixel, 1 per element)
WANT_REACH = {"no6": 0, "no8": 0, "no14": 0, "na": 1, "no": 1, "odd-ldp": 1, "z-4byte": 1, "raw-4byte": 1, "knob": 1}
assert R.SENTINELS[0] == nm.NAN_BITS[F32]


def run(launch):
    launch(ops.current_stream_ptr())
    torch.cuda.synchronize()


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32))


def signed(bits):
    return bits - (1 << 32) if bits >= (1 << 31) else bits      # numerics.bits views fp32 as int32


class Outputs:
    """z and logits with room for three levels (the launched one at position pos), raw for the launched level; all hold the sentinel"""

    def __init__(self, B, ny, nx, no, pos, sentinel, na=NA, z_guard=64, raw_guard=64):
        self.rows_total, self.off = R.three_levels(pos, na, ny, nx)
        self.n, self.sentinel = na * ny * nx, sentinel
        self.z = nm.PoisonedFlat((B, self.rows_total, no), F32, DEV, signed(sentinel), guard=z_guard)
        self.lg = nm.PoisonedFlat((B, self.rows_total, no - 5), F32, DEV, signed(sentinel))
        self.raw = nm.PoisonedFlat((B, na, ny, nx, no), F32, DEV, signed(sentinel), guard=raw_guard)

    def untouched(self, what=""):
        for t in (self.z, self.lg, self.raw):
            t.assert_outside_intact(what)
            assert bool((nm.bits(t.view) == signed(self.sentinel)).all()), f"{what}: a refused or absent output was written"

    def check(self, p, na, no, stride, anchors, what, use_raw=True, use_lg=True):
        """p: the level's map as numpy (B, ny, nx, na * no)"""
        for t in (self.z, self.lg, self.raw):
            t.assert_outside_intact(what)
        ratio = R.check_level(self.z.view.cpu().numpy(), self.sentinel, self.off, p, na, no, stride, anchors, what)
        _, lg, raw = R.decode64(p, na, no, stride, anchors)
        got_lg, got_raw = R.u32(self.lg.view.cpu().numpy()), R.u32(self.raw.view.cpu().numpy())
        want_lg = np.full(got_lg.shape, self.sentinel, np.uint32)
        if use_lg:
            want_lg[:, self.off:self.off + self.n] = R.u32(lg)
        assert np.array_equal(got_lg, want_lg), f"{what}: logits are not the input's class scores inside the level and the sentinel outside"
        assert np.array_equal(got_raw, R.u32(raw) if use_raw else np.full(got_raw.shape, self.sentinel, np.uint32)), f"{what}: raw"
        return ratio

    def same_bits(self, other, what):
        for a, b, name in ((self.z, other.z, "z"), (self.lg, other.lg, "logits"), (self.raw, other.raw, "raw")):
            nm.assert_same_bits(a.view, b.view, f"{what} {name}")


def padded(p, pad):
    """numpy (B, ny, nx, C) -> the device view of it inside a buffer with pad[0] floats before and pad[1] behind every pixel, all NaN"""
    return nm.Poisoned(p.shape[:3], p.shape[3], F32, DEV, signed(nm.NAN_BITS[F32]), torch.from_numpy(p).to(DEV), lo=pad[0], hi=pad[1])


def decode(path, pv, out, na, no, stride, anchors, use_raw=True, use_lg=True, reason=None):
    """one icaf_detect_decode launch on path P or E; the kernel the library reports is checked against the path and noted"""
    with (lib_option("detect_elementwise", 1) if path == "E" and reason in (None, "knob") else contextlib.nullcontext()):
        raw = out.raw.view if use_raw else None
        k = ops.detect_decode_kernel(pv.view, out.z.view, raw, na, no)
        assert k == (0 if path == "P" else 1), f"path {path}: the library chose kernel {k}"
        if reason:
            REACH[reason] = k
        run(ops.detect_decode(pv.view, out.z.view, out.lg.view if use_lg else None, raw, na, no, out.off, stride, anchors))
    pv.assert_outside_intact(f"input map, path {path}")


# ------------------------------------------------------------------------------------------------------------------------------------
# (a, b, c, d) the logit sweep into three-level buffers, both decode kernels, both sentinels
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("nc", R.SWEEP_NC)
def test_logit_sweep(nc, pos):
    """every listed logit at every o index and anchor: no NaN, the exact values in bits, the rest within tolerance; rows of the other two
    levels and all guards intact; P and E give the same bits (no = 7 has no per-pixel kernel: E alone, chosen by the library itself)"""
    no = nc + 5
    B, ny, nx = R.SWEEP_SHAPE
    p = R.sweep_map(B, ny, nx, NA, no)
    stride, anchors = R.LEVELS[pos]
    for s, sentinel in enumerate(R.SENTINELS):
        outs = {}
        for path in (("P", "E") if no in (6, 8, 14) else ("E",)):
            reason = (f"no{no}" if path == "P" else None) if no in (6, 8, 14) else "no"      # ("knob" is noted by test_knob_alone_...)
            what = f"sweep nc {nc} level {pos} path {path} sentinel {sentinel:#x}"
            outs[path] = out = Outputs(B, ny, nx, no, pos, sentinel)
            decode(path, padded(p, PADS[path][(s + pos) % 2]), out, NA, no, stride, anchors, reason=reason)
            assert not bool(torch.isnan(out.z.view[:, out.off:out.off + out.n]).any()), f"{what}: NaN in z"
            print(f"{what}: largest err / tolerance {out.check(p, NA, no, stride, anchors, what):.3f}")
        if len(outs) == 2:
            outs["P"].same_bits(outs["E"], f"sweep nc {nc} level {pos} P vs E")


def test_nan_logits_stay_where_they_are():
    """NaN in z, raw and logits exactly at the elements whose logit is NaN, on both kernels, and the two in the same bits"""
    no = 8
    p, m = R.nan_map(2, 5, 7, NA, no)
    stride, anchors = R.LEVELS[2]
    for sentinel in R.SENTINELS:
        outs = {}
        for path in ("P", "E"):
            outs[path] = out = Outputs(2, 5, 7, no, 1, sentinel)
            decode(path, padded(p, PADS[path][0]), out, NA, no, stride, anchors)
            out.check(p, NA, no, stride, anchors, f"nan path {path}")                   # (NaN in z exactly where decode64 has it; raw, logits in bits)
            level = out.z.view[:, out.off:out.off + out.n]
            assert int(torch.isnan(level).sum()) == int(m.sum()) and int(torch.isnan(out.raw.view).sum()) == int(m.sum())
        outs["P"].same_bits(outs["E"], f"nan sentinel {sentinel:#x} P vs E")


LEVEL_SHAPES = [(2, 12, 20, 1), (3, 7, 9, 3), (2, 33, 37, 9), (1, 1, 1, 3), (5, 1, 3, 9), (2, 19, 27, 1)]      # B, ny, nx, nc


@pytest.mark.parametrize("B,ny,nx,nc", LEVEL_SHAPES)
def test_random_levels_and_path_identity(B, ny, nx, nc):
    """Gaussian logits with a sixteenth of extreme values, several workgroups, ragged last one: both kernels against decode64 and each other"""
    no = nc + 5
    p = R.random_map(B, ny, nx, NA, no, seed=B * 1000 + ny * nx + nc)
    for pos, sentinel in ((0, R.SENTINELS[0]), (2, R.SENTINELS[1])):
        stride, anchors = R.LEVELS[pos]
        outs = {}
        for path in ("P", "E"):
            outs[path] = Outputs(B, ny, nx, no, pos, sentinel)
            decode(path, padded(p, PADS[path][pos // 2]), outs[path], NA, no, stride, anchors)
            outs[path].check(p, NA, no, stride, anchors, f"random {B}x{ny}x{nx} nc {nc} path {path}")
        outs["P"].same_bits(outs["E"], f"random {B}x{ny}x{nx} nc {nc} P vs E")


# ------------------------------------------------------------------------------------------------------------------------------------
# (g) every reason for which detect_select leaves the per-pixel kernels, one at a time and without the knob
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reason", ["na", "odd-ldp", "z-4byte", "raw-4byte"])
def test_fallback_reasons(reason):
    """a level the per-pixel kernel would take but for ONE property: the library reports the per-element kernel, and it is right"""
    B, ny, nx, no = 2, 5, 7, 8
    na = 2 if reason == "na" else NA
    anchors = [21.0, 35.0, 373.0, 326.0] if reason == "na" else R.ANCHORS3[2]
    p = R.random_map(B, ny, nx, na, no, seed=len(reason))
    for sentinel in R.SENTINELS:
        out = Outputs(B, ny, nx, no, 1, sentinel, na=na, z_guard=63 if reason == "z-4byte" else 64, raw_guard=63 if reason == "raw-4byte" else 64)
        assert (out.z.view.data_ptr() % 8 == 4) == (reason == "z-4byte") and (out.raw.view.data_ptr() % 8 == 4) == (reason == "raw-4byte")
        decode("E", padded(p, (2, 1) if reason == "odd-ldp" else (2, 0)), out, na, no, 33.0, anchors, reason=reason)
        out.check(p, na, no, 33.0, anchors, f"fallback {reason}")


def test_knob_alone_selects_the_element_kernel():
    """a level the per-pixel kernel takes — 3 anchors, no = 8, an even pixel stride, 8-byte aligned map, z and raw — runs the per-element
    kernel for no reason but the knob: the same buffers report kernel 0 without it; the two results are the same bits"""
    B, ny, nx, no = 2, 5, 7, 8
    p = R.random_map(B, ny, nx, NA, no, seed=4)
    stride, anchors = R.LEVELS[1]
    outs = {}
    for path in ("P", "E"):
        pv = padded(p, (2, 0))
        assert pv.view.data_ptr() % 8 == 0 and pv.view.stride(2) % 2 == 0
        outs[path] = Outputs(B, ny, nx, no, 1, R.SENTINELS[0])
        assert ops.detect_decode_kernel(pv.view, outs[path].z.view, outs[path].raw.view, NA, no) == 0       # knob off: the pixel kernel
        decode(path, pv, outs[path], NA, no, stride, anchors, reason="knob" if path == "E" else None)
        outs[path].check(p, NA, no, stride, anchors, f"knob alone, path {path}")
    outs["P"].same_bits(outs["E"], "knob alone, P vs E")


# ------------------------------------------------------------------------------------------------------------------------------------
# (d, F) the level in one launch
# ------------------------------------------------------------------------------------------------------------------------------------
FUSED_SHAPES = [(1, 1, 1, 64, 1), (1, 1, 127, 128, 3), (1, 3, 43, 512, 9), (1, 389, 1, 64, 9), (6, 80, 80, 128, 3)]        # B, ny, nx, cin, nc
#                M = 1 and 127: fewer pixel tiles than workgroups; 129 and 389: a ragged last tile; 38 400: 300 tiles, more than there are CUs


class Fused:
    """operands of one icaf_detect_conv level: a 16-bit map with NaN around its cin channels, packed weights and bias"""

    def __init__(self, B, ny, nx, cin, nc, dt, seed):
        self.B, self.ny, self.nx, self.cin, self.no, self.dt = B, ny, nx, cin, nc + 5, dt
        x = rnd((B, ny, nx, cin), seed)
        self.x = nm.Poisoned((B, ny, nx), cin, dt, DEV, nm.NAN_BITS[dt], x.to(dt).to(DEV), lo=8, hi=8)
        w = rnd((NA * self.no, cin, 1, 1), seed + 1, 2.0 / math.sqrt(cin))
        self.wp, self.kp = ops.pack_conv_weight(w.to(DEV), dt)
        self.bp = ops.pack_bias(rnd((NA * self.no,), seed + 2).to(DEV), NA * self.no)
        assert ops.detect_conv_ok(self.x.view, NA, self.no, cin)

    def launch(self, out, stride, anchors, use_raw=True, use_lg=True, off=None):
        return ops.detect_conv(self.x.view, self.wp, self.kp, self.bp, out.z.view, out.lg.view if use_lg else None,
                               out.raw.view if use_raw else None, NA, self.no, out.off if off is None else off, stride, anchors, self.cin)

    def conv_map(self):
        """the level's fp32 map as icaf_conv2d writes it, dense enough for the per-pixel kernel (an even pixel stride)"""
        c = NA * self.no
        pmap = torch.zeros((self.B, self.ny, self.nx, (c + 3) // 4 * 4), dtype=torch.float32, device=DEV)[..., :c]
        run(ops.conv2d(self.x.view, self.wp, self.kp, self.bp, pmap, 1, 1, 1, 1, 0, 0, self.cin, c, ops.ACT_NONE))
        return pmap


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(FUSED_SHAPES)), ids=[f"M{b * h * w}-c{c}-nc{n}" for b, h, w, c, n in FUSED_SHAPES])
def test_fused_level(i, dt):
    """F = icaf_conv2d followed by P in bits, within tolerance of decode64 on that map, and nothing outside the level's rows is written"""
    B, ny, nx, cin, nc = FUSED_SHAPES[i]
    f = Fused(B, ny, nx, cin, nc, dt, seed=300 + i)
    pmap = f.conv_map()
    p = pmap.cpu().numpy()
    assert np.isfinite(p).all()
    pos = i % 3
    stride, anchors = R.LEVELS[pos]
    for sentinel in R.SENTINELS:
        what = f"fused M {B * ny * nx} cin {cin} nc {nc} {dt} sentinel {sentinel:#x}"
        got, ref = Outputs(B, ny, nx, f.no, pos, sentinel), Outputs(B, ny, nx, f.no, pos, sentinel)
        run(f.launch(got, stride, anchors))
        f.x.assert_outside_intact(what)
        got.check(p, NA, f.no, stride, anchors, what)
        run(ops.detect_decode(pmap, ref.z.view, ref.lg.view, ref.raw.view, NA, f.no, ref.off, stride, anchors))
        got.same_bits(ref, what)


# ------------------------------------------------------------------------------------------------------------------------------------
# (e) null outputs
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_raw,use_lg", [(False, True), (True, False), (False, False)], ids=["no-raw", "no-logits", "neither"])
@pytest.mark.parametrize("path", ["P", "E", "F"])
def test_null_outputs(path, use_raw, use_lg):
    """z equals the full call in bits; the tensors not passed (allocated and poisoned all the same) stay as they were"""
    B, ny, nx, nc, pos = 2, 9, 15, 3, 1
    no = nc + 5
    stride, anchors = R.LEVELS[pos]
    sentinel = R.SENTINELS[0]
    full, part = Outputs(B, ny, nx, no, pos, sentinel), Outputs(B, ny, nx, no, pos, sentinel)
    if path == "F":
        f = Fused(B, ny, nx, 128, nc, BF16, seed=77)
        p = f.conv_map().cpu().numpy()
        run(f.launch(full, stride, anchors))
        run(f.launch(part, stride, anchors, use_raw, use_lg))
    else:
        p = R.random_map(B, ny, nx, NA, no, seed=78)
        decode(path, padded(p, PADS[path][0]), full, NA, no, stride, anchors)
        decode(path, padded(p, PADS[path][0]), part, NA, no, stride, anchors, use_raw, use_lg)
    full.check(p, NA, no, stride, anchors, f"null {path} full")
    part.check(p, NA, no, stride, anchors, f"null {path} raw={use_raw} logits={use_lg}", use_raw, use_lg)
    nm.assert_same_bits(part.z.view, full.z.view, f"null {path}: z")


# ------------------------------------------------------------------------------------------------------------------------------------
# (f) the second trip of the grid-stride loops
# ------------------------------------------------------------------------------------------------------------------------------------
def test_element_kernel_second_trip():
    """2 150 400 elements > 8192 workgroups x 256 threads, against decode64"""
    B, ny, nx, no = 8, 80, 80, 14
    assert B * NA * ny * nx * no > 8192 * 256
    p = R.random_map(B, ny, nx, NA, no, seed=8)
    stride, anchors = R.LEVELS[2]
    out = Outputs(B, ny, nx, no, 1, R.SENTINELS[0])
    decode("E", padded(p, (1, 0)), out, NA, no, stride, anchors)
    out.check(p, NA, no, stride, anchors, "element kernel, second trip")


def test_pixel_kernel_second_trip():
    """2 113 536 pixels > 8192 x 256, raw and logits null; compared on the device, bit for bit, with the element kernel on the same buffers
    (which test_element_kernel_second_trip and the sweeps hold to decode64)"""
    B, ny, nx, no = 2, 1024, 1032, 6
    assert B * ny * nx > 8192 * 256
    p = torch.randn((B, ny, nx, NA * no), dtype=torch.float32, device=DEV) * 4.0
    stride, anchors = R.LEVELS[2]
    zs = []
    for path in ("P", "E"):
        z = torch.empty((B, NA * ny * nx, no), dtype=torch.float32, device=DEV)
        nm.bits(z).fill_(signed(R.SENTINELS[0]))
        with (lib_option("detect_elementwise", 1) if path == "E" else contextlib.nullcontext()):
            assert ops.detect_decode_kernel(p, z, None, NA, no) == (0 if path == "P" else 1)
            run(ops.detect_decode(p, z, None, None, NA, no, 0, stride, anchors))
        assert not bool((nm.bits(z) == signed(R.SENTINELS[0])).any()), f"path {path}: elements never written"
        zs.append(z)
    assert torch.equal(nm.bits(zs[0]), nm.bits(zs[1]))
    assert float(zs[0][..., 2].max()) > 4 * 100.0 and float(zs[0][..., 4].min()) >= 0.0


# ------------------------------------------------------------------------------------------------------------------------------------
# (h) refusals: raised by the host-side argument checks, before any launch
# ------------------------------------------------------------------------------------------------------------------------------------
def test_decode_refusals_leave_the_outputs_alone():
    B, ny, nx, no = 2, 5, 7, 8
    p = padded(R.random_map(B, ny, nx, NA, no, seed=1), (2, 0))
    stride, anchors = R.LEVELS[0]
    for pos in (1, 2):                                     # one row too many for z, behind the middle and behind the last level
        out = Outputs(B, ny, nx, no, pos, R.SENTINELS[0])
        over = out.rows_total - out.n + 1
        with pytest.raises(IcafError, match="icaf_detect_decode: level does not fit in z"):
            run(ops.detect_decode(p.view, out.z.view, out.lg.view, out.raw.view, NA, no, over, stride, anchors))
        out.untouched("level does not fit in z")
    out = Outputs(B, ny, nx, no, 1, R.SENTINELS[0])
    narrow = torch.zeros((B, ny, nx, NA * no - 2), dtype=torch.float32, device=DEV)       # a pixel stride below na * no
    with pytest.raises(IcafError, match="icaf_detect_decode: bad na/no/ldp"):
        run(ops.detect_decode(narrow, out.z.view, out.lg.view, out.raw.view, NA, no, out.off, stride, anchors))
    out.untouched("ldp < na * no")


def test_fused_refusals_leave_the_outputs_alone():
    B, ny, nx, nc = 2, 5, 7, 3
    f = Fused(B, ny, nx, 128, nc, BF16, seed=2)
    stride, anchors = R.LEVELS[0]

    def refused(out, what, message, mutate=None, **kw):
        """the launch raises with `message` — the check of icaf_detect_conv that is meant, not an earlier one — and writes nothing"""
        launch = f.launch(out, stride, anchors, **kw)
        if mutate:
            mutate(next(k for k in launch.keep if isinstance(k, ops.ConvArgs)))
        with pytest.raises(IcafError, match=re.escape(message)):
            run(launch)
        out.untouched(what)
        f.x.assert_outside_intact(what)

    out = Outputs(B, ny, nx, f.no, 2, R.SENTINELS[0])
    refused(out, "level does not fit in z", "icaf_detect_conv: level does not fit in z", off=out.rows_total - out.n + 1)
    refused(Outputs(B, ny, nx, f.no, 1, R.SENTINELS[0], z_guard=63), "z 4-byte aligned", "icaf_detect_conv: z / raw must be 8-byte aligned")
    refused(Outputs(B, ny, nx, f.no, 1, R.SENTINELS[0], raw_guard=63), "raw 4-byte aligned", "icaf_detect_conv: z / raw must be 8-byte aligned")

    def other_cout(a):
        a.Cout = NA * f.no - 1
    refused(Outputs(B, ny, nx, f.no, 1, R.SENTINELS[0]), "Cout != na * no", "icaf_detect_conv: built for 3 anchors, no in {6, 8, 14}", mutate=other_cout)


def test_every_decode_choice_was_reached():
    """the kernel icaf_detect_decode_kernel reported for every reason listed in detect_select, as the tests above noted them"""
    if not REACH:
        pytest.fail("run together with the decode tests of this file (same process): nothing was recorded")
    print("\n[coverage] " + ", ".join(f"{k}: kernel {v}" for k, v in sorted(REACH.items())))
    assert REACH == WANT_REACH, f"never reached: {sorted(set(WANT_REACH) - set(REACH))}; wrong: {[k for k in REACH if REACH[k] != WANT_REACH.get(k)]}"
