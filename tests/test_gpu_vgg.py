"""The VGG16 two-stream backbone on the MI355X: ReLU convolutions, icaf_maxpool2d, icaf_vgg_stem, the stand-alone VGGblock and the four
yolov5_VGG16_* models.

ReLU convolutions run on the exact lattice of tests/test_gpu_exact.py (tests/numerics.py): every partial sum is exact in fp32, so the
output of EVERY launch configuration that accepts the layer must equal torch's CPU relu(conv2d) rounded once to the storage type, and
max(the same configuration without activation, 0).  The pool must return torch's bits.  The image-fed stem is exact on lattice images and
within one unit of the output type of the fp64 result on synth images (27 fp32 terms cost far less than half a 16-bit unit, so only a
result next to a tie can move, and only by one unit).  The models are held to the recorded outputs of the real reference
(tests/golden/model_vgg16_*.npz): fp32 to 1e-3 of each quantity's scale, 16 bit to 1.5 x the reference's OWN deviation in that type.
Every measured error is printed and appended to parity_vgg16.jsonl in the results folder; profiles/parity_vgg16.json is one run."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import numerics as nm                                           # noqa: E402
import tta_helpers as T                                         # noqa: E402
from helpers import REPO, golden_logits, load_cfg, load_golden, sample_idx      # noqa: E402
from numerics import ACT_NONE, ACT_SILU, BF16, F16, F32         # noqa: E402
from icafusion_amd import ops                                   # noqa: E402
from icafusion_amd.models.common import VGGblock                # noqa: E402
from icafusion_amd.models.yolo import Model, tta_sizes          # noqa: E402
from icafusion_amd.synth import synth_images, synth_state_dict  # noqa: E402

DEV = "cuda:0"
ACT_RELU = ops.ACT_RELU
DTYPES = [F32, BF16, F16]
DT_ID = {F32: "f32", BF16: "bf16", F16: "f16"}
SILU_ONLY = set(range(41, 46)) | {71} | set(range(81, 86))      # ctile, cstream, cwide


def record(**rec):
    print(json.dumps(rec))
    try:
        out = os.path.join(REPO, os.environ.get("OUT") or "results")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_vgg16.jsonl"), "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


def run(launch):
    launch(ops.current_stream_ptr())
    torch.cuda.synchronize()


def config_ids():
    ids = (ctypes.c_int * 64)()
    return list(ids[:ops.lib().icaf_conv2d_config_ids(ids, 64)])


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt)


# ------------------------------------------------------------------------------------------------------------------------------------
# ReLU convolutions
# ------------------------------------------------------------------------------------------------------------------------------------
# name -> (B, H, W, cin, cout, k): the VGG layers at the smallest maps that still leave partial tiles, and a 1x1
RELU_SHAPES = {"c64_3x3": (2, 9, 12, 64, 64, 3), "c128_256_3x3": (1, 6, 10, 128, 256, 3), "c512_3x3": (1, 4, 4, 512, 512, 3),
               "c128_64_1x1": (2, 5, 7, 128, 64, 1)}


class ReluCase:
    def __init__(self, name, dt):
        B, H, W, cin, cout, k = RELU_SHAPES[name]
        self.B, self.H, self.W, self.cin, self.cout, self.k, self.dt = B, H, W, cin, cout, k, dt
        d = nm.lattice(dt, B, H, W, cin, cout, k, H, W, nm.shape_seed("vgg_" + name, dt))
        self.z = nm.ref64(d["x"], d["w"], d["bias"], 1, k // 2, ACT_NONE)[0]            # exact pre-activation (asserted there)
        assert bool((self.z > 0).any()) and bool((self.z < 0).any()), "both signs must occur"
        cpu = torch.relu(F.conv2d(d["x"], d["w"], d["bias"], 1, k // 2))                # torch's CPU relu(conv2d), exact on the lattice
        assert torch.equal(cpu.double(), torch.relu(self.z))
        self.want = nm.rne(torch.relu(self.z), dt).permute(0, 2, 3, 1).contiguous()
        fill = int(nm.bits(torch.tensor([7.0], dtype=dt))[0])
        self.x = nm.Poisoned((B, H, W), cin, dt, DEV, fill, nhwc(d["x"], dt).to(DEV))
        self.wp, self.kp, self.bp = ops.pack_streams([(d["w"].to(DEV), d["bias"].to(DEV))], dt)

    def launch(self, y, act, tile):
        return ops.conv2d(self.x.view, self.wp, self.kp, self.bp, y, self.k, self.k, 1, 1, self.k // 2, self.k // 2, self.cin, self.cout,
                          act, tile=tile)

    def poisoned(self):
        return nm.Poisoned((self.B, self.H, self.W), self.cout, self.dt, DEV, nm.NAN_BITS[self.dt])


@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
@pytest.mark.parametrize("name", list(RELU_SHAPES))
def test_relu_conv_on_every_accepting_configuration(name, dt):
    case = ReluCase(name, dt)
    ids, ran, failures = config_ids(), [], []
    for tile in ids:
        probe = case.launch(case.poisoned().view, ACT_RELU, tile)
        if not ops.config_valid(probe, tile):
            continue
        assert tile not in SILU_ONLY, f"configuration {tile} accepted a ReLU layer"
        kname = ops.conv_kernel_name(probe)
        yp, yn = case.poisoned(), case.poisoned()
        plain = torch.full((case.B, case.H, case.W, case.cout), float("nan"), dtype=dt, device=DEV)       # ldy == Cout, nothing around it
        run(case.launch(yp.view, ACT_RELU, tile))
        run(case.launch(yn.view, ACT_NONE, tile))
        run(case.launch(plain, ACT_RELU, tile))
        got, none = yp.view.cpu(), yn.view.cpu()
        try:
            yp.assert_outside_intact(f"tile {tile}: ReLU output")
            yn.assert_outside_intact(f"tile {tile}: linear output")
            assert not bool(torch.isnan(got.float()).any()), "unwritten outputs"
            assert torch.equal(got.float(), none.float().clamp_min(0.0)), "ReLU != max(ACT_NONE, 0) of the same configuration"
            assert torch.equal(got.float(), case.want.float()), "ReLU != torch relu(conv2d) rounded to the type"
            assert torch.equal(plain.cpu().float(), case.want.float()), "contiguous output differs"
        except AssertionError as e:
            failures.append(f"{name} {DT_ID[dt]} tile {tile} ({kname}): {str(e)[:300]}")
            continue
        ran.append(tile)
    case.x.assert_outside_intact(name + ": x")
    offered = [t for t in ops.conv_candidates(case.launch(case.poisoned().view, ACT_RELU, 0).keep[0])]
    print(f"\n[relu] {name} {DT_ID[dt]}: ran {ran}; offered {offered}")
    assert ran and not failures, "\n".join(failures[:10])
    assert not (set(offered) & SILU_ONLY)
    if dt != F32:
        assert {52} <= set(ran) and (case.cout <= 64 or 61 in ran), "the streaming / register-fed GEMMs must take ReLU layers"
    assert {2, 12, 22} <= set(ran)


@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
@pytest.mark.parametrize("name", ["c64_3x3", "c128_64_1x1"])
def test_refusing_configurations_refuse_identically_and_write_nothing(name, dt):
    case = ReluCase(name, dt)
    refused = []
    for tile in config_ids():
        y = case.poisoned()
        launch = case.launch(y.view, ACT_RELU, tile)
        named = ops.lib().icaf_conv2d_kernel_name(launch.args[0], ctypes.create_string_buffer(256), 256)
        st = launch.fn(*launch.args, ops.current_stream_ptr())
        torch.cuda.synchronize()
        assert named == st, f"tile {tile}: icaf_conv2d_kernel_name says {named}, icaf_conv2d {st}"
        if st != 0:
            assert st in (-1, -3)
            assert torch.equal(nm.bits(y.buf), nm.bits(y.before)), f"tile {tile}: refused ({st}) but the output was written"
            refused.append(tile)
    print(f"\n[relu] {name} {DT_ID[dt]}: refused {refused}")
    assert SILU_ONLY <= set(refused)
    if dt != F32 and name == "c64_3x3":              # the same layer with SiLU IS accepted by the SiLU-only families built for it
        y = case.poisoned()
        ok = [t for t in SILU_ONLY if ops.config_valid(case.launch(y.view, ACT_SILU, t), t)]
        assert 71 in ok and set(ok) & {42, 43}, ok
    bad = case.launch(case.poisoned().view, 4, 0)     # one past the last activation code
    assert bad.fn(*bad.args, ops.current_stream_ptr()) == -1


# ------------------------------------------------------------------------------------------------------------------------------------
# icaf_maxpool2d
# ------------------------------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(2, 6, 10), (1, 7, 9), (1, 2, 2)]
POOL_C = [8, 64, 72]


def pool_want(x_nhwc, k, s, p):
    """torch's CPU max_pool2d of the NHWC tensor (values of the storage type), NHWC"""
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2).contiguous(), k, s, p).permute(0, 2, 3, 1).contiguous()


def pool_data(dt, shape, seed, negative=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 3.0
    x = -x.abs() - 0.25 if negative else x
    return x.to(dt)


@pytest.mark.parametrize("window", [(2, 2, 0), (3, 2, 1)], ids=["k2s2p0", "k3s2p1"])
@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
def test_maxpool_equals_torch_bit_for_bit(dt, window):
    k, s, p = window
    n = 0
    for (B, H, W) in POOL_SHAPES:
        for C in POOL_C:
            for variant in ("slice", "negative", "pair", "unaligned"):
                if variant == "negative" and (k, C) != (3, 64):
                    continue                                   # an all-negative map, which a zero pad would change: the padded window only
                if variant in ("pair", "unaligned") and C != 72:
                    continue
                lead = (2, B, H, W) if variant == "pair" else (B, H, W)
                Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
                lead_o = (2, B, Ho, Wo) if variant == "pair" else (B, Ho, Wo)
                x = pool_data(dt, (*lead, C), 1000 * H + 10 * C + k, negative=variant == "negative")
                lo_hi = dict(lo=3, hi=2) if variant == "unaligned" else {}          # odd pixel strides and bases: the one-element-per-thread kernel
                xin = nm.Poisoned(lead, C, dt, DEV, nm.INF_BITS[dt], x.to(DEV), **lo_hi)
                y = nm.Poisoned(lead_o, C, dt, DEV, nm.NAN_BITS[dt], **lo_hi)
                run(ops.maxpool2d(xin.view, y.view, k, s, p))
                want = pool_want(x.reshape(-1, H, W, C), k, s, p).reshape(*lead_o, C)
                what = f"maxpool {DT_ID[dt]} {window} {lead} C={C} {variant}"
                nm.assert_same_bits(y.view.cpu(), want, what)
                y.assert_outside_intact(what + ": y")
                xin.assert_outside_intact(what + ": x")
                if variant == "negative":
                    assert bool((want < 0).all())
                n += 1
    print(f"\n[maxpool] {DT_ID[dt]} {window}: {n} launches bit-equal to torch")


@pytest.mark.parametrize("window", [(2, 2, 0), (3, 2, 1)], ids=["k2s2p0", "k3s2p1"])
@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
def test_maxpool_propagates_nan_and_inf_like_torch(dt, window):
    """NaN, +Inf and -Inf INSIDE the slice: a window holding a NaN returns NaN, as torch's CPU kernel does (icaf.h), on both kernels."""
    k, s, p = window
    B, H, W, C = 1, 7, 9, 16
    x = pool_data(dt, (B, H, W, C), 99)
    x[0, 2, 3, 1], x[0, 0, 0, 0], x[0, 6, 8, 15] = float("nan"), float("nan"), float("nan")
    x[0, 4, 4, 2], x[0, 5, 1, 3] = float("inf"), float("-inf")
    x[0, 3:5, 6:8, 4] = float("-inf")
    want = pool_want(x, k, s, p)
    assert bool(torch.isnan(want.float()).any()) and bool(torch.isinf(want.float()).any())
    for lo_hi in ({}, dict(lo=3, hi=2)):
        xin = nm.Poisoned((B, H, W), C, dt, DEV, nm.INF_BITS[dt], x.to(DEV), **lo_hi)
        y = nm.Poisoned(tuple(want.shape[:3]), C, dt, DEV, nm.NAN_BITS[dt], **lo_hi)
        run(ops.maxpool2d(xin.view, y.view, k, s, p))
        got = y.view.cpu()
        assert torch.equal(torch.isnan(got.float()), torch.isnan(want.float()))
        assert torch.equal(torch.nan_to_num(got.float(), nan=0.0), torch.nan_to_num(want.float(), nan=0.0))
        y.assert_outside_intact("maxpool nan")


def test_maxpool_second_pass_of_the_grid_stride_loop():
    """More vectors than one pass of the capped grid covers (4096 workgroups x 256 threads)."""
    B, H, W, C = 2, 384, 384, 128
    x = pool_data(BF16, (B, H, W, C), 7)
    y = torch.full((B, H // 2, W // 2, C), float("nan"), dtype=BF16, device=DEV)
    assert y.numel() // 8 > nm.STRIDE_ITEMS
    run(ops.maxpool2d(x.to(DEV), y))
    nm.assert_same_bits(y.cpu(), pool_want(x, 2, 2, 0), "maxpool second pass")


def test_maxpool_refuses_bad_arguments_before_launch():
    lib = ops.lib()
    x = torch.zeros((1, 8, 8, 16), dtype=BF16, device=DEV)
    y = torch.full((1, 8, 8, 16), float("nan"), dtype=BF16, device=DEV)
    sp = ops.current_stream_ptr()

    def call(xp=None, ldx=16, yp=None, ldy=16, dtype=ops.BF16, B=1, H=8, W=8, C=16, k=2, s=2, p=0):
        return lib.icaf_maxpool2d(x.data_ptr() if xp is None else xp, ldx, y.data_ptr() if yp is None else yp, ldy, dtype, B, H, W, C, k, s, p, sp)
    assert call(k=2, s=1) == -3 and call(k=3, s=1, p=1) == -3 and call(k=5, s=2, p=2) == -3 and call(k=3, s=2, p=0) == -3
    assert call(C=12) == -1 and call(dtype=ops.F32, C=6) == -1          # not whole 16-byte vectors
    assert call(ldx=8) == -1 and call(ldy=8) == -1
    assert call(xp=0) == -1 and call(yp=0) == -1 and call(dtype=3) == -1
    assert call(H=1) == -1 and call(B=0) == -1 and call(xp=x.data_ptr() + 1) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all()), "a refused call wrote its output"
    assert b"icaf_maxpool2d" in lib.icaf_last_error()
    assert call() == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# icaf_vgg_stem
# ------------------------------------------------------------------------------------------------------------------------------------
def stem_weights(dt, seed, lattice=True):
    """per stream (w [64][3][3][3], bias [64]) fp32 on the CPU"""
    out = []
    for st in range(2):
        if lattice:
            d = nm.lattice(dt, 1, 4, 4, 3, 64, 3, 4, 4, seed + st)
            out.append((d["w"], d["bias"]))
        else:
            g = torch.Generator().manual_seed(seed + st)
            out.append((torch.randn((64, 3, 3, 3), generator=g) * 0.2, torch.randn((64,), generator=g) * 0.1))
    return out


def run_stem(img, wb, dt, B, H, W, paired=True, c0=0):
    """-> (Poisoned output, CPU result (G, B, H, W, 64))"""
    G = 2 if paired else 1
    w = torch.stack([ops.vgg_stem_weight(w.to(DEV), dt) for w, _ in wb[:G]]).contiguous()
    b = torch.stack([b.to(DEV) for _, b in wb[:G]]).contiguous()
    y = nm.Poisoned((G, B, H, W) if paired else (B, H, W), 64, dt, DEV, nm.NAN_BITS[dt])
    run(ops.vgg_stem(img, w if paired else w[0], b if paired else b[0], y.view, c0=c0))
    y.assert_outside_intact("vgg_stem output")
    got = y.view.cpu()
    return y, got if paired else got[None]


@pytest.mark.parametrize("hw", [(10, 12), (33, 40)], ids=["10x12", "33x40"])
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_vgg_stem_exact_on_lattice_images(dt, hw):
    B, (H, W) = 2, hw
    wb = stem_weights(dt, 4100 + H)
    g = torch.Generator().manual_seed(H * W)
    # fp32 source: integers in [-8, 8] (both signs); uint8 source: 0 / 255, the two values whose / 255 is exact
    x32 = torch.randint(-8, 9, (2, B, 3, H, W), generator=g).float()
    u8 = (torch.randint(0, 2, (B, 6, H, W), generator=g) * 255).to(torch.uint8)
    xu = (u8.float() / 255.0).view(B, 2, 3, H, W).transpose(0, 1).contiguous()
    for src, x, name in ((x32.to(DEV), x32, "fp32"), (u8.to(DEV), xu, "uint8")):
        _, got = run_stem(src, wb, dt, B, H, W)
        for st in range(2):
            z = nm.ref64(x[st], wb[st][0], wb[st][1], 1, 1, ACT_NONE)[0]
            cpu = torch.relu(F.conv2d(x[st], wb[st][0], wb[st][1], 1, 1))
            assert torch.equal(cpu.double(), torch.relu(z)) and bool((z < 0).any()) and bool((z > 0).any())
            want = nm.rne(torch.relu(z), dt).permute(0, 2, 3, 1)
            assert torch.equal(got[st].float(), want.float()), f"vgg_stem {name} {DT_ID[dt]} {H}x{W} stream {st}"
    # one stream alone (fp32 image of that stream; uint8 channels [3, 6)) gives that stream's bits
    _, solo = run_stem(x32[1].contiguous().to(DEV), wb[1:], dt, B, H, W, paired=False)
    _, pair = run_stem(x32.to(DEV), wb, dt, B, H, W)
    assert torch.equal(nm.bits(solo[0]), nm.bits(pair[1]))
    _, solo8 = run_stem(u8.to(DEV), wb[1:], dt, B, H, W, paired=False, c0=3)
    _, pair8 = run_stem(u8.to(DEV), wb, dt, B, H, W)
    assert torch.equal(nm.bits(solo8[0]), nm.bits(pair8[1]))


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_vgg_stem_on_synth_images_within_one_unit(dt):
    B, H, W = 2, 33, 40
    rgb, ir = synth_images(B, H, W, seed=41)
    wb = stem_weights(dt, 77, lattice=False)
    x = torch.stack((rgb, ir)).contiguous()
    _, got = run_stem(x.to(DEV), wb, dt, B, H, W)
    u8 = (torch.cat((rgb, ir), 1) * 255).round().to(torch.uint8)
    _, got8 = run_stem(u8.to(DEV), wb, dt, B, H, W)
    f8 = (u8.float() / 255.0).view(B, 2, 3, H, W).transpose(0, 1).contiguous()
    _, got8f = run_stem(f8.to(DEV), wb, dt, B, H, W)
    assert torch.equal(nm.bits(got8), nm.bits(got8f)), "the uint8 path differs from the fp32 path fed u8 / 255"
    worst, moved, total = 0.0, 0, 0
    for st in range(2):
        ref = torch.relu(F.conv2d(x[st].to(dt).double(), wb[st][0].to(dt).double(), wb[st][1].double(), 1, 1)).permute(0, 2, 3, 1)
        err = (got[st].double() - ref).abs()
        u = nm.ulp(ref, dt)
        worst = max(worst, float((err / u).max()))
        moved += int((got[st].float() != ref.float().to(dt).float()).sum())
        total += ref.numel()
    record(test="vgg_stem_synth", dtype=DT_ID[dt], worst_err_in_units=worst, share_not_nearest=moved / total)
    assert worst <= 1.0


def test_vgg_stem_refuses_before_launch():
    lib, sp = ops.lib(), ops.current_stream_ptr()
    img = torch.zeros((2, 1, 3, 8, 8), device=DEV)
    w = torch.zeros((2, 64, 32), dtype=BF16, device=DEV)
    b = torch.zeros((2, 64), device=DEV)
    y = torch.full((2, 1, 8, 8, 64), float("nan"), dtype=BF16, device=DEV)

    def call(dtype=ops.BF16, cout=64, kp=32, ldy=64, ctot=3, yp=None):
        return lib.icaf_vgg_stem(img.data_ptr(), 0, ctot, w.data_ptr(), b.data_ptr(), y.data_ptr() if yp is None else yp, ldy, dtype, 2, 1, 8, 8,
                                 cout, kp, 64 * 32, 64, 8 * 8 * 64, sp)
    assert call(dtype=ops.F32) == -3 and call(cout=32) == -3 and call(kp=64) == -3
    assert call(ldy=60) == -1 and call(ldy=68) == -1 and call(ctot=6) == -1 and call(yp=y.data_ptr() + 2) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.float()).all())
    assert call() == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# stand-alone VGGblock
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [(2, 64, 128), (3, 128, 256)], ids=["2x64-128", "3x128-256"])
def test_standalone_block_against_torch(args):
    n, c1, c2 = args
    torch.manual_seed(n * c1)
    blk = VGGblock(n, c1, c2).eval()
    twin = torch.nn.Sequential(*[torch.nn.Sequential(torch.nn.Conv2d(c1 if j == 0 else c2, c2, 3, padding=1), torch.nn.ReLU()) for j in range(n)],
                               torch.nn.MaxPool2d(2, 2)).eval()
    twin.load_state_dict({k[len("vggblock."):]: v for k, v in blk.state_dict().items()})
    x = torch.randn(2, c1, 18, 22)
    with torch.no_grad():
        ref = twin(x)
        ref16 = {dt: twin.to(dt)(x.to(dt)).float() for dt in (BF16, F16)}
        twin.float()
    blk = blk.to(DEV)
    got = blk(x.to(DEV)).cpu()
    assert got.shape == ref.shape == (2, c2, 9, 11)
    e32 = float((got - ref).abs().max() / ref.abs().max())
    rec = dict(test="standalone_vggblock", args=list(args), fp32_rel=e32)
    for dt in (BF16, F16):
        blk.compute_dtype = dt
        g16 = blk(x.to(DEV)).float().cpu()
        e_hip, e_ref = (g16 - ref).abs(), (ref16[dt] - ref).abs()
        rec[DT_ID[dt]] = dict(hip_max=float(e_hip.max()), hip_mean=float(e_hip.mean()), torch_max=float(e_ref.max()), torch_mean=float(e_ref.mean()))
    record(**rec)
    assert e32 <= 1e-3
    for dt in (BF16, F16):
        r = rec[DT_ID[dt]]
        assert r["hip_max"] <= 1.5 * r["torch_max"] and r["hip_mean"] <= 1.5 * r["torch_mean"], (DT_ID[dt], r)


# ------------------------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------------------------
GOLDENS = ["model_vgg16_kaist_320_b1", "model_vgg16_ninfusion_flir_320x352_b2"]
_MODELS = {}


def model_of(golden):
    """(golden, fp32-master model on the device, CPU images): built once per fixture and shared; tests restore every switch they flip."""
    if golden not in _MODELS:
        g = load_golden(golden)
        batch, h, w, seed, _ = [int(v) for v in g["meta"]]
        m = Model(load_cfg(str(g["yaml"]))).eval()
        m.load_state_dict(synth_state_dict(m, seed))
        _MODELS[golden] = (g, m.to(DEV), synth_images(batch, h, w, seed))
    g, m, imgs = _MODELS[golden]
    m.compute_dtype = None
    m.pair_streams, m.use_graph = True, False
    VGGblock.fuse_stem = False               # the class default (profiles/vgg_bench.json: the generic first layer is faster)
    m.invalidate()
    return g, m, imgs


def z16_of(g, name):
    a = torch.from_numpy(g["z_" + name])
    return (a.view(torch.bfloat16) if name == "bf16" else a).float().numpy()


def dev16(g, name):
    """[box max, box mean, score max, score mean] of the reference's own deviation in that 16-bit type, recomputed from its recorded outputs"""
    d = np.abs(z16_of(g, name) - g["z"])
    out = [float(d[..., :4].max()), float(d[..., :4].mean()), float(d[..., 4:].max()), float(d[..., 4:].mean())]
    assert np.allclose(out, g["dev_" + name], rtol=1e-5)
    return out


def within16(a, b, dev):
    """errors of a against b and whether they stay within 1.5 x the reference-in-16-bit deviation, maximum and mean, boxes and scores"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    e = [float(d[..., :4].max()), float(d[..., :4].mean()), float(d[..., 4:].max()), float(d[..., 4:].mean())]
    return e, all(x <= 1.5 * y for x, y in zip(e, dev))


@pytest.mark.parametrize("golden", GOLDENS)
def test_fp32_model_matches_reference_golden(golden):
    g, m, (rgb, ir) = model_of(golden)
    z, logits, raws = m(rgb.to(DEV), ir.to(DEV))
    zc, ref = z.cpu().numpy(), g["z"]
    assert zc.shape == ref.shape
    lg, ref_lg = golden_logits(g, logits.cpu().numpy())
    err = {"box_px": float(np.abs(zc[..., :4] - ref[..., :4]).max()), "score": float(np.abs(zc[..., 4:] - ref[..., 4:]).max()),
           "logit": float(np.abs(lg - ref_lg).max()), "raw": 0.0}
    scale = {"box_px": max(1.0, float(np.abs(ref[..., :4]).max())), "logit": max(1.0, float(np.abs(g["logits"]).max())), "raw": 1.0}
    for l, r in enumerate(raws):
        assert tuple(r.shape) == tuple(g[f"raw{l}_shape"])
        got = r.cpu().reshape(-1)[torch.from_numpy(sample_idx(r.numel(), 100 + l))].numpy()
        err["raw"] = max(err["raw"], float(np.abs(got - g[f"raw{l}"]).max()))
        scale["raw"] = max(scale["raw"], float(np.abs(g[f"raw{l}"]).max()))
    # the fp32 bound of the project for a fixture without a committed measurement: 1e-3 of each quantity's scale
    bound = {"box_px": 1e-3 * scale["box_px"], "score": 1e-3, "logit": 1e-3 * scale["logit"], "raw": 1e-3 * scale["raw"]}
    names = [l.name for l in m.plan_for(*rgb.shape[:1], *rgb.shape[2:]).launches]
    assert names.count("vgg_conv3x3") == 13 and "preprocess_pad" in names and "vgg_stem" not in names       # fp32: the generic first layer, paired streams
    assert names.count("vgg_maxpool") == 2 + 3 * 2           # blocks 1, 2: one launch over both streams; 3 - 5 write the fusion buffers' halves
    record(test="model_fp32", golden=golden, **err, bound=bound)
    for k in err:
        assert err[k] <= bound[k], f"{golden}: {k} error {err[k]:.3g} > {bound[k]:.3g}"


@pytest.mark.parametrize("dn,dt", [("bf16", BF16), ("fp16", F16)])
@pytest.mark.parametrize("golden", GOLDENS)
def test_16bit_model_within_the_reference_deviation(golden, dn, dt):
    g, m, (rgb, ir) = model_of(golden)
    m.compute_dtype = dt
    dev = dev16(g, dn)
    z_off = m(rgb.to(DEV), ir.to(DEV))[0].cpu().numpy()                 # the default: the generic first layer
    names = [l.name for l in m.plan_for(rgb.shape[0], *rgb.shape[2:]).launches]
    assert "vgg_stem" not in names and names.count("vgg_conv3x3") == 13 and "preprocess_pad" in names
    VGGblock.fuse_stem = True
    try:
        m.invalidate()
        z_on = m(rgb.to(DEV), ir.to(DEV))[0].cpu().numpy()
        names = [l.name for l in m.plan_for(rgb.shape[0], *rgb.shape[2:]).launches]
        assert names.count("vgg_stem") == 1 and names.count("vgg_conv3x3") == 12 and "preprocess_pad" not in names
    finally:
        VGGblock.fuse_stem = False
        m.invalidate()
    assert np.isfinite(z_on).all() and np.isfinite(z_off).all()
    e_on, ok_on = within16(z_on, g["z"], dev)
    e_off, ok_off = within16(z_off, g["z"], dev)
    e_ab, ok_ab = within16(z_on, z_off, dev)
    record(test="model_16bit", golden=golden, dtype=dn, reference_dev=dev, hip_fused_stem=e_on, hip_generic_stem=e_off, fused_vs_generic=e_ab,
           order="box max, box mean, score max, score mean")
    assert ok_on, (e_on, dev)
    assert ok_off, (e_off, dev)
    assert ok_ab, (e_ab, dev)


@pytest.mark.parametrize("dt,stem", [(F32, False), (BF16, False), (BF16, True)], ids=["f32", "bf16", "bf16-fused-stem"])
def test_model_entry_points_are_bit_equal(dt, stem):
    """forward_u8 == float forward, unpaired == paired streams, a batch shard == the same rows of the full batch, hipGraph replay == eager;
    in 16 bit with the generic first layer (the default) and with icaf_vgg_stem."""
    g, m, _ = model_of("model_vgg16_ninfusion_flir_320x352_b2")
    m.compute_dtype = None if dt == F32 else dt
    VGGblock.fuse_stem = stem
    m.invalidate()
    B, H, W = 2, 96, 128
    gen = np.random.default_rng(5)
    img6 = torch.from_numpy(gen.integers(0, 256, (B, 6, H, W), dtype=np.uint8)).to(DEV)
    f = (img6.cpu().float() / 255.0).to(DEV)
    rgb, ir = f[:, :3].contiguous(), f[:, 3:].contiguous()
    z = m(rgb, ir)[0]
    assert torch.equal(m.forward_u8(img6)[0], z)
    shard = m(rgb[1:].contiguous(), ir[1:].contiguous())[0]
    assert torch.equal(shard, z[1:])
    try:
        m.pair_streams = False
        m.invalidate()
        assert [l.name for l in m.plan_for(B, H, W).launches].count("vgg_maxpool") == 10        # one per block and stream
        assert torch.equal(m(rgb, ir)[0], z)
        assert torch.equal(m.forward_u8(img6)[0], z)
        m.pair_streams, m.use_graph = True, True
        m.invalidate()
        assert m.plan_for(B, H, W).graph is not None
        assert torch.equal(m(rgb, ir)[0], z) and torch.equal(m(rgb, ir)[0], z)
    finally:
        m.pair_streams, m.use_graph = True, False
        VGGblock.fuse_stem = False
        m.invalidate()


def test_transfusion_model_graph_and_u8():
    g, m, (rgb, ir) = model_of("model_vgg16_kaist_320_b1")
    m.compute_dtype = BF16
    z = m(rgb.to(DEV), ir.to(DEV))[0]
    try:
        m.use_graph = True
        m.invalidate()
        assert torch.equal(m(rgb.to(DEV), ir.to(DEV))[0], z)
    finally:
        m.use_graph = False
        m.invalidate()


def test_tta_on_the_smallest_size():
    """forward(augment=True) of the NiNfusion config at tta_min_size = 32 x 32, where every pass pads to 32 x 32: the three passes must run
    on three plans of their own (one plan cannot hold three passes' inputs), the staged inputs are the images fed and scale_img of them,
    and the result equals the three plain forwards merged on the host — for the fp32 pair and for the uint8 batch."""
    g, m, _ = model_of("model_vgg16_ninfusion_flir_320x352_b2")
    m.compute_dtype = BF16
    H, W = m.tta_min_size()
    assert (H, W) == (32, 32) and [p[4:] for p in tta_sizes(H, W)] == [(32, 32)] * 3
    B = 2
    rgb, ir = synth_images(B, H, W, seed=9)
    img6 = (torch.cat((rgb, ir), 1) * 255).round().to(torch.uint8)
    f = img6.float() / 255.0
    for name, feed, src in (("fp32", lambda: m(rgb.to(DEV), ir.to(DEV), augment=True), (rgb, ir)),
                            ("uint8", lambda: m.forward_u8(img6.to(DEV), augment=True), (f[:, :3].contiguous(), f[:, 3:].contiguous()))):
        z, second = feed()
        assert second is None and z.dtype == torch.float32
        tp = m.tta_plan_for(B, H, W, u8=name == "uint8")
        assert len({id(p) for p in tp.plans}) == 3, f"{name}: passes padded to the same size share a plan"
        assert len({p.outputs[0].data_ptr() for p in tp.plans}) == 3
        if name == "fp32":
            assert torch.equal(tp.plans[0].input_pair[0].cpu(), rgb) and torch.equal(tp.plans[0].input_pair[1].cpu(), ir)
        else:
            assert torch.equal(tp.plans[0].inputs[0].cpu(), img6)
        xis = [torch.stack(src)] + [p.input_pair.clone().cpu() for p in tp.plans[1:]]
        for xi, (scale, flip) in list(zip(xis, zip(T.SCALES, T.FLIPS)))[1:]:
            for k in range(2):                             # the staging kernel against torch's CPU scale_img (its own test's bound: 2^-21)
                want_x = T.scale_img_cpu(src[k], scale, flip == 3)
                assert xi[k].shape == want_x.shape and float((xi[k] - want_x).abs().max()) <= 2.0 ** -21, (name, scale, k)
        assert not torch.equal(xis[1], xis[2]) and not torch.equal(xis[0], xis[1])
        zs = [m(xi[0].to(DEV), xi[1].to(DEV))[0].cpu().numpy() for xi in xis]
        want = T.merge_cpu(zs, W)
        assert z.shape[1] == sum(a.shape[1] for a in zs)
        assert np.array_equal(z.cpu().numpy(), want), name
        assert not np.array_equal(zs[0], zs[2])
    record(test="tta_min_size", height=H, width=W, rows=int(z.shape[1]))


def test_forward_frames_and_detection_pipeline_on_a_vgg_config():
    """The remaining entry points on a VGG16 config: forward_frames (device letterbox) is forward_u8 of the host-letterboxed batch bit for bit,
    and every step of a DetectionPipeline with two batches in flight equals forward + NMS run one at a time."""
    from test_gpu_frames import frames_of, host_batch
    from icafusion_amd.pipeline import DetectionPipeline
    from icafusion_amd.utils.general import non_max_suppression
    g, m, _ = model_of("model_vgg16_ninfusion_flir_320x352_b2")
    m.compute_dtype = BF16
    shapes = [(60, 80), (96, 64)]
    rgb, ir = frames_of(shapes, 3, 31), frames_of(shapes, 3, 131)
    (z, logits, raws), info = m.forward_frames([torch.from_numpy(x).to(DEV) for x in rgb], [torch.from_numpy(x).to(DEV) for x in ir], 96)
    wz, wlogits, wraws = m.forward_u8(host_batch(rgb, ir, 96).to(DEV))
    assert torch.equal(z, wz) and torch.equal(logits, wlogits) and all(torch.equal(a, b) for a, b in zip(raws, wraws))
    assert np.array_equal(info.scale.cpu().numpy(), ops.frame_geometry(shapes, 96)[1])
    B, H, W = 2, 96, 128
    try:
        m.use_graph = True
        pipe = DetectionPipeline(m, B, H, W, DEV, conf_thres=0.001, iou_thres=0.45, depth=2)
        batches = [synth_images(B, H, W, seed=70 + k) for k in range(4)]
        outs = [tuple(t[0] for t in pipe.submit(a.to(DEV), b.to(DEV))) for a, b in batches]
        pipe.synchronize()
        last = [(d.clone(), c.clone()) for d, c in outs[-2:]]             # the last `depth` steps still own their buffers
    finally:
        m.use_graph, m.static_outputs = False, False
        m.invalidate()
    total = 0
    for (det, count), (a, b) in zip(last, batches[-2:]):
        want = non_max_suppression(m(a.to(DEV), b.to(DEV))[0], 0.001, 0.45)
        assert all(torch.equal(det[i, :n], w) for (i, n), w in zip(enumerate(count.tolist()), want))
        total += sum(count.tolist())
    assert total > 0, "no detections: the comparison would be empty"
