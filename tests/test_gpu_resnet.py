"""The ResNet50 two-stream backbone on the MI355X: the residual-in-front-of-the-ReLU epilogue (icaf_conv_args.res_mode = 1), the
key-streaming attention kernel, icaf_layernorm's wide fp32 rows, the stand-alone ResNetblock and the yolov5_ResNet50_* models.

Residual epilogue: on the exact lattice of tests/numerics.py every partial sum, the bias and the residual are exact in fp32, so the output
of EVERY launch configuration that accepts the layer must equal torch's CPU relu(conv2d(x) + res) rounded ONCE to the storage type.
Streaming attention: the project's bound for the resident kernel (close(..., factor=2) / TOL of tests/test_gpu_kernels.py against the fp32
softmax reference).  Models: the recorded outputs of the real reference (tests/golden/model_resnet50_*.npz): fp32 to 1e-3 of each
quantity's scale, 16 bit to 1.5 x the reference's OWN deviation in that type.  Every measured error is printed and appended to
parity_resnet50.jsonl in the results folder; profiles/parity_resnet50.json is one run."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import numerics as nm                                           # noqa: E402
from helpers import REPO, golden_logits, lib_option, load_cfg, load_golden, sample_idx      # noqa: E402
from numerics import ACT_NONE, ACT_SILU, BF16, F16, F32         # noqa: E402
from test_gpu_exact import ln_check, ln_rows                    # noqa: E402
from test_gpu_kernels import TOL, _attn_ref, close, q, rnd      # noqa: E402,F401
from icafusion_amd import ops                                   # noqa: E402
from icafusion_amd.models.common import ResNetblock             # noqa: E402
from icafusion_amd.models.yolo import Model                     # noqa: E402
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
        with open(os.path.join(out, "parity_resnet50.jsonl"), "a") as f:
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
# residual in front of the ReLU
# ------------------------------------------------------------------------------------------------------------------------------------
# name -> (B, H, W, cin, cout, k, s, p, residual): ResNet50's launches at the smallest maps that still leave partial tiles
RES_SHAPES = {"conv3_l1": (2, 9, 12, 64, 256, 1, 1, 0, True), "conv3_l4": (1, 5, 7, 512, 2048, 1, 1, 0, True),
              "c128_3x3s2": (1, 6, 10, 128, 128, 3, 2, 1, True), "shortcut_s2": (2, 5, 7, 256, 512, 1, 2, 0, False),
              "stem7x7": (1, 12, 14, 8, 64, 7, 2, 3, False)}
_CASES = {}


class ResCase:
    """One layer on the lattice: operands on the device (x inside a poisoned wider buffer), the expected bits computed once on the CPU."""

    def __init__(self, name, dt):
        B, H, W, cin, cout, k, s, p, use_res = RES_SHAPES[name]
        self.geo, self.dt, self.cout, self.use_res = (k, s, p, cin), dt, cout, use_res
        Ho, Wo = nm.out_hw(H, W, k, s, p)
        self.out = (B, Ho, Wo)
        d = nm.lattice(dt, B, H, W, cin, cout, k, Ho, Wo, nm.shape_seed("resnet_" + name, dt))
        z = nm.ref64(d["x"], d["w"], d["bias"], s, p, ACT_NONE)[0]                      # exact pre-activation (asserted there)
        res = d["res"] if use_res else None
        pre = z + res.double() if use_res else z
        assert torch.equal(pre.float().double(), pre), "conv + bias + residual must be exact in fp32"
        assert bool((pre > 0).any()) and bool((pre < 0).any()), "both signs of the pre-activation sum must occur"
        cpu = torch.relu(F.conv2d(d["x"], d["w"], d["bias"], s, p) + (res if use_res else 0.0))       # torch's CPU expression, exact here
        assert torch.equal(cpu.double(), torch.relu(pre))
        if use_res:                                              # the Bottleneck order (add behind the activation) must not pass
            old = nm.rne(nm.rne(torch.relu(z), dt).double() + res.double(), dt)
            assert not torch.equal(old, nm.rne(torch.relu(pre), dt)), "relu(z) + res equals relu(z + res) everywhere"
        self.want = nm.rne(torch.relu(pre), dt).permute(0, 2, 3, 1).contiguous()
        fill = int(nm.bits(torch.tensor([7.0], dtype=dt))[0])
        self.x = nm.Poisoned((B, H, W), cin, dt, DEV, fill, nhwc(d["x"], dt).to(DEV))
        self.res = nm.Poisoned(self.out, cout, dt, DEV, nm.NAN_BITS[dt], nhwc(res, dt).to(DEV)) if use_res else None
        self.wp, self.kp, self.bp = ops.pack_streams([(d["w"].to(DEV), d["bias"].to(DEV))], dt)

    def launch(self, y, tile, act=ACT_RELU, res_pre_act=None, **kw):
        k, s, p, cin = self.geo
        res_pre_act = self.use_res if res_pre_act is None else res_pre_act
        return ops.conv2d(self.x.view, self.wp, self.kp, self.bp, y, k, k, s, s, p, p, cin, self.cout, act,
                          res=self.res.view if self.use_res else None, tile=tile, res_pre_act=res_pre_act, **kw)

    def poisoned(self):
        return nm.Poisoned(self.out, self.cout, self.dt, DEV, nm.NAN_BITS[self.dt])


def case_of(name, dt):
    if (name, dt) not in _CASES:
        _CASES[(name, dt)] = ResCase(name, dt)
    return _CASES[(name, dt)]


@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
@pytest.mark.parametrize("name", list(RES_SHAPES))
def test_residual_in_front_of_relu_on_every_accepting_configuration(name, dt):
    case = case_of(name, dt)
    ran, failures = [], []
    for tile in config_ids():
        probe = case.launch(case.poisoned().view, tile)
        if not ops.config_valid(probe, tile):
            continue
        assert tile not in SILU_ONLY, f"configuration {tile} accepted a ReLU layer"
        kname = ops.conv_kernel_name(probe)
        yp = case.poisoned()
        plain = torch.full((*case.out, case.cout), float("nan"), dtype=dt, device=DEV)       # ldy == Cout, nothing around it
        run(case.launch(yp.view, tile))
        run(case.launch(plain, tile))
        got = yp.view.cpu()
        try:
            yp.assert_outside_intact(f"tile {tile}: output")
            assert not bool(torch.isnan(got.float()).any()), "unwritten outputs"
            assert torch.equal(got.float(), case.want.float()), "!= torch relu(conv2d + res) rounded once to the type"
            assert torch.equal(plain.cpu().float(), case.want.float()), "contiguous output differs"
        except AssertionError as e:
            failures.append(f"{name} {DT_ID[dt]} tile {tile} ({kname}): {str(e)[:300]}")
            continue
        ran.append(tile)
    case.x.assert_outside_intact(name + ": x")
    if case.res is not None:
        case.res.assert_outside_intact(name + ": res")
    offered = ops.conv_candidates(case.launch(case.poisoned().view, 0).keep[0])
    print(f"\n[res_mode] {name} {DT_ID[dt]}: ran {ran}; offered {offered}")
    assert ran and not failures, "\n".join(failures[:10])
    assert not (set(offered) & SILU_ONLY)
    assert {2, 12, 22} <= set(ran)
    if dt != F32 and case.geo[3] % 64 == 0:                     # whole 128-byte taps: the streaming and register-fed GEMMs take the layer
        assert 52 in ran and (case.cout <= 64 or 61 in ran), ran


@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
@pytest.mark.parametrize("name", ["conv3_l1", "c128_3x3s2"])
def test_refusing_configurations_refuse_identically_and_write_nothing(name, dt):
    case = case_of(name, dt)
    sp = ops.current_stream_ptr()
    refused = []
    for tile in config_ids():
        y = case.poisoned()
        launch = case.launch(y.view, tile)
        named = ops.lib().icaf_conv2d_kernel_name(launch.args[0], ctypes.create_string_buffer(256), 256)
        st = launch.fn(*launch.args, sp)
        torch.cuda.synchronize()
        assert named == st, f"tile {tile}: icaf_conv2d_kernel_name says {named}, icaf_conv2d {st}"
        if st != 0:
            assert st in (-1, -3)
            assert torch.equal(nm.bits(y.buf), nm.bits(y.before)), f"tile {tile}: refused ({st}) but the output was written"
            refused.append(tile)
    print(f"\n[res_mode] {name} {DT_ID[dt]}: refused {refused}")
    assert SILU_ONLY <= set(refused)


@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
def test_other_forms_of_the_mode_are_refused_before_launch(dt):
    case = case_of("conv3_l1", dt)
    sp = ops.current_stream_ptr()
    y = case.poisoned()
    pre = torch.zeros((*case.out, case.cout), dtype=torch.float32, device=DEV)
    y32 = torch.full((*case.out, case.cout), float("nan"), dtype=torch.float32, device=DEV)
    requests = {"silu": (case.launch(y.view, 0, act=ACT_SILU), -3), "alpha_res": (case.launch(y.view, 0, alpha_res=0.5), -3),
                "alpha_acc": (case.launch(y.view, 0, alpha_acc=2.0), -3), "pre": (case.launch(y.view, 0, pre=pre), -3)}
    if dt != F32:
        requests["fp32 output"] = (case.launch(y32, 0), -3)
    two = case.launch(y.view, 0)
    two.keep[0].res_mode = 2
    requests["res_mode 2"] = (two, -1)
    none = case.launch(y.view, 0)
    none.keep[0].res = None
    requests["no residual"] = (none, -3)
    for what, (launch, want) in requests.items():
        named = ops.lib().icaf_conv2d_kernel_name(launch.args[0], ctypes.create_string_buffer(256), 256)
        st = launch.fn(*launch.args, sp)
        assert st == want == named, f"{what}: icaf_conv2d {st}, icaf_conv2d_kernel_name {named}, expected {want}"
    torch.cuda.synchronize()
    assert torch.equal(nm.bits(y.buf), nm.bits(y.before)) and bool(torch.isnan(y32).all()), "a refused call wrote its output"
    run(case.launch(y.view, 0))                                 # the accepted form, same operands
    assert torch.equal(y.view.cpu().float(), case.want.float())


# ------------------------------------------------------------------------------------------------------------------------------------
# key-streaming attention
# ------------------------------------------------------------------------------------------------------------------------------------
HEADS = 8
STREAM_CASES = [(1, 100, 2048), (2, 77, 2048), (1, 36, 2048), (1, 40, 1536), (1, 256, 1024)]
FORCED_CASES = [(1, 100, 1024), (2, 256, 512)]


def attn_data(B, N, C, seed):
    qkv = rnd((2, B * N, 3 * C), seed, 1.0)
    qkv[:, :, :2 * C] *= 1.5                      # sharpen the softmax a little (as test_cross_attention)
    return qkv


def attn_run(qkv, B, N, C, dt):
    """-> fp32 CPU output of icaf_cross_attention written into a NaN-filled buffer, no NaN left"""
    out = torch.full((2, B * N, C), float("nan"), dtype=dt, device=DEV)
    run(ops.cross_attention(qkv[:, :B * N].contiguous().to(DEV).to(dt), out, B, N, HEADS))
    got = out.float().cpu()
    assert not bool(torch.isnan(got).any()), "outputs left unwritten"
    return got


@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
@pytest.mark.parametrize("case", STREAM_CASES, ids=lambda c: "B%d-N%d-C%d" % c)
def test_streaming_attention_against_the_softmax_reference(case, dt):
    B, N, C = case
    form = ops.cross_attention_form(dt, B, N, C, HEADS)
    dkp, qsplit, remap = ops.cross_attention_config(dt, B, N, C, HEADS)
    if C == 1024:         # N = 256 at d_k = 128: 268 KB of resident K / V^T in fp32, 134 KB in 16 bit
        assert form == (1 if dt == F32 else 0) and dkp == 128
    else:
        assert form == 1 and dkp == 256
    qkv = attn_data(B, N, C, 5000 + N + C)
    ref = _attn_ref(q(qkv, dt), B, N, C, HEADS)
    got = attn_run(qkv, B, N, C, dt)
    err = float((got - ref).abs().max() / ref.abs().max())
    record(test="streaming_attention", case=list(case), dtype=DT_ID[dt], form=form, dkp=dkp, qsplit=qsplit, remap=remap, rel_err=err,
           bound=2 * TOL[dt])
    close(got, ref, dt, f"attention {case} form {form}", factor=2)
    # every forced query-split count gives the same bits
    nqt = (N + 31) // 32
    for forced in (1, 2, nqt, nqt + 5):
        with lib_option("attn_qsplit", forced):
            assert ops.cross_attention_form(dt, B, N, C, HEADS) == form
            assert torch.equal(attn_run(qkv, B, N, C, dt), got), f"{forced} forced query splits give other bits"


@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
@pytest.mark.parametrize("case", FORCED_CASES, ids=lambda c: "B%d-N%d-C%d" % c)
def test_forced_streaming_form_on_shapes_the_resident_kernel_accepts(case, dt):
    B, N, C = case
    qkv = attn_data(B, N, C, 6000 + N + C)
    ref = _attn_ref(q(qkv, dt), B, N, C, HEADS)
    assert ops.cross_attention_form(dt, B, N, C, HEADS) == 0
    resident = attn_run(qkv, B, N, C, dt)
    with ops.attn_stream():
        assert ops.cross_attention_form(dt, B, N, C, HEADS) == 1
        assert ops.cross_attention_config(dt, B, N, C, HEADS)[0] == C // HEADS
        streamed = attn_run(qkv, B, N, C, dt)
        for forced in (1, 3):
            with lib_option("attn_qsplit", forced):
                assert torch.equal(attn_run(qkv, B, N, C, dt), streamed)
    assert ops.cross_attention_form(dt, B, N, C, HEADS) == 0
    close(resident, ref, dt, f"resident {case}", factor=2)
    close(streamed, ref, dt, f"streamed {case}", factor=2)
    record(test="forced_streaming", case=list(case), dtype=DT_ID[dt], same_bits_as_resident=bool(torch.equal(resident, streamed)),
           rel_diff=float((resident - streamed).abs().max() / ref.abs().max()))


@pytest.mark.parametrize("dt", DTYPES, ids=[DT_ID[d] for d in DTYPES])
def test_streaming_attention_same_bits_at_every_batch(dt):
    """An image gives the same bits at batch 1, 3, 4 and 8: the XCD-remapped one-dimensional grid (2B % 8 == 0) or the plain one."""
    N, C = 36, 2048
    qkv = attn_data(8, N, C, 77)
    ref = _attn_ref(q(qkv, dt), 8, N, C, HEADS)
    outs = {}
    for B in (1, 3, 4, 8):
        # (2, B * N) rows of the first B images of each modality
        sub = torch.stack([qkv[g, :B * N] for g in range(2)])
        assert ops.cross_attention_form(dt, B, N, C, HEADS) == 1
        assert ops.cross_attention_config(dt, B, N, C, HEADS)[2] == int((2 * B) % 8 == 0)
        outs[B] = attn_run(sub, B, N, C, dt)
        close(outs[B], ref[:, :B * N], dt, f"batch {B}", factor=2)
    for B in (1, 3, 4):
        assert torch.equal(outs[8][:, :B * N], outs[B]), f"batch 8 differs from batch {B} on the same images"


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_streaming_attention_late_spikes(dt):
    """Keys that dominate LATE in the key order — by less and by much more than the deferral slack of the 16-bit loop, the last one in the
    partly padded last key tile — at d_k = 256 (modelled on test_cross_attention_late_spikes_in_16_bit)."""
    B, N, C = 2, 100, 2048
    dk = C // HEADS
    spikes = ((13, 1.2), (44, 3.0), (74, 7.0), (99, 12.0))
    qkv = rnd((2, B * N, 3 * C), 47, 0.4)
    qkv[:, :, :C] = qkv[:, :, :C].abs() + 0.3                     # positive queries: a large positive key raises every score of its column
    for key, amp in spikes:
        qkv[0, key, C:2 * C] = amp * math.sqrt(128.0 / dk)        # the same score excess as the d_k = 128 case of the model test
        qkv[1, N + key, C:2 * C] = amp * 0.9 * math.sqrt(128.0 / dk)
    assert ops.cross_attention_form(dt, B, N, C, HEADS) == 1 and N % 32 != 0
    got = attn_run(qkv, B, N, C, dt)
    ref = _attn_ref(q(qkv, dt), B, N, C, HEADS)
    for d in range(2):
        close(got[d], ref[d], dt, f"late spikes dir {d}", factor=2)


def test_head_dimensions_beyond_256_are_refused():
    qkv = torch.zeros((2, 32, 3 * 4096), dtype=BF16, device=DEV)
    out = torch.full((2, 32, 4096), float("nan"), dtype=BF16, device=DEV)
    launch = ops.cross_attention(qkv, out, 1, 32, HEADS)
    assert launch.fn(*launch.args, ops.current_stream_ptr()) == -3
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# icaf_layernorm: fp32 rows up to C = 2048
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1024, 1536, 2048])
def test_layernorm_fp32_wide_rows(C):
    """C = 2048 and 1536 run the instantiation with eight vectors per lane, C = 1024 the one it always ran (its device code is unchanged:
    tools/kernel_fingerprint.py); all are held to the reference expression and per-element bound ln_check pins for the existing kernel."""
    dt, rows, eps = F32, 39, 1e-5
    gen = torch.Generator().manual_seed(C)
    gam = [torch.randint(-64, 65, (C,), generator=gen).float() / 32.0 for _ in range(2)]
    bet = [torch.randint(-2 ** 15, 2 ** 15, (C,), generator=gen).float() / 2 ** 14 for _ in range(2)]
    xs = [ln_rows(dt, rows, C, 10 * C + g) for g in range(2)]
    if C & (C - 1):       # ln_rows' outlier rows are exact for a power of two only: 2 C (mean 2, sum of squares below 2^24) keeps them exact
        for x, kind in xs:
            x[kind == 2] = torch.where(x[kind == 2] != 0, torch.tensor(2.0 * C), torch.tensor(0.0))
            assert float(x[kind == 2].sum(1).min()) == 2.0 * C and (2 * C - 2) ** 2 + 4 * (C - 1) < 2 ** 24
    xg = torch.stack([x for x, _ in xs]).to(DEV)
    y = torch.full_like(xg, float("nan"))
    run(ops.layernorm(xg, y, gam[0].to(DEV), bet[0].to(DEV), gam[1].to(DEV), bet[1].to(DEV), eps))
    assert not bool(torch.isnan(y).any())
    for g in range(2):
        ln_check(y[g].cpu(), xs[g][0], xs[g][1], gam[g], bet[g], eps, dt, f"icaf_layernorm C={C} f32 group {g}")


def test_layernorm_refuses_rows_beyond_2048():
    x = torch.zeros((1, 4, 2052), device=DEV)
    y = torch.full_like(x, float("nan"))
    g = torch.ones(2052, device=DEV)
    launch = ops.layernorm(x, y, g, g, g, g)
    assert launch.fn(*launch.args, ops.current_stream_ptr()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# stand-alone ResNetblock
# ------------------------------------------------------------------------------------------------------------------------------------
class TorchBlock(torch.nn.Module):
    """torch twin of models.common.ResNetblock with the same state_dict keys"""

    def __init__(self, c1, c2, stride):
        super().__init__()
        nn = torch.nn
        self.conv1, self.bn1 = nn.Conv2d(c1, c2, 1, bias=False), nn.BatchNorm2d(c2)
        self.conv2, self.bn2 = nn.Conv2d(c2, c2, 3, stride, 1, bias=False), nn.BatchNorm2d(c2)
        self.conv3, self.bn3 = nn.Conv2d(c2, 4 * c2, 1, bias=False), nn.BatchNorm2d(4 * c2)
        self.shortcut = nn.Sequential()
        if stride != 1 or c1 != 4 * c2:
            self.shortcut = nn.Sequential(nn.Conv2d(c1, 4 * c2, 1, stride, bias=False), nn.BatchNorm2d(4 * c2))

    def forward(self, x):
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out += self.shortcut(x)
        return F.relu(out)


@pytest.mark.parametrize("args", [(64, 64, 1), (256, 128, 2), (512, 128, 1)], ids=["64-64-s1", "256-128-s2", "512-128-identity"])
def test_standalone_block_against_torch(args):
    c1, c2, s = args
    blk = ResNetblock(c1, c2, s).eval()
    blk.load_state_dict(synth_state_dict(blk, c1 + s))
    twin = TorchBlock(c1, c2, s).eval()
    twin.load_state_dict(blk.state_dict(), strict=True)
    assert bool(len(blk.shortcut)) == (args != (512, 128, 1))
    x = torch.randn(2, c1, 18, 22, generator=torch.Generator().manual_seed(c1))
    with torch.no_grad():
        ref = twin(x)
        ref16 = {dt: twin.to(dt)(x.to(dt)).float() for dt in (BF16, F16)}
        twin.float()
    blk = blk.to(DEV)
    got = blk(x.to(DEV)).cpu()
    assert got.shape == ref.shape == (2, 4 * c2, (18 - 1) // s + 1, (22 - 1) // s + 1)
    e32 = float((got - ref).abs().max() / ref.abs().max())
    rec = dict(test="standalone_resnetblock", args=list(args), fp32_rel=e32)
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
GOLDENS = ["model_resnet50_kaist_320_b1", "model_resnet50_ninfusion_flir_320x352_b2"]
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
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    e = [float(d[..., :4].max()), float(d[..., :4].mean()), float(d[..., 4:].max()), float(d[..., 4:].mean())]
    return e, all(x <= 1.5 * y for x, y in zip(e, dev))


def check_names(m, golden, rgb):
    names = [l.name for l in m.plan_for(rgb.shape[0], *rgb.shape[2:]).launches]
    assert names.count("resnet_conv1x1+res") == 16 and names.count("resnet_stem7x7s2") == 1 and names.count("preprocess_pad") == 1
    assert names.count("resnet_maxpool") == 1 and names.count("resnet_conv1x1") == 16
    if "ninfusion" not in golden:
        assert names.count("cross_attention") == 3, "every DMFF level runs icaf_cross_attention"
    return names


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
    check_names(m, golden, rgb)
    record(test="model_fp32", golden=golden, **err, bound=bound)
    for k in err:
        assert err[k] <= bound[k], f"{golden}: {k} error {err[k]:.3g} > {bound[k]:.3g}"


@pytest.mark.parametrize("dn,dt", [("bf16", BF16), ("fp16", F16)])
@pytest.mark.parametrize("golden", GOLDENS)
def test_16bit_model_within_the_reference_deviation(golden, dn, dt):
    g, m, (rgb, ir) = model_of(golden)
    m.compute_dtype = dt
    dev = dev16(g, dn)
    z = m(rgb.to(DEV), ir.to(DEV))[0].cpu().numpy()
    check_names(m, golden, rgb)
    assert np.isfinite(z).all()
    e, ok = within16(z, g["z"], dev)
    record(test="model_16bit", golden=golden, dtype=dn, reference_dev=dev, hip=e, order="box max, box mean, score max, score mean")
    assert ok, (e, dev)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_model_entry_points_are_bit_equal(dt):
    """forward_u8 == float forward, unpaired == paired streams, a batch shard == the same rows of the full batch, hipGraph replay == eager."""
    g, m, _ = model_of("model_resnet50_ninfusion_flir_320x352_b2")
    m.compute_dtype = None if dt == F32 else dt
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
        assert [l.name for l in m.plan_for(B, H, W).launches].count("resnet_conv1x1+res") == 32        # one per block and stream
        assert torch.equal(m(rgb, ir)[0], z)
        m.pair_streams, m.use_graph = True, True
        m.invalidate()
        assert m.plan_for(B, H, W).graph is not None
        assert torch.equal(m(rgb, ir)[0], z) and torch.equal(m(rgb, ir)[0], z)
    finally:
        m.pair_streams, m.use_graph = True, False
        m.invalidate()


def test_transfusion_model_graph_equals_eager_in_bf16():
    g, m, (rgb, ir) = model_of("model_resnet50_kaist_320_b1")
    m.compute_dtype = BF16
    z = m(rgb.to(DEV), ir.to(DEV))[0]
    names = check_names(m, "model_resnet50_kaist_320_b1", rgb)
    B, N = rgb.shape[0], 100
    assert ops.cross_attention_form(BF16, B, N, 2048, 8) == 1 and ops.cross_attention_form(BF16, B, 256, 1024, 8) == 0
    # no fp32 fallback: every convolution of the plan computes in bf16 (the type field of its argument block), every attention launch
    # reads and writes bf16 tokens
    launches = m.plan_for(B, *rgb.shape[2:]).launches
    convs = [l for l in launches if l.fn is ops.lib().icaf_conv2d]
    assert len(convs) >= 2 * 16 + 1 and all(l.keep[0].dtype == ops.dtype_code(BF16) for l in convs), "a bf16 plan must not run fp32 convolutions"
    attn = [l for l in launches if l.name == "cross_attention"]
    assert len(attn) == 3 and all(t.dtype is BF16 for l in attn for t in l.keep), "a bf16 plan must not run fp32 attention"
    try:
        m.use_graph = True
        m.invalidate()
        assert m.plan_for(B, *rgb.shape[2:]).graph is not None
        assert torch.equal(m(rgb.to(DEV), ir.to(DEV))[0], z)
    finally:
        m.use_graph = False
        m.invalidate()


def test_tta_on_the_smallest_size():
    g, m, _ = model_of("model_resnet50_ninfusion_flir_320x352_b2")
    m.compute_dtype = BF16
    H, W = m.tta_min_size()
    assert (H, W) == (32, 32)
    rgb, ir = synth_images(1, H, W, seed=9)
    z, second = m(rgb.to(DEV), ir.to(DEV), augment=True)
    assert second is None and z.dtype == torch.float32 and bool(torch.isfinite(z).all())
    plain = m(rgb.to(DEV), ir.to(DEV))[0]
    assert z.shape[1] == 3 * plain.shape[1] and torch.equal(z[:, :plain.shape[1]], plain)       # the first pass is the plain forward
    record(test="tta_min_size", height=H, width=W, rows=int(z.shape[1]))
