"""Test-time augmentation on the MI355X (Model.forward(augment=True), reference models/yolo_test.py:116-131): the staging kernel against
torch's CPU resize, the composition against the plain forward bit for bit, the whole step against the CPU oracle, the serving pipeline
and the detect front end."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tta_helpers as T                                                     # noqa: E402
from helpers import REPO, load_cfg                                         # noqa: E402
from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.models.yolo import Model, tta_sizes                     # noqa: E402
from icafusion_amd.pipeline import DetectionPipeline                       # noqa: E402
from icafusion_amd.synth import synth_images, synth_state_dict             # noqa: E402
from icafusion_amd.utils.general import non_max_suppression                # noqa: E402
from oracle import icaf_oracle as oracle                                   # noqa: E402

DEV = "cuda:0"
GUARD = 4096                        # poisoned floats / bytes on each side of every buffer the kernel touches
NAN_A, NAN_B = 0x7FC0BEEF, 0x7FC0FACE           # two quiet-NaN patterns: the surroundings, the output prefill


def build(yaml_name, seed, dtype=torch.float32):
    cfg = load_cfg(yaml_name)
    m = Model(cfg).eval()
    sd = synth_state_dict(m, seed)
    m.load_state_dict(sd)
    m = m.to(DEV)
    if dtype != torch.float32:
        m.compute_dtype = dtype
    return cfg, sd, m


def guarded(shape, dtype, fill_bits):
    """(whole buffer, view of `shape` in its middle): the view starts GUARD elements in (16-byte aligned for fp32), everything — the view
    included — filled with a NaN pattern (fp32) or 0xA5 (uint8)."""
    n = int(np.prod(shape))
    if dtype == torch.uint8:
        whole = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    else:
        whole = torch.full((n + 2 * GUARD,), fill_bits, dtype=torch.int32, device=DEV).view(torch.float32)
    return whole, whole[GUARD:GUARD + n].view(shape)


def guards_intact(whole, n, fill_bits):
    w = whole.view(torch.int32) if whole.dtype == torch.float32 else whole
    want = fill_bits if whole.dtype == torch.float32 else 0xA5
    return bool((w[:GUARD] == want).all()) and bool((w[GUARD + n:] == want).all())


def run_stage(src, passes, shift=0):
    """passes: [(Hr, Wr, Hp, Wp, flip)].  src is copied into a poisoned buffer; every output is a NaN-prefilled view inside poisoned
    surroundings.  Returns the outputs (CPU) after checking that nothing around them changed.  shift: move the source view by that many
    elements (an address the aligned vector loads of the LDS-staged kernel cannot take: the launcher then runs the gather kernel)."""
    B = src.shape[-4]
    swhole, sview = guarded(tuple(src.shape), src.dtype, NAN_A)
    if shift:
        sview = swhole[GUARD + shift:GUARD + shift + src.numel()].view(src.shape)
    sview.copy_(src)
    outs = [guarded((2, B, 3, hp, wp), torch.float32, NAN_A) for (_, _, hp, wp, _) in passes]
    for whole, view in outs:
        view.view(torch.int32).fill_(NAN_B)
    launch = ops.tta_stage(sview, [(view, hr, wr, flip) for (whole, view), (hr, wr, _, _, flip) in zip(outs, passes)])
    launch(ops.current_stream_ptr())
    torch.cuda.synchronize()
    w = swhole.view(torch.int32) if swhole.dtype == torch.float32 else swhole
    fill = NAN_A if swhole.dtype == torch.float32 else 0xA5
    assert bool((w[:GUARD + shift] == fill).all()) and bool((w[GUARD + shift + sview.numel():] == fill).all()) and torch.equal(sview, src.to(DEV))
    for whole, view in outs:
        assert guards_intact(whole, view.numel(), NAN_A), "the kernel wrote outside its output"
        assert not torch.isnan(view).any(), "an output element was not written, or a poisoned source byte was read"
    return [view.cpu() for _, view in outs]


SHAPES = [(448, 448), (480, 640), (640, 640), (544, 672)]


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("ratio", [0.83, 0.67])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_stage_kernel_matches_torch_cpu(shape, ratio, flip):
    """icaf_tta_stage against F.pad(F.interpolate(x.flip(3)?, size, 'bilinear', align_corners=False), value=0.447) on the CPU, fp32 and
    uint8 sources.  Interior within 2^-21 absolute for inputs in [0, 1] (seven interpolation operations on each side, each worth at most
    2^-25); padding bit-equal to float32(0.447); the uint8 result bit-equal to the result from u8.float() / 255; NaN-prefilled output,
    poisoned surroundings of source and output."""
    H, W = shape
    B = 2
    g = np.random.default_rng([7, H, W, int(ratio * 100), int(flip)])
    hr, wr, hp, wp = T.sizes(H, W, ratio)
    x32 = torch.from_numpy(g.random((2, B, 3, H, W), dtype=np.float32))
    u8 = torch.from_numpy(g.integers(0, 256, (B, 6, H, W), dtype=np.uint8))
    xu = u8.float() / 255.0                                              # true division on the CPU, as the reference
    xu_pair = torch.stack((xu[:, :3], xu[:, 3:])).contiguous()
    got32, = run_stage(x32.to(DEV), [(hr, wr, hp, wp, flip)])
    got_u8, = run_stage(u8.to(DEV), [(hr, wr, hp, wp, flip)])
    got_uf, = run_stage(xu_pair.to(DEV), [(hr, wr, hp, wp, flip)])
    assert torch.equal(got_u8, got_uf), "staging from uint8 differs from staging from u8.float() / 255"
    pad = torch.tensor(0.447, dtype=torch.float32)
    for name, got, x in (("fp32", got32, x32), ("uint8", got_u8, xu_pair)):
        want = T.scale_img_cpu(x.view(2 * B, 3, H, W), ratio, flip).view(2, B, 3, hp, wp)
        err = float((got[..., :hr, :wr] - want[..., :hr, :wr]).abs().max())
        print(f"stage {H}x{W} ratio {ratio} flip {int(flip)} {name}: {hr}x{wr} in {hp}x{wp}, interior max error {err:.3g} ({err * 2 ** 24:.2f} x 2^-24)")
        assert err <= 2.0 ** -21, (name, err)
        assert torch.equal(got[..., hr:, :], pad.expand_as(got[..., hr:, :])) and torch.equal(got[..., :, wr:], pad.expand_as(got[..., :, wr:]))
        assert torch.equal(want[..., hr:, :], pad.expand_as(want[..., hr:, :]))


def test_stage_kernel_both_passes_in_one_launch():
    """The launch the TTA plan makes (0.83 flipped and 0.67 plain of one source) equals the two single-pass launches bit for bit."""
    H, W, B = 544, 672, 3
    g = np.random.default_rng(11)
    x = torch.from_numpy(g.random((2, B, 3, H, W), dtype=np.float32)).to(DEV)
    passes = [T.sizes(H, W, 0.83) + (True,), T.sizes(H, W, 0.67) + (False,)]
    both = run_stage(x, passes)
    for p, got in zip(passes, both):
        assert torch.equal(got, run_stage(x, [p])[0])


@pytest.mark.parametrize("dtype,graph", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True)], ids=["fp32", "bf16", "bf16-graph"])
def test_composition_is_exact(dtype, graph):
    """m(x, x2, augment=True)[0] is bit-equal to a CPU merge (/ float32(si), W - x, cat) of m(xi, xi2)[0], xi being the staging kernel's
    own output read back and each plain forward going through the existing path; the second return value is None, the rows sum N_i;
    forward_u8(augment=True) equals forward(u8 / 255, augment=True); static_outputs returns the plan's own buffer."""
    cfg, sd, m = build("yolov5s_Transfusion_kaist.yaml", 31, dtype)
    m.use_graph = graph
    B, H, W = 2, 480, 640
    rgb, ir = synth_images(B, H, W, seed=31)
    z, second = m(rgb.to(DEV), ir.to(DEV), augment=True)
    assert second is None and z.dtype == torch.float32
    tp = m.tta_plan_for(B, H, W)
    assert [p[2:] for p in tp.passes] == [p[2:] for p in tta_sizes(H, W)] and len(tp.plans) == 3
    xis = [p.input_pair.clone() for p in tp.plans]
    assert torch.equal(xis[0][0].cpu(), rgb) and torch.equal(xis[0][1].cpu(), ir)
    zs = [m(xi[0], xi[1])[0].cpu().numpy() for xi in xis]
    want = T.merge_cpu(zs, W)
    assert z.shape[1] == sum(a.shape[1] for a in zs) == want.shape[1]
    assert np.array_equal(z.cpu().numpy(), want)
    # uint8 batch: the scaled passes staged straight from it
    img6 = (torch.cat((rgb, ir), 1) * 255).round().to(torch.uint8)
    f = img6.float() / 255.0
    zf = m(f[:, :3].contiguous().to(DEV), f[:, 3:].contiguous().to(DEV), augment=True)[0]
    zu, none = m.forward_u8(img6.to(DEV), augment=True)
    assert none is None and torch.equal(zu, zf)
    m.static_outputs = True
    try:
        zs_ = m(rgb.to(DEV), ir.to(DEV), augment=True)[0]
        assert zs_.data_ptr() == m.tta_plan_for(B, H, W).outputs.data_ptr() and torch.equal(zs_, z)
    finally:
        m.static_outputs = False


def test_replay_allocates_nothing_and_survives_cache_eviction():
    """A replay of the TTA plan allocates no device memory; the plan keeps its sub-plans alive when the LRU cache drops them."""
    cfg, sd, m = build("yolov5s_Transfusion_kaist.yaml", 33, torch.bfloat16)
    B, H, W = 1, 448, 448
    rgb, ir = synth_images(B, H, W, seed=33)
    tp = m.tta_plan_for(B, H, W)
    tp.inputs[0].copy_(rgb); tp.inputs[1].copy_(ir)
    tp.run()
    torch.cuda.synchronize()
    first = tp.outputs.clone()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    for _ in range(3):
        tp.run()
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    m.__dict__["_plans"].clear()                                   # what eviction does: the cache forgets every plan
    tp.run()
    torch.cuda.synchronize()
    assert torch.equal(tp.outputs, first)


def test_too_small_input_raises_on_the_device_path():
    cfg, sd, m = build("yolov5s_Transfusion_kaist.yaml", 1)
    x = torch.zeros(1, 3, 416, 448, device=DEV)
    with pytest.raises(ValueError, match="448x448"):
        m(x, x, augment=True)
    with pytest.raises(ValueError, match="448x448"):
        m.forward_u8(torch.zeros(1, 6, 416, 448, dtype=torch.uint8, device=DEV), augment=True)


@pytest.mark.parametrize("B,H,W", [(2, 448, 448), (1, 480, 640)])
def test_fp32_tta_matches_oracle(B, H, W):
    """End to end, fp32 build: forward(augment=True) against OracleModel.forward on CPU-resized inputs merged on the CPU.  The project's
    absolute bounds (tests/test_gpu_model.py::_assert_abs: 2e-2 px, 2e-4 score); the box bound of pass i is divided by si, because the
    merge scales the error by 1 / si.  Measured errors are appended to parity_tta.jsonl in the results folder
    of the evidence scripts ($OUT, default results/; profiles/parity_tta.json: one committed run)."""
    seed = 300 + (0 if H == 448 else 1)
    cfg, sd, m = build("yolov5s_Transfusion_kaist.yaml", seed)
    rgb, ir = synth_images(B, H, W, seed)
    ref, ref_passes = T.oracle_tta(oracle.OracleModel(cfg, sd), rgb, ir)
    z = m(rgb.to(DEV), ir.to(DEV), augment=True)[0].cpu().numpy()
    assert z.shape == ref.shape
    rec = {"yaml": "yolov5s_Transfusion_kaist.yaml", "batch": B, "height": H, "width": W, "rows": int(z.shape[1]), "passes": []}
    off, ok = 0, True
    for zp, (s, f, hr, wr, hp, wp) in zip(ref_passes, tta_sizes(H, W)):
        n = zp.shape[1]
        a, b = z[:, off:off + n], ref[:, off:off + n]
        e_box, e_sc = float(np.abs(a[..., :4] - b[..., :4]).max()), float(np.abs(a[..., 4:] - b[..., 4:]).max())
        bound = 2e-2 / s
        print(f"TTA {B}x{H}x{W} pass scale {s} flip {f} ({hp}x{wp}, {n} rows): box error {e_box:.3g} px (bound {bound:.3g}), score error {e_sc:.3g}")
        rec["passes"].append({"scale": s, "flip": bool(f), "height": hp, "width": wp, "rows": n, "box_px": e_box, "box_px_bound": bound,
                              "score": e_sc, "score_bound": 2e-4})
        ok = ok and e_box <= bound and e_sc <= 2e-4
        off += n
    try:
        out = os.path.join(REPO, os.environ.get("OUT") or "results")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_tta.jsonl"), "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    assert off == z.shape[1] and ok, rec


@pytest.mark.parametrize("depth", [1, 2])
def test_pipeline_with_augment_equals_forward_plus_nms(depth):
    """DetectionPipeline(augment=True): every step's detections are bit-equal to non_max_suppression(m(x, x2, augment=True)[0])."""
    cfg, sd, m = build("yolov5s_Transfusion_FLIR.yaml", 0, torch.bfloat16)
    m.use_graph = True
    B, H, W = 2, 448, 480
    pipe = DetectionPipeline(m, B, H, W, DEV, conf_thres=0.25, iou_thres=0.45, depth=depth, augment=True)
    rows = sum((p[4] // s) * (p[5] // s) * 3 for p in tta_sizes(H, W) for s in (8, 16, 32))
    assert all(p.outputs.shape == (B, rows, 8) for p in pipe.plans) and len({p.outputs.data_ptr() for p in pipe.plans}) == depth
    batches = [synth_images(B, H, W, seed=70 + k) for k in range(4)]
    outs = [tuple(t[0] for t in pipe.submit(rgb.to(DEV), ir.to(DEV))) for rgb, ir in batches]
    pipe.synchronize()
    cfg, sd, ref = build("yolov5s_Transfusion_FLIR.yaml", 0, torch.bfloat16)          # an independent model, one batch at a time
    for k in range(len(batches) - depth, len(batches)):                                # the last `depth` steps still own their buffers
        rgb, ir = batches[k]
        want = non_max_suppression(ref(rgb.to(DEV), ir.to(DEV), augment=True)[0], 0.25, 0.45)
        det, count = outs[k]
        assert sum(count.tolist()) > 0
        assert all(torch.equal(det[i, :n], w) for (i, n), w in zip(enumerate(count.tolist()), want)), f"step {k}"


def test_detect_twostream_augment_runs(tmp_path):
    """detect_twostream.py --augment on two synthetic frames: label files and annotated images are written."""
    sys.path.insert(0, REPO)
    import detect_twostream as dt
    from icafusion_amd.utils.datasets import imwrite_bgr
    g = np.random.default_rng(9)
    rgb_dir, ir_dir = str(tmp_path / "visible"), str(tmp_path / "infrared")
    for d in (rgb_dir, ir_dir):
        os.makedirs(d)
        for i in range(2):
            imwrite_bgr(os.path.join(d, f"im{i:03d}.png"), g.integers(0, 256, (200, 224, 3), dtype=np.uint8))
    cfg_path = os.path.join(REPO, "models", "transformer", "yolov5s_Transfusion_FLIR.yaml")
    argv = ["--cfg", cfg_path, "--source1", rgb_dir, "--source2", ir_dir, "--img-size", "480", "--conf-thres", "0.3", "--save-txt",
            "--save-conf", "--project", str(tmp_path / "runs")]
    plain = dt.detect(dt.parse_opt(argv + ["--name", "plain"]))
    aug = dt.detect(dt.parse_opt(argv + ["--name", "aug", "--augment"]))
    assert len(list(aug.glob("*_rgb.png"))) == 2 and len(list(aug.glob("*_ir.png"))) == 2
    n_plain = sum(len(open(t).readlines()) for t in (plain / "labels").glob("*.txt"))
    n_aug = sum(len(open(t).readlines()) for t in (aug / "labels").glob("*.txt"))
    print(f"detect_twostream: {n_plain} detections plain, {n_aug} with --augment")
    assert n_aug >= 1
    rows = np.loadtxt(sorted((aug / "labels").glob("*.txt"))[0], ndmin=2)
    assert rows.shape[1] == 6 and (rows[:, 1:5] >= 0).all() and (rows[:, 1:5] <= 1).all()
