"""Calibrated RGB / IR pairs on the MI355X: icaf_letterbox_warp_frames against letterbox(warp_perspective(...)) of utils/datasets.py byte for
byte (default and with the letterbox_direct knob), the forward from a calibrated pair against forward_u8 of the host-built batch, the serving
pipeline fed with pinned native frames and a matrix per submit, and detect_twostream.py --align-ir.  Every comparison is exact."""
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import REPO, load_cfg                                         # noqa: E402
from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.models.yolo import Model                                # noqa: E402
from icafusion_amd.pipeline import DetectionPipeline                       # noqa: E402
from icafusion_amd.synth import synth_state_dict                           # noqa: E402
from icafusion_amd.utils import datasets as D                              # noqa: E402
from icafusion_amd.utils.general import non_max_suppression                # noqa: E402

DEV = "cuda:0"
GUARD = 4096
BOTH = pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])


def build(yaml_name, dtype, seed=0):
    m = Model(load_cfg(yaml_name)).eval()
    m.load_state_dict(synth_state_dict(m, seed))
    m = m.to(DEV)
    m.compute_dtype = None if dtype == torch.float32 else dtype
    m.autotune = False
    return m


def noise(h, w, ch, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, ch), dtype=np.uint8)


def rot(deg, shift=(0.0, 0.0), persp=(0.0, 0.0)):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, shift[0]], [s, c, shift[1]], [persp[0], persp[1], 1.0]], np.float64)


def stretch(src_hw, aligned_hw):
    return D.stretch_alignment(src_hw, aligned_hw).astype(np.float64)


def shift(dx, dy):
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1]], np.float64)


def host_planes(frame, new, swap_rb):
    """(3, H, W) uint8: letterbox() of the frame (a grey frame replicated to three channels first), channels reversed for swap_rb."""
    img = frame if frame.shape[2] == 3 else np.repeat(frame, 3, axis=2)
    lb = D.letterbox(img, new)[0]
    return np.ascontiguousarray((lb[:, :, ::-1] if swap_rb else lb).transpose(2, 0, 1))


class Warped:
    """A source frame of a kind-1 row with its aligned -> source matrix and border."""

    def __init__(self, frame, M, border=0):
        self.frame, self.M, self.border = frame, np.asarray(M, np.float64).astype(np.float32), border

    def aligned(self, hw):
        return D.warp_perspective(self.frame, self.M, hw, self.border)


def want_planes(item, hw, new, swap_rb):
    return host_planes(item.aligned(hw) if isinstance(item, Warped) else item, new, swap_rb)


def run_warp(mods, aligned, new, swap_rb, direct, pitch_extra=0):
    """mods: per modality a list of B items, each a plain frame of the pair's aligned size (a kind-0 row) or a Warped (a kind-1 row);
    aligned: the B aligned (h0, w0).  Frames go into an arena pre-filled with a sentinel (between frames and behind every row when pitch
    exceeds the row), the destination is pre-filled with 0xAB inside guarded surroundings.  ONE launch; returns the (B, 3 * len(mods), H,
    W) result after checking that nothing around it changed."""
    B = len(aligned)
    H, W = (new, new) if isinstance(new, int) else new
    items = [it for m in mods for it in m]
    frames = [it.frame if isinstance(it, Warped) else it for it in items]
    geom1, _ = ops.frame_geometry(aligned, new)
    sources = [tuple(it.frame.shape) if isinstance(it, Warped) else it.shape[2] for it in items]
    for it, hw in zip(items, list(aligned) * len(mods)):
        assert isinstance(it, Warped) or it.shape[:2] == tuple(hw)
    geom, end = ops.pack_warp_frames(np.concatenate([geom1] * len(mods)), sources, [it.M if isinstance(it, Warped) else None for it in items],
                                     [it.border if isinstance(it, Warped) else 0 for it in items],
                                     pitch=[f.shape[1] * f.shape[2] + pitch_extra for f in frames])
    host = np.full((end + 64,), 0x5C, np.uint8)
    for q, f in zip(geom, frames):
        h, w, ch = f.shape
        off, pitch = int(q["g"]["offset"]), int(q["g"]["pitch"])
        host[off:off + h * pitch].reshape(h, pitch)[:, :w * ch] = f.reshape(h, w * ch)
    arena = torch.from_numpy(host).to(DEV)[:end]
    n = B * 3 * len(mods) * H * W
    whole = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    dst = whole[GUARD:GUARD + n].view(B, 3 * len(mods), H, W)
    launch = ops.letterbox_warp_frames(arena, geom, ops.geom_tensor(geom, DEV), dst, swap_rb=swap_rb)
    with ops.letterbox_direct(direct):
        launch(ops.current_stream_ptr())
        torch.cuda.synchronize()
    assert bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + n:] == 0xAB).all()), "the kernel wrote outside its output"
    return dst.cpu().numpy(), geom


def check(mods, aligned, new, swap_rb, direct, pitch_extra=0):
    got, geom = run_warp(mods, aligned, new, swap_rb, direct, pitch_extra)
    for m, mod in enumerate(mods):
        for b, item in enumerate(mod):
            assert np.array_equal(got[b, 3 * m:3 * m + 3], want_planes(item, aligned[b], new, swap_rb)), (m, b)
    return got, geom


# name -> (aligned size, network size, source (hs, ws, ch), aligned -> source matrix)
CASES = {
    "identity-grey": ((48, 60), 64, (48, 60, 1), np.eye(3)),
    "identity-colour": ((48, 60), 64, (48, 60, 3), np.eye(3)),
    "stretch-up": ((48, 60), 64, (24, 30, 1), stretch((24, 30), (48, 60))),
    "stretch-down": ((48, 60), 64, (96, 120, 3), stretch((96, 120), (48, 60))),
    "general": ((120, 128), (96, 160), (53, 37, 3), stretch((53, 37), (120, 128)) @ rot(7, (4.25, -3.5), (2e-4, -1e-4))),
    "horizon": ((37, 53), (64, 96), (37, 53, 1), rot(0, persp=(-0.05, 0.0))),
    "outside": ((48, 60), 64, (20, 20, 1), shift(500, 500)),
    "squeeze": ((300, 400), 64, (150, 200, 1), stretch((150, 200), (300, 400)) @ shift(199.5, 149.5) @ rot(3) @ shift(-199.5, -149.5)),
}


@BOTH
@pytest.mark.parametrize("swap_rb", [True, False], ids=["bgr", "rgb"])
@pytest.mark.parametrize("name", list(CASES))
def test_warp_kernel_equals_host_warp_then_letterbox(name, swap_rb, direct):
    """A plain 3-channel frame of the aligned size (kind 0) beside the warped source (kind 1) in one launch, swap_rb on and off: every
    byte of the six planes equals letterbox(), of the frame and of warp_perspective() of the source — the 0xAB prefill is gone
    everywhere, the sentinel around the frames was never read."""
    hw, new, (hs, ws, ch), M = CASES[name]
    seed = sum(map(ord, name))
    plain, w = noise(*hw, 3, seed), Warped(noise(hs, ws, ch, seed + 1), M, border=0)
    got, geom = check([[plain], [w]], [hw], new, swap_rb, direct)
    # which path the DEFAULT run takes is the host's stage rule, tile by tile: every tile of the cases in view stages its box; behind the
    # horizon (a corner with Z <= 0) and with the source wholly out of view (an empty box) every tile taps global memory
    H, W = got.shape[2:]
    tiles = [(by, bx) for by in range(-(-H // 32)) for bx in range(-(-W // 64))]
    assert ops.warp_letterbox_staged(geom[0], tiles[0]) == ops.letterbox_staged(geom[0]["g"])
    assert [ops.warp_letterbox_staged(geom[1], t) for t in tiles] == [name not in ("horizon", "outside")] * len(tiles)
    if name.startswith("identity"):                                # ... and icaf_letterbox_frames' own bytes for that frame
        again, _ = run_warp([[w.frame]], [hw], new, swap_rb, direct)
        assert np.array_equal(got[:, 3:], again)
    if name == "outside":                                          # the block is all border, the pads 114
        g = ops.frame_geometry([hw], new)[0][0]
        block = np.full(got.shape[2:], 114, np.uint8)
        block[int(g["top"]):int(g["top"] + g["nh"]), int(g["left"]):int(g["left"] + g["nw"])] = 0
        assert np.array_equal(got[0, 3], block) and block.min() == 0 and block.max() == 114
    if name == "horizon":
        assert (w.aligned(hw)[:, 21:] == 0).all() and w.aligned(hw)[:, :10].any()


@BOTH
@pytest.mark.parametrize("border", [0, 114, 255])
def test_warp_kernel_partly_outside(border, direct):
    """Translation by (-20.5, 13.25): a band of the aligned frame lies outside the source, and the blend at its rim mixes source bytes
    with the border."""
    w = Warped(noise(64, 64, 1, 40), shift(-20.5, 13.25), border)
    a = w.aligned((64, 64))
    assert (a[:, :20] == border).all() and (a[51:] == border).all() and len(np.unique(a[:50, 21:])) > 100
    check([[noise(64, 64, 3, 41)], [w]], [(64, 64)], 64, True, direct)


@BOTH
def test_warp_kernel_mixed_batch_row_pitch_and_either_modality(direct):
    """One batch of four pairs — four aligned sizes, four source sizes, a matrix and a border per pair, pitch 7 bytes beyond every row —
    with the thermal modality warped beside a plain visible one in ONE launch, then the visible modality warped onto the thermal one."""
    aligned = [(48, 60), (130, 70), (200, 9), (300, 400)]
    sources = [(24, 30), (53, 37), (64, 64), (150, 200)]
    mats = [stretch(s, a) @ shift((a[1] - 1) / 2, (a[0] - 1) / 2) @ rot(deg, sh, p) @ shift(-(a[1] - 1) / 2, -(a[0] - 1) / 2)
            for s, a, deg, sh, p in zip(sources, aligned, (2, -5, 0, 3), ((1.5, -2.25), (0, 0), (-3.75, 20.5), (10, 4)),
                                        ((0, 0), (1e-4, -2e-4), (0, 0), (-5e-5, 0)))]
    grey = [Warped(noise(*s, 1, 50 + k), M, b) for k, (s, M, b) in enumerate(zip(sources, mats, (0, 114, 255, 7)))]
    colour = [noise(*a, 3, 60 + k) for k, a in enumerate(aligned)]
    check([colour, grey], aligned, 64, True, direct, pitch_extra=7)
    visible = [Warped(noise(*s, 3, 70 + k), M, b) for k, (s, M, b) in enumerate(zip(sources, mats, (0, 114, 255, 7)))]
    thermal = [noise(*a, 1, 80 + k) for k, a in enumerate(aligned)]
    check([visible, thermal], aligned, 64, True, direct, pitch_extra=7)


def host_batch(rgb, ir, new):
    """The uint8 (B, 6, H, W) batch LoadImages + np.concatenate hand to forward_u8, from BGR frames."""
    return torch.from_numpy(np.stack([np.concatenate((host_planes(a, new, True), host_planes(b, new, True)), 0) for a, b in zip(rgb, ir)]))


def pair_matrices(src_shapes, shapes, seed):
    g = np.random.default_rng(seed)
    return np.stack([stretch(s, a) @ shift((a[1] - 1) / 2, (a[0] - 1) / 2) @ rot(g.uniform(-4, 4), g.uniform(-6, 6, 2), g.uniform(-1e-4, 1e-4, 2)) @
                     shift(-(a[1] - 1) / 2, -(a[0] - 1) / 2) for s, a in zip(src_shapes, shapes)]).astype(np.float32)


def dev(frames):
    return [torch.from_numpy(f).to(DEV) for f in frames]


def test_forward_from_a_calibrated_pair_equals_forward_from_the_host_warp():
    """yolov5s kaist, bf16, 320 x 320, two pairs whose thermal frames have other sizes than the visible ones, a matrix per pair:
    forward_frames(align=(None, M)) is forward_u8 of letterbox(warp_perspective(...)) beside the plain letterbox bit for bit.  The second
    call has other source sizes and matrices (no stale table), the third the first shapes and NEW matrices (the matrices are not part of
    the cached state)."""
    m = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    ref = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    first = ([(240, 300), (256, 320)], [(120, 160), (100, 90)])
    for seed, (shapes, src_shapes), border in ((21, first, 0), (22, ([(240, 300), (256, 320)], [(64, 80), (128, 160)]), 114), (23, first, 0)):
        rgb = [noise(*s, 3, seed + k) for k, s in enumerate(shapes)]
        ir = [noise(*s, 1, seed + 10 + k) for k, s in enumerate(src_shapes)]
        M = pair_matrices(src_shapes, shapes, seed)
        (z, logits, raws), info = m.forward_frames(dev(rgb), dev(ir), 320, align=(None, M), align_border=border)
        warped = [D.warp_perspective(f, M[k], shapes[k], border) for k, f in enumerate(ir)]
        wz, wlogits, wraws = ref.forward_u8(host_batch(rgb, warped, 320).to(DEV))
        assert torch.equal(z, wz) and torch.equal(logits, wlogits) and all(torch.equal(a, b) for a, b in zip(raws, wraws)), seed
        assert np.array_equal(info.scale.cpu().numpy(), ops.frame_geometry(shapes, 320)[1])
    assert sum(1 for k in m._frame_states if "align" in k) == 2                # the third call found the first call's state
    one = torch.from_numpy(np.stack([noise(120, 160, 1, 30), noise(120, 160, 1, 31)])).to(DEV)      # a (B, hs, ws, 1) tensor, "stretch"
    (z, _, _), _ = m.forward_frames(dev(rgb), one, 320, align=(None, "stretch"))
    warped = [D.warp_perspective(f, D.stretch_alignment((120, 160), s), s) for f, s in zip(one.cpu().numpy(), shapes)]
    assert torch.equal(z, ref.forward_u8(host_batch(rgb, warped, 320).to(DEV))[0])
    for kw, msg in (({"align": (M, M)}, "both"), ({"align": (None, M), "val_size": 320}, "val_size"),
                    ({"align": (None, M), "formats": (None, "nv12")}, "YUV"), ({"align": (None, M[:, :2])}, r"\(3, 3\)"),
                    ({"align": (None, M * np.float32("nan"))}, "non-finite")):
        with pytest.raises(ValueError, match=msg):
            m.forward_frames(dev(rgb), dev(ir), 320, **kw)


@pytest.mark.parametrize("depth", [1, 2])
def test_pipeline_fed_with_pinned_calibrated_pairs(depth):
    """Four steps from pinned host memory, other sizes and matrices each: submit_frames(align=M) returns the detections of
    forward_frames(align=M) + non_max_suppression + scale_detections, in the visible frame's native space — step by step, then with all
    steps enqueued without waiting."""
    m, ref = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16), build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    m.use_graph = True
    B, S = 2, 320
    pipe = DetectionPipeline(m, B, S, S, DEV, conf_thres=0.1, iou_thres=0.5, depth=depth, frames=(320, 320), frame_channels=(3, 1),
                             frame_align=(None, True), align_frames=(160, 200), align_border=114)
    sizes = [([(240, 300), (256, 320)], [(120, 160), (100, 90)]), ([(256, 320), (256, 320)], [(128, 160), (128, 160)]),
             ([(320, 200), (100, 320)], [(160, 100), (50, 200)]), ([(256, 320), (256, 320)], [(128, 160), (128, 160)])]
    steps, want = [], []
    for k, (shapes, src_shapes) in enumerate(sizes):
        rgb = [noise(*s, 3, 50 + 2 * k + i) for i, s in enumerate(shapes)]
        ir = [noise(*s, 1, 70 + 2 * k + i) for i, s in enumerate(src_shapes)]
        M = "stretch" if k == 3 else pair_matrices(src_shapes, shapes, 90 + k)[0] if k == 1 else pair_matrices(src_shapes, shapes, 90 + k)
        if shapes[0] == shapes[1]:                                          # uniform batches: one (B, H0, W0, ch) tensor per modality
            feed = (torch.from_numpy(np.stack(rgb)).pin_memory(), torch.from_numpy(np.stack(ir)).pin_memory())
        else:
            feed = ([torch.from_numpy(f).pin_memory() for f in rgb], [torch.from_numpy(f).pin_memory() for f in ir])
        steps.append((feed, M))
        (z, _, _), info = ref.forward_frames(dev(rgb), dev(ir), S, align=(None, M), align_border=114)
        dets = non_max_suppression(z, 0.1, 0.5)
        for b, d in enumerate(dets):
            if len(d):
                block = d.unsqueeze(0).contiguous()
                ops.scale_detections(block, torch.tensor([len(d)], dtype=torch.int32, device=DEV), info.scale[b:b + 1].contiguous())(ops.current_stream_ptr())
                dets[b] = block[0]
        torch.cuda.synchronize()
        want.append([d.cpu() for d in dets])
    assert sum(len(d) for w in want for d in w) > 0

    def check_step(k, det, count):
        assert count.cpu().tolist() == [len(d) for d in want[k]], k
        for b, d in enumerate(want[k]):
            assert torch.equal(det[b, :len(d)].cpu(), d), (k, b)
            assert not det[b, len(d):].cpu().any()
    for k, (feed, M) in enumerate(steps):                                   # step by step
        det, count = (t[0] for t in pipe.submit_frames(*feed, align=M))
        pipe.synchronize()
        check_step(k, det, count)
    outs = [tuple(t[0] for t in pipe.submit_frames(*feed, align=M)) for feed, M in steps]      # all in flight
    pipe.synchronize()
    for k in range(len(steps) - pipe.nplans, len(steps)):                   # the last `nplans` steps still own their output buffers
        check_step(k, *outs[k])
    with pytest.raises(ValueError, match="align_frames"):
        pipe.submit_frames(torch.zeros((B, 320, 320, 3), dtype=torch.uint8), torch.zeros((B, 161, 200, 1), dtype=torch.uint8), align="stretch")
    with pytest.raises(ValueError, match="both or neither"):
        pipe.submit_frames(*steps[0][0])


def test_detect_twostream_align_ir_device_equals_host(tmp_path, capsys):
    """Two pairs whose thermal images are half the size of the visible ones, --align-ir file.txt with and without --device-letterbox: the
    same printed detections, label files and annotated images (timings apart)."""
    sys.path.insert(0, REPO)
    import detect_twostream as dt
    from test_frontends import make_dataset
    rgb_dir, ir_full = make_dataset(str(tmp_path), n=2, size=(120, 128), nc=3, seed=5)
    ir_dir = tmp_path / "thermal"
    ir_dir.mkdir()
    for name in sorted(os.listdir(ir_full)):
        D.imwrite_bgr(str(ir_dir / name), D.resize_bilinear(D.imread_bgr(os.path.join(ir_full, name)), (64, 60)))
    M = stretch((60, 64), (120, 128)) @ shift(63.5, 59.5) @ rot(1.5, (1.25, -0.75)) @ shift(-63.5, -59.5)
    (tmp_path / "rig.txt").write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in M))
    cfg_path = os.path.join(REPO, "models", "transformer", "yolov5s_Transfusion_FLIR.yaml")
    runs = {}
    for name, extra in (("host", []), ("device", ["--device-letterbox"])):
        opt = dt.parse_opt(["--cfg", cfg_path, "--source1", rgb_dir, "--source2", str(ir_dir), "--img-size", "320", "--conf-thres", "0.3",
                            "--save-txt", "--save-conf", "--project", str(tmp_path / "runs"), "--name", name, "--align-ir", str(tmp_path / "rig.txt"),
                            "--align-border", "114"] + extra)
        capsys.readouterr()
        out_dir = dt.detect(opt)
        printed = [re.sub(r"Done\. \(.*", "", ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("image ")]
        files = {str(p.relative_to(out_dir)): p.read_bytes() for p in sorted(out_dir.rglob("*")) if p.is_file()}
        runs[name] = (printed, files)
    assert len(runs["host"][0]) == 2 and runs["host"][0] == runs["device"][0]
    assert any(k.startswith("labels") for k in runs["host"][1]) and sum(k.endswith(".png") for k in runs["host"][1]) == 4
    assert runs["host"][1].keys() == runs["device"][1].keys()
    for k, v in runs["host"][1].items():
        assert v == runs["device"][1][k], k
