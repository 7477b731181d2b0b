"""Native camera frames on the MI355X: the device letterbox against utils.datasets.letterbox byte for byte (both of its paths), the forward and
the TTA step from frames against forward_u8 of the host-letterboxed batch, scale_detections against scale_coords, the serving pipeline fed
with pinned native frames, and detect_twostream.py --device-letterbox.  Every comparison is exact."""
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
from icafusion_amd.utils.general import scale_coords                       # noqa: E402

DEV = "cuda:0"
GUARD = 4096
# the shapes of tests/test_frames_host.py plus one with several tiles in each direction (96 rows = three 32-row tiles, 160 columns); every
# output is a whole multiple of the 32 x 64 tile (letterbox always pads to the requested size)
SHAPES = [((48, 60), 64), ((60, 48), 64), ((37, 53), (64, 96)), ((64, 64), 64), ((200, 9), 64), ((130, 70), 64), ((33, 64), 64),
          ((120, 128), (96, 160))]
# one more frame, squeezed 4.7 x: the rectangle a tile taps (154 rows of 1216 bytes) exceeds the LDS budget, so its tiles tap global memory
# by DEFAULT — the path a 4K frame takes, at a size a test can afford
DIRECT = ((300, 400), 64)
IDS = [f"{h}x{w}" for (h, w), _ in SHAPES + [DIRECT]]


def build(yaml_name, dtype, seed=0):
    m = Model(load_cfg(yaml_name)).eval()
    m.load_state_dict(synth_state_dict(m, seed))
    m = m.to(DEV)
    m.compute_dtype = None if dtype == torch.float32 else dtype
    m.autotune = False
    return m


def host_planes(frame, new, swap_rb):
    """(3, H, W) uint8: letterbox() of the frame (a grey frame replicated to three channels first), channels reversed for swap_rb."""
    img = frame if frame.shape[2] == 3 else np.repeat(frame, 3, axis=2)
    lb = D.letterbox(img, new)[0]
    return np.ascontiguousarray((lb[:, :, ::-1] if swap_rb else lb).transpose(2, 0, 1))


def host_batch(rgb, ir, new):
    """The uint8 (B, 6, H, W) batch LoadImages + np.concatenate hand to forward_u8, from BGR frames."""
    return torch.from_numpy(np.stack([np.concatenate((host_planes(a, new, True), host_planes(b, new, True)), 0) for a, b in zip(rgb, ir)]))


def run_letterbox(mods, new, swap_rb, direct, pitch_extra=0):
    """mods: per modality a list of B frames (h0, w0, ch).  Frames go into an arena pre-filled with a sentinel (between frames and behind
    every row when pitch > w0 * ch), the destination is pre-filled with 0xAB inside poisoned surroundings.  Returns the (B, 3 * len(mods),
    H, W) result after checking that nothing around it changed."""
    B = len(mods[0])
    H, W = (new, new) if isinstance(new, int) else new
    frames = [f for m in mods for f in m]
    geom1, _ = ops.frame_geometry([f.shape[:2] for f in mods[0]], new)
    geom = np.concatenate([geom1] * len(mods))
    pitches = [f.shape[1] * f.shape[2] + pitch_extra for f in frames]
    end = ops.pack_frames(geom, [f.shape[2] for f in frames], pitch=pitches)
    host = np.full((end + 64,), 0x5C, np.uint8)
    for g, f in zip(geom, frames):
        h0, w0, ch = f.shape
        rows = host[int(g["offset"]):int(g["offset"]) + h0 * int(g["pitch"])].reshape(h0, int(g["pitch"]))
        rows[:, :w0 * ch] = f.reshape(h0, w0 * ch)
    arena = torch.from_numpy(host).to(DEV)[:end]
    n = B * 3 * len(mods) * H * W
    whole = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    dst = whole[GUARD:GUARD + n].view(B, 3 * len(mods), H, W)
    launch = ops.letterbox_frames(arena, geom, ops.geom_tensor(geom, DEV), dst, swap_rb=swap_rb)
    with ops.letterbox_direct(direct):
        launch(ops.current_stream_ptr())
        torch.cuda.synchronize()
    assert bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + n:] == 0xAB).all()), "the kernel wrote outside its output"
    return dst.cpu().numpy(), geom


def frames_of(shapes, ch, seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (h, w, ch), dtype=np.uint8) for h, w in shapes]


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
@pytest.mark.parametrize("swap_rb", [True, False], ids=["bgr", "rgb"])
@pytest.mark.parametrize("shape,new", SHAPES + [DIRECT], ids=IDS)
def test_letterbox_kernel_equals_host_letterbox(shape, new, swap_rb, direct):
    """One 3-channel and one grey frame of the shape (two modalities, one launch), default path and forced direct path: every byte of
    the six planes equals letterbox() — the 0xAB prefill is gone everywhere, the sentinel around the frames was never read."""
    rgb, ir = frames_of([shape], 3, 11 + shape[0]), frames_of([shape], 1, 12 + shape[1])
    got, geom = run_letterbox([rgb, ir], new, swap_rb, direct)
    assert np.array_equal(got[0, :3], host_planes(rgb[0], new, swap_rb))
    assert np.array_equal(got[0, 3:], host_planes(ir[0], new, swap_rb))
    # which branch the DEFAULT path takes is the host's budget rule: everything in the list stages, the squeezed frame does not
    assert all(ops.letterbox_staged(g) for g in geom) == ((shape, new) != DIRECT)


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
def test_letterbox_kernel_mixed_batch_and_row_pitch(direct):
    """One batch of four different frame sizes (up-scale, down-scale, a 3-pixel-wide block, one whose tiles go direct by default), with
    pitch > w0 * ch; the second modality is grey."""
    shapes = [(48, 60), (130, 70), (200, 9), (300, 400)]
    rgb, ir = frames_of(shapes, 3, 3), frames_of(shapes, 1, 4)
    got, geom = run_letterbox([rgb, ir], 64, True, direct, pitch_extra=7)
    assert [ops.letterbox_staged(g) for g in geom[:4]] == [True, True, True, False]
    for b in range(4):
        assert np.array_equal(got[b, :3], host_planes(rgb[b], 64, True)), b
        assert np.array_equal(got[b, 3:], host_planes(ir[b], 64, True)), b


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_forward_from_frames_equals_forward_from_the_host_letterbox(dtype):
    """yolov5s kaist at 320 x 320, two pairs of different native sizes: forward_frames is forward_u8 of the host-letterboxed batch bit for
    bit; a second call with other frames of other sizes shows no stale arena or table."""
    m = build("yolov5s_Transfusion_kaist.yaml", dtype)
    ref = build("yolov5s_Transfusion_kaist.yaml", dtype)
    for seed, shapes in ((21, [(240, 300), (256, 320)]), (22, [(320, 200), (100, 320)]), (23, [(240, 300), (256, 320)])):
        rgb, ir = frames_of(shapes, 3, seed), frames_of(shapes, 3, seed + 100)
        (z, logits, raws), info = m.forward_frames([torch.from_numpy(f).to(DEV) for f in rgb], [torch.from_numpy(f).to(DEV) for f in ir], 320)
        wz, wlogits, wraws = ref.forward_u8(host_batch(rgb, ir, 320).to(DEV))
        assert torch.equal(z, wz) and torch.equal(logits, wlogits) and all(torch.equal(a, b) for a, b in zip(raws, wraws)), shapes
        assert np.array_equal(info.scale.cpu().numpy(), ops.frame_geometry(shapes, 320)[1])
    uniform = np.stack(frames_of([(256, 320)] * 2, 3, 5))                      # a (B, H0, W0, ch) tensor, frames in RGB order
    (z, _, _), _ = m.forward_frames(torch.from_numpy(uniform).to(DEV), torch.from_numpy(uniform).to(DEV), 320, bgr=False)
    flipped = [np.ascontiguousarray(f[:, :, ::-1]) for f in uniform]
    assert torch.equal(z, ref.forward_u8(host_batch(flipped, flipped, 320).to(DEV))[0])


def test_forward_frames_of_every_kind_from_one_state_cache():
    """One yolov5s bf16 model at 320 x 320, the smallest size its DMFF blocks take (20 x 20 tokens at stride 16), two pairs of 48 x 80 and
    60 x 44 (one padded above and below, the other left and right): forward_frames as plain, NV12 visible, 16-bit thermal, a 36 x 50 thermal
    source through a rotation, plain again, then the four in reverse.  The four kinds of table (ops.KINDS) share ONE cache of states and
    rebind their launches to one plan input: every result is forward_u8 of the host-prepared batch bit for bit, and the second visit of a
    kind equals its first."""
    m, ref = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16), build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    new, shapes = 320, [(48, 80), (60, 44)]
    g = np.random.default_rng(70)
    rgb, grey, src = frames_of(shapes, 3, 71), frames_of(shapes, 1, 72), frames_of([(36, 50)] * 2, 1, 73)
    planes = [(g.integers(0, 256, (h, w), dtype=np.uint8), g.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
               g.integers(0, 256, (h // 2, w // 2), dtype=np.uint8)) for h, w in shapes]
    nv12 = [np.concatenate((y, np.stack((cb, cr), -1).reshape(y.shape[0] // 2, y.shape[1]))) for y, cb, cr in planes]
    raw = [g.integers(28000, 34000, s).astype(np.uint16) for s in shapes]
    M = np.array([[0.6 * np.cos(0.1), -0.6 * np.sin(0.1), 3.0], [0.6 * np.sin(0.1), 0.6 * np.cos(0.1), 1.5], [0.0, 0.0, 1.0]], np.float32)
    dev = lambda frames: [torch.from_numpy(f).to(DEV) for f in frames]
    calls = {"plain": (rgb, grey, {}, (rgb, grey)),
             "yuv": (nv12, grey, {"formats": ("nv12", None)}, ([D.yuv420_to_bgr(*p) for p in planes], grey)),
             "y16": (rgb, [f.view(np.int16) for f in raw], {"formats": (None, "y16")}, (rgb, [D.agc_u16_to_u8(f, *D.agc_window(f))[:, :, None] for f in raw])),
             "align": (rgb, src, {"align": (None, M), "align_border": 7}, (rgb, [D.warp_perspective(f, M, s, 7) for f, s in zip(src, shapes)]))}
    want = {k: ref.forward_u8(host_batch(*host, new).to(DEV)) for k, (_, _, _, host) in calls.items()}
    assert not torch.equal(want["plain"][0], want["y16"][0]) and not torch.equal(want["plain"][0], want["align"][0])
    first = {}
    for k in ("plain", "yuv", "y16", "align", "plain", "align", "y16", "yuv", "plain"):
        a, b, kw, _ = calls[k]
        (z, logits, raws), info = m.forward_frames(dev(a), dev(b), new, **kw)
        wz, wlogits, wraws = want[k]
        assert torch.equal(z, wz) and torch.equal(logits, wlogits) and all(torch.equal(x, y) for x, y in zip(raws, wraws)), k
        assert np.array_equal(info.scale.cpu().numpy(), ops.frame_geometry(shapes, new)[1]) and info.geom.dtype == ops.KINDS[k].dtype
        assert torch.equal(z, first.setdefault(k, z.clone())), k
    assert sorted(key[0] for key in m._frame_states) == ["align", "plain", "y16", "yuv"]


def test_tta_from_frames_equals_tta_from_the_host_letterbox():
    m = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    ref = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    assert m.tta_min_size() == (448, 448)
    rgb, ir = frames_of([(300, 400)], 3, 31), frames_of([(300, 400)], 3, 32)
    (z, none), _ = m.forward_frames(torch.from_numpy(rgb[0])[None].to(DEV), torch.from_numpy(ir[0])[None].to(DEV), 448, augment=True)
    want = ref.forward_u8(host_batch(rgb, ir, 448).to(DEV), augment=True)[0]
    assert none is None and z.shape == want.shape and torch.equal(z, want)


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
@pytest.mark.parametrize("rnd", [False, True], ids=["exact", "round"])
def test_scale_detections_equals_scale_coords(rnd, inplace):
    """Seeded boxes, some outside the image on every side, counts 0 / 1 / max_det, gains above and below one: rows < count equal
    scale_coords (+ .round()) on the CPU and the predn of match_predictions on the same rows; rows >= count are zero."""
    shapes, new, max_det = [(48, 60), (130, 70), (200, 9)], 64, 9
    counts = [0, 1, max_det]
    _, scale = ops.frame_geometry(shapes, new)
    assert scale[0, 0] > 1 and scale[1, 0] < 1
    g = np.random.default_rng(17)
    det = g.uniform(-25, 90, (3, max_det, 6)).astype(np.float32)
    det[:, 0, :4] = (-3.5, -7.25, 70.5, 80.0)                                 # outside on all four sides
    det[:, 1, :4] = (12.5, 10.0, 40.5, 30.25)
    det[:, :, 4] = g.uniform(0, 1, (3, max_det))
    det[:, :, 5] = g.integers(0, 3, (3, max_det))
    d = torch.from_numpy(det).to(DEV)
    c = torch.tensor(counts, dtype=torch.int32, device=DEV)
    s = torch.from_numpy(scale).to(DEV)
    predn = torch.zeros((3, max_det, 4), device=DEV)
    ops.match_predictions(d, c, torch.zeros((0, 5), device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV),
                          torch.tensor([0.5], device=DEV), scale=s, predn=predn)
    out = d.clone() if inplace else torch.full_like(d, 7.0)
    src = out if inplace else d
    ops.scale_detections(src, c, s, out=None if inplace else out, round=rnd)(ops.current_stream_ptr())
    torch.cuda.synchronize()
    out, predn = out.cpu(), predn.cpu()
    assert inplace or torch.equal(d.cpu(), torch.from_numpy(det))
    for b, n in enumerate(counts):
        want = torch.from_numpy(det[b, :n].copy())
        want[:, :4] = scale_coords((new, new), want[:, :4], shapes[b])
        assert torch.equal(predn[b, :n], want[:, :4])
        if rnd:
            want[:, :4] = want[:, :4].round()
        assert torch.equal(out[b, :n], want), b
        assert not out[b, n:].any(), b
        if n:
            assert want[0, 0] == 0 and want[0, 1] == 0 and want[0, 2] == shapes[b][1] and want[0, 3] == shapes[b][0]     # clipped on every side


@pytest.mark.parametrize("depth", [1, 2])
def test_pipeline_fed_with_pinned_native_frames(depth):
    """Five steps, other frames (and frame sizes) each, from pinned host memory: submit_frames returns what submit_u8 of the
    host-letterboxed batch followed by scale_coords on the host gives, for det[:count] and count, on every step — checked once step by
    step and once with all five steps enqueued without waiting."""
    m, ref = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16), build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    m.use_graph = ref.use_graph = True
    B, S = 2, 320
    pipe = DetectionPipeline(m, B, S, S, DEV, conf_thres=0.1, iou_thres=0.5, depth=depth, frames=(320, 320))
    base = DetectionPipeline(ref, B, S, S, DEV, conf_thres=0.1, iou_thres=0.5, depth=depth, u8=True)
    sizes = [[(240, 300), (256, 320)], [(256, 320), (256, 320)], [(320, 200), (100, 320)], [(240, 320), (240, 320)], [(200, 200), (317, 203)]]
    steps, want = [], []
    for k, shapes in enumerate(sizes):
        rgb, ir = frames_of(shapes, 3, 50 + k), frames_of(shapes, 3, 70 + k)
        if shapes[0] == shapes[1]:                                          # a uniform batch: one (B, H0, W0, 3) tensor per modality
            feed = (torch.from_numpy(np.stack(rgb)).pin_memory(), torch.from_numpy(np.stack(ir)).pin_memory())
        else:
            feed = ([torch.from_numpy(f).pin_memory() for f in rgb], [torch.from_numpy(f).pin_memory() for f in ir])
        steps.append(feed)
        det, count = (t[0] for t in base.submit_u8(host_batch(rgb, ir, S).pin_memory()))
        base.synchronize()
        det, count = det.cpu().clone(), count.cpu().clone()
        for b, n in enumerate(count.tolist()):
            det[b, :n, :4] = scale_coords((S, S), det[b, :n, :4], shapes[b])
        want.append((det, count))
    assert sum(int(c.sum()) for _, c in want) > 0

    def check(k, det, count):
        wd, wc = want[k]
        assert torch.equal(count.cpu(), wc), k
        for b, n in enumerate(wc.tolist()):
            assert torch.equal(det[b, :n].cpu(), wd[b, :n]), (k, b)
            assert not det[b, n:].cpu().any()
    for k, feed in enumerate(steps):                                        # step by step
        det, count = (t[0] for t in pipe.submit_frames(*feed))
        pipe.synchronize()
        check(k, det, count)
    outs = [tuple(t[0] for t in pipe.submit_frames(*feed)) for feed in steps]      # all in flight
    pipe.synchronize()
    for k in range(len(steps) - pipe.nplans, len(steps)):                   # the last `nplans` steps still own their output buffers
        check(k, *outs[k])
    with pytest.raises(ValueError, match="exceeds"):
        pipe.submit_frames(torch.zeros((B, 321, 320, 3), dtype=torch.uint8), torch.zeros((B, 321, 320, 3), dtype=torch.uint8))


def test_detect_twostream_device_letterbox_equals_the_default_path(tmp_path, capsys):
    """Three synthetic pairs through detect_twostream.py with and without --device-letterbox: the same label files, the same annotated
    images, the same printed summary (timings apart)."""
    sys.path.insert(0, REPO)
    import os
    import detect_twostream as dt
    from test_frontends import make_dataset
    rgb_dir, ir_dir = make_dataset(str(tmp_path), n=3, size=(120, 128), nc=3, seed=5)
    cfg_path = os.path.join(REPO, "models", "transformer", "yolov5s_Transfusion_FLIR.yaml")
    runs = {}
    for name, extra in (("host", []), ("device", ["--device-letterbox"])):
        opt = dt.parse_opt(["--cfg", cfg_path, "--source1", rgb_dir, "--source2", ir_dir, "--img-size", "320", "--conf-thres", "0.3",
                            "--save-txt", "--save-conf", "--project", str(tmp_path / "runs"), "--name", name] + extra)
        capsys.readouterr()
        out_dir = dt.detect(opt)
        printed = [re.sub(r"Done\. \(.*", "", ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("image ")]
        files = {str(p.relative_to(out_dir)): p.read_bytes() for p in sorted(out_dir.rglob("*")) if p.is_file()}
        runs[name] = (printed, files)
    assert len(runs["host"][0]) == 3 and runs["host"][0] == runs["device"][0]
    assert any(k.startswith("labels") for k in runs["host"][1]) and sum(k.endswith(".png") for k in runs["host"][1]) == 6
    assert runs["host"][1].keys() == runs["device"][1].keys()
    for k, v in runs["host"][1].items():
        assert v == runs["device"][1][k], k
