"""Validation from native frames on the MI355X: icaf_resize_frames against resize_area_scalar + padding byte for byte (staged and direct
path), a batch that mixes area, bilinear and copied frames in one launch against icaf_letterbox_frames, forward_frames(val_size=...)
against forward_u8 of the batch composed on the host, and test(device_letterbox=True) against test().  Every comparison is exact."""
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import REPO, load_cfg, val_module                             # noqa: E402
from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.models.yolo import Model                                # noqa: E402
from icafusion_amd.synth import synth_state_dict                           # noqa: E402
from icafusion_amd.utils import datasets as D                              # noqa: E402

DEV = "cuda:0"
GUARD = 4096


def rect_shape(h0, w0, img_size, stride=32, pad=0.5):
    """The rectangular batch shape the loader gives a batch of such frames (PairedValSet, utils/datasets.py:826-849)."""
    ar = h0 / w0
    s = [ar, 1.0] if ar < 1 else [1.0, 1.0 / ar] if ar > 1 else [1.0, 1.0]
    return tuple(int(v) for v in np.ceil(np.array(s) * img_size / stride + pad).astype(np.int64) * stride)


# (native (h0, w0), img_size): s = 2 with exact weights; three taps and another s per axis; a 2-pixel-wide block with 5 taps; s barely above
# 1; odd sizes; s = 6.25 with 8 taps; several tiles in both directions
CASES = [((96, 128), 64), ((130, 70), 64), ((200, 9), 64), ((65, 64), 64), ((37, 53), 32), ((300, 400), 64), ((240, 300), 160)]
IDS = [f"{h}x{w}@{s}" for (h, w), s in CASES]


def frames_of(shapes, ch, seed):
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, (h, w, ch), dtype=np.uint8) for h, w in shapes]


def host_planes(frame, img_size, shape, swap_rb):
    """(3, H, W) uint8: the loader's two steps on the host with the fixed-order area statement (a grey frame replicated first)."""
    img = frame if frame.shape[2] == 3 else np.repeat(frame, 3, axis=2)
    h0, w0 = img.shape[:2]
    r = img_size / max(h0, w0)
    if r != 1:
        img = (D.resize_area_scalar if r < 1 else D.resize_bilinear)(img, (int(w0 * r), int(h0 * r)))
    lb = D.letterbox(img, shape, auto=False, scaleup=False)[0]
    assert lb.shape[:2] == tuple(shape)
    return np.ascontiguousarray((lb[:, :, ::-1] if swap_rb else lb).transpose(2, 0, 1))


def host_batch(rgb, ir, img_size, shape):
    return torch.from_numpy(np.stack([np.concatenate((host_planes(a, img_size, shape, True), host_planes(b, img_size, shape, True)), 0)
                                      for a, b in zip(rgb, ir)]))


def run(mods, geom1, mode1, shape, swap_rb, direct=False, pitch_extra=0, entry="resize"):
    """mods: per modality a list of B frames (h0, w0, ch).  The arena is pre-filled with a sentinel (between frames and behind every row
    when pitch > w0 * ch), the destination with 0xAB inside poisoned surroundings.  entry: "resize" (mode table), "resize-null" (mode
    NULL) or "letterbox" (icaf_letterbox_frames on the same descriptors).  Returns the (B, 3 * len(mods), H, W) result after checking
    that nothing around it changed."""
    B = len(mods[0])
    H, W = shape
    frames = [f for m in mods for f in m]
    geom = np.concatenate([geom1] * len(mods))
    mode = np.concatenate([mode1] * len(mods)).astype(np.int32)
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
    tab = ops.geom_tensor(geom, DEV)
    if entry == "letterbox":
        launch = ops.letterbox_frames(arena, geom, tab, dst, swap_rb=swap_rb)
    elif entry == "resize-null":
        launch = ops.resize_frames(arena, geom, None, tab, dst, swap_rb=swap_rb)
    else:
        launch = ops.resize_frames(arena, geom, torch.from_numpy(mode).to(DEV), tab, dst, swap_rb=swap_rb, mode=mode)
    with ops.area_direct(direct):
        launch(ops.current_stream_ptr())
        torch.cuda.synchronize()
    assert bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + n:] == 0xAB).all()), "the kernel wrote outside its output"
    return dst.cpu().numpy(), geom


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
@pytest.mark.parametrize("swap_rb", [True, False], ids=["bgr", "rgb"])
@pytest.mark.parametrize("shape,img_size", CASES, ids=IDS)
def test_area_kernel_equals_the_scalar_statement(shape, img_size, swap_rb, direct):
    """One 3-channel and one grey frame of the shape (two modalities, one launch) into the loader's rectangular batch shape: every byte
    of the six planes equals resize_area_scalar + letterbox's padding, on the default path and on the forced direct path."""
    out_shape = rect_shape(*shape, img_size)
    rgb, ir = frames_of([shape], 3, 11 + shape[0]), frames_of([shape], 1, 12 + shape[1])
    geom1, mode1, _ = ops.val_geometry([shape], img_size, out_shape)
    assert mode1.tolist() == [1]
    got, geom = run([rgb, ir], geom1, mode1, out_shape, swap_rb, direct)
    assert np.array_equal(got[0, :3], host_planes(rgb[0], img_size, out_shape, swap_rb))
    assert np.array_equal(got[0, 3:], host_planes(ir[0], img_size, out_shape, swap_rb))
    # the default path of every case keeps its vertical sums in LDS — 300 x 400 with 4 rows of 400 pixels at a time (its 3-channel rows
    # are the widest the list has), which is the budget rule's statement on the host
    assert all(ops.area_staged(g) for g in geom)
    if shape == (300, 400):
        assert (int(geom[0]["nh"]), int(geom[0]["nw"])) == (48, 64)


@pytest.mark.parametrize("swap_rb", [True, False], ids=["bgr", "rgb"])
def test_area_kernel_beyond_the_weight_tables(swap_rb):
    """288 x 40 at 32: s = 9 down and 10 across, 11 and 12 taps — more than the LDS tables hold, so the weights are computed on the spot
    and the tiles go direct by default (the path of a 4K frame validated at 320)."""
    shape, img_size = (288, 40), 32
    out_shape = rect_shape(*shape, img_size)
    rgb, ir = frames_of([shape], 3, 41), frames_of([shape], 1, 42)
    geom1, mode1, _ = ops.val_geometry([shape], img_size, out_shape)
    assert out_shape == (64, 32) and (int(geom1[0]["nh"]), int(geom1[0]["nw"])) == (32, 4) and mode1.tolist() == [1]
    got, geom = run([rgb, ir], geom1, mode1, out_shape, swap_rb)
    assert not any(ops.area_staged(g) for g in geom)
    assert np.array_equal(got[0, :3], host_planes(rgb[0], img_size, out_shape, swap_rb))
    assert np.array_equal(got[0, 3:], host_planes(ir[0], img_size, out_shape, swap_rb))


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
def test_mixed_batch_in_one_launch(direct):
    """Four frames of one batch — area, up-scaled, copied, area — with pitch > w0 * ch (no row phase is a multiple of 4), the second modality
    grey.  Every frame equals the host; mode-0 rows equal icaf_letterbox_frames of the same descriptors; a NULL mode table is
    icaf_letterbox_frames on the whole batch."""
    shapes, img_size, out_shape = [(130, 70), (48, 60), (64, 50), (100, 120)], 64, (96, 96)
    rgb, ir = frames_of(shapes, 3, 3), frames_of(shapes, 1, 4)
    geom1, mode1, _ = ops.val_geometry(shapes, img_size, out_shape)
    assert mode1.tolist() == [1, 0, 0, 1] and (int(geom1[2]["nh"]), int(geom1[2]["nw"])) == (64, 50) and int(geom1[1]["nw"]) == 64
    got, _ = run([rgb, ir], geom1, mode1, out_shape, True, direct, pitch_extra=7)
    for b in range(4):
        assert np.array_equal(got[b, :3], host_planes(rgb[b], img_size, out_shape, True)), b
        assert np.array_equal(got[b, 3:], host_planes(ir[b], img_size, out_shape, True)), b
    lb, _ = run([rgb, ir], geom1, mode1, out_shape, True, direct, pitch_extra=7, entry="letterbox")
    assert np.array_equal(got[1:3], lb[1:3])
    assert not np.array_equal(got[0], lb[0])                               # the bilinear shrink of frame 0 is another picture
    null, _ = run([rgb, ir], geom1, mode1, out_shape, True, direct, pitch_extra=7, entry="resize-null")
    assert np.array_equal(null, lb)


def build(yaml_name, dtype, seed=0):
    m = Model(load_cfg(yaml_name)).eval()
    m.load_state_dict(synth_state_dict(m, seed))
    m = m.to(DEV)
    m.compute_dtype = None if dtype == torch.float32 else dtype
    m.autotune = False
    return m


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_forward_with_val_size_equals_forward_from_the_host_batch(dtype):
    """yolov5s Add, validation size 128: pairs of other native sizes per call (shrinking, growing and copied frames in one batch);
    forward_frames(val_size=...) is forward_u8 of the batch composed on the host bit for bit, the scale rows are test.py's, and a
    repeated first call shows no stale arena, descriptor or mode table."""
    m, ref = build("yolov5s_Add_kaist.yaml", dtype), build("yolov5s_Add_kaist.yaml", dtype)
    for seed, shapes, out_shape in ((21, [(240, 300), (256, 320)], (128, 160)), (22, [(100, 120), (128, 90), (300, 200)], (160, 160)),
                                    (23, [(240, 300), (256, 320)], (128, 160))):
        rgb, ir = frames_of(shapes, 3, seed), frames_of(shapes, 3, seed + 100)
        (z, logits, raws), info = m.forward_frames([torch.from_numpy(f).to(DEV) for f in rgb], [torch.from_numpy(f).to(DEV) for f in ir],
                                                   out_shape, val_size=128)
        wz, wlogits, wraws = ref.forward_u8(host_batch(rgb, ir, 128, out_shape).to(DEV))
        assert torch.equal(z, wz) and torch.equal(logits, wlogits) and all(torch.equal(a, b) for a, b in zip(raws, wraws)), shapes
        assert np.array_equal(info.scale.cpu().numpy(), ops.val_geometry(shapes, 128, out_shape)[2])
    # the same frames without val_size are letterboxed as before: another geometry, another cached state
    (z2, _, _), info2 = m.forward_frames([torch.from_numpy(f).to(DEV) for f in rgb], [torch.from_numpy(f).to(DEV) for f in ir], out_shape)
    assert np.array_equal(info2.scale.cpu().numpy(), ops.frame_geometry(shapes, out_shape)[1]) and not torch.equal(z2, z)


def test_validation_loop_from_native_frames_equals_the_host_loop(tmp_path, capsys):
    """test(device_letterbox=True) against test() on five 96 x 128 / 128 x 96 pairs at img-size 64 (r = 0.5; rectangular batches of 64 x 96
    and 96 x 64, a ragged last batch; tests/test_val_frames_host.py shows this set's bytes equal between the two area statements): the
    same return tuple, the same maps, the same --save-txt / --save-json files."""
    sys.path.insert(0, REPO)
    from test_frontends import make_dataset
    val = val_module()
    rgb_dir, ir_dir = make_dataset(str(tmp_path / "set"), n=5, size=(96, 128), nc=2, seed=3)
    data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 2, "names": ["person", "car"]}
    model = build("yolov5s_Add_kaist.yaml", torch.bfloat16)
    model.use_graph = True
    runs = {}
    for name, flag in (("host", False), ("device", True)):
        out_dir = tmp_path / name
        res, maps, _ = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, save_txt=True, save_json=True, save_dir=out_dir,
                                device_letterbox=flag)
        files = {str(p.relative_to(out_dir)): p.read_bytes() for p in sorted(out_dir.rglob("*")) if p.is_file()}
        runs[name] = (res, maps.tolist(), files)
    assert runs["host"][0] == runs["device"][0] and runs["host"][1] == runs["device"][1]
    assert runs["host"][2].keys() == runs["device"][2].keys() and len(runs["host"][2]) >= 2
    for k, v in runs["host"][2].items():
        assert v == runs["device"][2][k], k
