"""Native YUV 4:2:0 frames on the MI355X: icaf_letterbox_yuv_frames against letterbox(yuv420_to_bgr(...)) byte for byte on both of its paths,
its kind-0 rows against icaf_letterbox_frames on the same arena, the exact conversion lattice, and forward_frames / DetectionPipeline fed
with NV12 against the same calls fed with the host-converted frames.  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.pipeline import DetectionPipeline                       # noqa: E402
from icafusion_amd.utils import datasets as D                              # noqa: E402
from test_gpu_frames import DEV, DIRECT, GUARD, SHAPES, build, frames_of, host_batch, host_planes         # noqa: E402
from test_yuv_host import buffer_of, fill_arena, lattice, lattice_rgb, planes_of                          # noqa: E402

# the shapes of the BGR test plus a single pixel, a single chroma sample and an odd frame smaller than a vector; the squeezed frame last
YUV_SHAPES = SHAPES + [((1, 1), 64), ((2, 2), 64), ((3, 5), 64), DIRECT]
IDS = [f"{h}x{w}" for (h, w), _ in YUV_SHAPES]


def run_yuv_letterbox(mods, new, swap_rb=True, direct=False, matrix=0, pitch_extra=0, c_pitch_extra=0, sentinel=0x5C):
    """mods: per modality a list of B frames, each ("nv12" | "nv21" | "i420" | "yv12", (y, cb, cr)) or an interleaved (h0, w0, ch) array.
    The frames go into an arena pre-filled with `sentinel` (between planes and frames and behind every row whose pitch exceeds it), the
    destination is 0xAB inside guard bands.  Returns (the (B, 3 * len(mods), H, W) result, the table rows, the device arena) after
    checking that nothing around the output changed."""
    B = len(mods[0])
    H, W = (new, new) if isinstance(new, int) else new
    frames = [f for m in mods for f in m]
    shapes = [f[1][0].shape if isinstance(f, tuple) else f.shape[:2] for f in frames]
    geom1, _ = ops.frame_geometry(shapes[:B], new)
    assert shapes == shapes[:B] * len(mods)
    layouts = [f[0] if isinstance(f, tuple) else f.shape[2] for f in frames]
    pitches = [w + pitch_extra if isinstance(f, tuple) else w * f.shape[2] + pitch_extra for f, (_, w) in zip(frames, shapes)]
    c_pitches = [(w + 1) // 2 * ops.YUV_LAYOUTS[f[0]][0] + c_pitch_extra if isinstance(f, tuple) else None for f, (_, w) in zip(frames, shapes)]
    rows, end = ops.pack_yuv_frames(np.concatenate([geom1] * len(mods)), layouts, pitch=pitches, c_pitch=c_pitches, matrix=matrix)
    host = np.full((end + 64,), sentinel, np.uint8)
    for q, f in zip(rows, frames):
        if isinstance(f, tuple):
            fill_arena(host, q, *f[1])
        else:
            h0, w0, ch = f.shape
            o, p = int(q["g"]["offset"]), int(q["g"]["pitch"])
            host[o:o + h0 * p].reshape(h0, p)[:, :w0 * ch] = f.reshape(h0, w0 * ch)
    arena = torch.from_numpy(host).to(DEV)[:end]
    n = B * 3 * len(mods) * H * W
    whole = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    dst = whole[GUARD:GUARD + n].view(B, 3 * len(mods), H, W)
    launch = ops.letterbox_yuv_frames(arena, rows, ops.geom_tensor(rows, DEV), dst, swap_rb=swap_rb)
    with ops.letterbox_direct(direct):
        launch(ops.current_stream_ptr())
        torch.cuda.synchronize()
    assert bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + n:] == 0xAB).all()), "the kernel wrote outside its output"
    return dst.cpu().numpy(), rows, arena


def yuv_planes_on_host(planes, new, matrix):
    """(3, H, W): convert at native resolution, letterbox, BGR -> RGB planes."""
    return host_planes(D.yuv420_to_bgr(*planes, matrix), new, True)


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
@pytest.mark.parametrize("matrix", [0, 1, 2], ids=["bt601", "bt709", "full"])
@pytest.mark.parametrize("layout", ["nv12", "i420"])
@pytest.mark.parametrize("shape,new", YUV_SHAPES, ids=IDS)
def test_yuv_letterbox_kernel_equals_host(shape, new, layout, matrix, direct):
    """Modality 0 a YUV frame of the shape, modality 1 a grey kind-0 frame, one launch, default path and forced direct path: all six planes
    equal the host's.  Which branch the default path takes is the host's budget rule: only the squeezed frame goes direct."""
    planes, ir = planes_of(*shape, seed=11 + shape[0] + matrix), frames_of([shape], 1, 12 + shape[1])
    got, rows, _ = run_yuv_letterbox([[(layout, planes)], ir], new, direct=direct, matrix=matrix)
    assert np.array_equal(got[0, :3], yuv_planes_on_host(planes, new, matrix))
    assert np.array_equal(got[0, 3:], host_planes(ir[0], new, True))
    assert [ops.yuv_letterbox_staged(q) for q in rows] == [(shape, new) != DIRECT] * 2


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
def test_yuv_letterbox_mixed_batch_pitches_and_kind0_rows(direct):
    """Four frame sizes (one goes direct by default), luma pitch w0 + 7 and chroma pitch padded by 5, nv12 / nv21 / i420 / yv12 rows in
    modality 0 and interleaved BGR kind-0 rows in modality 1.  The BGR rows equal icaf_letterbox_frames run on the same arena with both
    values of swap_rb; a second run with another sentinel in every padding byte gives the same output."""
    shapes = [(48, 60), (130, 70), (37, 53), (300, 400)]
    layouts = ["nv12", "nv21", "i420", "yv12"]
    yuv = [(lay, planes_of(*s, seed=40 + i)) for i, (lay, s) in enumerate(zip(layouts, shapes))]
    bgr = frames_of(shapes, 3, 5)
    outs = {}
    for swap_rb in (True, False):
        for sentinel in (0x5C, 0xE3):
            got, rows, arena = run_yuv_letterbox([yuv, bgr], 64, swap_rb=swap_rb, direct=direct, matrix=1, pitch_extra=7, c_pitch_extra=5, sentinel=sentinel)
            outs[swap_rb, sentinel] = got
        assert np.array_equal(outs[swap_rb, 0x5C], outs[swap_rb, 0xE3])
        assert [ops.yuv_letterbox_staged(q) for q in rows] == [True, True, True, False] * 2
        assert [int(q["g"]["pitch"]) - int(q["g"]["w0"]) for q in rows[:4]] == [7] * 4 and not rows["kind"][4:].any()
        plain = rows["g"][4:].copy()                                      # the same arena through icaf_letterbox_frames: modality 1 alone
        ref = torch.full((4, 3, 64, 64), 0xAB, dtype=torch.uint8, device=DEV)
        with ops.letterbox_direct(direct):
            ops.letterbox_frames(arena, plain, ops.geom_tensor(plain, DEV), ref, swap_rb=swap_rb)(ops.current_stream_ptr())
            torch.cuda.synchronize()
        assert np.array_equal(got[:, 3:], ref.cpu().numpy())
        for b in range(4):
            assert np.array_equal(got[b, :3], yuv_planes_on_host(yuv[b][1], 64, 1)), (b, swap_rb)      # swap_rb is not read for YUV rows
            assert np.array_equal(got[b, 3:], host_planes(bgr[b], 64, swap_rb)), (b, swap_rb)


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
@pytest.mark.parametrize("matrix", [0, 1, 2], ids=["bt601", "bt709", "full"])
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_yuv_conversion_lattice_on_the_device(layout, matrix, direct):
    """The host lattice as a 22 x 112 frame letterboxed 1:1, so that the taps are the pixels: the planes are the rule's bytes in Python
    integers, both clips of every channel among them (tests/test_yuv_host.py asserts that they occur)."""
    got, rows, _ = run_yuv_letterbox([[(layout, lattice())]], (22, 112), direct=direct, matrix=matrix)
    g = rows[0]["g"]
    assert (int(g["nh"]), int(g["nw"]), int(g["top"]), int(g["left"]), float(g["sx"]), float(g["sy"])) == (22, 112, 0, 0, 1.0, 1.0)
    assert np.array_equal(got[0], lattice_rgb(matrix).transpose(2, 0, 1))


def nv12_of(planes):
    """(B, 3 * H0 // 2, W0) uint8: the decoder's NV12 buffers of B (y, cb, cr) frames of one even size."""
    return torch.from_numpy(np.stack([buffer_of(*p, "nv12").reshape(3 * p[0].shape[0] // 2, p[0].shape[1]) for p in planes]))


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "tta"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_forward_frames_with_formats_equals_forward_u8_of_the_host_conversion(dtype, augment):
    """yolov5n kaist, two pairs of 240 x 320 frames, the visible stream as NV12 (BT.709) and the thermal one as BGR: forward_frames(formats=
    ("nv12", None)) is forward_u8 of the host-converted, host-letterboxed batch bit for bit.  To 320 x 320; the augmented run to the model's
    smallest TTA size where that is larger (the plain size is below what forward(augment=True) accepts)."""
    m, ref = build("yolov5n_Transfusion_kaist.yaml", dtype), build("yolov5n_Transfusion_kaist.yaml", dtype)
    size = max(320, *m.tta_min_size()) if augment else 320
    planes = [planes_of(240, 320, seed=60 + i) for i in range(2)]
    ir = frames_of([(240, 320)] * 2, 3, 61)
    rgb = [D.yuv420_to_bgr(*p, 1) for p in planes]
    want = ref.forward_u8(host_batch(rgb, ir, size).to(DEV), augment=augment)
    feeds = [(nv12_of(planes).to(DEV), torch.from_numpy(np.stack(ir)).to(DEV)),                          # batch tensors
             ([t.to(DEV) for t in nv12_of(planes)], [torch.from_numpy(f).to(DEV) for f in ir])]         # lists of frames
    for a, b in feeds:
        got, info = m.forward_frames(a, b, size, augment=augment, formats=("nv12", None), yuv_matrix="bt709")
        if augment:
            assert got[1] is None and torch.equal(got[0], want[0])
        else:
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and all(torch.equal(x, y) for x, y in zip(got[2], want[2]))
        assert np.array_equal(info.scale.cpu().numpy(), ops.frame_geometry([(240, 320)] * 2, size)[1])
    if not augment:                                                        # both modalities YUV: the buffers state the frame size
        both, _ = m.forward_frames(nv12_of(planes).to(DEV), nv12_of(planes).to(DEV), size, formats=("nv12", "nv12"), yuv_matrix=1)
        assert torch.equal(both[0], ref.forward_u8(host_batch(rgb, rgb, size).to(DEV))[0])


@pytest.mark.parametrize("depth", [1, 2])
def test_pipeline_with_frame_formats_equals_the_pipeline_fed_with_converted_frames(depth):
    """Five steps of other frames and frame sizes from pinned host memory: det and count of a pipeline fed NV12 + BGR equal those of a second
    pipeline fed the host-converted BGR frames, step by step and with all steps in flight."""
    m, ref = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16), build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    m.use_graph = ref.use_graph = True
    B, S = 2, 320
    pipe = DetectionPipeline(m, B, S, S, DEV, conf_thres=0.1, iou_thres=0.5, depth=depth, frames=(320, 320), frame_formats=("nv12", None))
    base = DetectionPipeline(ref, B, S, S, DEV, conf_thres=0.1, iou_thres=0.5, depth=depth, frames=(320, 320))
    assert pipe.frames["cap"][0] * 2 == pipe.frames["cap"][1] == base.frames["cap"][0]                  # 1.5 bytes a pixel against 3
    sizes = [[(240, 300), (256, 320)], [(256, 320), (256, 320)], [(320, 200), (100, 320)], [(240, 320), (240, 320)], [(200, 200), (316, 202)]]
    steps, want = [], []
    for k, shapes in enumerate(sizes):
        planes, ir = [planes_of(*s, seed=50 + 2 * k + i) for i, s in enumerate(shapes)], frames_of(shapes, 3, 70 + k)
        if shapes[0] == shapes[1]:                                          # a uniform batch: one tensor per modality, one copy each
            feed = (nv12_of(planes).pin_memory(), torch.from_numpy(np.stack(ir)).pin_memory())
        else:
            feed = ([nv12_of([p])[0].pin_memory() for p in planes], [torch.from_numpy(f).pin_memory() for f in ir])
        steps.append(feed)
        rgb = [torch.from_numpy(D.yuv420_to_bgr(*p, 0)).pin_memory() for p in planes]
        det, count = (t[0] for t in base.submit_frames(rgb, [torch.from_numpy(f).pin_memory() for f in ir]))
        base.synchronize()
        want.append((det.cpu().clone(), count.cpu().clone()))
    assert sum(int(c.sum()) for _, c in want) > 0

    def check(k, det, count):
        assert torch.equal(count.cpu(), want[k][1]), k
        assert torch.equal(det.cpu(), want[k][0]), k
    for k, feed in enumerate(steps):                                        # step by step
        det, count = (t[0] for t in pipe.submit_frames(*feed))
        pipe.synchronize()
        check(k, det, count)
    outs = [tuple(t[0] for t in pipe.submit_frames(*feed)) for feed in steps]      # all in flight
    pipe.synchronize()
    for k in range(len(steps) - pipe.nplans, len(steps)):                   # the last `nplans` steps still own their output buffers
        check(k, *outs[k])
    with pytest.raises(ValueError, match="exceeds"):
        pipe.submit_frames(torch.zeros((B, 483, 320), dtype=torch.uint8), torch.zeros((B, 322, 320, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="3 \\* H0 // 2"):
        pipe.submit_frames(torch.zeros((B, 480, 320), dtype=torch.uint8), torch.zeros((B, 300, 320, 3), dtype=torch.uint8))
