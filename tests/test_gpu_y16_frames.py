"""16-bit thermal frames on the MI355X: icaf_y16_window against utils.datasets.agc_window, icaf_letterbox_y16_frames against
letterbox(agc_u16_to_u8(...)) byte for byte on both of its paths, its kind-0 rows against icaf_letterbox_frames on the same arena, and
forward_frames / DetectionPipeline fed with raw counts against the same calls fed with the host-mapped frames.  Every comparison is exact."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.pipeline import DetectionPipeline                       # noqa: E402
from icafusion_amd.utils import datasets as D                              # noqa: E402
from test_gpu_frames import DEV, DIRECT, GUARD, SHAPES, build, frames_of, host_batch, host_planes, run_letterbox      # noqa: E402
from test_y16_host import content, fill_y16, lattice_frame, overflow_frame                                             # noqa: E402

# the shapes of the BGR test plus a single pixel, an odd frame smaller than a vector, and the squeezed frame last
Y16_SHAPES = SHAPES + [((1, 1), 64), ((3, 5), 64), DIRECT]
IDS = [f"{h}x{w}" for (h, w), _ in Y16_SHAPES]
UNSET = -7                                                                  # what the window table holds before a launch


def run_y16(mods, new, swap_rb=True, direct=False, pad_px=0, sentinel=0x5C, clip=None, window=None, letterbox=True, launches=1):
    """mods: per modality a list of B frames, each a (h0, w0) uint16 array (a Y16 row) or an interleaved (h0, w0, ch) uint8 array (a
    kind-0 row); every pitch is padded by `pad_px` pixels.  The frames go into an arena pre-filled with `sentinel` (between frames and
    behind every row), the destination is 0xAB inside guard bands, the window table UNSET inside guard rows.  icaf_y16_window runs
    `launches` times, then icaf_letterbox_y16_frames.  Returns (the (B, 3 * len(mods), H, W) result or None, the (n, 2) windows, the table
    rows, the device arena) after checking that nothing around the outputs changed."""
    B = len(mods[0])
    H, W = (new, new) if isinstance(new, int) else new
    frames = [f for m in mods for f in m]
    shapes = [f.shape[:2] for f in frames]
    assert shapes == shapes[:B] * len(mods)
    geom1, _ = ops.frame_geometry(shapes[:B], new)
    layouts = ["y16" if f.dtype == np.uint16 else f.shape[2] for f in frames]
    pitches = [2 * (w + pad_px) if f.dtype == np.uint16 else (w + pad_px) * f.shape[2] for f, (_, w) in zip(frames, shapes)]
    rows, end = ops.pack_y16_frames(np.concatenate([geom1] * len(mods)), layouts, pitch=pitches, clip=clip, window=window)
    host = np.full((end + 64,), sentinel, np.uint8)
    for q, f in zip(rows, frames):
        if f.dtype == np.uint16:
            fill_y16(host, q, f)
        else:
            h0, w0, ch = f.shape
            o, p = int(q["g"]["offset"]), int(q["g"]["pitch"])
            host[o:o + h0 * p].reshape(h0, p)[:, :w0 * ch] = f.reshape(h0, w0 * ch)
    arena = torch.from_numpy(host).to(DEV)[:end]
    n, nrow = B * 3 * len(mods) * H * W, len(rows)
    whole = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    dst = whole[GUARD:GUARD + n].view(B, 3 * len(mods), H, W)
    wwhole = torch.full((nrow + 16, 2), UNSET, dtype=torch.int32, device=DEV)
    wtab = wwhole[8:8 + nrow]
    tab = ops.geom_tensor(rows, DEV)
    select = ops.y16_window(arena, rows, tab, wtab, B, H, W)
    tables = []
    for _ in range(launches):
        select(ops.current_stream_ptr())
        torch.cuda.synchronize()
        tables.append(wtab.cpu().numpy().copy())
    assert all(np.array_equal(t, tables[0]) for t in tables), "two launches of icaf_y16_window gave different tables"
    if letterbox:
        launch = ops.letterbox_y16_frames(arena, rows, tab, wtab, dst, swap_rb=swap_rb)
        with ops.letterbox_direct(direct):
            launch(ops.current_stream_ptr())
            torch.cuda.synchronize()
        assert bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + n:] == 0xAB).all()), "the kernel wrote outside its output"
    assert bool((wwhole[:8] == UNSET).all()) and bool((wwhole[8 + nrow:] == UNSET).all()), "icaf_y16_window wrote outside its table"
    assert (tables[0][rows["kind"] == 0] == UNSET).all(), "a kind-0 row's window entry was written"
    return (dst.cpu().numpy() if letterbox else None), tables[0], rows, arena


def mapped(frame, window):
    """(h0, w0, 1) uint8: the host-mapped thermal frame, as host_planes takes a grey frame."""
    return D.agc_u16_to_u8(frame, *window)[:, :, None]


# ---- the window ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,new", Y16_SHAPES, ids=IDS)
def test_window_kernel_equals_agc_window(shape, new):
    """Random, flat, narrow, two-valued and full-range content of the shape in one batch, pitches padded by 3 pixels, default clip and the
    two extremes: the device table equals agc_window row by row; a second launch gives the same table."""
    frames = [content(kind, *shape, seed=7 + i) for i, kind in enumerate(("random", "flat", "narrow", "two", "ends"))]
    for clip in ((100, 100), (0, 0), (4999, 4999), (250, 3)):
        _, win, _, _ = run_y16([frames], new, pad_px=3, clip=clip, letterbox=False, launches=2)
        assert win.tolist() == [list(D.agc_window(f, clip)) for f in frames], clip


@pytest.mark.parametrize("clip", [(100, 100), (100, 0), (0, 100), (0, 0), (4999, 4999)], ids=lambda c: f"{c[0]}-{c[1]}")
def test_window_kernel_on_the_rank_lattice(clip):
    """The four 100 x 100 lattice frames (exactly clip pixels at the end code, and one more): both strict inequalities, on the device."""
    frames = [lattice_frame(side, exact) for side in ("lo", "hi") for exact in (True, False)]
    _, win, _, _ = run_y16([frames], 64, clip=clip, letterbox=False, launches=2)
    assert win.tolist() == [list(D.agc_window(f, clip)) for f in frames]
    if clip[0] == 100:
        assert win[0, 0] == 650 and win[1, 0] == 500
    if clip[1] == 100:
        assert win[2, 1] == 59000 and win[3, 1] == 60000


def test_window_kernel_64_bit_products_and_byte_order():
    """The one large frame of this file: 512 x 640 with 220,000 pixels at its lowest code, where a signed 32-bit 10000 * C is negative (the
    overflow cannot occur below 214,749 pixels).  Beside it, a frame of 0x0102 against one of 0x0201."""
    f = overflow_frame()
    _, win, _, _ = run_y16([[f]], 64, letterbox=False, launches=2)
    assert win.tolist() == [list(D.agc_window(f))] and win[0, 0] == 1000
    a, b = np.full((5, 9), 0x0102, np.uint16), np.full((5, 9), 0x0201, np.uint16)
    _, win, _, _ = run_y16([[a, b]], 64, letterbox=False)
    assert win.tolist() == [[0x0102, 0x0102], [0x0201, 0x0201]]


def test_window_kernel_mode_0_rows_copy_their_pair():
    frames = [content("random", 37, 53, seed=i) for i in range(4)]
    given = [None, (0, 65535), (1234, 1234), None]
    _, win, rows, _ = run_y16([frames], 64, window=given, letterbox=False, launches=2)
    assert rows["mode"].tolist() == [1, 0, 0, 1]
    assert win.tolist() == [list(D.agc_window(f) if w is None else w) for f, w in zip(frames, given)]


# ---- the letterbox ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
@pytest.mark.parametrize("shape,new", Y16_SHAPES, ids=IDS)
def test_y16_letterbox_kernel_equals_host(shape, new, direct):
    """Modality 0 a kind-0 BGR frame, modality 1 a Y16 frame of the shape, one launch, default path and forced direct path: all six planes
    equal the host's.  Which branch the default path takes is the host's budget rule: only the squeezed frame goes direct."""
    bgr = frames_of([shape], 3, 12 + shape[1])
    raw = content("narrow" if shape[0] % 2 else "random", *shape, seed=11 + shape[0])
    got, win, rows, _ = run_y16([bgr, [raw]], new, direct=direct)
    window = D.agc_window(raw)
    assert win[1].tolist() == list(window)
    assert np.array_equal(got[0, :3], host_planes(bgr[0], new, True))
    assert np.array_equal(got[0, 3:], host_planes(mapped(raw, window), new, True))
    assert [ops.y16_letterbox_staged(q) for q in rows] == [(shape, new) != DIRECT] * 2


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
def test_y16_letterbox_mixed_batch_pitches_and_kind0_rows(direct):
    """Four frame sizes (one goes direct by default), every pitch padded by 7 pixels (an odd number), BGR kind-0 rows in modality 0 and
    Y16 rows in modality 1, two of them with a given window.  The BGR rows equal icaf_letterbox_frames run on the same arena with both
    values of swap_rb; a second run with another sentinel in every padding byte gives the same output and the same windows: padding
    reaches neither the histogram nor a tap."""
    shapes = [(48, 60), (130, 70), (37, 53), (300, 400)]
    bgr = frames_of(shapes, 3, 5)
    raw = [content(kind, *s, seed=40 + i) for i, (kind, s) in enumerate(zip(("narrow", "random", "ends", "narrow"), shapes))]
    given = [None] * 4 + [None, (20000, 40000), None, (30100, 30100)]
    windows = [D.agc_window(f) if w is None else w for f, w in zip(raw, given[4:])]
    for swap_rb in (True, False):
        outs = {}
        for sentinel in (0x5C, 0xE3):
            outs[sentinel] = run_y16([bgr, raw], 64, swap_rb=swap_rb, direct=direct, pad_px=7, sentinel=sentinel, window=given)
        got, win, rows, arena = outs[0x5C]
        assert np.array_equal(got, outs[0xE3][0]) and np.array_equal(win, outs[0xE3][1])
        assert win[4:].tolist() == [list(w) for w in windows]
        assert [ops.y16_letterbox_staged(q) for q in rows] == [True, True, True, False] * 2
        assert [int(q["g"]["pitch"]) - 2 * int(q["g"]["w0"]) for q in rows[4:]] == [14] * 4 and not rows["kind"][:4].any()
        plain = rows["g"][:4].copy()                                      # the same arena through icaf_letterbox_frames: modality 0 alone
        ref = torch.full((4, 3, 64, 64), 0xAB, dtype=torch.uint8, device=DEV)
        with ops.letterbox_direct(direct):
            ops.letterbox_frames(arena, plain, ops.geom_tensor(plain, DEV), ref, swap_rb=swap_rb)(ops.current_stream_ptr())
            torch.cuda.synchronize()
        assert np.array_equal(got[:, :3], ref.cpu().numpy())
        for b in range(4):
            assert np.array_equal(got[b, :3], host_planes(bgr[b], 64, swap_rb)), (b, swap_rb)
            assert np.array_equal(got[b, 3:], host_planes(mapped(raw[b], windows[b]), 64, True)), (b, swap_rb)      # swap_rb is not read for Y16 rows


@pytest.mark.parametrize("direct", [False, True], ids=["default", "direct"])
def test_the_257_frame_equals_the_plain_grey_letterbox(direct):
    """A uint8 frame f presented as 257 * f under the window (0, 65535), and as f << 8 under (0, 65280), maps back to f: the planes are
    icaf_letterbox_frames' planes of the grey frame, on the device and on the host."""
    shapes = [(48, 60), (130, 70), (37, 53), (300, 400)]
    grey = frames_of(shapes, 1, 9)
    want, _ = run_letterbox([grey], 64, True, direct)
    for scale, window in ((lambda f: f.astype(np.uint16) * 257, (0, 65535)), (lambda f: f.astype(np.uint16) << 8, (0, 65280))):
        got, win, _, _ = run_y16([[scale(f[:, :, 0]) for f in grey]], 64, direct=direct, window=window)
        assert win.tolist() == [list(window)] * 4
        assert np.array_equal(got, want)
    for b in range(4):
        assert np.array_equal(want[b], host_planes(grey[b], 64, True))


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def u16_tensor(frames):
    """(B, H0, W0) int16: the same bits as the uint16 counts, a dtype every torch release moves and views."""
    return torch.from_numpy(np.stack(frames).view(np.int16))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_forward_frames_with_y16_equals_forward_u8_of_the_host_mapping(dtype):
    """yolov5n kaist, two pairs of 240 x 320 frames, the visible stream BGR and the thermal one raw counts: forward_frames(formats=(None,
    "y16")) is forward_u8 of the host-mapped, host-letterboxed batch bit for bit, in percentile mode, in window mode (one window, one per
    frame) and for ragged lists; FrameGeometry.window holds the windows used."""
    m, ref = build("yolov5n_Transfusion_kaist.yaml", dtype), build("yolov5n_Transfusion_kaist.yaml", dtype)
    size, shapes = 320, [(240, 320)] * 2
    rgb = frames_of(shapes, 3, 61)
    raw = [content("narrow", 240, 320, seed=3), content("random", 240, 320, seed=4)]

    def same(got, want):
        return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and all(torch.equal(x, y) for x, y in zip(got[2], want[2]))
    vis = torch.from_numpy(np.stack(rgb)).to(DEV)
    cases = [({}, [D.agc_window(f) for f in raw]),
             ({"agc_clip": (250, 3)}, [D.agc_window(f, (250, 3)) for f in raw]),
             ({"agc_window": (20000, 40000)}, [(20000, 40000)] * 2),
             ({"agc_window": np.array([[29000, 31000], [0, 65535]])}, [(29000, 31000), (0, 65535)])]
    for kw, windows in cases:
        want = ref.forward_u8(host_batch(rgb, [mapped(f, w) for f, w in zip(raw, windows)], size).to(DEV))
        feeds = [(vis, u16_tensor(raw).to(DEV)),                                                              # 16-bit batch tensor
                 (vis, u16_tensor(raw).view(torch.uint8).to(DEV)),                                            # its bytes, (B, H0, 2 * W0)
                 ([torch.from_numpy(f).to(DEV) for f in rgb], [t.to(DEV) for t in u16_tensor(raw)])]          # lists of frames
        for a, b in feeds:
            got, info = m.forward_frames(a, b, size, formats=(None, "y16"), **kw)
            assert same(got, want), kw
            assert info.window[0] is None and info.window[1].dtype == torch.int32 and info.window[1].is_cuda
            assert info.window[1].cpu().tolist() == [list(w) for w in windows], kw
            assert np.array_equal(info.scale.cpu().numpy(), ops.frame_geometry(shapes, size)[1])
    # both modalities thermal, ragged sizes
    sizes = [(200, 300), (256, 320)]
    a, b = [content("random", *s, seed=20 + i) for i, s in enumerate(sizes)], [content("narrow", *s, seed=30 + i) for i, s in enumerate(sizes)]
    got, info = m.forward_frames([t.to(DEV) for t in map(torch.from_numpy, (f.view(np.int16) for f in a))],
                                 [t.to(DEV) for t in map(torch.from_numpy, (f.view(np.int16) for f in b))], size, formats=("y16", "y16"))
    want = ref.forward_u8(host_batch([mapped(f, D.agc_window(f)) for f in a], [mapped(f, D.agc_window(f)) for f in b], size).to(DEV))
    assert same(got, want)
    assert [w.cpu().tolist() for w in info.window] == [[list(D.agc_window(f)) for f in a], [list(D.agc_window(f)) for f in b]]


def test_y16_refuses_val_size_and_align():
    m = build("yolov5n_Transfusion_kaist.yaml", torch.bfloat16)
    vis, raw = torch.zeros((1, 48, 64, 3), dtype=torch.uint8, device=DEV), torch.zeros((1, 48, 64), dtype=torch.int16, device=DEV)
    with pytest.raises(ValueError, match="'y16'.*val_size"):
        m.forward_frames(vis, raw, 64, formats=(None, "y16"), val_size=64)
    with pytest.raises(ValueError, match="align=.*'y16'"):
        m.forward_frames(vis, raw, 64, formats=(None, "y16"), align=(None, "stretch"))
    with pytest.raises(ValueError, match="basis points"):
        m.forward_frames(vis, raw, 64, formats=(None, "y16"), agc_clip=(5000, 0))
    with pytest.raises(ValueError, match="0 <= lo <= hi <= 65535"):
        m.forward_frames(vis, raw, 64, formats=(None, "y16"), agc_window=(9, 8))
    with pytest.raises(ValueError, match="same size"):
        m.forward_frames(vis, raw[:, :, :60], 64, formats=(None, "y16"))
    with pytest.raises(ValueError, match="frame_align.*'y16'"):
        DetectionPipeline(m, 1, 64, 64, DEV, frames=(64, 64), frame_formats=(None, "y16"), frame_align=(None, True), align_frames=(64, 64))
    with pytest.raises(ValueError, match="'y16'.*YUV"):
        DetectionPipeline(m, 1, 64, 64, DEV, frames=(64, 64), frame_formats=("nv12", "y16"))


@pytest.mark.parametrize("depth", [1, 2])
def test_pipeline_with_y16_equals_the_pipeline_fed_with_mapped_frames(depth):
    """Five steps of other frames and frame sizes from pinned host memory, the last with a window given: det and count of a pipeline fed
    BGR + raw counts equal those of a second pipeline fed the host-mapped grey frames, step by step and with all steps in flight."""
    m, ref = build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16), build("yolov5s_Transfusion_kaist.yaml", torch.bfloat16)
    m.use_graph = ref.use_graph = True
    B, S = 2, 320
    pipe = DetectionPipeline(m, B, S, S, DEV, conf_thres=0.1, iou_thres=0.5, depth=depth, frames=(320, 320), frame_formats=(None, "y16"), agc_clip=(200, 50))
    base = DetectionPipeline(ref, B, S, S, DEV, conf_thres=0.1, iou_thres=0.5, depth=depth, frames=(320, 320), frame_channels=(3, 1))
    assert pipe.frames["cap"][0] == base.frames["cap"][0] and pipe.frames["cap"][1] == 2 * base.frames["cap"][1]      # 2 bytes a pixel against 1
    sizes = [[(240, 300), (256, 320)], [(256, 320), (256, 320)], [(320, 200), (100, 320)], [(240, 320), (240, 320)], [(200, 200), (317, 203)]]
    steps, want, used = [], [], []
    for k, shapes in enumerate(sizes):
        rgb = frames_of(shapes, 3, 50 + k)
        raw = [content("narrow" if (k + i) % 2 else "random", *s, seed=70 + 2 * k + i) for i, s in enumerate(shapes)]
        given = (29900, 30200) if k == 4 else None
        windows = [given or D.agc_window(f, (200, 50)) for f in raw]
        if shapes[0] == shapes[1]:                                          # a uniform batch: one tensor per modality, one copy each
            feed = (torch.from_numpy(np.stack(rgb)).pin_memory(), u16_tensor(raw).pin_memory())
        else:
            feed = ([torch.from_numpy(f).pin_memory() for f in rgb], [torch.from_numpy(f.view(np.int16)).pin_memory() for f in raw])
        steps.append((feed, given))
        used.append(windows)
        grey = [torch.from_numpy(mapped(f, w)).pin_memory() for f, w in zip(raw, windows)]
        det, count = (t[0] for t in base.submit_frames([torch.from_numpy(f).pin_memory() for f in rgb], grey))
        base.synchronize()
        want.append((det.cpu().clone(), count.cpu().clone()))
    assert sum(int(c.sum()) for _, c in want) > 0

    def check(k, det, count):
        assert torch.equal(count.cpu(), want[k][1]), k
        assert torch.equal(det.cpu(), want[k][0]), k
    for k, (feed, given) in enumerate(steps):                               # step by step
        pi = pipe.n % pipe.nplans
        det, count = (t[0] for t in pipe.submit_frames(*feed, agc_window=given))
        pipe.synchronize()
        check(k, det, count)
        assert pipe.frames["window"][pi][B:].cpu().tolist() == [list(w) for w in used[k]], k
    outs = [tuple(t[0] for t in pipe.submit_frames(*feed, agc_window=given)) for feed, given in steps]      # all in flight
    pipe.synchronize()
    for k in range(len(steps) - pipe.nplans, len(steps)):                   # the last `nplans` steps still own their output buffers
        check(k, *outs[k])
    with pytest.raises(ValueError, match="exceeds"):
        pipe.submit_frames(torch.zeros((B, 321, 320, 3), dtype=torch.uint8), torch.zeros((B, 321, 320), dtype=torch.int16))
    with pytest.raises(ValueError, match="agc_window"):
        base.submit_frames(torch.zeros((B, 320, 320, 3), dtype=torch.uint8), torch.zeros((B, 320, 320, 1), dtype=torch.uint8), agc_window=(0, 1))
