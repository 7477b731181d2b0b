"""Host side of the native-frame path (no GPU): the letterbox geometry against utils.datasets.letterbox, the scale_coords rows against
utils.general.scale_coords, the validation in front of the launches, and the kernel's arithmetic restated in scalar fp32."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import REPO, load_cfg
from icafusion_amd import ops
from icafusion_amd.models.yolo import Model
from icafusion_amd.utils import datasets as D
from icafusion_amd.utils.general import scale_coords

# (native (h0, w0), network size): pad 6.5 split 6 / 7; portrait; rectangular output; identity; a 3-pixel-wide resized block; down-scale;
# one side already at size
SHAPES = [((48, 60), 64), ((60, 48), 64), ((37, 53), (64, 96)), ((64, 64), 64), ((200, 9), 64), ((130, 70), 64), ((33, 64), 64)]
IDS = [f"{h}x{w}" for (h, w), _ in SHAPES]


@pytest.mark.parametrize("shape,new", SHAPES, ids=IDS)
def test_frame_geometry_agrees_with_letterbox(shape, new):
    """Output shape, placement of the resized block and the pads of letterbox() are what frame_geometry says."""
    g = np.random.default_rng(sum(shape))
    img = g.integers(0, 256, (*shape, 3), dtype=np.uint8)
    out, ratio, pad = D.letterbox(img, new)
    H, W = (new, new) if isinstance(new, int) else new
    geom, scale = ops.frame_geometry([shape], new)
    r = geom[0]
    top, left, nh, nw = int(r["top"]), int(r["left"]), int(r["nh"]), int(r["nw"])
    assert out.shape == (H, W, 3) and (int(r["h0"]), int(r["w0"])) == shape
    assert np.array_equal(out[top:top + nh, left:left + nw], D.resize_bilinear(img, (nw, nh)))
    mask = np.ones((H, W), bool)
    mask[top:top + nh, left:left + nw] = False
    assert (out[mask] == 114).all()
    assert (H - nh - top, W - nw - left) == (int(round(pad[1] + 0.1)), int(round(pad[0] + 0.1)))       # bottom, right
    assert r["sx"] == np.float32(shape[1] / nw) and r["sy"] == np.float32(shape[0] / nh)
    if shape == (48, 60):
        assert (top, H - nh - top) == (6, 7)
    if shape == (200, 9):
        assert nw == 3


@pytest.mark.parametrize("shape,new", SHAPES, ids=IDS)
def test_scale_rows_agree_with_scale_coords(shape, new):
    """(x - pad) / gain clipped, evaluated in fp32 from the rows, is scale_coords(new, boxes, shape) of the torch CPU path bit for bit."""
    H, W = (new, new) if isinstance(new, int) else new
    _, scale = ops.frame_geometry([shape], new)
    gain, px, py, w0, h0 = scale[0]
    assert (w0, h0) == (shape[1], shape[0]) and scale.dtype == np.float32
    g = np.random.default_rng(7)
    boxes = g.uniform(-30, max(H, W) + 30, (64, 4)).astype(np.float32)
    want = scale_coords((H, W), torch.from_numpy(boxes.copy()), shape).numpy()
    got = boxes.copy()
    got[:, [0, 2]] = np.clip((got[:, [0, 2]] - px) / gain, np.float32(0), w0)
    got[:, [1, 3]] = np.clip((got[:, [1, 3]] - py) / gain, np.float32(0), h0)
    assert got.dtype == np.float32 and np.array_equal(got, want)


def _rows(shapes, new, ch=3):
    geom, _ = ops.frame_geometry(shapes, new)
    end = ops.pack_frames(geom, ch)
    return geom, end


def test_validation_fires_before_any_device_call(monkeypatch):
    """Every reason validate_frames knows, and the launch wrappers raising ValueError with nothing sent to the library."""
    def no_device():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(ops, "lib", no_device)
    geom, end = _rows([(48, 60), (60, 48)], 64)
    ops.validate_frames(geom, end, 64, 64)
    assert int(geom[1]["offset"]) % 16 == 0 and int(geom[1]["offset"]) >= 48 * 60 * 3

    def bad(field, value, match, arena=end, size=(64, 64)):
        g = geom.copy()
        g[1][field] = value
        with pytest.raises(ValueError, match=match):
            ops.validate_frames(g, arena, *size)
    bad("ch", 2, "channels")
    bad("ch", 4, "channels")
    bad("pitch", 48 * 3 - 1, "pitch")
    bad("offset", int(geom[1]["offset"]) + 8, "multiple of 16")
    bad("offset", int(geom[1]["offset"]) + 16, "leave the arena")
    bad("h0", 61, "leave the arena")
    bad("top", 1, "leaves the 64x64 output")                 # (60, 48) -> 64 x 51 rows: nh + top <= H
    bad("left", 14, "leaves the 64x64 output")
    bad("nw", 65, "leaves the 64x64 output")
    bad("sx", 0.0, "positive")
    with pytest.raises(ValueError, match="leave the arena"):
        ops.validate_frames(geom, end - 1, 64, 64)
    # the wrappers: CPU tensors stand in for the device buffers — the geometry is refused first, then the tensors themselves
    arena, tab, dst = torch.zeros(end, dtype=torch.uint8), torch.zeros(2 * 48, dtype=torch.uint8), torch.zeros((2, 6, 64, 64), dtype=torch.uint8)
    g = geom.copy()
    g[0]["pitch"] = 1
    with pytest.raises(ValueError, match="pitch"):
        ops.letterbox_frames(arena, g, tab, dst)
    with pytest.raises(ValueError, match="descriptors"):
        ops.letterbox_frames(arena, geom[:1], tab, dst)
    with pytest.raises(ValueError, match="multiple of 16"):
        ops.letterbox_frames(arena, geom, tab, torch.zeros((2, 6, 64, 72), dtype=torch.uint8))
    with pytest.raises(ValueError, match="cuda"):
        ops.letterbox_frames(arena, geom, tab, dst)
    det, count, scale = torch.zeros((2, 4, 6)), torch.zeros(2, dtype=torch.int32), torch.zeros((2, 5))
    with pytest.raises(ValueError, match="cuda"):
        ops.scale_detections(det, count, scale)


def test_budget_rule_sends_small_rectangles_to_lds_and_large_ones_to_global_memory():
    """ops.letterbox_staged restates the kernel's descriptor-level rule: every shape of the list stages (scale <= 3.2, small frames), a
    300 x 400 frame squeezed into 64 x 64 taps a rectangle of 154 rows x 1216 bytes and goes direct, a KAIST frame stages."""
    for shape, new in SHAPES:
        geom, _ = _rows([shape], new)
        assert ops.letterbox_staged(geom[0]), shape
    geom, _ = _rows([(300, 400)], 64)
    assert not ops.letterbox_staged(geom[0])
    geom, _ = _rows([(512, 640)], 640)
    assert ops.letterbox_staged(geom[0]) and (int(geom[0]["top"]), int(geom[0]["nh"]), float(geom[0]["sx"])) == (64, 512, 1.0)
    geom, _ = _rows([(2160, 3840)], 640)
    assert not ops.letterbox_staged(geom[0])


def test_forward_frames_rejects_what_forward_u8_rejects():
    m = Model(load_cfg("yolov5s_Transfusion_kaist.yaml"))
    f = torch.zeros((1, 48, 64, 3), dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        m.train().forward_frames(f, f, 64)
    m.eval()
    with pytest.raises(ValueError, match="cuda uint8"):
        m.forward_frames(f, f, 64)                                        # CPU tensors
    with pytest.raises(ValueError, match="cuda uint8"):
        m.forward_frames(f.float(), f.float(), 64)                        # wrong dtype
    with pytest.raises(ValueError):
        m.forward_frames(f, [f[0], f[0]], 64)                             # unequal batch
    with pytest.raises(ValueError):
        m.forward_frames(f[0], f[0], 64)                                  # not a batch


def test_frame_lists_parses_and_refuses():
    """ops.frame_lists, the one parser of forward_frames and submit_frames: a 4-D pair and a ragged list come back as frame lists with their
    shapes and the per-modality `uniform` flag; every other form of input is a ValueError."""
    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8)
    rgb, ir = u8(2, 48, 64, 3), u8(2, 48, 64, 1)
    fr, fi, shapes, uniform = ops.frame_lists(rgb, ir)
    assert shapes == [(48, 64), (48, 64)] and uniform == (True, True)
    assert [tuple(f.shape) for f in fr] == [(48, 64, 3)] * 2 and [tuple(f.shape) for f in fi] == [(48, 64, 1)] * 2
    assert fr[1].data_ptr() == rgb[1].data_ptr() and fi[1].data_ptr() == ir[1].data_ptr()          # views, not copies
    ragged = [u8(48, 64, 3), u8(9, 31, 3)]
    fr, fi, shapes, uniform = ops.frame_lists(ragged, (u8(48, 64, 1), u8(9, 31, 1)))
    assert shapes == [(48, 64), (9, 31)] and uniform == (False, False) and fr[1] is ragged[1] and len(fi) == 2
    assert ops.frame_lists(rgb, [ir[0], ir[1]])[3] == (True, False)                                # one modality as a tensor, one as a list
    for bad_rgb, bad_ir, match in [
            (rgb[0], ir[0], "two"),                                   # 3-D tensors: not a batch
            (rgb, None, "two"),
            ([], [], "two"),                                          # empty lists
            (u8(0, 48, 64, 3), u8(0, 48, 64, 1), "two"),              # an empty batch
            (rgb, [ir[0]], "equally long"),
            (ragged, ragged[:1], "equally long"),
            (rgb.float(), ir, "uint8"),
            ([u8(48, 64, 3), np.zeros((48, 64, 3), np.uint8)], ragged, "uint8"),       # not a tensor
            ([u8(48, 64)], [u8(48, 64)], r"\(H0, W0, ch\)"),          # a frame without its channel axis
            (u8(2, 48, 64, 2), ir, "ch = 3 or 1"),
            (u8(2, 48, 64, 4), ir, "ch = 3 or 1"),
            (rgb, u8(2, 48, 60, 1), "same size"),
            (ragged, ragged[::-1], "same size")]:
        with pytest.raises(ValueError, match=match):
            ops.frame_lists(bad_rgb, bad_ir)


def test_device_letterbox_flag_parses():
    sys.path.insert(0, REPO)
    import detect_twostream as dt
    base = ["--source1", "a", "--source2", "b"]
    assert dt.parse_opt(base).device_letterbox is False
    assert dt.parse_opt(base + ["--device-letterbox"]).device_letterbox is True
    assert os.path.exists(os.path.join(REPO, "detect_twostream.py"))


def scalar_letterbox_plane(img, nw, nh):
    """The kernel's arithmetic, one output element at a time, every operation a rounded fp32 operation (include/icaf.h)."""
    f32 = np.float32
    h0, w0, ch = img.shape
    sx, sy = f32(w0 / nw), f32(h0 / nh)

    def tap(j, scale, n):
        s = (f32(j) + f32(0.5)) * scale
        s = s - f32(0.5)
        fl = np.floor(s)
        frac = f32(s - fl)
        i = int(fl)
        return min(max(i, 0), n - 1), min(max(i + 1, 0), n - 1), frac
    out = np.empty((nh, nw, ch), np.uint8)
    xt = [tap(j, sx, w0) for j in range(nw)]
    for r in range(nh):
        y0, y1, fy = tap(r, sy, h0)
        gy = f32(1) - fy
        for j, (x0, x1, fx) in enumerate(xt):
            gx = f32(1) - fx
            for c in range(ch):
                a00, a01, a10, a11 = f32(img[y0, x0, c]), f32(img[y0, x1, c]), f32(img[y1, x0, c]), f32(img[y1, x1, c])
                top = f32(f32(a00 * gx) + f32(a01 * fx))
                bot = f32(f32(a10 * gx) + f32(a11 * fx))
                v = f32(f32(top * gy) + f32(bot * fy))
                v = np.floor(f32(v + f32(0.5)))
                out[r, j, c] = np.uint8(min(max(v, f32(0)), f32(255)))
    return out


@pytest.mark.parametrize("src,dst", [((12, 15), (17, 16)), ((15, 12), (13, 10)), ((40, 9), (13, 3)), ((9, 31), (20, 11)), ((26, 14), (13, 7)),
                                     ((7, 16), (14, 32))], ids=lambda v: f"{v[0]}x{v[1]}")
def test_scalar_fp32_restatement_equals_resize_bilinear(src, dst):
    """Up-scale, down-scale, mixed, a 3-pixel-wide result, an exact 2:1 and 1:2: the element-by-element statement of the arithmetic
    (what the kernel executes) equals the vectorised numpy of utils.datasets.resize_bilinear byte for byte."""
    g = np.random.default_rng(src[0] * 100 + src[1])
    img = g.integers(0, 256, (*src, 3), dtype=np.uint8)
    img[0, 0], img[-1, -1] = 255, 0
    nh, nw = dst
    assert np.array_equal(scalar_letterbox_plane(img, nw, nh), D.resize_bilinear(img, (nw, nh)))
