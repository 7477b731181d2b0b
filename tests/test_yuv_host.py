"""Host side of the native YUV 4:2:0 path (no GPU): utils.datasets.yuv420_to_bgr against a scalar restatement of the rule of include/icaf.h, on
an exact lattice and against Pillow; the table rows of ops.pack_yuv_frames read back through their offsets; every refusal in front of the
launch; and the entry point in the header and the built library.  Every comparison is exact."""
import itertools

import numpy as np
import pytest
import torch

from helpers import load_cfg
from icafusion_amd import _lib, ops
from icafusion_amd.models.yolo import Model
from icafusion_amd.utils import datasets as D

LAYOUTS = ("nv12", "nv21", "i420", "yv12")
LATTICE_Y = (0, 1, 15, 16, 17, 128, 234, 235, 236, 254, 255)
LATTICE_C = (0, 1, 127, 128, 129, 254, 255)


def clip8(v):
    return 0 if v < 0 else 255 if v > 255 else v


def scalar_rgb(Y, Cb, Cr, matrix):
    """(R, G, B) of one sample in Python integers: the table of the rule, line by line (`>>` floors on Python integers as on int32)."""
    c, d, e = Y - 16, Cb - 128, Cr - 128
    if matrix == 0:
        return clip8((298 * c + 409 * e + 128) >> 8), clip8((298 * c - 100 * d - 208 * e + 128) >> 8), clip8((298 * c + 516 * d + 128) >> 8)
    if matrix == 1:
        return clip8((298 * c + 459 * e + 128) >> 8), clip8((298 * c - 55 * d - 136 * e + 128) >> 8), clip8((298 * c + 541 * d + 128) >> 8)
    return clip8(Y + ((91881 * e + 32768) >> 16)), clip8(Y + ((-22554 * d - 46802 * e + 32768) >> 16)), clip8(Y + ((116130 * d + 32768) >> 16))


def scalar_bgr(y, cb, cr, matrix):
    """yuv420_to_bgr as a per-pixel loop: pixel (i, j) with chroma sample (i >> 1, j >> 1)."""
    h0, w0 = y.shape
    out = np.zeros((h0, w0, 3), np.uint8)
    for i in range(h0):
        for j in range(w0):
            out[i, j] = scalar_rgb(int(y[i, j]), int(cb[i >> 1, j >> 1]), int(cr[i >> 1, j >> 1]), matrix)[::-1]
    return out


def planes_of(h0, w0, seed):
    g = np.random.default_rng(seed)
    ch, cw = (h0 + 1) // 2, (w0 + 1) // 2
    return g.integers(0, 256, (h0, w0), dtype=np.uint8), g.integers(0, 256, (ch, cw), dtype=np.uint8), g.integers(0, 256, (ch, cw), dtype=np.uint8)


def buffer_of(y, cb, cr, layout):
    """The flat buffer a decoder hands over: luma, then CbCr / CrCb pairs (nv12 / nv21) or the two chroma planes (i420: Cb first; yv12: Cr)."""
    first, second = (cb, cr) if layout in ("nv12", "i420") else (cr, cb)
    chroma = np.stack((first, second), axis=2) if layout in ("nv12", "nv21") else np.stack((first, second), axis=0)
    return np.concatenate((y.reshape(-1), chroma.reshape(-1)))


def fill_arena(host, q, y, cb, cr):
    """Write the planes of one frame where table row `q` says they are (any pitch)."""
    g = q["g"]
    for plane, off, pitch, step in ((y, int(g["offset"]), int(g["pitch"]), 1), (cb, int(q["cb_offset"]), int(q["c_pitch"]), int(q["c_step"])),
                                    (cr, int(q["cr_offset"]), int(q["c_pitch"]), int(q["c_step"]))):
        for i, row in enumerate(plane):
            host[off + i * pitch:off + i * pitch + (len(row) - 1) * step + 1:step] = row


def row_planes(host, q):
    """(y, cb, cr) of one kind-1 table row read back from the arena through its offsets, pitches and c_step."""
    g = q["g"]
    h0, w0 = int(g["h0"]), int(g["w0"])
    ch, cw = (h0 + 1) // 2, (w0 + 1) // 2

    def plane(off, pitch, step, rows, cols):
        return np.stack([host[off + i * pitch:off + i * pitch + (cols - 1) * step + 1:step] for i in range(rows)])
    return (plane(int(g["offset"]), int(g["pitch"]), 1, h0, w0), plane(int(q["cb_offset"]), int(q["c_pitch"]), int(q["c_step"]), ch, cw),
            plane(int(q["cr_offset"]), int(q["c_pitch"]), int(q["c_step"]), ch, cw))


def lattice():
    """Every (Y, Cb, Cr) of LATTICE_Y x LATTICE_C x LATTICE_C as a frame of 22 x 112: luma rows 2i and 2i + 1 hold LATTICE_Y[i], chroma
    column j holds pair j % 49 of the Cb x Cr square.  Returns (y, cb, cr)."""
    pairs = list(itertools.product(LATTICE_C, LATTICE_C))
    y = np.repeat(np.array(LATTICE_Y, np.uint8), 2)[:, None].repeat(112, axis=1)
    cb = np.array([pairs[j % 49][0] for j in range(56)], np.uint8)[None].repeat(11, axis=0)
    cr = np.array([pairs[j % 49][1] for j in range(56)], np.uint8)[None].repeat(11, axis=0)
    return np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr)


def lattice_rgb(matrix):
    """(22, 112, 3) uint8 R, G, B the lattice frame converts to, in Python integers."""
    y, cb, cr = lattice()
    return np.array([[scalar_rgb(int(y[i, j]), int(cb[i >> 1, j >> 1]), int(cr[i >> 1, j >> 1]), matrix) for j in range(112)] for i in range(22)], np.uint8)


@pytest.mark.parametrize("matrix", [0, 1, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(5, 7), (6, 8)], ids=["5x7", "6x8"])
def test_yuv420_to_bgr_equals_the_scalar_rule(shape, layout, matrix):
    """An odd and an even frame through the decoder buffer of every layout: the planes come back, and the image is the per-pixel rule."""
    y, cb, cr = planes_of(*shape, seed=shape[0] * 10 + matrix)
    py, pcb, pcr = D.yuv420_planes(buffer_of(y, cb, cr, layout), *shape, layout)
    assert np.array_equal(py, y) and np.array_equal(pcb, cb) and np.array_equal(pcr, cr)
    got = D.yuv420_to_bgr(py, pcb, pcr, matrix)
    assert got.dtype == np.uint8 and got.shape == (*shape, 3)
    assert np.array_equal(got, scalar_bgr(y, cb, cr, matrix))


@pytest.mark.parametrize("matrix", [0, 1, 2])
def test_yuv420_to_bgr_on_the_exact_lattice(matrix):
    """Every triple of the lattice: the bytes of the rule in Python integers, with both clips of all three channels among them."""
    want = lattice_rgb(matrix)
    assert np.array_equal(D.yuv420_to_bgr(*lattice(), matrix), want[:, :, ::-1])
    y, cb, cr = lattice()
    for ch, name in enumerate("RGB"):
        raw = [scalar_rgb_unclipped(int(y[i, j]), int(cb[i >> 1, j >> 1]), int(cr[i >> 1, j >> 1]), matrix)[ch] for i in range(22) for j in range(98)]
        assert min(raw) < 0 and max(raw) > 255, (name, min(raw), max(raw))
    assert len({(int(y[i, j]), int(cb[i >> 1, j >> 1]), int(cr[i >> 1, j >> 1])) for i in range(22) for j in range(112)}) == 11 * 49


def scalar_rgb_unclipped(Y, Cb, Cr, matrix):
    c, d, e = Y - 16, Cb - 128, Cr - 128
    if matrix == 2:
        return Y + ((91881 * e + 32768) >> 16), Y + ((-22554 * d - 46802 * e + 32768) >> 16), Y + ((116130 * d + 32768) >> 16)
    rv, gu, gv, bu = (409, -100, -208, 516) if matrix == 0 else (459, -55, -136, 541)
    return (298 * c + rv * e + 128) >> 8, (298 * c + gu * d + gv * e + 128) >> 8, (298 * c + bu * d + 128) >> 8


@pytest.mark.parametrize("matrix", [0, 1, 2])
def test_grey_axis_stays_grey(matrix):
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    c = np.full((8, 8), 128, np.uint8)
    bgr = D.yuv420_to_bgr(y, c, c, matrix)
    assert np.array_equal(bgr[:, :, 0], bgr[:, :, 1]) and np.array_equal(bgr[:, :, 1], bgr[:, :, 2])
    if matrix == 2:
        assert np.array_equal(bgr[:, :, 0], y)


def test_full_range_matrix_against_pillow():
    """Pillow's YCbCr -> RGB is the JFIF conversion from coarser tables: over the whole Cb x Cr square at 16 luma values it never differs from
    matrix 2 by more than 1 (a wrong coefficient or shift gives 2 or more)."""
    from PIL import Image
    ys = np.array([0, 1, 16, 17, 50, 77, 100, 127, 128, 150, 180, 200, 235, 240, 254, 255], np.uint8)
    sq = np.arange(65536)
    cb, cr = (sq >> 8).astype(np.uint8)[None].repeat(16, axis=0), (sq & 255).astype(np.uint8)[None].repeat(16, axis=0)      # (16, 65536) chroma
    y = ys.repeat(2)[:, None].repeat(2 * 65536, axis=1)                                                                      # (32, 131072) luma
    ours = D.yuv420_to_bgr(y, cb, cr, 2)[::2, ::2, ::-1]
    packed = np.stack((ys[:, None].repeat(65536, axis=1), cb, cr), axis=2)
    pil = np.asarray(Image.frombytes("YCbCr", (65536, 16), packed.tobytes()).convert("RGB"))
    assert np.abs(ours.astype(np.int32) - pil.astype(np.int32)).max() <= 1


def test_layouts_pack_to_different_tables_and_the_same_image():
    """One content as nv12, nv21, i420 and yv12 buffers (odd 9 x 13 frame): four different table rows and arenas, one BGR image; nv21 and yv12
    are nv12 and i420 with Cb and Cr exchanged."""
    h0, w0 = 9, 13
    y, cb, cr = planes_of(h0, w0, 4)
    want = D.yuv420_to_bgr(y, cb, cr, 1)
    geom1, _ = ops.frame_geometry([(h0, w0)], 32)
    rows, arenas = {}, {}
    for layout in LAYOUTS:
        q, end = ops.pack_yuv_frames(geom1, layout, matrix="bt709")
        assert end == h0 * w0 + 2 * 5 * 7 and int(q[0]["kind"]) == 1 and int(q[0]["matrix"]) == 1 and int(q[0]["g"]["ch"]) == 1
        ops.validate_yuv_frames(q, end, 32, 32)
        host = np.zeros((end,), np.uint8)
        fill_arena(host, q[0], y, cb, cr)
        assert np.array_equal(host, buffer_of(y, cb, cr, layout))                     # the decoder's buffer, byte for byte
        assert all(np.array_equal(a, b) for a, b in zip(row_planes(host, q[0]), (y, cb, cr)))
        assert np.array_equal(D.yuv420_to_bgr(*row_planes(host, q[0]), 1), want)
        rows[layout], arenas[layout] = q[0], host
    assert (int(rows["nv12"]["c_step"]), int(rows["i420"]["c_step"])) == (2, 1)
    assert int(rows["nv12"]["cr_offset"]) == int(rows["nv12"]["cb_offset"]) + 1 and int(rows["nv21"]["cb_offset"]) == int(rows["nv21"]["cr_offset"]) + 1
    assert rows["nv12"].tobytes() != rows["i420"].tobytes() and not np.array_equal(arenas["nv12"], arenas["i420"])
    for a, b in (("nv12", "nv21"), ("i420", "yv12")):
        assert (int(rows[a]["cb_offset"]), int(rows[a]["cr_offset"])) == (int(rows[b]["cr_offset"]), int(rows[b]["cb_offset"]))
        assert np.array_equal(D.yuv420_to_bgr(*D.yuv420_planes(arenas[a], h0, w0, b), 1), D.yuv420_to_bgr(y, cr, cb, 1))


def test_pack_yuv_frames_passes_interleaved_rows_through_and_takes_pitches():
    geom1, _ = ops.frame_geometry([(10, 12), (10, 12), (6, 8)], 32)
    plain = geom1.copy()
    end_plain = ops.pack_frames(plain, [3, 1, 3], pitch=[40, None, None])
    rows, end = ops.pack_yuv_frames(geom1, [3, 1, 3], pitch=[40, None, None])
    assert end == end_plain and np.array_equal(rows["g"], plain) and not rows["kind"].any()
    rows, end = ops.pack_yuv_frames(geom1, ["i420", 1, "nv12"], pitch=[16, None, 11], c_pitch=[9, None, 10], matrix=2)
    a, b, c = rows
    assert (int(a["g"]["pitch"]), int(a["c_pitch"]), int(a["cb_offset"]), int(a["cr_offset"])) == (16, 9, 160, 160 + 5 * 9)
    assert int(b["kind"]) == 0 and int(b["g"]["offset"]) == 256 and int(c["g"]["offset"]) == 512
    assert (int(c["cb_offset"]), int(c["cr_offset"]), int(c["c_step"])) == (512 + 66, 512 + 67, 2) and end == 512 + 66 + 3 * 10
    ops.validate_yuv_frames(rows, end, 32, 32)
    assert ops.yuv_matrix_code("bt601") == 0 and ops.yuv_matrix_code("bt601-full") == 2 and ops.yuv_matrix_code(1) == 1
    for bad in ("bt2020", 3, None, True):
        with pytest.raises(ValueError, match="unknown YUV matrix"):
            ops.yuv_matrix_code(bad)
    with pytest.raises(ValueError, match="unknown layout"):
        ops.pack_yuv_frames(geom1, "yuyv")


def test_yuv_budget_rule_on_the_host():
    """ops.yuv_letterbox_staged restates the header's rule: HD and 512 x 640 frames to 640 stage, a 4.7 x squeeze does not; a kind-0 row
    follows letterbox_staged."""
    def row(shape, new, layout):
        return ops.pack_yuv_frames(ops.frame_geometry([shape], new)[0], layout)[0][0]
    for layout in ("nv12", "i420"):
        assert ops.yuv_letterbox_staged(row((512, 640), 640, layout)) and ops.yuv_letterbox_staged(row((1080, 1920), 640, layout))
        assert not ops.yuv_letterbox_staged(row((300, 400), 64, layout)) and not ops.yuv_letterbox_staged(row((2160, 3840), 640, layout))
    # 1080 x 1920 to 640 is a 3 x squeeze: 100 luma rows of 14 vectors; nv12: 51 rows of 14 vectors of pairs, i420: 2 x 51 rows of 8 vectors
    assert (100 * 14 + 51 * 14) * 16 <= _lib.YUV_LDS_BYTES and (100 * 14 + 2 * 51 * 8) * 16 <= _lib.YUV_LDS_BYTES
    tight = row((1080, 1920), 640, "nv12")
    tight["g"]["sy"] = np.float32(3.7)                                    # 122 luma rows, 62 chroma rows: 41,216 bytes, one vector row too many
    assert (122 * 14 + 62 * 14) * 16 > _lib.YUV_LDS_BYTES and not ops.yuv_letterbox_staged(tight)
    for ch in (3, 1):                                                     # a kind-0 row follows letterbox_staged
        for shape, new in (((300, 400), 64), ((48, 60), 64), ((1080, 1920), 640)):
            q = row(shape, new, ch)
            assert ops.yuv_letterbox_staged(q) == ops.letterbox_staged(q["g"])


def test_validate_yuv_frames_refuses_with_row_and_reason():
    geom1, _ = ops.frame_geometry([(48, 60), (37, 53)], 64)
    for layout in ("nv12", "i420"):
        good, end = ops.pack_yuv_frames(geom1, [3, layout])
        ops.validate_yuv_frames(good, end, 64, 64)

        def bad(match, arena_bytes=end, **fields):
            rows = good.copy()
            for k, v in fields.items():
                if k in rows.dtype.names:
                    rows[k][1] = v
                else:
                    rows["g"][k][1] = v
            with pytest.raises(ValueError, match=match):
                ops.validate_yuv_frames(rows, arena_bytes, 64, 64)
        bad("frame 1: Cr bytes .* leave the arena" if layout == "i420" else "frame 1: C[br] bytes .* leave the arena", arena_bytes=end - 1)
        bad("frame 1: Cb bytes .* leave the arena", cb_offset=-2, cr_offset=-1 if layout == "nv12" else int(good[1]["cr_offset"]))
        bad("frame 1: c_pitch .* is less than a chroma row of 27 samples", c_pitch=27 * int(good[1]["c_step"]) - 1)
        bad("frame 1: c_step 3", c_step=3)
        bad("frame 1: c_step 0", c_step=0)
        bad("frame 1: matrix 3", matrix=3)
        bad("frame 1: matrix -1", matrix=-1)
        bad("frame 1: kind 2", kind=2)
        bad("frame 1: a YUV 4:2:0 row describes its Y plane with ch 1, got 3", arena_bytes=end + 37 * 106, ch=3, pitch=53 * 3)
        # everything validate_frames refuses, on a YUV row and on the interleaved row beside it
        bad("frame 1: pitch 52 is less than a row", pitch=52)
        bad("frame 1: offset .* multiple of 16", offset=int(good[1]["g"]["offset"]) + 8)
        bad("frame 1: bytes .* leave the arena", arena_bytes=int(good[1]["g"]["offset"]) + 37 * 53 - 1)
        bad("frame 1: resized block", top=60)
        bad("frame 1: tap scales", sx=0.0)
        bad("frame 1: 2 interleaved channels", ch=2)
        rows = good.copy()
        rows["g"]["ch"][0] = 4
        with pytest.raises(ValueError, match="frame 0: 4 interleaved channels"):
            ops.validate_yuv_frames(rows, end, 64, 64)
    nv, end = ops.pack_yuv_frames(geom1, [3, "nv12"])
    nv["cr_offset"][1] += 1
    with pytest.raises(ValueError, match="frame 1: interleaved chroma needs cb_offset and cr_offset one byte apart"):
        ops.validate_yuv_frames(nv, end + 8, 64, 64)


def test_letterbox_yuv_frames_validates_before_any_device_call():
    """CPU tensors reach the refusals in order: the rows, then 'no CPU fallback'."""
    geom1, _ = ops.frame_geometry([(48, 60)], 64)
    rows, end = ops.pack_yuv_frames(np.concatenate((geom1, geom1)), ["nv12", 1])
    arena, dst = torch.zeros((end,), dtype=torch.uint8), torch.zeros((1, 6, 64, 64), dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda tensors"):
        ops.letterbox_yuv_frames(arena, rows, ops.geom_tensor(rows), dst)
    with pytest.raises(ValueError, match="leave the arena"):
        ops.letterbox_yuv_frames(arena[:-1], rows, ops.geom_tensor(rows), dst)
    with pytest.raises(ValueError, match="YUV_GEOM_DTYPE"):
        ops.letterbox_yuv_frames(arena, rows["g"].copy(), ops.geom_tensor(rows), dst)
    with pytest.raises(ValueError, match="smaller than the descriptor rows"):
        ops.letterbox_yuv_frames(arena, rows, ops.geom_tensor(rows)[:-1], dst)


def test_tensor_level_refusals():
    """What forward_frames(formats=...) and submit_frames refuse of the tensors, before any device call: odd H0 or W0, a YUV buffer whose row
    count is not 3 * H0 / 2, unknown layouts, and YUV together with val_size."""
    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8)
    fr, fi, shapes, uniform = ops.yuv_frame_lists(u8(2, 72, 64), u8(2, 48, 64, 1), ("nv12", None))
    assert shapes == [(48, 64)] * 2 and uniform == (True, True) and [tuple(f.shape) for f in fr] == [(72, 64)] * 2
    assert ops.yuv_frame_lists([u8(72, 64), u8(9, 4)], [u8(72, 64), u8(9, 4)], ("i420", "yv12"))[2] == [(48, 64), (6, 4)]
    assert ops.yuv_frame_lists(u8(2, 48, 64, 3), [u8(72, 64)] * 2, (None, "nv21"))[2:] == ([(48, 64)] * 2, (True, False))
    for rgb, ir, formats, match in [
            (u8(1, 69, 64), u8(1, 46 + 1, 64, 1), ("nv12", None), "even H0 and W0, got 47x64"),
            (u8(1, 72, 63), u8(1, 48, 63, 1), ("nv12", None), "even H0 and W0, got 48x63"),
            (u8(1, 70, 64), u8(1, 48, 64, 1), ("nv12", None), r"shape \(3 \* H0 // 2, W0\)"),
            (u8(1, 72, 60), u8(1, 48, 64, 1), ("i420", None), r"shape \(3 \* H0 // 2, W0\)"),
            (u8(1, 70, 64), u8(1, 70, 64), ("nv12", "nv12"), r"3 \* H0 // 2 rows, got 70"),
            (u8(1, 72, 64), u8(1, 36, 64), ("nv12", "nv12"), r"shape \(3 \* H0 // 2, W0\)"),
            (u8(1, 48, 64, 3), u8(1, 48, 64, 1), ("nv12", None), "two batch tensors"),                 # an interleaved batch handed over as nv12
            ([u8(48, 64, 3)], [u8(48, 64, 1)], ("nv12", None), "nv12 frames must be uint8 tensors of shape"),
            (u8(1, 72, 64), u8(1, 48, 64, 1), ("yuyv", None), "formats="),
            (u8(1, 72, 64), u8(1, 48, 64, 1), ("nv12",), "formats="),
            (u8(1, 72, 64).float(), u8(1, 48, 64, 1), ("nv12", None), "uint8"),
            (u8(2, 72, 64), u8(1, 48, 64, 1), ("nv12", None), "equally long")]:
        with pytest.raises(ValueError, match=match):
            ops.yuv_frame_lists(rgb, ir, formats)
    m = Model(load_cfg("yolov5n_Transfusion_kaist.yaml")).eval()
    with pytest.raises(ValueError, match="even H0 and W0"):
        m.forward_frames(u8(1, 69, 64), u8(1, 47, 64, 1), 64, formats=("nv12", None))
    with pytest.raises(ValueError, match=r"3 \* H0 // 2"):
        m.forward_frames(u8(1, 70, 64), u8(1, 48, 64, 1), 64, formats=("nv12", None))
    with pytest.raises(ValueError, match="val_size"):
        m.forward_frames(u8(1, 72, 64), u8(1, 48, 64, 1), 64, formats=("nv12", None), val_size=64)
    with pytest.raises(ValueError, match="unknown YUV matrix"):
        m.forward_frames(u8(1, 72, 64), u8(1, 48, 64, 1), 64, formats=("nv12", None), yuv_matrix="bt2020")
    with pytest.raises(ValueError, match="cuda uint8"):
        m.forward_frames(u8(1, 72, 64), u8(1, 48, 64, 1), 64, formats=("nv12", None))             # CPU tensors: refused after the shapes
    with pytest.raises(ValueError, match="cuda uint8"):
        m.forward_frames(u8(1, 48, 64, 3), u8(1, 48, 64, 1), 64, formats=(None, None))            # no YUV modality: today's path, today's refusal


def test_entry_point_is_declared_and_exported():
    """icaf_letterbox_yuv_frames: in include/icaf.h with its 80-byte row, bound from there, and exported by the built library."""
    assert "icaf_letterbox_yuv_frames" in _lib.HEADER.funcs and "icaf_yuv_geom" in _lib.HEADER.structs
    assert [p[0] for p in _lib.HEADER.funcs["icaf_letterbox_yuv_frames"][1]] == ["arena", "geom", "nstreams", "B", "dst", "ctot", "H", "W", "swap_rb", "s"]
    assert ops.YUV_GEOM_DTYPE.itemsize == 80 and ops.YUV_GEOM_DTYPE.names == ("g", "cb_offset", "cr_offset", "c_pitch", "c_step", "matrix", "kind")
    assert [ops.YUV_GEOM_DTYPE.fields[k][1] for k in ops.YUV_GEOM_DTYPE.names] == [0, 48, 56, 64, 68, 72, 76]
    assert _lib.YUV_LDS_BYTES == 40960
    assert hasattr(_lib.lib(), "icaf_letterbox_yuv_frames")
