"""16-bit thermal frames on the host (no GPU): the gain-control rule of include/icaf.h as utils.datasets.agc_window / agc_u16_to_u8 against a
scalar restatement in Python integers, the rank lattice of both strict inequalities, degenerate content, the 64-bit products, the byte
order, the 257 * f identity, the multiply-and-shift division the kernels use, the table rows of ops.pack_y16_frames, every refusal of
ops.validate_y16_frames and the two entry points in the header and in the built library.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from icafusion_amd import _lib, ops
from icafusion_amd.utils import datasets as D


# ---- the rule, restated pixel by pixel in Python integers ---------------------------------------------------------------------------
def scalar_window(frame, clip=(100, 100)):
    clip_lo, clip_hi = clip
    count = [0] * 65536
    n = 0
    for v in frame.reshape(-1).tolist():
        count[v] += 1
        n += 1
    c, lo = 0, None
    for v in range(65536):                       # C(v): pixels <= v
        c += count[v]
        if 10000 * c > clip_lo * n:
            lo = v
            break
    d, hi = 0, None
    for v in range(65535, -1, -1):               # D(v): pixels >= v
        d += count[v]
        if 10000 * d > clip_hi * n:
            hi = v
            break
    return lo, hi


def scalar_map(frame, lo, hi):
    d = max(hi - lo, 1)
    out = [min(255, ((max(v, lo) - lo) * 255 + (d >> 1)) // d) for v in frame.reshape(-1).tolist()]
    return np.array(out, np.uint8).reshape(frame.shape)


# ---- frames the device tests share ---------------------------------------------------------------------------------------------------
def content(kind, h0, w0, seed):
    """One (h0, w0) uint16 frame: "random" uniform counts, "flat" one code, "narrow" a scene of sigma 60 counts around one level (a few
    hundred adjacent codes), "two" two codes, "ends" random counts with codes 0 and 65535 present."""
    g = np.random.default_rng(seed)
    if kind == "random":
        return g.integers(0, 65536, (h0, w0), dtype=np.uint16)
    if kind == "flat":
        return np.full((h0, w0), 12345, np.uint16)
    if kind == "narrow":
        return np.clip(np.rint(g.normal(30000 + 37 * seed, 60.0, (h0, w0))), 0, 65535).astype(np.uint16)
    if kind == "two":
        return np.where(g.random((h0, w0)) < 0.3, 4000, 4007).astype(np.uint16)
    if kind == "ends":
        f = g.integers(0, 65536, (h0, w0), dtype=np.uint16)
        f.reshape(-1)[0], f.reshape(-1)[-1] = 65535, 0
        return f
    raise KeyError(kind)


def lattice_frame(side, exact, clip=100, seed=0):
    """100 x 100 (n = 10000, so `clip` basis points are exactly `clip` pixels): side "lo" puts clip (+ 1 unless `exact`) pixels at the
    lowest code 500 and one pixel at 650, side "hi" the mirror at 60000 and 59000; everything else is 800 .. 899, shuffled."""
    g = np.random.default_rng(seed)
    f = g.integers(800, 900, (10000,)).astype(np.uint16)
    k = clip + (0 if exact else 1)
    f[:k] = 500 if side == "lo" else 60000
    f[k] = 650 if side == "lo" else 59000
    return g.permutation(f).reshape(100, 100)


def overflow_frame():
    """512 x 640: 220,000 pixels at code 1000, the rest in 1001 .. 3000.  10000 * C(1000) = 2.2e9 exceeds 2^31: a signed 32-bit product is
    negative there and at every later code, so a 32-bit implementation never finds lo = 1000."""
    g = np.random.default_rng(3)
    f = g.integers(1001, 3001, (512 * 640,)).astype(np.uint16)
    f[:220000] = 1000
    return g.permutation(f).reshape(512, 640)


def fill_y16(host, q, frame):
    """Write `frame` into the host arena where row q says, little-endian, row by row at q's pitch; the padding keeps what it held."""
    g = q["g"]
    h0, w0, o, p = int(g["h0"]), int(g["w0"]), int(g["offset"]), int(g["pitch"])
    rows = host[o:o + h0 * p].reshape(h0, p)
    rows[:, 0:2 * w0:2] = (frame & 0xFF).astype(np.uint8)
    rows[:, 1:2 * w0:2] = (frame >> 8).astype(np.uint8)


def read_y16(host, q):
    g = q["g"]
    h0, w0, o, p = int(g["h0"]), int(g["w0"]), int(g["offset"]), int(g["pitch"])
    rows = host[o:o + h0 * p].reshape(h0, p)[:, :2 * w0].astype(np.uint16)
    return rows[:, 0::2] | (rows[:, 1::2] << 8)


# ---- the rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [(100, 100), (0, 0), (4999, 4999), (250, 3)], ids=lambda c: f"{c[0]}-{c[1]}")
@pytest.mark.parametrize("kind", ["random", "flat", "narrow", "two", "ends"])
def test_window_and_mapping_equal_the_scalar_rule(kind, clip):
    for seed, (h0, w0) in enumerate([(37, 53), (1, 1), (3, 5), (64, 64)]):
        f = content(kind, h0, w0, seed)
        lo, hi = D.agc_window(f, clip)
        assert (lo, hi) == scalar_window(f, clip) and 0 <= lo <= hi <= 65535
        assert np.array_equal(D.agc_u16_to_u8(f, lo, hi), scalar_map(f, lo, hi))
        for window in ((0, 65535), (lo, lo), (hi, min(hi + 1, 65535)), (0, 0), (65535, 65535)):
            assert np.array_equal(D.agc_u16_to_u8(f, *window), scalar_map(f, *window)), window
    assert D.agc_window(content(kind, 9, 11, 5)) == D.agc_window(content(kind, 9, 11, 5), D.AGC_CLIP) and D.AGC_CLIP == (100, 100)


def test_rank_lattice_both_inequalities_are_strict():
    """Exactly clip pixels at the lowest code do not satisfy 10000 C > clip n: lo is the NEXT code; one more pixel there and lo is that
    code.  The mirror for hi.  The other end of each frame is untouched by the lattice pixels."""
    assert D.agc_window(lattice_frame("lo", True), (100, 0))[0] == 650
    assert D.agc_window(lattice_frame("lo", False), (100, 0))[0] == 500
    assert D.agc_window(lattice_frame("hi", True), (0, 100))[1] == 59000
    assert D.agc_window(lattice_frame("hi", False), (0, 100))[1] == 60000
    for side in ("lo", "hi"):
        for exact in (True, False):
            for clip in ((100, 100), (0, 0), (100, 0), (0, 100), (4999, 4999)):
                f = lattice_frame(side, exact)
                assert D.agc_window(f, clip) == scalar_window(f, clip)
    f = lattice_frame("lo", True)
    assert D.agc_window(f, (0, 0)) == (int(f.min()), int(f.max())) == (500, 899)
    lo, hi = D.agc_window(f, (4999, 4999))
    assert 800 <= lo <= hi <= 899


def test_degenerate_and_edge_content():
    flat = content("flat", 7, 9, 0)
    assert D.agc_window(flat) == (12345, 12345) and not D.agc_u16_to_u8(flat, 12345, 12345).any()       # a flat frame maps to 0
    two = content("two", 40, 40, 1)
    assert D.agc_window(two, (0, 0)) == (4000, 4007)
    assert set(np.unique(D.agc_u16_to_u8(two, 4000, 4007)).tolist()) == {0, 255}
    ends = content("ends", 20, 20, 2)
    assert D.agc_window(ends, (0, 0)) == (0, 65535)
    m = D.agc_u16_to_u8(ends, 0, 65535)
    assert m.reshape(-1)[0] == 255 and m.reshape(-1)[-1] == 0
    f = np.array([[10, 20, 30, 40, 50]], np.uint16)
    assert D.agc_u16_to_u8(f, 20, 40).tolist() == [[0, 0, 128, 255, 255]]                              # (10 * 255 + 10) // 20 = 128
    for bad in ((5, 4), (-1, 4), (0, 65536)):
        with pytest.raises(ValueError, match="0 <= lo <= hi <= 65535"):
            D.agc_u16_to_u8(f, *bad)
    for bad in ((5000, 0), (0, -1), (1.5, 2), (1,)):
        with pytest.raises(ValueError, match="basis points"):
            D.agc_window(f, bad)
    with pytest.raises(ValueError, match="uint16"):
        D.agc_window(f.astype(np.uint8))
    assert D.agc_window(f.view(np.int16)) == D.agc_window(f)                                            # int16 carries the same bits


def test_products_are_64_bit():
    f = overflow_frame()
    assert f.size == 327680 and int((f == 1000).sum()) == 220000
    assert D.agc_window(f) == scalar_window(f) and D.agc_window(f)[0] == 1000
    c = np.cumsum(np.bincount(f.reshape(-1), minlength=65536))
    wrapped = (10000 * c.astype(np.int64)).astype(np.int32)                                             # what a signed 32-bit product holds
    assert not (wrapped[1000:3001] > 100 * f.size).any()                                                # it never finds a lo among the codes present


def test_byte_order_is_little_endian():
    a, b = np.full((4, 6), 0x0102, np.uint16), np.full((4, 6), 0x0201, np.uint16)
    geom1, _ = ops.frame_geometry([(4, 6)] * 2, 64)
    rows, end = ops.pack_y16_frames(geom1, "y16")
    host = np.zeros((end,), np.uint8)
    fill_y16(host, rows[0], a)
    fill_y16(host, rows[1], b)
    oa, ob = int(rows[0]["g"]["offset"]), int(rows[1]["g"]["offset"])
    assert host[oa:oa + 2].tolist() == [0x02, 0x01] and host[ob:ob + 2].tolist() == [0x01, 0x02]
    assert np.array_equal(host[oa:oa + 48].view("<u2").reshape(4, 6), a)
    assert D.agc_window(a) == (0x0102, 0x0102) and D.agc_window(b) == (0x0201, 0x0201)
    t = torch.from_numpy(a.view(np.int16))
    assert ops.y16_bytes(t)[0, :2].tolist() == [0x02, 0x01] and tuple(ops.y16_bytes(t).shape) == (4, 12)


def test_the_257_identity():
    g = np.random.default_rng(8)
    f = g.integers(0, 256, (33, 47), dtype=np.uint8)
    f.reshape(-1)[:256] = np.arange(256)
    assert np.array_equal(D.agc_u16_to_u8(f.astype(np.uint16) * 257, 0, 65535), f)
    assert np.array_equal(D.agc_u16_to_u8(f.astype(np.uint16) << 8, 0, 65280), f)


def test_multiply_and_shift_division_is_exact():
    """(x * m) >> 40 with m = 2^40 // d + 1 equals x // d: at every multiple of d and the number in front of it (where a wrong reciprocal
    shows first) below 2^24, for every divisor up to 300, the largest ones, powers of two and their neighbours, and 1,500 random ones."""
    g = np.random.default_rng(4)
    ds = set(range(1, 301)) | {65535, 65534, 65280, 32768, 32767, 32769, 16384, 4096, 255, 257} | set(g.integers(301, 65536, 1500).tolist())
    top = 65535 * 255 + 32767
    assert top < 1 << 24
    for d in sorted(ds):
        m = (1 << 40) // d + 1
        k = np.arange(1, top // d + 2, dtype=np.uint64) * np.uint64(d)
        x = np.concatenate((k - np.uint64(1), k[k <= top], np.array([0, top], np.uint64)))
        assert top * m < 1 << 64
        assert np.array_equal((x * np.uint64(m)) >> np.uint64(40), x // np.uint64(d)), d


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def test_pack_y16_frames_rows_read_back_through_their_offsets():
    shapes = [(48, 60), (37, 53), (1, 1)]
    geom1, _ = ops.frame_geometry(shapes, 64)
    frames = [content("random", h, w, 20 + i) for i, (h, w) in enumerate(shapes)]
    bgr = [np.random.default_rng(30 + i).integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(shapes)]
    pitches = [3 * w + 5 for _, w in shapes] + [2 * w + 6 for _, w in shapes]
    rows, end = ops.pack_y16_frames(np.concatenate((geom1, geom1)), [3] * 3 + ["y16"] * 3, pitch=pitches, clip=(250, 3),
                                    window=[None] * 3 + [None, (7, 900), None])
    assert rows.dtype == ops.Y16_GEOM_DTYPE and rows["kind"].tolist() == [0, 0, 0, 1, 1, 1] and rows["mode"].tolist() == [0, 0, 0, 1, 0, 1]
    assert rows["clip_lo"][3:].tolist() == [250] * 3 and rows["clip_hi"][3:].tolist() == [3] * 3 and (rows["lo"][4], rows["hi"][4]) == (7, 900)
    assert not (rows["g"]["offset"] % ops.FRAME_ALIGN).any() and rows["g"]["ch"].tolist() == [3, 3, 3, 1, 1, 1]
    assert rows["g"]["pitch"].tolist() == pitches and end == int(rows[5]["g"]["offset"]) + 1 * 8
    host = np.full((end,), 0x5C, np.uint8)
    for q, f in zip(rows[:3], bgr):
        h0, w0, _ = f.shape
        host[int(q["g"]["offset"]):int(q["g"]["offset"]) + h0 * int(q["g"]["pitch"])].reshape(h0, -1)[:, :3 * w0] = f.reshape(h0, 3 * w0)
    for q, f in zip(rows[3:], frames):
        fill_y16(host, q, f)
    for q, f in zip(rows[3:], frames):
        assert np.array_equal(read_y16(host, q), f)
    ends = sorted((int(q["g"]["offset"]), int(q["g"]["offset"]) + int(q["g"]["h0"]) * int(q["g"]["pitch"])) for q in rows)
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))                                             # no two frames overlap
    ops.validate_y16_frames(rows, end, 64, 64)
    # defaults: tight pitch, the default clip, one window for every Y16 row; Y16 rows repacked keep their geometry
    tight, _ = ops.pack_y16_frames(geom1, "y16", window=(100, 200))
    assert tight["g"]["pitch"].tolist() == [120, 106, 2] and tight["mode"].tolist() == [0] * 3 and tight["hi"].tolist() == [200] * 3
    again, _ = ops.pack_y16_frames(tight, "y16")
    assert again["mode"].tolist() == [1] * 3 and (again["clip_lo"][0], again["clip_hi"][0]) == D.AGC_CLIP
    assert np.array_equal(again["g"], tight["g"])
    with pytest.raises(ValueError, match="unknown layout"):
        ops.pack_y16_frames(geom1, "y8")
    with pytest.raises(ValueError, match="basis points"):
        ops.pack_y16_frames(geom1, "y16", clip=(5000, 0))
    with pytest.raises(ValueError, match="2 gain-control windows for 3 frames"):
        ops.pack_y16_frames(geom1, "y16", window=[(1, 2), (3, 4)])


def test_y16_budget_rule_on_the_host():
    """A Y16 row stages its MAPPED bytes: the rule of a grey frame of the same size, whatever its pitch."""
    shapes = [(48, 60), (300, 400), (512, 640), (1080, 1920), (2160, 3840)]
    geom1, _ = ops.frame_geometry(shapes, 64)
    rows, _ = ops.pack_y16_frames(np.concatenate((geom1, geom1)), [1] * 5 + ["y16"] * 5)
    assert [ops.y16_letterbox_staged(q) for q in rows[5:]] == [ops.letterbox_staged(q["g"]) for q in rows[:5]]
    assert [ops.y16_letterbox_staged(q) for q in rows[:5]] == [ops.letterbox_staged(q["g"]) for q in rows[:5]]
    assert ops.y16_letterbox_staged(rows[5]) and not ops.y16_letterbox_staged(rows[9])
    big, _ = ops.frame_geometry([(512, 640)], 640)
    assert ops.y16_letterbox_staged(ops.pack_y16_frames(big, "y16")[0][0])
    assert _lib.Y16_LDS_BYTES == _lib.LETTERBOX_LDS_BYTES


def test_validate_y16_frames_refuses_with_row_and_reason():
    geom1, _ = ops.frame_geometry([(48, 60), (37, 53)], 64)
    good, end = ops.pack_y16_frames(geom1, [3, "y16"], window=[None, (10, 20)])
    ops.validate_y16_frames(good, end, 64, 64)

    def bad(match, arena_bytes=end, **fields):
        rows = good.copy()
        for k, v in fields.items():
            if k in rows.dtype.names:
                rows[k][1] = v
            else:
                rows["g"][k][1] = v
        with pytest.raises(ValueError, match=match):
            ops.validate_y16_frames(rows, arena_bytes, 64, 64)
    bad("frame 1: offset .* multiple of 16", offset=int(good[1]["g"]["offset"]) + 8)
    bad("frame 1: pitch 107 must be an even number of bytes", arena_bytes=end + 64, pitch=107)
    bad("frame 1: pitch 104 must be an even number of bytes, at least 2 \\* w0 = 106", pitch=104)
    bad("frame 1: pitch 52 is less than a row", pitch=52)
    bad("frame 1: bytes .* leave the arena", arena_bytes=end - 1)
    bad("frame 1: clip \\(5000, 100\\) must lie in 0..4999", clip_lo=5000)
    bad("frame 1: clip \\(100, -1\\) must lie in 0..4999", clip_hi=-1)
    bad("frame 1: window \\(21, 20\\) must satisfy 0 <= lo <= hi <= 65535", lo=21)
    bad("frame 1: window \\(10, 65536\\)", hi=65536)
    bad("frame 1: window \\(-1, 20\\)", lo=-1)
    bad("frame 1: mode 2", mode=2)
    bad("frame 1: kind 2", kind=2)
    bad("frame 1: a 16-bit thermal row has ch 1, got 3", arena_bytes=end + 37 * 160, ch=3, pitch=160)
    bad("frame 1: resized block", top=60)
    bad("frame 1: tap scales", sx=0.0)
    rows = good.copy()
    rows["mode"][1], rows["lo"][1] = 1, 70000                                # a percentile row does not read its window
    ops.validate_y16_frames(rows, end, 64, 64)
    rows["g"]["ch"][0] = 4
    with pytest.raises(ValueError, match="frame 0: 4 interleaved channels"):
        ops.validate_y16_frames(rows, end, 64, 64)


def test_launches_validate_before_any_device_call():
    """CPU tensors reach the refusals in order: the rows and tables, then 'no CPU fallback'."""
    geom1, _ = ops.frame_geometry([(48, 60)], 64)
    rows, end = ops.pack_y16_frames(np.concatenate((geom1, geom1)), [3, "y16"])
    arena, dst, win = torch.zeros((end,), dtype=torch.uint8), torch.zeros((1, 6, 64, 64), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.int32)
    tab = ops.geom_tensor(rows)
    for launch in (lambda a, r, t, w: ops.y16_window(a, r, t, w, 1, 64, 64), lambda a, r, t, w: ops.letterbox_y16_frames(a, r, t, w, dst)):
        with pytest.raises(ValueError, match="cuda tensors"):
            launch(arena, rows, tab, win)
        with pytest.raises(ValueError, match="leave the arena"):
            launch(arena[:-1], rows, tab, win)
        with pytest.raises(ValueError, match="Y16_GEOM_DTYPE"):
            launch(arena, rows["g"].copy(), tab, win)
        with pytest.raises(ValueError, match="smaller than the"):
            launch(arena, rows, tab[:-1], win)
        with pytest.raises(ValueError, match="window table"):
            launch(arena, rows, tab, win[:1])
        with pytest.raises(ValueError, match="window table"):
            launch(arena, rows, tab, win.float())


def test_y16_frame_lists_and_tensor_level_refusals():
    def u8(*shape):
        return torch.zeros(shape, dtype=torch.uint8)

    def i16(*shape):
        return torch.zeros(shape, dtype=torch.int16)
    fr, fi, shapes, uniform = ops.y16_frame_lists(u8(2, 48, 64, 3), i16(2, 48, 64), (None, "y16"))
    assert shapes == [(48, 64)] * 2 and uniform == (True, True) and [tuple(f.shape) for f in fi] == [(48, 128)] * 2 and fi[0].dtype == torch.uint8
    assert ops.y16_frame_lists(u8(2, 48, 64, 3), u8(2, 48, 128), (None, "y16"))[2] == [(48, 64)] * 2
    assert ops.y16_frame_lists([i16(48, 64), u8(9, 8)], [u8(48, 128), i16(9, 4)], ("y16", "y16"))[2:] == ([(48, 64), (9, 4)], (False, False))
    if hasattr(torch, "uint16"):
        assert ops.y16_frame_lists(u8(1, 5, 7, 1), torch.zeros((1, 5, 7), dtype=torch.uint16), (None, "y16"))[2] == [(5, 7)]
    for rgb, ir, formats, match in [
            (u8(1, 48, 64, 3), i16(1, 48, 60), (None, "y16"), "same size"),
            (u8(1, 48, 64, 3), u8(1, 48, 127), (None, "y16"), "y16 frames must be 16-bit tensors"),
            (u8(1, 48, 64, 3), i16(1, 48, 64).float(), (None, "y16"), "y16 frames must be 16-bit tensors"),
            (u8(1, 48, 64, 3), i16(1, 48, 64, 1), (None, "y16"), "two batch tensors"),
            (u8(1, 48, 64, 3), i16(1, 48, 64), (None, "y12"), "formats="),
            (u8(1, 72, 64), i16(1, 48, 64), ("nv12", "y16"), "formats="),
            (u8(2, 48, 64, 3), i16(1, 48, 64), (None, "y16"), "equally long")]:
        with pytest.raises(ValueError, match=match):
            ops.y16_frame_lists(rgb, ir, formats)


def test_entry_points_are_declared_and_exported():
    """icaf_y16_window and icaf_letterbox_y16_frames: in include/icaf.h with their 72-byte row, bound from there, exported by the library."""
    assert {"icaf_y16_window", "icaf_letterbox_y16_frames"} <= set(_lib.HEADER.funcs) and "icaf_y16_geom" in _lib.HEADER.structs
    assert [p[0] for p in _lib.HEADER.funcs["icaf_y16_window"][1]] == ["arena", "geom", "nstreams", "B", "window", "s"]
    assert [p[0] for p in _lib.HEADER.funcs["icaf_letterbox_y16_frames"][1]] == ["arena", "geom", "window", "nstreams", "B", "dst", "ctot", "H", "W",
                                                                                  "swap_rb", "s"]
    assert ops.Y16_GEOM_DTYPE.itemsize == 72 and ops.Y16_GEOM_DTYPE.itemsize % 8 == 0
    assert ops.Y16_GEOM_DTYPE.names == ("g", "kind", "mode", "lo", "hi", "clip_lo", "clip_hi")
    assert [ops.Y16_GEOM_DTYPE.fields[k][1] for k in ops.Y16_GEOM_DTYPE.names] == [0, 48, 52, 56, 60, 64, 68]
    assert _lib.Y16_LDS_BYTES == 20480
    assert hasattr(_lib.lib(), "icaf_y16_window") and hasattr(_lib.lib(), "icaf_letterbox_y16_frames")
