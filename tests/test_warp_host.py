"""Calibrated RGB / IR pairs on the host: utils.datasets.warp_perspective (the rule icaf_letterbox_warp_frames reproduces byte for byte) on the
cases whose result is known in closed form and against the same rule evaluated in float64, the alignment helpers, and every refusal that needs
no device."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import REPO
from icafusion_amd import ops
from icafusion_amd.utils import datasets as D


def noise(h, w, ch, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (h, w, ch) if ch else (h, w), dtype=np.uint8)


def warp64(img, M, out_hw, border):
    """warp_perspective's rule with every operation in float64 (M still rounded to float32 once)."""
    img = img[:, :, None] if img.ndim == 2 else img
    hs, ws, _ = img.shape
    h, w = out_hw
    m = np.asarray(M, np.float64).astype(np.float32).astype(np.float64)
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        X, Y, Z = ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] for r in range(3))
        u, v = X / Z, Y / Z
        ok = (Z > 0) & (u > -1) & (u < ws) & (v > -1) & (v < hs)
    u, v = np.where(ok, u, 0.0), np.where(ok, v, 0.0)
    i0, j0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = (u - i0)[:, :, None], (v - j0)[:, :, None]
    src = img.astype(np.float64)

    def tap(j, i):
        inside = ((j >= 0) & (j < hs) & (i >= 0) & (i < ws))[:, :, None]
        return np.where(inside, src[np.clip(j, 0, hs - 1), np.clip(i, 0, ws - 1)], float(border))
    top = tap(j0, i0) * (1 - fu) + tap(j0, i0 + 1) * fu
    bot = tap(j0 + 1, i0) * (1 - fu) + tap(j0 + 1, i0 + 1) * fu
    out = np.clip(np.floor(top * (1 - fv) + bot * fv + 0.5), 0, 255).astype(np.uint8)
    return np.where(ok[:, :, None], out, np.uint8(border))


def rig(src_hw, aligned_hw, angle, scale, shift, persp):
    """aligned -> source: the stretch between the two sizes times `scale`, rotated by `angle` about the aligned centre, shifted, with
    perspective terms."""
    (hs, ws), (h0, w0) = src_hw, aligned_hw
    c, s = np.cos(angle), np.sin(angle)
    centre = np.array([[1, 0, -(w0 - 1) / 2], [0, 1, -(h0 - 1) / 2], [0, 0, 1]], np.float64)
    rot = np.array([[c, -s, 0], [s, c, 0], [persp[0], persp[1], 1]], np.float64)
    back = np.array([[scale * ws / w0, 0, (ws - 1) / 2 + shift[0]], [0, scale * hs / h0, (hs - 1) / 2 + shift[1]], [0, 0, 1]], np.float64)
    return (back @ rot @ centre).astype(np.float32)


@pytest.mark.parametrize("ch", [0, 1, 3])
def test_identity_is_exact(ch):
    img = noise(37, 53, ch, 1)
    out = D.warp_perspective(img, np.eye(3), (37, 53), border=77)
    assert out.dtype == np.uint8 and out.shape == (37, 53, max(ch, 1))
    assert np.array_equal(out, img.reshape(out.shape))


@pytest.mark.parametrize("border", [0, 114, 255])
@pytest.mark.parametrize("ch", [1, 3])
def test_integer_translation_copies_and_fills_the_band(ch, border):
    """u = x + 5, v = y - 3: aligned (y, x) is source (y - 3, x + 5) where that exists, `border` in the three uncovered rows and five
    uncovered columns."""
    img = noise(40, 50, ch, 2)
    out = D.warp_perspective(img, [[1, 0, 5], [0, 1, -3], [0, 0, 1]], (40, 50), border)
    want = np.full((40, 50, ch), border, np.uint8)
    want[3:, :45] = img[:37, 5:]
    assert np.array_equal(out, want)


def test_horizon_turns_the_far_side_into_border():
    """m20 = -0.05 on a 53-wide frame: Z = 1 - 0.05 x reaches 0 at column 20 (the float32 product decides whether 20 or 21 is the first
    column with Z <= 0); from there on, and certainly from column 21 on, every pixel is border whatever u and v come out as."""
    img = noise(37, 53, 1, 3)
    out = D.warp_perspective(img, [[1, 0, 0], [0, 1, 0], [-0.05, 0, 1]], (37, 53), border=9)
    z = np.float32(-0.05) * np.arange(53, dtype=np.float32) + np.float32(1)
    first = int(np.argmax(~(z > 0)))
    assert first in (20, 21)
    assert (out[:, 21:] == 9).all() and (out[:, first:] == 9).all()
    assert np.array_equal(out[0, 0], img[0, 0])                      # (0, 0) maps to itself: Z = 1


def test_wholly_outside_is_all_border():
    out = D.warp_perspective(noise(20, 20, 1, 4), [[1, 0, 500], [0, 1, 500], [0, 0, 1]], (48, 60), border=200)
    assert out.shape == (48, 60, 1) and (out == 200).all()


def test_non_finite_coordinates_are_border():
    out = D.warp_perspective(noise(8, 8, 1, 5), [[1, 0, 0], [0, 1, 0], [0, 0, 0]], (8, 8), border=31)      # Z = 0 everywhere: u, v inf or NaN
    assert (out == 31).all()


def test_stretch_alignment():
    assert np.array_equal(D.stretch_alignment((48, 60), (48, 60)), np.eye(3, dtype=np.float32))
    m = D.stretch_alignment((24, 30), (48, 60))
    assert m.dtype == np.float32 and np.array_equal(m, np.array([[0.5, 0, -0.25], [0, 0.5, -0.25], [0, 0, 1]], np.float32))
    with pytest.raises(ValueError, match="empty"):
        D.stretch_alignment((0, 3), (4, 4))


CASES = [((53, 37), (120, 128), 0.12, 1.0, (4.25, -3.5), (2e-4, -1e-4), 3), ((200, 260), (300, 400), -0.2, 1.3, (20, -20), (-2e-4, 2e-4), 1),
         ((150, 200), (300, 400), 0.05, 0.8, (-7.5, 11.0), (1e-4, 0), 1), ((96, 120), (48, 60), 0.2, 1.1, (0.5, 0.25), (0, -2e-4), 3),
         ((24, 30), (48, 60), -0.07, 0.9, (-20, 20), (5e-5, 5e-5), 1), ((199, 257), (255, 399), 0.17, 1.2, (13.3, 7.7), (-1e-4, -1e-4), 3)]


@pytest.mark.parametrize("border", [0, 114, 255])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_fp32_rule_is_within_one_level_of_the_fp64_rule(case, border):
    """Rotations up to +-0.2 rad, 0.8 - 1.3 x the size ratio, shifts up to +-20 px, perspective terms up to +-2e-4, noise sources of 1 and 3
    channels up to 200 x 260 under aligned frames up to 300 x 400: every pixel within one grey level, no exclusions (the blend is
    continuous across integer coordinates and across the frame edge)."""
    src_hw, aligned_hw, angle, scale, shift, persp, ch = CASES[case]
    img = noise(*src_hw, ch, 10 + case)
    M = rig(src_hw, aligned_hw, angle, scale, shift, persp)
    got, want = D.warp_perspective(img, M, aligned_hw, border), warp64(img, M, aligned_hw, border)
    assert got.shape == want.shape == aligned_hw + (ch,)
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"case {case} border {border}: max |fp32 - fp64| = {diff.max()}, differing pixels {np.count_nonzero(diff) / diff.size:.5f}")
    assert diff.max() <= 1
    assert (got != border).any()                                      # the source is in view: the case compares blends, not a constant


def test_warp_perspective_refusals():
    img = noise(8, 8, 1, 6)
    for bad, kw, msg in ((img.astype(np.float32), {}, "uint8"), (img, {"M": np.eye(2)}, "3 x 3"), (img, {"border": 256}, "border")):
        with pytest.raises(ValueError, match=msg):
            D.warp_perspective(bad, kw.get("M", np.eye(3)), (8, 8), kw.get("border", 0))


def test_load_alignment(tmp_path):
    m = rig((53, 37), (120, 128), 0.1, 1.0, (2, 3), (1e-4, 0)).astype(np.float64)
    txt, csv, npy = tmp_path / "a.txt", tmp_path / "a.csv", tmp_path / "a.npy"
    txt.write_text("\n".join(" ".join(repr(float(v)) for v in row) for row in m))
    csv.write_text(",\n".join(", ".join(repr(float(v)) for v in row) for row in m))
    np.save(npy, m)
    for p in (txt, csv, npy):
        got = D.load_alignment(str(p))
        assert got.dtype == np.float32 and got.shape == (3, 3) and np.array_equal(got, m.astype(np.float32)), p
    inv = D.load_alignment(str(npy), inverse=True)
    assert np.allclose(inv.astype(np.float64) @ m, np.eye(3), atol=1e-4)
    (tmp_path / "eight.txt").write_text("1 0 0 0 1 0 0 0")
    (tmp_path / "nan.txt").write_text("1 0 0 0 1 0 0 0 nan")
    (tmp_path / "singular.txt").write_text("1 2 3 2 4 6 0 0 1")
    with pytest.raises(ValueError, match="nine"):
        D.load_alignment(str(tmp_path / "eight.txt"))
    with pytest.raises(ValueError, match="non-finite"):
        D.load_alignment(str(tmp_path / "nan.txt"))
    with pytest.raises(ValueError, match="singular"):
        D.load_alignment(str(tmp_path / "singular.txt"), inverse=True)
    assert D.load_alignment(str(tmp_path / "singular.txt")).shape == (3, 3)      # only the inversion needs a regular matrix


def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_frame_lists_names_align():
    with pytest.raises(ValueError, match="align="):
        ops.frame_lists(u8(2, 48, 60, 3), u8(2, 24, 30, 1))


def test_warp_frame_lists():
    rgb, ir = u8(2, 48, 60, 3), [u8(24, 30, 1), u8(20, 31, 1)]
    fr, fi, shapes, uniform, m, src, mats = ops.warp_frame_lists(rgb, ir, (None, "stretch"))
    assert (len(fr), len(fi), shapes, uniform, m, src) == (2, 2, [(48, 60), (48, 60)], (True, False), 1, [(24, 30), (20, 31)])
    assert mats.dtype == np.float32 and mats.shape == (2, 3, 3) and np.array_equal(mats[1], D.stretch_alignment((20, 31), (48, 60)))
    one = np.array([[1, 0, 2], [0, 1, 3], [0, 0, 1]], np.float64)
    *_, m, src, mats = ops.warp_frame_lists(ir, rgb, (one, None))                      # the visible modality aligned onto the thermal one
    assert m == 0 and src == [(24, 30), (20, 31)] and np.array_equal(mats, np.stack([one, one]).astype(np.float32))
    *_, mats = ops.warp_frame_lists(rgb, ir, (None, torch.from_numpy(np.stack([one, 2 * one]))))
    assert np.array_equal(mats[1], (2 * one).astype(np.float32))
    bad = one.copy()
    bad[1, 1] = np.inf
    for align, msg in (((one, one), "both"), ((None, None), "neither"), (one, "one entry per modality"), ((None, np.eye(4)), r"\(3, 3\)"),
                       ((None, np.zeros((3, 3, 3))), r"\(3, 3\)"), ((None, bad), "non-finite"), ((None, "shear"), "stretch")):
        with pytest.raises(ValueError, match=msg):
            ops.warp_frame_lists(rgb, ir, align)
    with pytest.raises(ValueError, match="equally long"):
        ops.warp_frame_lists(rgb, ir[:1], (None, one))
    with pytest.raises(ValueError, match="uint8"):
        ops.warp_frame_lists(rgb, [t.float() for t in ir], (None, one))


def table(border=0, matrix=None):
    """Two rows to a 64 x 64 output: a plain 48 x 60 x 3 frame and a 24 x 30 grey source aligned onto it."""
    geom1, _ = ops.frame_geometry([(48, 60)], 64)
    return ops.pack_warp_frames(np.concatenate((geom1, geom1)), [3, (24, 30, 1)], [None, np.eye(3) if matrix is None else matrix], border)


def test_pack_and_validate_warp_frames():
    rows, end = table(border=114)
    assert rows.dtype == ops.WARP_GEOM_DTYPE and ops.WARP_GEOM_DTYPE.itemsize == 104
    assert rows["kind"].tolist() == [0, 1] and rows["border"].tolist() == [0, 114] and (rows[1]["hs"], rows[1]["ws"]) == (24, 30)
    assert rows["g"]["offset"].tolist() == [0, -(-48 * 180 // ops.FRAME_ALIGN) * ops.FRAME_ALIGN] and end == int(rows[1]["g"]["offset"]) + 24 * 30
    assert (rows[1]["g"]["h0"], rows[1]["g"]["w0"], rows[1]["g"]["pitch"], rows[1]["g"]["ch"]) == (48, 60, 30, 1)
    assert np.array_equal(rows[1]["m"], np.eye(3, dtype=np.float32).reshape(9))
    ops.validate_warp_frames(rows, end, 64, 64)
    geom1, _ = ops.frame_geometry([(48, 60)], 64)
    for sources, mats, msg in (([(24, 30, 1)], [None], "needs its 3 x 3 matrix"), ([3], [np.eye(3)], "unwarped"), ([(24, 30)], [np.eye(3)], "source is"),
                               ([(24, 30, 1)], [np.eye(4)], "3 x 3")):
        with pytest.raises(ValueError, match=msg):
            ops.pack_warp_frames(geom1, sources, mats)

    def broken(**kw):
        r = rows.copy()
        for k, v in kw.items():
            if k in ("offset", "pitch", "ch", "nh", "top", "sx"):
                r["g"][k][1] = v
            elif k == "m0":
                r["m"][1, 0] = v
            else:
                r[k][1] = v
        return r
    for kw, nbytes, msg in (({"kind": 2}, end, "kind 2"), ({"hs": 0}, end, "empty source"), ({"pitch": 29}, end, "pitch 29"), ({"ch": 2}, end, "channels"),
                            ({"offset": int(rows[1]["g"]["offset"]) + 8}, end + 64, "multiple of 16"), ({}, end - 1, "leave the arena"),
                            ({"border": 256}, end, "border 256"), ({"m0": np.nan}, end, "non-finite"), ({"top": 40}, end, "leaves the 64x64 output"),
                            ({"sx": 0.0}, end, "positive")):
        with pytest.raises(ValueError, match=msg):
            ops.validate_warp_frames(broken(**kw), nbytes, 64, 64)
    plain = rows.copy()
    plain["g"]["pitch"][0] = 10
    with pytest.raises(ValueError, match="frame 0: pitch 10"):
        ops.validate_warp_frames(plain, end, 64, 64)


def test_letterbox_warp_frames_refuses_before_any_device_call():
    rows, end = table()
    arena, dst, tab = u8(end), u8(1, 6, 64, 64), ops.geom_tensor(rows)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.letterbox_warp_frames(arena, rows, tab, dst)
    with pytest.raises(ValueError, match="WARP_GEOM_DTYPE"):
        ops.letterbox_warp_frames(arena, rows["g"].copy(), tab, dst)
    with pytest.raises(ValueError, match="smaller than the descriptor rows"):
        ops.letterbox_warp_frames(arena, rows, tab[:100], dst)
    with pytest.raises(ValueError, match="leave the arena"):
        ops.letterbox_warp_frames(arena[:-1], rows, tab, dst)


def test_detect_twostream_takes_the_alignment_flags():
    sys.path.insert(0, REPO)
    import detect_twostream as dt
    opt = dt.parse_opt(["--source1", "a", "--source2", "b"])
    assert opt.align_ir is None and opt.align_inverse is False and opt.align_border == 0
    opt = dt.parse_opt(["--source1", "a", "--source2", "b", "--align-ir", os.path.join("rig", "h.txt"), "--align-inverse", "--align-border", "114",
                        "--device-letterbox"])
    assert opt.align_ir == os.path.join("rig", "h.txt") and opt.align_inverse is True and opt.align_border == 114 and opt.device_letterbox
    assert dt.parse_opt(["--source1", "a", "--source2", "b", "--align-ir", "stretch"]).align_ir == "stretch"
