"""Image loading for the two-stream front ends, without OpenCV (cv2 is not in this image).

Same entry points and return conventions as the reference's utils/datasets.py for the inference / validation paths:
`letterbox` (:1404-1444 — note the reference's `auto` / `scaleFill` branches are commented out, so every image is padded
to the full `new_shape`), `LoadImages` (:172-241, image files only) and the paired RGB+IR validation set that yields the
6-channel uint8 batches `test.py:115-123` consumes, following LoadMultiModalImagesAndLabels' evaluation protocol
(:690-1024): longest side resized to `img_size` (:1116-1122), RECTANGULAR batches — images sorted by aspect ratio, one
letterbox shape per batch, `ceil(shape * img_size / stride + pad) * stride` (:826-849; test.py:100 passes rect=True,
pad=0.5, which makes KAIST's 512x640 frames 544x672 batches) — `scaleup=False`, labels re-normalised to the letterboxed
image (:961-986), label files found by replacing the `visible` / `infrared` path component with `labels` (:391-401).
Not carried over: augmentation / mosaic (training), the label cache file, image caching.

Decoding goes through PIL.  Up-sampling is a half-pixel-centre bilinear filter evaluated in float32 and rounded to nearest
(cv2.INTER_LINEAR's geometry; OpenCV evaluates it in 11-bit fixed point, so results can differ by one grey level);
down-sampling is the exact pixel-area average (cv2.INTER_AREA's definition, float32).  Arrays are BGR HWC uint8 like
cv2.imread's, so downstream code is unchanged."""
import glob
import os
from pathlib import Path

import numpy as np
import torch

IMG_FORMATS = ("bmp", "jpg", "jpeg", "png", "tif", "tiff", "dng", "webp", "mpo")


def imread_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def imwrite_bgr(path, img):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(img[:, :, ::-1])).save(path)


def resize_bilinear(img, new_wh):
    """(H, W, C) uint8 -> (new_h, new_w, C) uint8, bilinear with half-pixel centres and edge clamping."""
    h, w = img.shape[:2]
    nw, nh = new_wh
    if (nw, nh) == (w, h):
        return img

    def taps(n_in, n_out):
        src = (np.arange(n_out, dtype=np.float32) + 0.5) * (n_in / n_out) - 0.5
        i0 = np.floor(src).astype(np.int64)
        frac = (src - i0).astype(np.float32)
        return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), frac
    y0, y1, fy = taps(h, nh)
    x0, x1, fx = taps(w, nw)
    f = img.astype(np.float32)
    top = f[y0][:, x0] * (1 - fx)[None, :, None] + f[y0][:, x1] * fx[None, :, None]
    bot = f[y1][:, x0] * (1 - fx)[None, :, None] + f[y1][:, x1] * fx[None, :, None]
    out = top * (1 - fy)[:, None, None] + bot * fy[:, None, None]
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


def resize_area(img, new_wh):
    """(H, W, C) uint8 -> (new_h, new_w, C) uint8 by pixel-area averaging (the definition of cv2.INTER_AREA for
    down-scaling, which load_image_rgb_ir uses when r < 1: utils/datasets.py:1119-1122): output pixel j covers the input
    interval [j * s, (j + 1) * s), s = n_in / n_out, and averages the input pixels weighted by their overlap with it."""
    h, w = img.shape[:2]
    nw, nh = new_wh
    if (nw, nh) == (w, h):
        return img

    def weights(n_in, n_out):
        s = n_in / n_out
        lo = np.arange(n_out, dtype=np.float64) * s
        hi = lo + s
        px = np.arange(n_in, dtype=np.float64)
        ov = np.clip(np.minimum(hi[:, None], px[None] + 1.0) - np.maximum(lo[:, None], px[None]), 0.0, None)
        return (ov / s).astype(np.float32)                       # (n_out, n_in), rows sum to 1
    wy, wx = weights(h, nh), weights(w, nw)
    f = img.astype(np.float32)
    out = np.einsum("oh,hwc->owc", wy, f, optimize=True)
    out = np.einsum("pw,owc->opc", wx, out, optimize=True)
    return np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)


def resize_area_scalar(img, new_wh):
    """resize_area with the order of every operation fixed, so that a kernel can reproduce it bit for bit (icaf_resize_frames, mode 1).
    Weights exactly as resize_area.weights (float64 overlap over s, rounded to float32).  Vertical pass first: v[o][x][c] = sum over h of
    w_y[o][h] * f[h][x][c], taps in ascending h, float32 accumulator from 0, each product rounded to float32 and then added (no FMA);
    then the horizontal pass over the float32 v in ascending x by the same rule; floor(out + 0.5) clipped to 0..255.  Zero-weight taps
    add +0 to a non-negative sum and change nothing, so only the (int)s + 2 pixels from floor(j s) on are visited.  Equal to resize_area
    except where the exact average is a tie k + 0.5 (within 1e-4): there BLAS' undefined summation order and this one can fall on
    different sides, one grey level apart (tests/test_val_frames_host.py)."""
    h, w = img.shape[:2]
    nw, nh = new_wh
    if (nw, nh) == (w, h):
        return img

    def taps(n_in, n_out):
        s = n_in / n_out
        lo = np.arange(n_out, dtype=np.float64) * s
        hi = lo + s
        px = lo.astype(np.int64)[:, None] + np.arange(int(s) + 2, dtype=np.int64)[None]            # (n_out, taps), ascending
        ov = np.clip(np.minimum(hi[:, None], px + 1.0) - np.maximum(lo[:, None], px.astype(np.float64)), 0.0, None)
        wgt = np.where(px < n_in, (ov / s).astype(np.float32), np.float32(0))
        return np.minimum(px, n_in - 1), wgt.astype(np.float32)

    def one_pass(f, idx, wgt):                                                                     # along axis 0 of f
        acc = np.zeros((idx.shape[0],) + f.shape[1:], np.float32)
        for t in range(idx.shape[1]):                                                              # tap t of every output at once
            acc = acc + wgt[:, t].reshape((-1,) + (1,) * (f.ndim - 1)) * f[idx[:, t]]
        return acc
    f = img.astype(np.float32)
    v = one_pass(f, *taps(h, nh))
    out = one_pass(np.ascontiguousarray(v.swapaxes(0, 1)), *taps(w, nw)).swapaxes(0, 1)
    return np.clip(np.floor(out + np.float32(0.5)), 0, 255).astype(np.uint8)


def letterbox_geometry(shape, new_shape=(640, 640), scaleup=True):
    """THE numbers of the letterbox (reference utils/datasets.py:1404-1444) for a native (h0, w0): r, new_unpad = (nw, nh), the
    per-side paddings (dw, dh) and the integer split (top, bottom, left, right) of an odd pad, round(d -+ 0.1).  `letterbox` below and
    the device letterbox's descriptors (icafusion_amd.ops.frame_geometry) both take them from here."""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:
        r = min(r, 1.0)
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = (new_shape[1] - new_unpad[0]) / 2, (new_shape[0] - new_unpad[1]) / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return r, new_unpad, (dw, dh), (top, bottom, left, right)


def letterbox(img, new_shape=(640, 640), color=(114, 114, 114), auto=True, scaleFill=False, scaleup=True, stride=32):
    """Resize keeping the aspect ratio, then pad to `new_shape` with `color` (reference utils/datasets.py:1404-1444).
    `auto` / `scaleFill` / `stride` are accepted and — exactly as in the reference, whose branches for them are
    commented out — have no effect.  Returns (image, (ratio_w, ratio_h), (pad_w, pad_h)) with per-side paddings."""
    shape = img.shape[:2]
    r, new_unpad, (dw, dh), (top, bottom, left, right) = letterbox_geometry(shape, new_shape, scaleup)
    if shape[::-1] != new_unpad:
        img = resize_bilinear(img, new_unpad)
    out = np.empty((img.shape[0] + top + bottom, img.shape[1] + left + right, img.shape[2]), np.uint8)
    out[...] = np.asarray(color, np.uint8)
    out[top:top + img.shape[0], left:left + img.shape[1]] = img
    return out, (r, r), (dw, dh)


YUV_LAYOUTS = ("nv12", "nv21", "i420", "yv12")


def yuv420_planes(buf, h0, w0, layout):
    """The planes of one YUV 4:2:0 frame as a decoder hands it over — `buf`: uint8, h0 * w0 luma bytes followed by the chroma of
    ceil(h0 / 2) x ceil(w0 / 2) samples, interleaved CbCr (nv12) / CrCb (nv21) or as two planes Cb, Cr (i420) / Cr, Cb (yv12); for even
    sizes that is the (3 * h0 // 2, w0) array every decoder binding returns.  Returns views (y, cb, cr)."""
    if layout not in YUV_LAYOUTS:
        raise ValueError(f"unknown YUV 4:2:0 layout {layout!r} (one of {', '.join(YUV_LAYOUTS)})")
    ch, cw = (h0 + 1) // 2, (w0 + 1) // 2
    flat = np.asarray(buf).reshape(-1)
    if flat.dtype != np.uint8 or flat.size != h0 * w0 + 2 * ch * cw:
        raise ValueError(f"a {h0}x{w0} {layout} frame is {h0 * w0 + 2 * ch * cw} uint8 bytes, got {flat.size} of {flat.dtype}")
    y, c = flat[:h0 * w0].reshape(h0, w0), flat[h0 * w0:]
    if layout in ("nv12", "nv21"):
        c = c.reshape(ch, cw, 2)
        first, second = c[:, :, 0], c[:, :, 1]
    else:
        first, second = c[:ch * cw].reshape(ch, cw), c[ch * cw:].reshape(ch, cw)
    return (y, first, second) if layout in ("nv12", "i420") else (y, second, first)


def yuv420_to_bgr(y, cb, cr, matrix=0):
    """THE colour conversion of native YUV 4:2:0 frames (icaf_letterbox_yuv_frames equals letterbox() of this image byte for byte): y
    (h0, w0) uint8, cb / cr (ceil(h0 / 2), ceil(w0 / 2)) uint8 -> (h0, w0, 3) uint8 BGR.  Pixel (i, j) takes chroma sample (i >> 1,
    j >> 1): nearest replication, no chroma filtering.  32-bit integer arithmetic, `>>` flooring, results clamped to 0..255; with
    c = Y - 16, d = Cb - 128, e = Cr - 128:
      matrix 0, BT.601 limited range:      R = (298c + 409e + 128) >> 8, G = (298c - 100d - 208e + 128) >> 8, B = (298c + 516d + 128) >> 8
      matrix 1, BT.709 limited range:      R = (298c + 459e + 128) >> 8, G = (298c - 55d - 136e + 128) >> 8,  B = (298c + 541d + 128) >> 8
      matrix 2, BT.601 full range (JFIF):  R = Y + ((91881e + 32768) >> 16), G = Y + ((-22554d - 46802e + 32768) >> 16),
                                           B = Y + ((116130d + 32768) >> 16)"""
    y, cb, cr = (np.asarray(a) for a in (y, cb, cr))
    h0, w0 = y.shape
    if any(a.dtype != np.uint8 for a in (y, cb, cr)) or cb.shape != ((h0 + 1) // 2, (w0 + 1) // 2) or cr.shape != cb.shape:
        raise ValueError(f"a {h0}x{w0} luma plane takes uint8 chroma planes of {(h0 + 1) // 2}x{(w0 + 1) // 2}, got {cb.shape} / {cr.shape}")
    if matrix not in (0, 1, 2):
        raise ValueError(f"unknown YUV matrix {matrix!r} (0 = BT.601, 1 = BT.709, 2 = BT.601 full range)")
    rows, cols = np.arange(h0) >> 1, np.arange(w0) >> 1
    Y = y.astype(np.int32)
    d = cb.astype(np.int32)[rows][:, cols] - 128
    e = cr.astype(np.int32)[rows][:, cols] - 128
    if matrix == 2:
        r = Y + ((91881 * e + 32768) >> 16)
        g = Y + ((-22554 * d - 46802 * e + 32768) >> 16)
        b = Y + ((116130 * d + 32768) >> 16)
    else:
        c = 298 * (Y - 16) + 128
        rv, gu, gv, bu = (409, -100, -208, 516) if matrix == 0 else (459, -55, -136, 541)
        r, g, b = (c + rv * e) >> 8, (c + gu * d + gv * e) >> 8, (c + bu * d) >> 8
    return np.clip(np.stack((b, g, r), axis=2), 0, 255).astype(np.uint8)


AGC_CLIP = (100, 100)        # basis points clipped at the low / high end of a 16-bit thermal frame's histogram: 1 % each


def _u16_frame(frame):
    f = np.asarray(frame)
    if f.dtype == np.int16:                       # torch has no uint16 on older releases: the same bits
        f = f.view(np.uint16)
    if f.dtype != np.uint16 or f.ndim != 2 or f.size == 0:
        raise ValueError(f"a 16-bit thermal frame is a non-empty (h0, w0) uint16 array, got {f.dtype} {f.shape}")
    return f


def agc_clip(clip):
    """(clip_lo, clip_hi) as two ints in basis points, each 0..4999; ValueError names the limit."""
    try:
        lo, hi = clip
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= v <= 4999 for v in (lo, hi))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"the gain-control clip is (clip_lo, clip_hi) in basis points, integers in 0..4999 each, got {clip!r}")
    return int(lo), int(hi)


def agc_window(frame, clip=AGC_CLIP):
    """THE gain-control window of a 16-bit thermal frame (icaf_y16_window equals it): (lo, hi) with n = h0 * w0, C(v) = pixels <= v,
    D(v) = pixels >= v, lo the smallest v with 10000 * C(v) > clip_lo * n and hi the largest v with 10000 * D(v) > clip_hi * n.  Integers
    only, 64-bit products, both inequalities strict; clip in basis points, 0..4999 each; (0, 0) gives the frame's minimum and maximum."""
    f = _u16_frame(frame)
    clip_lo, clip_hi = agc_clip(clip)
    n = f.size
    hist = np.bincount(f.reshape(-1), minlength=65536).astype(np.int64)
    c = np.cumsum(hist)                           # C(v)
    d = n - c + hist                              # D(v)
    lo = int(np.argmax(10000 * c > clip_lo * n))
    hi = 65535 - int(np.argmax((10000 * d > clip_hi * n)[::-1]))
    return lo, hi


def agc_u16_to_u8(frame, lo, hi):
    """THE 16-to-8-bit mapping of a thermal frame (icaf_letterbox_y16_frames equals letterbox() of this image byte for byte): d =
    max(hi - lo, 1), out(v) = min(255, ((max(v, lo) - lo) * 255 + (d >> 1)) // d).  Integers only, no special cases: v <= lo gives 0,
    v >= hi gives 255 when hi > lo, a flat frame maps to 0."""
    f = _u16_frame(frame)
    lo, hi = int(lo), int(hi)
    if not 0 <= lo <= hi <= 65535:
        raise ValueError(f"a gain-control window is 0 <= lo <= hi <= 65535, got ({lo}, {hi})")
    d = max(hi - lo, 1)
    x = (np.maximum(f.astype(np.int64), lo) - lo) * 255 + (d >> 1)
    return np.minimum(x // d, 255).astype(np.uint8)


def imread_u16(path):
    """A 16-bit single-channel PNG or TIFF (raw thermal counts) as an (h0, w0) uint16 array."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("I;16", "I;16L", "I;16B", "I;16N"):
            raise ValueError(f"{path}: expected a 16-bit greyscale image (mode I;16), got mode {im.mode}")
        return np.ascontiguousarray(np.asarray(im).astype(np.uint16))


def warp_perspective(img, M, out_hw, border=0):
    """THE registration of a calibrated RGB / IR pair (icaf_letterbox_warp_frames equals letterbox() of this image byte for byte): img
    (hs, ws) or (hs, ws, ch) uint8 -> (h, w, ch) uint8, the source frame seen through the homography M.  M (3 x 3, rounded to float32
    once) maps ALIGNED pixel coordinates to SOURCE pixel coordinates — x right, y down, an integer is a pixel centre: the matrix
    cv2.warpPerspective takes with WARP_INVERSE_MAP, the inverse of findHomography(src_pts, aligned_pts).  All float32, every operation
    rounded on its own, for aligned pixel (x, y):
      X = (m00 x + m01 y) + m02, Y = (m10 x + m11 y) + m12, Z = (m20 x + m21 y) + m22, u = X / Z, v = Y / Z (IEEE divisions);
      ok = Z > 0 and -1 < u < ws and -1 < v < hs (false on NaN: the far side of a horizon is not ok); not ok: `border` in every channel;
      i0 = floor(u), fu = u - i0, j0 / fv likewise from v; a tap (j, i) inside the frame is its byte, outside it `border` (constant
      border, no clamping); top = a00 (1 - fu) + a01 fu, bot likewise, out = top (1 - fv) + bot fv, result floor(out + 0.5) clipped to 0..255."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError(f"warp_perspective takes a uint8 (hs, ws) or (hs, ws, ch) frame, got {img.dtype} {img.shape}")
    if img.ndim == 2:
        img = img[:, :, None]
    hs, ws, ch = img.shape
    h, w = int(out_hw[0]), int(out_hw[1])
    border = int(border)
    if hs < 1 or ws < 1 or h < 1 or w < 1 or not 0 <= border <= 255:
        raise ValueError(f"warp_perspective: empty frame ({hs}x{ws} -> {h}x{w}) or border {border} outside 0..255")
    m = np.asarray(M, np.float64).astype(np.float32)
    if m.shape != (3, 3):
        raise ValueError(f"warp_perspective takes a 3 x 3 matrix, got shape {m.shape}")
    f32 = np.float32
    x, y = np.arange(w, dtype=f32)[None, :], np.arange(h, dtype=f32)[:, None]
    with np.errstate(all="ignore"):
        X = (m[0, 0] * x + m[0, 1] * y) + m[0, 2]
        Y = (m[1, 0] * x + m[1, 1] * y) + m[1, 2]
        Z = (m[2, 0] * x + m[2, 1] * y) + m[2, 2]
        u, v = X / Z, Y / Z
        ok = (Z > 0) & (u > f32(-1)) & (u < f32(ws)) & (v > f32(-1)) & (v < f32(hs))
    u, v = np.where(ok, u, f32(0)), np.where(ok, v, f32(0))
    fi, fj = np.floor(u), np.floor(v)
    fu, fv = (u - fi)[:, :, None], (v - fj)[:, :, None]
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    src = img.astype(f32)

    def tap(j, i):
        inside = ((j >= 0) & (j < hs) & (i >= 0) & (i < ws))[:, :, None]
        return np.where(inside, src[np.clip(j, 0, hs - 1), np.clip(i, 0, ws - 1)], f32(border))
    top = tap(j0, i0) * (f32(1) - fu) + tap(j0, i0 + 1) * fu
    bot = tap(j0 + 1, i0) * (f32(1) - fu) + tap(j0 + 1, i0 + 1) * fu
    out = top * (f32(1) - fv) + bot * fv
    out = np.clip(np.floor(out + f32(0.5)), 0, 255).astype(np.uint8)
    return np.where(ok[:, :, None], out, np.uint8(border))


def stretch_alignment(src_hw, aligned_hw):
    """The alignment matrix of "same field of view, other resolution" (half-pixel centres): a (hs, ws) source under an (h0, w0) aligned
    frame, u = (x + 0.5) ws / w0 - 0.5 and v likewise, computed in float64 and rounded to float32.  Equal sizes give the identity."""
    (hs, ws), (h0, w0) = (int(v) for v in src_hw), (int(v) for v in aligned_hw)
    if min(hs, ws, h0, w0) < 1:
        raise ValueError(f"stretch_alignment: empty size {hs}x{ws} / {h0}x{w0}")
    return np.array([[ws / w0, 0.0, 0.5 * ws / w0 - 0.5], [0.0, hs / h0, 0.5 * hs / h0 - 0.5], [0.0, 0.0, 1.0]], np.float64).astype(np.float32)


def load_alignment(path, inverse=False):
    """A rig's 3 x 3 alignment matrix from a .npy file or a text file of nine numbers separated by white space and / or commas, as
    float32.  The file holds the ALIGNED -> SOURCE matrix warp_perspective takes; inverse=True: it holds SOURCE -> aligned
    (findHomography(src_pts, aligned_pts)) and is inverted in float64 first.  ValueError for a wrong count, a non-finite entry and,
    under inverse, a singular matrix."""
    path = str(path)
    if path.endswith(".npy"):
        a = np.asarray(np.load(path, allow_pickle=False), np.float64).reshape(-1)
    else:
        with open(path) as f:
            words = f.read().replace(",", " ").split()
        try:
            a = np.array([float(t) for t in words], np.float64)
        except ValueError:
            raise ValueError(f"{path}: an alignment file holds nine numbers, got {words[:12]!r}") from None
    if a.size != 9:
        raise ValueError(f"{path}: an alignment matrix has nine entries, got {a.size}")
    if not np.isfinite(a).all():
        raise ValueError(f"{path}: the alignment matrix has a non-finite entry")
    a = a.reshape(3, 3)
    if inverse:
        if not abs(np.linalg.det(a)) > 0 or not np.isfinite(np.linalg.cond(a)) or np.linalg.cond(a) > 1e15:
            raise ValueError(f"{path}: the matrix is singular and has no inverse (--align-inverse / inverse=True)")
        a = np.linalg.inv(a)
        if not np.isfinite(a).all():
            raise ValueError(f"{path}: the matrix is singular and has no inverse (--align-inverse / inverse=True)")
    return a.astype(np.float32)


def _list_images(path):
    p = str(Path(path).absolute())
    if "*" in p:
        files = sorted(glob.glob(p, recursive=True))
    elif os.path.isdir(p):
        files = sorted(glob.glob(os.path.join(p, "*.*")))
    elif os.path.isfile(p):
        files = [p]
    else:
        raise FileNotFoundError(f"{p} does not exist")
    return [f for f in files if f.rsplit(".", 1)[-1].lower() in IMG_FORMATS]


class LoadImages:
    """Iterate the image files of a folder / glob / single path: yields (path, CHW RGB uint8 letterboxed, BGR original,
    None) like the reference's LoadImages.__next__ (utils/datasets.py:205-241).  Video files are out of scope.
    native=True: no host letterbox — the second item is None and the consumer letterboxes the BGR original on the device
    (Model.forward_frames).  raw16=True: the files are 16-bit greyscale PNG / TIFF (raw thermal counts, imread_u16): the third item
    is the (h0, w0) uint16 original, the second None — the consumer picks the gain-control window (agc_window / agc_u16_to_u8 on the
    host, or Model.forward_frames(formats=(None, "y16")) on the device)."""

    def __init__(self, path, img_size=640, stride=32, native=False, raw16=False):
        self.native = bool(native)
        self.raw16 = bool(raw16)
        self.files = _list_images(path)
        self.nf = len(self.files)
        self.img_size, self.stride, self.mode, self.cap = img_size, stride, "image", None
        if self.nf == 0:
            raise FileNotFoundError(f"no images found in {path} (supported: {IMG_FORMATS})")

    def __iter__(self):
        self.count = 0
        return self

    def __len__(self):
        return self.nf

    def __next__(self):
        if self.count == self.nf:
            raise StopIteration
        path = self.files[self.count]
        self.count += 1
        if self.raw16:
            return path, None, imread_u16(path), self.cap
        img0 = imread_bgr(path)
        if self.native:
            return path, None, img0, self.cap
        img = letterbox(img0, self.img_size, stride=self.stride)[0]
        img = np.ascontiguousarray(img[:, :, ::-1].transpose(2, 0, 1))
        return path, img, img0, self.cap


def img2label_paths(img_paths):
    """.../visible/<split>/x.jpg or .../infrared/<split>/x.jpg -> .../labels/<split>/x.txt: the first `visible` (else
    `infrared`) in the path becomes `labels`, the extension `txt` (reference utils/datasets.py:391-401).  The shipped
    data/multispectral/*.yaml files use exactly this layout."""
    out = []
    for x in img_paths:
        parts = x.split("/")
        if "visible" in parts:
            sa = "visible"
        elif "infrared" in parts:
            sa = "infrared"
        else:
            raise ValueError(f"{x}: paired datasets keep images under a 'visible' or 'infrared' directory and labels under "
                             "'labels' (reference utils/datasets.py:391-401)")
        out.append("txt".join(x.replace(sa, "labels", 1).rsplit(x.split(".")[-1], 1)))
    return out


def _image_files(path):
    """Directory (recursive), glob, or a text file listing image paths ('./' = relative to the list) — :709-722."""
    if isinstance(path, (list, tuple)):
        return sorted(f for p in path for f in _image_files(p))
    p = Path(path)
    if p.is_dir():
        files = glob.glob(str(p / "**" / "*.*"), recursive=True)
    elif p.is_file() and p.suffix.lower()[1:] not in IMG_FORMATS:
        parent = str(p.parent) + os.sep
        with open(p) as f:
            files = [ln.replace("./", parent) if ln.startswith("./") else ln for ln in f.read().strip().splitlines()]
    else:
        return _list_images(path)
    return sorted(f for f in files if f.rsplit(".", 1)[-1].lower() in IMG_FORMATS)


def _read_labels(path):
    if not os.path.isfile(path):
        return None
    with open(path) as f:
        rows = [ln.split() for ln in f.read().strip().splitlines() if ln.strip()]
    lab = np.array(rows, np.float32).reshape(-1, 5) if rows else np.zeros((0, 5), np.float32)
    if len(lab) and ((lab < 0).any() or (lab[:, 1:] > 1).any()):
        raise ValueError(f"{path}: labels must be non-negative, normalised [cls cx cy w h] rows (reference :1049-1052)")
    return lab


class PairedValSet:
    """RGB + IR validation pairs with YOLO txt labels.  `__getitem__` -> (6xHxW uint8 tensor = cat(rgb, ir) as
    utils/datasets.py:1022-1024, labels (n, 6) [0, cls, cx, cy, w, h] normalised to the letterboxed image, rgb path,
    ((h0, w0), ((h / h0, w / w0), (pad_w, pad_h))) for scale_coords).  native=True: no host resize — the first item is (rgb BGR frame, ir BGR
    frame, (H, W) letterbox shape of the batch) as decoded, everything else is the same; collate_fn then yields (rgb list, ir list, (H, W))."""

    def __init__(self, path_rgb, path_ir, img_size=640, batch_size=16, rect=False, pad=0.0, stride=32, single_cls=False,
                 label_paths=None, native=False):
        self.native = bool(native)
        self.rgb, self.ir = _image_files(path_rgb), _image_files(path_ir)
        if not self.rgb or len(self.rgb) != len(self.ir):
            raise FileNotFoundError(f"{len(self.rgb)} RGB images under {path_rgb} vs {len(self.ir)} IR images under {path_ir}")
        self.img_size, self.rect, self.stride = img_size, bool(rect), stride
        self.label_files = list(label_paths) if label_paths is not None else img2label_paths(self.rgb)
        labels = [_read_labels(f) for f in self.label_files]
        self.n_missing = sum(l is None for l in labels)
        if self.n_missing == len(labels):
            # the reference prints "No labels found" and asserts (:781) unless augmenting: validation without a single label
            # file means the paths are wrong, and every metric would silently come out as zero
            raise FileNotFoundError(f"no label file found for any of {len(labels)} images, e.g. {self.label_files[0]}")
        self.labels = [np.zeros((0, 5), np.float32) if l is None else l for l in labels]
        if single_cls:
            for l in self.labels:
                l[:, 0] = 0
        n = len(self.rgb)
        self.batch = np.floor(np.arange(n) / batch_size).astype(np.int64)      # batch index of each image (:800-803)
        self.batch_shapes = None
        if self.rect:
            from PIL import Image
            shapes = []
            for f in self.rgb:
                with Image.open(f) as im:
                    shapes.append(im.size)                                    # (w, h), header only
            s = np.array(shapes, dtype=np.float64)
            ar = s[:, 1] / s[:, 0]                                            # aspect ratio h / w
            order = ar.argsort()
            self.rgb = [self.rgb[i] for i in order]
            self.ir = [self.ir[i] for i in order]                             # pairs share their shape (:851-859 sorts IR by its own)
            self.label_files = [self.label_files[i] for i in order]
            self.labels = [self.labels[i] for i in order]
            ar = ar[order]
            nb = int(self.batch[-1]) + 1
            bshapes = [[1.0, 1.0]] * nb
            for i in range(nb):
                ari = ar[self.batch == i]
                mini, maxi = ari.min(), ari.max()
                if maxi < 1:
                    bshapes[i] = [maxi, 1.0]
                elif mini > 1:
                    bshapes[i] = [1.0, 1.0 / mini]
            self.batch_shapes = np.ceil(np.array(bshapes) * img_size / stride + pad).astype(np.int64) * stride     # (h, w)

    def __len__(self):
        return len(self.rgb)

    def val_size(self, h0, w0):
        """(h, w) after load_image_rgb_ir's first step (:1116-1122): longest side -> img_size, int() truncation; and r."""
        r = self.img_size / max(h0, w0)
        return ((int(h0 * r), int(w0 * r)) if r != 1 else (h0, w0)), r

    def _labels_shapes(self, i, h0, w0):
        """What __getitem__ returns beside the pixels, from the geometry alone (both modes): labels (n, 6) normalised to the letterboxed
        image, the `shapes` tuple for scale_coords and the letterbox shape (H, W) of the item's batch."""
        (h, w), _ = self.val_size(h0, w0)
        shape = tuple(int(v) for v in self.batch_shapes[self.batch[i]]) if self.rect else (self.img_size, self.img_size)
        r, new_unpad, pad, (top, bottom, left, right) = letterbox_geometry((h, w), shape, scaleup=False)
        ratio = (r, r)
        H, W = new_unpad[1] + top + bottom, new_unpad[0] + left + right
        lab = self.labels[i]
        out = np.zeros((len(lab), 6), np.float32)
        if len(lab):        # normalised xywh of the file -> pixel xyxy of the letterboxed image -> normalised xywh of it (:961-986)
            gw, gh = ratio[0] * w, ratio[1] * h
            x1, y1 = gw * (lab[:, 1] - lab[:, 3] / 2) + pad[0], gh * (lab[:, 2] - lab[:, 4] / 2) + pad[1]
            x2, y2 = gw * (lab[:, 1] + lab[:, 3] / 2) + pad[0], gh * (lab[:, 2] + lab[:, 4] / 2) + pad[1]
            out[:, 1] = lab[:, 0]
            out[:, 2], out[:, 3] = (x1 + x2) / 2 / W, (y1 + y2) / 2 / H
            out[:, 4], out[:, 5] = (x2 - x1) / W, (y2 - y1) / H
        return torch.from_numpy(out), ((h0, w0), ((h / h0, w / w0), pad)), (H, W)

    def __getitem__(self, i):
        a, b = imread_bgr(self.rgb[i]), imread_bgr(self.ir[i])
        h0, w0 = a.shape[:2]
        labels, shapes, shape = self._labels_shapes(i, h0, w0)
        if self.native:     # decode only: the consumer resizes and pads on the device (Model.forward_frames(val_size=...))
            return (torch.from_numpy(a), torch.from_numpy(b), shape), labels, self.rgb[i], shapes
        (h, w), r = self.val_size(h0, w0)               # longest side -> img_size (load_image_rgb_ir, :1116-1122)
        if r != 1:
            resize = resize_area if r < 1 else resize_bilinear
            a, b = resize(a, (w, h)), resize(b, (w, h))
        a = letterbox(a, shape, auto=False, scaleup=False)[0]
        b = letterbox(b, shape, auto=False, scaleup=False)[0]
        chw = lambda x: np.ascontiguousarray(x[:, :, ::-1].transpose(2, 0, 1))      # noqa: E731
        img6 = torch.from_numpy(np.concatenate((chw(a), chw(b)), 0))
        return img6, labels, self.rgb[i], shapes

    @staticmethod
    def collate_fn(batch):
        img, label, path, shapes = zip(*batch)
        for i, l in enumerate(label):
            l[:, 0] = i                 # image index inside the batch (reference :1053-1058)
        if isinstance(img[0], tuple):   # native items: the frames stay lists (a batch can be ragged), one letterbox shape per batch
            rgb, ir, shape = zip(*img)
            if len(set(shape)) != 1:
                raise ValueError(f"native frames of one batch must share their letterbox shape, got {sorted(set(shape))}")
            return (list(rgb), list(ir), shape[0]), torch.cat(label, 0), path, shapes
        return torch.stack(img, 0), torch.cat(label, 0), path, shapes


def create_dataloader_rgb_ir(path1, path2, imgsz, batch_size, stride=32, opt=None, hyp=None, augment=False, cache=False, pad=0.0,
                             rect=False, rank=-1, world_size=1, workers=0, image_weights=False, quad=False, prefix="", sampler=None,
                             native=False):
    """Reference signature (utils/datasets.py:102-129) -> (loader, dataset); test.py:100 calls it with rect=True, pad=0.5.
    augment / hyp / image_weights / quad belong to training and must be off."""
    if augment or image_weights or quad:
        raise NotImplementedError("training-time loading (augment / image_weights / quad) is outside the inference hot path")
    ds = PairedValSet(path1, path2, imgsz, batch_size, rect=rect, pad=pad, stride=int(stride),
                      single_cls=bool(getattr(opt, "single_cls", False)), native=native)
    batch_size = min(batch_size, len(ds))
    loader = torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=False, num_workers=int(workers),
                                         collate_fn=PairedValSet.collate_fn)
    return loader, ds
