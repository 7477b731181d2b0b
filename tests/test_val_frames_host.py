"""Host side of validation from native frames (no GPU): the fixed-order statement of the area resize against resize_area, the validation
geometry against the loader and letterbox, the native mode of the loader against its pixel mode, the validation in front of the launch,
the header and the flags."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import REPO, load_cfg, val_module
from icafusion_amd import _lib, ops
from icafusion_amd.models.yolo import Model
from icafusion_amd.utils import datasets as D
from test_frontends import make_dataset

# native (h0, w0) -> resized (nh, nw): the sizes on which the two statements were found equal, up to 300 x 400, and the LLVIP frame
AREA_SIZES = [((96, 128), (48, 64)), ((120, 128), (90, 96)), ((130, 70), (64, 34)), ((200, 9), (64, 2)), ((300, 400), (48, 64)),
              ((37, 53), (22, 32)), ((100, 320), (20, 64)), ((240, 300), (128, 160)), ((256, 320), (128, 160)), ((129, 257), (64, 128)),
              ((65, 64), (64, 63)), ((1024, 1280), (512, 640))]


def weights64(n_in, n_out):
    """resize_area.weights before its rounding to float32"""
    s = n_in / n_out
    lo = np.arange(n_out, dtype=np.float64) * s
    px = np.arange(n_in, dtype=np.float64)
    return np.clip(np.minimum((lo + s)[:, None], px[None] + 1.0) - np.maximum(lo[:, None], px[None]), 0.0, None) / s


@pytest.mark.parametrize("src,dst", AREA_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_resize_area_scalar_equals_resize_area(src, dst):
    """Uniform random images, 3 channels and 1: the fixed-order statement equals the BLAS one byte for byte on these sizes."""
    g = np.random.default_rng(src[0] * 1000 + src[1])
    for ch in (3, 1):
        img = g.integers(0, 256, (*src, ch), dtype=np.uint8)
        got = D.resize_area_scalar(img, dst[::-1])
        assert got.shape == (*dst, ch) and got.dtype == np.uint8
        assert np.array_equal(got, D.resize_area(img, dst[::-1])), ch


def test_resize_area_scalar_tie_contract_and_identity():
    """A two-level image makes exact averages of k + 0.5 common: there the two summation orders may fall on different sides.  The contract:
    at most one grey level apart, and only where the float64 average lies within 1e-4 of a half."""
    g = np.random.default_rng(0)
    img = (g.integers(0, 2, (60, 48, 3)) * 255).astype(np.uint8)
    a, b = D.resize_area(img, (25, 32)).astype(np.int64), D.resize_area_scalar(img, (25, 32)).astype(np.int64)
    assert np.abs(a - b).max() <= 1
    avg = np.einsum("oh,hwc,pw->opc", weights64(60, 32), img.astype(np.float64), weights64(48, 25))
    frac = avg - np.floor(avg)
    assert (np.abs(frac[a != b] - 0.5) < 1e-4).all()
    same = g.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    assert D.resize_area_scalar(same, (23, 17)) is same


def loader_numbers(h0, w0, img_size, batch_shape):
    """(nh, nw, top, left, mode, scale row) from the loader's own code: load_image_rgb_ir's step on a blank frame, then letterbox()."""
    r = img_size / max(h0, w0)
    img = np.zeros((h0, w0, 3), np.uint8)
    if r != 1:
        img = (D.resize_area if r < 1 else D.resize_bilinear)(img, (int(w0 * r), int(h0 * r)))
    h, w = img.shape[:2]
    out, ratio, pad = D.letterbox(img, batch_shape, auto=False, scaleup=False)
    assert out.shape[:2] == tuple(batch_shape)
    rows, cols = np.nonzero((out[:, :, 0] == 0))
    shapes = ((h0, w0), ((h / h0, w / w0), pad))                                      # what __getitem__ hands to test.py
    (h0_, w0_), ((gain, _), (padw, padh)) = shapes[0], shapes[1]
    row = torch.tensor([[gain, padw, padh, w0_, h0_]], dtype=torch.float32).numpy()[0]   # test.py's `scale` list
    return h, w, int(rows.min()), int(cols.min()), int(r < 1), row, (int(rows.max()) + 1 - int(rows.min()), int(cols.max()) + 1 - int(cols.min()))


@pytest.mark.parametrize("img_size,batch_shape", [(64, (96, 96)), (64, (64, 96)), (128, (160, 160)), (160, (192, 224)), (320, (352, 352))],
                         ids=lambda v: str(v))
def test_val_geometry_equals_the_loader(img_size, batch_shape):
    """Mixed native sizes against one batch shape, square and rectangular: r < 1 (area), r == 1 (copy) and r > 1 (bilinear) all occur
    over the list; every number equals what the loader's code produces."""
    shapes = [(96, 128), (120, 128), (37, 53), (128, 100), (60, 64), (130, 70)]
    fit = [s for s in shapes if max(int(s[0] * img_size / max(s)), 1) <= batch_shape[0] and max(int(s[1] * img_size / max(s)), 1) <= batch_shape[1]]
    assert len(fit) >= 3
    geom, mode, scale = ops.val_geometry(fit, img_size, batch_shape)
    assert geom.dtype == ops.GEOM_DTYPE and mode.dtype == np.int32 and scale.dtype == np.float32 and scale.shape == (len(fit), 5)
    for g, md, sc, (h0, w0) in zip(geom, mode, scale, fit):
        nh, nw, top, left, want_mode, row, block = loader_numbers(h0, w0, img_size, batch_shape)
        assert (int(g["h0"]), int(g["w0"]), int(g["nh"]), int(g["nw"]), int(g["top"]), int(g["left"]), int(md)) == (h0, w0, nh, nw, top, left, want_mode)
        assert block == (nh, nw) and np.array_equal(sc, row)
        assert g["sx"] == np.float32(w0 / nw) and g["sy"] == np.float32(h0 / nh)
    seen = {int(m) for m in mode} | ({"copy"} if any((int(g["nh"]), int(g["nw"])) == (int(g["h0"]), int(g["w0"])) for g in geom) else set())
    # 64 and 128: 130 x 70 shrinks, 37 x 53 grows, 60 x 64 (at 64) / 96 x 128 (at 128) have their longest side at size; above, all grow
    assert seen == ({0, 1, "copy"} if img_size <= 128 else {0})


def test_val_geometry_refuses_a_second_resize():
    """letterbox(scaleup=False) would shrink a frame that does not fit the batch shape: that is not the loader's protocol."""
    with pytest.raises(ValueError, match="padding alone"):
        ops.val_geometry([(96, 128)], 128, (64, 64))
    ops.val_geometry([(48, 64), (128, 96)], 64, (64, 64))                 # a square batch holds both orientations
    with pytest.raises(ValueError, match="padding alone"):
        ops.val_geometry([(48, 64), (128, 96)], 64, (32, 64))             # a landscape batch does not hold the portrait frame
    with pytest.raises(ValueError, match="no pixel"):
        ops.val_geometry([(200, 1)], 64, (64, 64))
    with pytest.raises(ValueError, match="empty"):
        ops.val_geometry([(0, 5)], 64, (64, 64))


def compose(frame, img_size, shape):
    """The pixel item from a native frame: resize_area_scalar or resize_bilinear, then padding, RGB planes."""
    h0, w0 = frame.shape[:2]
    r = img_size / max(h0, w0)
    if r != 1:
        frame = (D.resize_area_scalar if r < 1 else D.resize_bilinear)(frame, (int(w0 * r), int(h0 * r)))
    out = D.letterbox(frame, shape, auto=False, scaleup=False)[0]
    assert out.shape[:2] == tuple(shape)
    return np.ascontiguousarray(out[:, :, ::-1].transpose(2, 0, 1))


@pytest.mark.parametrize("img_size,rect", [(64, True), (64, False), (128, True), (160, True)], ids=["shrink-rect", "shrink-square", "copy", "grow"])
def test_native_items_equal_pixel_items(tmp_path, img_size, rect):
    """native=True decodes only: same labels, shapes, paths and order as native=False, item by item and batch by batch, and the pixel
    item is the native frame composed on the host (seed 3: no byte of this set is a tie between the two area statements)."""
    rgb_dir, ir_dir = make_dataset(str(tmp_path), n=5, size=(96, 128), nc=2, seed=3)
    kw = dict(pad=0.5 if rect else 0.0, rect=rect)
    _, pix = D.create_dataloader_rgb_ir(rgb_dir, ir_dir, img_size, 2, 32, None, **kw)
    _, nat = D.create_dataloader_rgb_ir(rgb_dir, ir_dir, img_size, 2, 32, None, native=True, **kw)
    assert pix.native is False and nat.native is True and pix.rgb == nat.rgb
    for i in range(len(pix)):
        img6, lab, path, shapes = pix[i]
        (a, b, shape), nlab, npath, nshapes = nat[i]
        assert torch.equal(lab, nlab) and path == npath and shapes == nshapes and shape == tuple(img6.shape[1:])
        assert a.dtype == torch.uint8 and tuple(a.shape) == (*shapes[0], 3) and np.array_equal(a.numpy(), D.imread_bgr(pix.rgb[i]))
        want = np.concatenate((compose(a.numpy(), img_size, shape), compose(b.numpy(), img_size, shape)), 0)
        assert np.array_equal(img6.numpy(), want), i
    lp = torch.utils.data.DataLoader(pix, batch_size=2, shuffle=False, collate_fn=D.PairedValSet.collate_fn)
    ln = torch.utils.data.DataLoader(nat, batch_size=2, shuffle=False, collate_fn=D.PairedValSet.collate_fn)
    nbatches = 0
    for (img6, targets, paths, shapes), ((rgb, ir, shape), ntargets, npaths, nshapes) in zip(lp, ln):
        assert isinstance(rgb, list) and len(rgb) == len(ir) == img6.shape[0] and shape == tuple(img6.shape[2:])
        assert torch.equal(targets, ntargets) and paths == npaths and shapes == nshapes
        nbatches += 1
    assert nbatches == 3                                                   # 2 + 2 + a ragged last batch of 1


def test_resize_frames_validates_before_any_device_call(monkeypatch):
    def no_device():
        raise AssertionError("the library was called before the arguments were validated")
    monkeypatch.setattr(ops, "lib", no_device)
    geom, mode, _ = ops.val_geometry([(96, 128), (48, 60)], 64, (64, 96))
    assert mode.tolist() == [1, 0]
    end = ops.pack_frames(geom, 3)
    arena, tab, dst = torch.zeros(end, dtype=torch.uint8), torch.zeros(2 * 48, dtype=torch.uint8), torch.zeros((2, 3, 64, 96), dtype=torch.uint8)
    mdev = torch.from_numpy(mode)
    g = geom.copy()
    g[0]["nh"] = 97                                                        # mode 1 with nh > h0 (still inside a taller output)
    with pytest.raises(ValueError, match="only shrinks"):
        ops.resize_frames(arena, g, mdev, tab, torch.zeros((2, 3, 128, 96), dtype=torch.uint8), mode=mode)
    g = geom.copy()
    g[1]["nw"] = 61                                                        # the same on a mode-0 row is a bilinear up-scale: no complaint about it
    with pytest.raises(ValueError, match="cuda"):
        ops.resize_frames(arena, g, mdev, tab, dst, mode=mode)
    with pytest.raises(ValueError, match="mode table"):
        ops.resize_frames(arena, geom, mdev[:1], tab, dst, mode=mode)      # a device table shorter than the descriptors
    with pytest.raises(ValueError, match="mode table"):
        ops.resize_frames(arena, geom, mdev, tab, dst, mode=mode[:1])
    with pytest.raises(ValueError, match="mode table"):
        ops.resize_frames(arena, geom, mdev, tab, dst)                     # device rows without their host twin
    with pytest.raises(ValueError, match="mode 2"):
        ops.resize_frames(arena, geom, mdev, tab, dst, mode=np.array([1, 2], np.int32))
    g = geom.copy()
    g[0]["pitch"] = 1
    with pytest.raises(ValueError, match="pitch"):
        ops.resize_frames(arena, g, mdev, tab, dst, mode=mode)
    with pytest.raises(ValueError, match="cuda"):
        ops.resize_frames(arena, geom, mdev, tab, dst, mode=mode)          # everything valid: refused only because nothing is on a GPU


def test_area_budget_rule():
    """ops.area_staged restates the kernel's rule: LLVIP's 2 x and a 6 x shrink keep several rows in LDS; 7 x and more has more taps than
    the tables hold and goes direct."""
    def row(shape, img_size, batch, ch=3):
        geom, mode, _ = ops.val_geometry([shape], img_size, batch)
        ops.pack_frames(geom, ch)
        assert mode[0] == 1
        return geom[0]
    assert ops.area_staged(row((1024, 1280), 640, (544, 672)))
    assert ops.area_staged(row((3840, 3840), 640, (640, 640)))             # s = 6
    assert ops.area_staged(row((300, 400), 64, (64, 96)))                  # s = 6.25: 8 taps, 4 rows of 400 x 3 floats
    assert not ops.area_staged(row((2160, 4480), 640, (320, 640)))         # s = 7
    assert ops.area_staged(row((2160, 4480), 640, (320, 640), ch=1)) is False
    assert _lib.RESIZE_LDS_BYTES == 20480 and _lib.RESIZE_MAX_TAPS == 8


def test_header_signature_and_flags():
    with open(os.path.join(REPO, "include", "icaf.h")) as f:
        header = f.read()
    assert "int icaf_resize_frames(const void* arena, const icaf_frame_geom* geom, const int* mode, int nstreams, int B" in header
    block = header[header.index("native validation frames"):header.index("int icaf_resize_frames(")]
    assert "utils/datasets.py:1116-1122" in block and "ICAF_RESIZE_LDS_BYTES = 20480" in block
    assert len(_lib.SIGNATURES["icaf_resize_frames"][1]) == 11
    sys.path.insert(0, REPO)
    val = val_module()
    assert val.parse_opt([]).device_letterbox is False and val.parse_opt(["--device-letterbox"]).device_letterbox is True
    import inspect
    assert list(inspect.signature(val.test).parameters)[-1] == "device_letterbox"
    assert list(inspect.signature(D.create_dataloader_rgb_ir).parameters)[-1] == "native"
    assert list(inspect.signature(D.PairedValSet.__init__).parameters)[-1] == "native"


def test_forward_frames_with_val_size_rejects_what_forward_frames_rejects():
    m = Model(load_cfg("yolov5s_Add_kaist.yaml"))
    f = torch.zeros((1, 48, 64, 3), dtype=torch.uint8)
    with pytest.raises(NotImplementedError):
        m.train().forward_frames(f, f, 64, val_size=64)
    m.eval()
    with pytest.raises(ValueError, match="cuda uint8"):
        m.forward_frames(f, f, 64, val_size=64)
    with pytest.raises(ValueError, match="cuda uint8"):
        m.forward_frames(f.float(), f.float(), 64, val_size=64)
    with pytest.raises(ValueError):
        m.forward_frames(f, [f[0], f[0]], 64, val_size=64)
    with pytest.raises(ValueError):
        m.forward_frames(f[0], f[0], 64, val_size=64)
