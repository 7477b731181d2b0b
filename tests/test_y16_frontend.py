"""16-bit thermal frames at the front end (no GPU): imread_u16 round trips 16-bit PNG and TIFF files, LoadImages(raw16=True) yields the
uint16 original, and detect_twostream.py --ir-16bit (forward + NMS replaced by the CPU oracle, as tests/test_result_files.py runs the
loop) writes the result files of a run fed with the host-mapped 8-bit frames."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from helpers import REPO
from icafusion_amd.utils import datasets as D
from test_y16_host import content

HERE = os.path.dirname(os.path.abspath(__file__))


def write_u16(path, frame):
    from PIL import Image
    Image.fromarray(frame).save(path)


@pytest.mark.parametrize("ext", ["png", "tif", "tiff"])
def test_imread_u16_round_trips_16_bit_files(tmp_path, ext):
    f = content("ends", 37, 53, 1)
    f[0, :4] = (0x0102, 0x0201, 255, 256)
    write_u16(str(tmp_path / f"a.{ext}"), f)
    got = D.imread_u16(str(tmp_path / f"a.{ext}"))
    assert got.dtype == np.uint16 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, f)


def test_imread_u16_refuses_8_bit_files(tmp_path):
    D.imwrite_bgr(str(tmp_path / "a.png"), np.zeros((4, 4, 3), np.uint8))
    with pytest.raises(ValueError, match="16-bit greyscale"):
        D.imread_u16(str(tmp_path / "a.png"))


def test_load_images_raw16_yields_the_uint16_original(tmp_path):
    frames = [content("narrow", 20, 31, i) for i in range(3)]
    for i, f in enumerate(frames):
        write_u16(str(tmp_path / f"im{i}.png"), f)
    items = list(D.LoadImages(str(tmp_path), 64, 32, raw16=True))
    assert len(items) == 3
    for (path, img, im0, cap), f in zip(items, frames):
        assert img is None and cap is None and im0.dtype == np.uint16 and np.array_equal(im0, f) and path.endswith(".png")


def test_detect_twostream_ir_16bit_equals_a_run_fed_with_the_mapped_frames(tmp_path, monkeypatch):
    """Three pairs whose thermal frames are 16-bit PNGs, through detect_twostream.py --ir-16bit with the default clip, another clip and a
    fixed window: label files and annotated pictures equal those of a plain run whose --source2 holds agc_u16_to_u8 of the same frames."""
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    from test_frontends import make_dataset
    import detect_twostream as dt
    from icafusion_amd.models.yolo import Model
    from icafusion_amd.synth import synth_state_dict
    from oracle import icaf_oracle as oracle
    rgb_dir, _ = make_dataset(str(tmp_path / "set"), n=3, size=(120, 128), nc=3, seed=6)
    names = sorted(os.listdir(rgb_dir))
    raw_dir = tmp_path / "raw"
    raw_dir.mkdir()
    raws = {}
    for i, name in enumerate(names):
        h, w = D.imread_bgr(os.path.join(rgb_dir, name)).shape[:2]
        g = np.random.default_rng(90 + i)
        f = np.clip(np.rint(g.normal(8000, 400, (h, w))), 0, 65535).astype(np.uint16)       # a 14-bit scene ...
        f[h // 4:h // 2, w // 4:w // 2] += 3000                                              # ... with a warm object
        f.reshape(-1)[:5] = (0, 1, 65535, 16383, 16384)                                      # and dead / saturated pixels
        raws[name] = f
        write_u16(str(raw_dir / name), f)
    cfg = yaml.safe_load(open(os.path.join(REPO, "models", "transformer", "yolov5s_Transfusion_FLIR.yaml")))
    om = oracle.OracleModel(cfg, synth_state_dict(Model(cfg), seed=0))

    class FakeModel:
        stride = torch.tensor([8.0, 16.0, 32.0])
        names = ["person", "car", "bicycle"]

        def forward_u8(self, img6):
            f = img6.float() / 255.0
            return (om.forward(f[:, :3].contiguous(), f[:, 3:].contiguous())[0],)

    def fake_nms(pred, conf_thres, iou_thres, classes=None, agnostic=False, **kw):
        return [torch.from_numpy(d.copy()) for d in oracle.non_max_suppression(pred.numpy(), conf_thres, iou_thres, classes=classes, agnostic=agnostic)]

    monkeypatch.setattr(dt, "load_model", lambda opt, device: FakeModel())
    monkeypatch.setattr(dt, "non_max_suppression", fake_nms)
    monkeypatch.setattr(dt, "select_device", lambda d: torch.device("cpu"))

    def run(name, source2, extra):
        out = dt.detect(dt.parse_opt(["--source1", rgb_dir, "--source2", str(source2), "--img-size", "320", "--conf-thres", "0.3", "--save-txt",
                                      "--save-conf", "--project", str(tmp_path / "runs"), "--name", name] + extra))
        return {str(p.relative_to(out)): p.read_bytes() for p in sorted(out.rglob("*")) if p.is_file()}
    cases = [("default", [], lambda f: D.agc_window(f)),
             ("clip", ["--ir-agc-clip", "2.5", "0.03"], lambda f: D.agc_window(f, (250, 3))),
             ("window", ["--ir-window", "7000", "12000"], lambda f: (7000, 12000))]
    for name, flags, window in cases:
        mapped_dir = tmp_path / f"mapped_{name}"
        mapped_dir.mkdir()
        for fname, f in raws.items():
            m8 = D.agc_u16_to_u8(f, *window(f))
            D.imwrite_bgr(str(mapped_dir / fname), np.repeat(m8[:, :, None], 3, axis=2))
        got, want = run(name + "16", raw_dir, ["--ir-16bit"] + flags), run(name + "8", mapped_dir, [])
        assert got.keys() == want.keys() and sum(k.endswith("_ir.png") for k in got) == 3
        if name == "default":
            assert any(k.startswith("labels") for k in got), "conf 0.3 leaves detections on the synthetic weights"
        for k, v in want.items():
            assert got[k] == v, (name, k)
    for flags, match in [(["--ir-window", "5", "4", "--ir-16bit"], "0 <= LO <= HI"), (["--ir-agc-clip", "50", "1", "--ir-16bit"], "49.99"),
                         (["--ir-window", "1", "2"], "pass --ir-16bit"), (["--ir-16bit", "--ir-window", "1", "2", "--ir-agc-clip", "1", "1"], "one of them"),
                         (["--ir-16bit", "--align-ir", "stretch"], "--align-ir")]:
        with pytest.raises(ValueError, match=match):
            run("bad", raw_dir, flags)
