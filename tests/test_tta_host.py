"""Host side of test-time augmentation (Model.forward(augment=True), reference models/yolo_test.py:116-131): the scaled / padded size
table, the input-size limit derived from the model, the C ABI entries — and, in the build container only, the oracle composition the
GPU parity test compares against, checked against the live reference.  No GPU."""
import copy
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from helpers import REPO, load_cfg
from icafusion_amd import _lib
from icafusion_amd.models import yolo
from icafusion_amd.models.yolo import Model

HERE = os.path.dirname(os.path.abspath(__file__))
_keep = (sys.dont_write_bytecode, os.environ.get("PYTHONDONTWRITEBYTECODE"))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden import REF          # noqa: E402  (where the build container keeps the reference tree; the module is a script and
sys.path.remove(os.path.join(HERE, "golden"))      # switches bytecode writing off for its own runs: put the session's settings back)
sys.dont_write_bytecode = _keep[0]
if _keep[1] is None:
    os.environ.pop("PYTHONDONTWRITEBYTECODE", None)
else:
    os.environ["PYTHONDONTWRITEBYTECODE"] = _keep[1]


def test_size_table_equals_the_reference_formula():
    """Every H, W from 448 to 1280 in steps of 32: resized size int(x * ratio), padded size ceil(x * ratio / gs) * gs
    (utils/torch_utils.py:262-266), ratio 1 untouched; pass order and flips of models/yolo_test.py:118-119."""
    for H in range(448, 1281, 32):
        for W in range(448, 1281, 32):
            got = yolo.tta_sizes(H, W, 32)
            assert [(p[0], p[1]) for p in got] == [(1, None), (0.83, 3), (0.67, None)]
            assert got[0][2:] == (H, W, H, W)
            for s, _, hr, wr, hp, wp in got[1:]:
                assert (hr, wr) == (int(H * s), int(W * s))
                assert (hp, wp) == tuple(math.ceil(x * s / 32) * 32 for x in (H, W))
                assert 0 <= hp - hr < 32 + 1 and 0 <= wp - wr < 32 + 1 and hp % 32 == 0 and wp % 32 == 0
    assert [p[2:] for p in yolo.tta_sizes(640, 640)] == [(640, 640, 640, 640), (531, 531, 544, 544), (428, 428, 448, 448)]


def test_minimum_size_is_derived_from_the_models_blocks():
    """The shipped DMFF configs need P5 >= 10 x 10 in the 0.67 pass: 448; another anchor grid or no DMFF block moves the limit."""
    cfg = load_cfg("yolov5s_Transfusion_kaist.yaml")
    assert Model(copy.deepcopy(cfg)).tta_min_size() == (448, 448)
    wide = copy.deepcopy(cfg)
    row = next(r for r in wide["backbone"] + wide["head"] if r[2] == "TransformerFusionBlock" and r[3][0] == 1024)
    row[3][1:3] = [12, 11]                                         # P5 grid 12 x 11: padded 0.67 pass >= 384 x 352
    assert Model(wide).tta_min_size() == (544, 480)
    assert math.ceil(544 * 0.67 / 32) * 32 == 384 and math.ceil(480 * 0.67 / 32) * 32 == 352       # and one step less falls short
    assert math.ceil(512 * 0.67 / 32) * 32 < 384 and math.ceil(448 * 0.67 / 32) * 32 < 352
    assert Model(load_cfg("yolov5s_Add_kaist.yaml")).tta_min_size() == (32, 32)


@pytest.mark.parametrize("shape", [(416, 640), (640, 416), (320, 320)])
def test_too_small_inputs_raise_before_anything_is_built(shape):
    m = Model(load_cfg("yolov5s_Transfusion_kaist.yaml")).eval()
    with pytest.raises(ValueError, match="448x448"):
        m.tta_plan_for(1, *shape, device="cpu")
    assert not m.__dict__.get("_plans")                            # no plan was built or cached on the way
    with pytest.raises(ValueError, match="multiple of the max stride"):
        m.tta_plan_for(1, 450, 640, device="cpu")


def test_augment_keeps_the_loud_failures_of_the_plain_forward():
    m = Model(load_cfg("yolov5s_Transfusion_kaist.yaml")).eval()
    x = torch.zeros(1, 3, 448, 448)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(x, x, augment=True)                                      # CPU tensors: no fallback
    with pytest.raises(NotImplementedError):
        m.train()(x, x, augment=True)


def test_header_declares_the_tta_entries_with_reference_citations():
    header = open(os.path.join(REPO, "include", "icaf.h")).read()
    for name in ("icaf_tta_stage", "icaf_tta_merge"):
        assert name in _lib.SIGNATURES and re.search(rf"\b{name}\s*\(", header)
    block = header[header.index("test-time augmentation"):header.index("int icaf_tta_merge")]
    assert "models/yolo_test.py:116-131" in block and "utils/torch_utils.py:257-267" in block
    assert _lib.TtaPass.dst.offset == 0 and __import__("ctypes").sizeof(_lib.TtaPass) == 32


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "models")), reason="the reference tree is only present in the build container")
def test_oracle_composition_equals_the_live_reference():
    """The live reference's scale_img + forward_once(xi, xi2), merged as its lines 125-131 do, against tta_helpers.oracle_tta."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "tta_differential.py")], capture_output=True, text=True, timeout=1500, env=env)
    assert r.returncode == 0 and "TTA_DIFFERENTIAL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
