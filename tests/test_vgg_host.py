"""Host side of the VGG16 two-stream backbone (no GPU): the four yolov5_VGG16_* configs construct with the reference's state_dict
surface (key names, shapes and parameter counts recorded from the real reference in tests/golden/model_vgg16_*.npz), parse_model /
_layer_shapes / stream_twins treat VGGblock rows as the issue states, the modules refuse CPU tensors and train mode like every other
module, the root shim resolves for pickled checkpoints, and a ReLU layer is never offered a SiLU-only launch configuration."""
import io
import os
import pickle

import pytest
import torch

from helpers import REPO, load_cfg, load_golden
from icafusion_amd import configs, ops
from icafusion_amd._lib import ConvArgs
from icafusion_amd.models.common import Conv, NiNfusion, TransformerFusionBlock, VGGblock
from icafusion_amd.models.yolo import Model

NAMES = [f"yolov5_VGG16_{fusion}_{tag}.yaml" for fusion, tag, _ in configs.VGG16_VARIANTS]
GOLDENS = {"yolov5_VGG16_Transfusion_kaist.yaml": ("model_vgg16_kaist_320_b1", 62170074, 480),
           "yolov5_VGG16_NiNfusion_FLIR.yaml": ("model_vgg16_ninfusion_flir_320x352_b2", 42686664, 303)}


def test_variant_list_is_the_four_files():
    assert sorted(NAMES) == sorted(["yolov5_VGG16_Transfusion_kaist.yaml", "yolov5_VGG16_Transfusion_FLIR.yaml",
                                    "yolov5_VGG16_NiNfusion_kaist.yaml", "yolov5_VGG16_NiNfusion_FLIR.yaml"])


@pytest.mark.parametrize("fusion,tag,nc", configs.VGG16_VARIANTS)
def test_yaml_files_equal_the_generator(fusion, tag, nc):
    name = f"yolov5_VGG16_{fusion}_{tag}.yaml"
    cfg = configs.vgg16_cfg(fusion, nc)
    assert load_cfg(name) == cfg, name
    with open(os.path.join(REPO, "models", "transformer", name)) as f:
        assert f.read() == configs._dump_model_yaml(cfg, name, streams="VGG16")
    assert cfg["nc"] == nc and [r[2] for r in cfg["backbone"][:10]] == ["VGGblock"] * 10 and cfg["backbone"][5][0] == -4


@pytest.mark.parametrize("name", NAMES)
def test_every_config_constructs(name):
    m = Model(os.path.join(REPO, "models", "transformer", name))
    assert len(m.model) == 28 and m.model[5].f == -4 and m.model[10].f == [2, 7]
    assert all(isinstance(m.model[i], VGGblock) for i in range(10))
    kind = NiNfusion if "NiNfusion" in name else TransformerFusionBlock
    assert all(isinstance(m.model[i], kind) for i in (10, 11, 12))
    assert m.stride.tolist() == [8.0, 16.0, 32.0]
    assert [len(b.convs()) for b in m.model[:5]] == [2, 2, 3, 3, 3]
    assert [(b.convs()[0].in_channels, b.convs()[-1].out_channels) for b in m.model[:5]] == [(3, 64), (64, 128), (128, 256), (256, 512), (512, 512)]
    assert m.fuse() is m                                     # nothing to fold in a VGGblock; the head's Convs lose their .bn
    assert not any(hasattr(c, "bn") for c in m.modules() if type(c) is Conv)
    assert "model.0.vggblock.0.0.weight" in m.state_dict() and "model.0.vggblock.0.0.bias" in m.state_dict()


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_state_dict_surface_equals_the_reference(name):
    golden, params, nkeys = GOLDENS[name]
    g = load_golden(golden)
    m = Model(load_cfg(name))
    sd = m.state_dict()
    keys = [str(k) for k in g["sd_keys"]]
    assert int(g["n_params"]) == params and len(keys) == nkeys
    assert list(sd) == keys
    shapes = [tuple(int(v) for v in row if v >= 0) for row in g["sd_shapes"]]
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert sum(p.numel() for p in m.parameters()) == params
    assert not [k for k in sd if ".blk." in k]               # the reference's plain list is not registered: only `vggblock` appears


def test_layer_shapes_and_twins():
    m = Model(load_cfg("yolov5_VGG16_Transfusion_kaist.yaml"))
    shapes = m._layer_shapes(1, 640, 640)
    assert shapes[:5] == [(64, 320, 320), (128, 160, 160), (256, 80, 80), (512, 40, 40), (512, 20, 20)]
    assert shapes[5:10] == shapes[:5] and shapes[10:13] == shapes[2:5]
    assert m._layer_shapes(1, 352, 416)[4] == (512, 11, 13)
    # each block halves with floor
    assert m._layer_shapes(2, 330, 362)[:2] == [(64, 165, 181), (128, 82, 90)]
    assert m.stream_twins() == {5: 0, 6: 1, 7: 2, 8: 3, 9: 4}
    m.pair_streams = False
    assert m.stream_twins() == {}
    assert m.tta_min_size() == Model(load_cfg("yolov5l_Transfusion_kaist.yaml")).tta_min_size()       # same strides and anchor grids


def test_twins_need_the_same_structure():
    cfg = load_cfg("yolov5_VGG16_NiNfusion_FLIR.yaml")
    m = Model(cfg)
    m.model[7].vggblock[-1] = torch.nn.MaxPool2d(3, 2, 1)     # another window in the IR stream: rows 7.. no longer pair
    assert m.stream_twins() == {5: 0, 6: 1}


def test_cpu_tensors_and_train_mode_raise():
    blk = VGGblock(2, 64, 128)
    with pytest.raises(NotImplementedError, match="eval"):
        blk.train()(torch.zeros(1, 64, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blk.eval()(torch.zeros(1, 64, 8, 8))
    m = Model(load_cfg("yolov5_VGG16_NiNfusion_kaist.yaml"))
    x = torch.zeros(1, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="eval"):
        m.train()(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval()(x, x)


def test_foreign_modules_in_a_block_are_refused_at_plan_build():
    """emit launches ReLU and icaf_maxpool2d: a block whose activation or closing module is something else must not run as if it were."""
    from icafusion_amd.engine import Plan
    for edit in ("act", "pool", "ceil"):
        blk = VGGblock(2, 64, 128).eval()
        if edit == "act":
            blk.vggblock[1][1] = torch.nn.SiLU()
        elif edit == "pool":
            blk.vggblock[-1] = torch.nn.AvgPool2d(2, 2)
        else:
            blk.vggblock[-1] = torch.nn.MaxPool2d(2, 2, ceil_mode=True)
        plan = Plan("cpu", torch.float32)
        with pytest.raises(NotImplementedError):
            blk.emit(plan, plan.act(1, 8, 8, 64))
        assert not plan.launches


def test_root_shim_resolves_and_pickles():
    import models.common as root_common
    assert root_common.VGGblock is VGGblock
    # a reference checkpoint names the class as models.common.VGGblock: what the unpickler looks up
    assert pickle.Unpickler(io.BytesIO(b"")).find_class("models.common", "VGGblock") is VGGblock
    blk = VGGblock(3, 128, 256)
    back = pickle.loads(pickle.dumps(blk))
    assert type(back) is VGGblock and list(back.state_dict()) == list(blk.state_dict()) and len(back.convs()) == 3


def _relu_args(dt, cin, cout, k, wf=False, hw=40):
    a = ConvArgs()
    a.B, a.H, a.W, a.Cin, a.ldx = 2, hw, hw, cin, cin
    a.Ho, a.Wo, a.Cout, a.ldy = hw, hw, cout, cout
    a.kh = a.kw = k
    a.sh = a.sw = 1
    a.ph = a.pw = k // 2
    a.groups, a.act, a.dtype, a.out_dtype = 1, ops.ACT_RELU, dt, dt
    a.Kp = -(-k * k * cin // 64) * 64
    if wf:
        a.wf = 4096                                            # any non-null address: the rules only ask whether the copy exists
    return a


@pytest.mark.parametrize("cin,cout,k", [(64, 64, 3), (64, 128, 3), (128, 128, 3), (128, 256, 3), (512, 512, 3), (8, 64, 3), (256, 128, 1)])
@pytest.mark.parametrize("dt", [ops.F32, ops.BF16, ops.F16])
def test_relu_layers_get_no_silu_only_configuration(cin, cout, k, dt):
    silu_only = set(range(41, 46)) | {71} | set(range(81, 86))
    a = _relu_args(dt, cin, cout, k, wf=True)
    cands = ops.conv_candidates(a)
    assert cands and not (set(cands) & silu_only), cands
    assert not ops.wants_wf(a) or dt != ops.F32
    a.act = ops.ACT_SILU                                       # the same layer with SiLU is offered them where they are built
    if dt != ops.F32 and (cin, cout, k) in ((64, 64, 3), (128, 128, 3)):
        assert set(ops.conv_candidates(a)) & silu_only
    # 16-bit ReLU layers with whole 128-byte taps keep the streaming and register-fed GEMMs
    a.act = ops.ACT_RELU
    if dt != ops.F32 and cin % 64 == 0:
        assert 52 in cands and (cout <= 64 or 61 in cands)


def test_activation_codes_agree_with_the_header():
    text = open(os.path.join(REPO, "include", "icaf.h")).read()
    assert "ICAF_ACT_RELU = 3" in text and ops.ACT_RELU == 3
