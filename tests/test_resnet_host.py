"""Host side of the ResNet50 two-stream backbone (no GPU): the four yolov5_ResNet50_* configs construct with the reference's state_dict
surface (key names, shapes and parameter counts recorded from the real reference in tests/golden/model_resnet50_*.npz), a strict
state_dict round trip works, Model.fuse() leaves the blocks' BatchNorms alone, the yaml files are the generator's output, parse_model /
_layer_shapes / stream_twins treat ResNetlayer rows as the reference does, a plan built on the CPU shows the two streams paired and
conv3 with the residual in front of its ReLU, and the candidate rules state what the library accepts for that launch form."""
import io
import os
import pickle

import pytest
import torch

from helpers import REPO, load_cfg, load_golden
from icafusion_amd import configs, ops
from icafusion_amd._lib import ConvArgs
from icafusion_amd.models.common import Conv, NiNfusion, ResNetblock, ResNetlayer, TransformerFusionBlock
from icafusion_amd.models.yolo import Model
from icafusion_amd.synth import synth_state_dict

NAMES = [f"yolov5_ResNet50_{fusion}_{tag}.yaml" for fusion, tag, _ in configs.RESNET50_VARIANTS]
GOLDENS = {"yolov5_ResNet50_Transfusion_kaist.yaml": ("model_resnet50_kaist_320_b1", 313767642, 1064),
           "yolov5_ResNet50_NiNfusion_FLIR.yaml": ("model_resnet50_ninfusion_flir_320x352_b2", 136152264, 887)}
_MODELS = {}


def model(name):
    if name not in _MODELS:
        _MODELS[name] = Model(load_cfg(name)).eval()
    return _MODELS[name]


def test_variant_list_is_the_four_files():
    assert sorted(NAMES) == sorted(["yolov5_ResNet50_Transfusion_kaist.yaml", "yolov5_ResNet50_Transfusion_FLIR.yaml",
                                    "yolov5_ResNet50_NiNfusion_kaist.yaml", "yolov5_ResNet50_NiNfusion_FLIR.yaml"])


@pytest.mark.parametrize("fusion,tag,nc", configs.RESNET50_VARIANTS)
def test_yaml_files_equal_the_generator(fusion, tag, nc):
    name = f"yolov5_ResNet50_{fusion}_{tag}.yaml"
    cfg = configs.resnet50_cfg(fusion, nc)
    assert load_cfg(name) == cfg, name
    with open(os.path.join(REPO, "models", "transformer", name)) as f:
        assert f.read() == configs._dump_model_yaml(cfg, name, streams="ResNet50", fusion=fusion)
    assert cfg["nc"] == nc and [r[2] for r in cfg["backbone"][:10]] == ["ResNetlayer"] * 10 and cfg["backbone"][5][0] == -4
    if fusion == "Transfusion":
        assert [r[3] for r in cfg["backbone"][10:]] == [[512, 20, 20], [1024, 16, 16], [2048, 10, 10]]
    assert [r[3][0] for r in cfg["head"] if r[2] in ("Conv", "C3")] == [1024, 1024, 512, 512, 512, 1024, 1024, 2048]


@pytest.mark.parametrize("name", NAMES)
def test_every_config_constructs(name):
    m = model(name)
    assert len(m.model) == 28 and m.model[5].f == -4 and m.model[10].f == [2, 7]
    assert all(isinstance(m.model[i], ResNetlayer) for i in range(10))
    kind = NiNfusion if "NiNfusion" in name else TransformerFusionBlock
    assert all(isinstance(m.model[i], kind) for i in (10, 11, 12))
    assert m.stride.tolist() == [8.0, 16.0, 32.0]
    assert m.model[0].is_first and [len(m.model[i].layer) for i in range(1, 5)] == [3, 4, 6, 3]
    assert [m.model[i].layer[-1].conv3.out_channels for i in range(1, 5)] == [256, 512, 1024, 2048]
    # the shortcut convolution exists where the reference builds one: the first block of every row
    assert [[len(b.shortcut) for b in m.model[i].layer] for i in (1, 2)] == [[2, 0, 0], [2, 0, 0, 0]]
    assert [m.model[i].layer[0].conv2.stride for i in range(1, 5)] == [(1, 1), (2, 2), (2, 2), (2, 2)]


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_state_dict_surface_equals_the_reference(name):
    golden, params, nkeys = GOLDENS[name]
    g = load_golden(golden)
    m = model(name)
    sd = m.state_dict()
    keys = [str(k) for k in g["sd_keys"]]
    assert int(g["n_params"]) == params and len(keys) == nkeys
    assert list(sd) == keys
    shapes = [tuple(int(v) for v in row if v >= 0) for row in g["sd_shapes"]]
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert sum(p.numel() for p in m.parameters()) == params
    assert not [k for k in sd if ".blk." in k]               # the reference's plain list is not registered: only `layer` appears
    for k in ("model.0.layer.0.weight", "model.0.layer.1.running_var", "model.1.layer.0.conv1.weight", "model.1.layer.0.bn3.weight",
              "model.1.layer.0.shortcut.0.weight", "model.1.layer.0.shortcut.1.bias", "model.4.layer.2.conv3.weight"):
        assert k in sd, k
    assert "model.1.layer.1.shortcut.0.weight" not in sd


def test_strict_round_trip_and_fuse_keeps_the_batchnorms():
    name = "yolov5_ResNet50_NiNfusion_kaist.yaml"
    a, b = Model(load_cfg(name)).eval(), Model(load_cfg(name)).eval()
    sd = synth_state_dict(a, 5)
    assert a.load_state_dict(sd, strict=True).missing_keys == []
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    res = b.load_state_dict(torch.load(buf), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    before = list(b.state_dict())
    assert b.fuse() is b
    blocks = [x for x in b.modules() if isinstance(x, ResNetblock)]
    assert len(blocks) == 32
    for blk in blocks:
        assert all(isinstance(getattr(blk, n), torch.nn.BatchNorm2d) for n in ("bn1", "bn2", "bn3"))
        assert not len(blk.shortcut) or isinstance(blk.shortcut[1], torch.nn.BatchNorm2d)
    assert all(isinstance(b.model[i].layer[1], torch.nn.BatchNorm2d) for i in (0, 5))
    assert not any(hasattr(c, "bn") for c in b.modules() if type(c) is Conv)          # the head's Convs are folded, as in the reference
    assert [k for k in before if ".layer." in k] == [k for k in b.state_dict() if ".layer." in k]
    assert all(bn.eps == 1e-3 for bn in b.modules() if isinstance(bn, torch.nn.BatchNorm2d))


def test_layer_shapes_twins_and_tta_size():
    m = model("yolov5_ResNet50_Transfusion_kaist.yaml")
    shapes = m._layer_shapes(1, 640, 640)
    assert shapes[:5] == [(64, 160, 160), (256, 160, 160), (512, 80, 80), (1024, 40, 40), (2048, 20, 20)]
    assert shapes[5:10] == shapes[:5] and shapes[10:13] == shapes[2:5]
    assert m._layer_shapes(1, 352, 416)[4] == (2048, 11, 13)
    # odd sizes: 7x7 / s2 / p3, 3 / 2 / 1 pool and the 3x3 / s2 / p1 convolutions all floor
    assert m._layer_shapes(2, 330, 362)[:3] == [(64, 83, 91), (256, 83, 91), (512, 42, 46)]
    assert m.stream_twins() == {5: 0, 6: 1, 7: 2, 8: 3, 9: 4}
    assert m.tta_min_size() == Model(load_cfg("yolov5l_Transfusion_kaist.yaml")).tta_min_size() == (448, 448)
    assert model("yolov5_ResNet50_NiNfusion_FLIR.yaml").tta_min_size() == (32, 32)


def test_twins_need_the_same_structure():
    m = Model(load_cfg("yolov5_ResNet50_NiNfusion_FLIR.yaml"))
    m.model[5].layer[3] = torch.nn.MaxPool2d(2, 2)            # another pool window in the IR stream's stem row: nothing pairs
    assert m.stream_twins() == {}
    m = Model(load_cfg("yolov5_ResNet50_NiNfusion_FLIR.yaml"))
    m.model[7].layer[1].conv2 = torch.nn.Conv2d(128, 128, 3, 1, 2, dilation=2, bias=False)     # same weights' shapes, another geometry
    assert m.stream_twins() == {5: 0, 6: 1}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_cpu_plan_build_pairs_the_streams(dt):
    """A plan built without a GPU: rows 0-4 / 5-9 are groups = 2 launches, every block ends on the residual-in-front-of-ReLU launch, the
    last blocks of rows 2-4 write the fusion buffers' halves directly."""
    m = model("yolov5_ResNet50_NiNfusion_FLIR.yaml")
    plan = m.build_plan(1, 96, 128, torch.device("cpu"), dt)
    by = {}
    for l in plan.launches:
        by.setdefault(l.name, []).append(l)
    assert len(by["resnet_conv1x1+res"]) == 16 and len(by["resnet_conv1x1"]) == 16 and len(by["resnet_stem7x7s2"]) == 1
    assert len(by["resnet_conv3x3s1"]) + len(by["resnet_conv3x3s2"]) == 16 and len(by["resnet_conv3x3s2"]) == 3
    assert len(by["resnet_shortcut1x1s1"]) == 1 and len(by["resnet_shortcut1x1s2"]) == 3
    assert len(by["preprocess_pad"]) == 1 and len(by["resnet_maxpool"]) == 1
    for name in ("resnet_conv1x1+res", "resnet_conv1x1", "resnet_stem7x7s2", "resnet_shortcut1x1s2"):
        assert all(l.keep[0].groups == 2 for l in by[name]), name
    for l in by["resnet_conv1x1+res"]:
        a = l.keep[0]
        assert a.res_mode == 1 and a.res and a.act == ops.ACT_RELU and (a.kh, a.kw, a.sh) == (1, 1, 1)
    assert all(l.keep[0].res_mode == 0 and not l.keep[0].res for n in by if n != "resnet_conv1x1+res" and n.startswith("resnet_") and "pool" not in n
               for l in by[n])
    assert all(l.keep[0].act == ops.ACT_NONE for l in by["resnet_shortcut1x1s2"])
    stem = by["resnet_stem7x7s2"][0].keep[0]
    assert (stem.kh, stem.sh, stem.ph, stem.Cout, stem.act) == (7, 2, 3, 64, ops.ACT_RELU) and stem.Cin == ops.VEC[dt]
    # rows 2-4 end in the (B, H, W, 2C) buffer NiNfusion reads: pixel stride 2C, the IR stream C elements behind the RGB one
    tails = [l.keep[0] for l in by["resnet_conv1x1+res"] if l.keep[0].ldy == 2 * l.keep[0].Cout]
    assert sorted(a.Cout for a in tails) == [512, 1024, 2048] and all(a.y_gs == a.Cout for a in tails)
    m.pair_streams = False
    try:
        names = [l.name for l in m.build_plan(1, 96, 128, torch.device("cpu"), dt).launches]
        assert names.count("resnet_conv1x1+res") == 32 and names.count("resnet_maxpool") == 2
    finally:
        m.pair_streams = True


def test_transfusion_plan_runs_cross_attention_at_all_three_levels():
    m = model("yolov5_ResNet50_Transfusion_kaist.yaml")
    for dt in (torch.float32, torch.bfloat16):
        names = [l.name for l in m.build_plan(1, 320, 320, torch.device("cpu"), dt).launches]
        assert names.count("cross_attention") == 3 and names.count("resnet_conv1x1+res") == 16


def test_cpu_tensors_and_train_mode_raise():
    blk = ResNetblock(64, 64)
    with pytest.raises(NotImplementedError, match="eval"):
        blk.train()(torch.zeros(1, 64, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blk.eval()(torch.zeros(1, 64, 8, 8))


def test_foreign_blocks_are_refused_at_plan_build():
    from icafusion_amd.engine import Plan
    for edit in ("dilation", "shortcut", "stem"):
        plan = Plan("cpu", torch.float32)
        if edit == "stem":
            lay = ResNetlayer(3, 64, 1, True, 1).eval()
            lay.layer[2] = torch.nn.SiLU()
            with pytest.raises(NotImplementedError):
                lay.emit(plan, plan.act(1, 8, 8, 4)[..., :3])
        else:
            blk = ResNetblock(64, 64, 1).eval()
            if edit == "dilation":
                blk.conv2 = torch.nn.Conv2d(64, 64, 3, 1, 2, dilation=2, bias=False)
            else:
                blk.shortcut = torch.nn.Sequential(torch.nn.Conv2d(64, 256, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(256))
            with pytest.raises(NotImplementedError):
                blk.emit(plan, plan.act(1, 8, 8, 64))
        assert not plan.launches


def test_root_shim_resolves_and_pickles():
    import models.common as root_common
    assert root_common.ResNetblock is ResNetblock and root_common.ResNetlayer is ResNetlayer
    assert pickle.Unpickler(io.BytesIO(b"")).find_class("models.common", "ResNetlayer") is ResNetlayer
    lay = ResNetlayer(256, 128, 2, False, 4)
    back = pickle.loads(pickle.dumps(lay))
    assert type(back) is ResNetlayer and list(back.state_dict()) == list(lay.state_dict()) and len(back.layer) == 4


def _args(dt, cin, cout, k=1, s=1, res_mode=1, act=ops.ACT_RELU, res=True, hw=20):
    a = ConvArgs()
    a.B, a.H, a.W, a.Cin, a.ldx = 2, hw, hw, cin, cin
    a.Ho = a.Wo = (hw + 2 * (k // 2) - k) // s + 1
    a.Cout, a.ldy, a.ldr = cout, cout, cout
    a.kh = a.kw = k
    a.sh = a.sw = s
    a.ph = a.pw = k // 2
    a.groups, a.act, a.dtype, a.out_dtype = 1, act, dt, dt
    a.Kp = -(-k * k * cin // 64) * 64
    a.alpha_acc[0] = a.alpha_acc[1] = a.alpha_res[0] = a.alpha_res[1] = 1.0
    a.res = 4096 if res else None
    a.res_mode = res_mode
    a.wf = 4096
    return a


@pytest.mark.parametrize("dt", [ops.F32, ops.BF16, ops.F16])
def test_candidates_of_the_residual_in_front_form(dt):
    silu_only = set(range(41, 46)) | {71} | set(range(81, 86))
    for cin, cout, k, s in ((64, 256, 1, 1), (512, 2048, 1, 1), (128, 128, 3, 2)):
        cands = ops.conv_candidates(_args(dt, cin, cout, k, s))
        assert cands and not (set(cands) & silu_only), cands
        assert {2, 12, 22} <= set(cands)
        if dt != ops.F32:
            assert 52 in cands and (cout <= 64 or 61 in cands)
        assert cands == ops.conv_candidates(_args(dt, cin, cout, k, s, res_mode=0))      # the families that run ReLU, no more and no less
    # any other request of the mode has no configuration at all
    assert ops.conv_candidates(_args(dt, 64, 256, act=ops.ACT_SILU)) == []
    assert ops.conv_candidates(_args(dt, 64, 256, res=False)) == []
    assert ops.conv_candidates(_args(dt, 64, 256, res_mode=2)) == []


def test_struct_field_and_header_agree():
    text = open(os.path.join(REPO, "include", "icaf.h")).read()
    assert "int res_mode;" in text and "reserved2" not in text
    import ctypes
    assert ctypes.sizeof(ConvArgs) == 312 and ConvArgs.res_mode.offset == 308
    assert "ICAF_ACT_RELU = 3 }" in text                      # no fifth activation code


def test_synth_gives_the_last_batchnorm_of_a_block_a_small_gain():
    from icafusion_amd.synth import synth_tensor
    w = synth_tensor("model.1.layer.0.bn3.weight", (256,), seed=23)
    assert float(w.min()) >= 0.15 and float(w.max()) <= 0.45
    w = synth_tensor("model.1.layer.0.bn2.weight", (64,), seed=23)
    assert float(w.min()) >= 0.7 and float(w.max()) <= 1.3
