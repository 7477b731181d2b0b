"""The convolution family's one launch builder (models/common.py: emit_conv) and its two records, on CPU plans: what every caller refuses and
with which exception, the image-fed first layer of the three backbones, and the chained fields a C3 records with and without a deferred lead."""
import pytest
import torch
import torch.nn as nn

from icafusion_amd import ops
from icafusion_amd.engine import ImageIn, Plan
from icafusion_amd.models.common import C3, Chained, Conv, Lead, NiNfusion, ResNetblock, ResNetlayer, VGGblock

BF16 = torch.bfloat16
CASES = {"channels": ValueError, "vector": NotImplementedError, "groups": NotImplementedError, "dilation": NotImplementedError}


def odd_conv(case, c1, c2, k, s=1, bias=False):
    """The Conv2d of a refusal case: twice the input channels, two groups, or dilation 2 (the padding keeps the output size)."""
    if case == "channels":
        return nn.Conv2d(2 * c1, c2, k, s, k // 2, bias=bias)
    return nn.Conv2d(c1, c2, k, s, k // 2 * (2 if case == "dilation" else 1), groups=2 if case == "groups" else 1,
                     dilation=2 if case == "dilation" else 1, bias=bias)


def refused_conv(plan, case):
    m = Conv(4, 8, 3) if case == "vector" else Conv(16, 16, 3)
    if case != "vector":
        m.conv = odd_conv(case, 16, 16, 3)
    return lambda: m.emit(plan, plan.act(1, 4, 4, 4 if case == "vector" else 16))


def refused_nin(plan, case):
    c = 4 if case == "vector" else 16
    m = NiNfusion(c, 16, 3)
    if case != "vector":
        m.conv = odd_conv(case, c, 16, 3)
    buf = plan.act(1, 4, 4, c)                           # the two streams as adjacent slices: the Concat in front launches nothing
    return lambda: m.emit(plan, [buf[..., :c // 2], buf[..., c // 2:]])


def refused_vgg(plan, case):
    m = VGGblock(2, 8, 4) if case == "vector" else VGGblock(2, 8, 8)           # the SECOND convolution is the odd one
    if case != "vector":
        m.vggblock[1][0] = odd_conv(case, 8, 8, 3, bias=True)
    return lambda: m.emit(plan, plan.act(1, 4, 4, 8))


def refused_resnetblock(plan, case):
    m = ResNetblock(4, 4) if case == "vector" else ResNetblock(16, 8)
    if case == "channels":
        return lambda: m.emit(plan, plan.act(1, 4, 4, 8))
    if case != "vector":
        m.conv2 = odd_conv(case, 8, 8, 3)
    return lambda: m.emit(plan, plan.act(1, 4, 4, 4 if case == "vector" else 16))


def refused_resnet_stem(plan, case):
    m = ResNetlayer(4 if case == "vector" else 8, 16, 1, True)
    if case != "vector":
        m.layer[0] = odd_conv(case, 8, 16, 7, 2)
    return lambda: m.emit(plan, plan.act(1, 4, 4, 4 if case == "vector" else 8))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("caller", [refused_conv, refused_nin, refused_vgg, refused_resnetblock, refused_resnet_stem], ids=lambda f: f.__name__[8:])
def test_refusals_keep_their_type_and_append_nothing(caller, case):
    """A wrong channel count is ValueError; a width that is no whole number of 16-byte vectors (4 channels in bf16), groups = 2 and
    dilation = 2 are NotImplementedError — through every emitter, and before its first launch."""
    plan = Plan("cpu", BF16)
    emit = caller(plan, case)
    with pytest.raises(CASES[case]) as e:
        emit()
    assert type(e.value) is CASES[case] and plan.launches == []


def image(form):
    if form == "u8 paired":
        return ImageIn(torch.zeros((1, 6, 8, 8), dtype=torch.uint8), pair=True)
    return ImageIn(torch.zeros((2, 1, 3, 8, 8) if form == "fp32 paired" else (1, 3, 8, 8)))


def first_layers():
    def stem():
        m = Conv(3, 32, 6, 2, 2)
        m.fuse_stem = False
        return m
    return {"Conv": (stem, "conv3x3s1", True), "VGGblock": (lambda: VGGblock(2, 3, 64), "vgg_conv3x3", False),
            "ResNetlayer": (lambda: ResNetlayer(3, 64, 1, True), "resnet_stem7x7s2", False)}


@pytest.mark.parametrize("dt", [BF16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("form", ["fp32", "fp32 paired", "u8 paired"])
@pytest.mark.parametrize("kind", ["Conv", "VGGblock", "ResNetlayer"])
def test_image_fed_first_layer_is_staged_once_then_convolved(kind, form, dt):
    make, name, s2d = first_layers()[kind]
    paired = form != "fp32"
    plan = Plan("cpu", dt)
    make().eval().emit(plan, image(form), **({"twin": make().eval()} if paired else {}))
    pre, conv = plan.launches[:2]
    assert sum(l.name.startswith("preprocess") for l in plan.launches) == 1
    assert pre.name == ("preprocess_u8_" if form == "u8 paired" else "preprocess_") + ("s2d" if s2d else "pad")
    assert conv.name == name and conv.fn is ops.lib().icaf_conv2d
    assert sum(l.fn is ops.lib().icaf_conv2d for l in plan.launches) == (2 if kind == "VGGblock" else 1)
    a, staged = conv.keep[0], conv.keep[1]
    vec = ops.VEC[dt]
    assert a.x == staged.data_ptr() == pre.keep[1].data_ptr()                 # (ops.preprocess keeps a pair act as one act of batch 2B)
    assert a.Cin == staged.shape[-1] == (-(-12 // vec) * vec if s2d else vec) and (not s2d or dt is not BF16 or a.Cin == 16)
    assert a.groups == (2 if paired else 1) and (staged.dim() == 5) == paired
    assert (a.kh, a.sh, a.ph) == {"Conv": (3, 1, 1), "VGGblock": (3, 1, 1), "ResNetlayer": (7, 2, 3)}[kind]


# launch name, Cout2, chain_keep, whether x2 is set — per launch of Conv(c, c, 3, 2) + C3(c, c, n=2) on a 1 x 4 x 4 map behind the Conv
C3_BODY_64 = [("conv1x1s1", 0, 0, False), ("conv3x3s1", 0, 0, False), ("conv1x1s1", 0, 0, False), ("conv3x3s1", 0, 0, False), ("conv1x1s1", 0, 0, False)]
# 128-wide Bottlenecks: the first 3x3 carries the second's 1x1 and keeps its own output, the second carries cv3 over [m | cv2]
C3_BODY_256 = [("conv1x1s1", 0, 0, False), ("conv3x3s1+1x1", 128, 1, False), ("conv3x3s1+cv3", 256, 0, True)]
RECORDS = {(64, True): [("conv3x3s2+1x1", 64, 0, False)] + C3_BODY_64,
           (64, False): [("conv3x3s2", 0, 0, False), ("conv1x1s1", 0, 0, False)] + C3_BODY_64,
           (256, True): [("conv3x3s2+1x1", 256, 0, False)] + C3_BODY_256,
           (256, False): [("conv3x3s2", 0, 0, False), ("conv1x1s1", 0, 0, False)] + C3_BODY_256}


@pytest.mark.parametrize("c,with_lead", list(RECORDS))
def test_c3_records_the_chained_fields(c, with_lead):
    down, c3 = Conv(c, c, 3, 2).eval(), C3(c, c, 2).eval()
    plan = Plan("cpu", BF16)
    x = plan.act(1, 8, 8, c)
    y = c3.emit(plan, x, lead=Lead(down)) if with_lead else c3.emit(plan, down.emit(plan, x))
    assert tuple(y.shape) == (1, 4, 4, c)
    got = [(l.name, l.keep[0].Cout2, l.keep[0].chain_keep, bool(l.keep[0].x2)) for l in plan.launches]
    assert got == RECORDS[c, with_lead]
    assert all((l.keep[7] is not None) == bool(l.keep[0].w2) for l in plan.launches)          # ops.conv2d: keep[7] = the ops.Chain it was given


def test_records_have_defaults_and_say_what_they_are():
    a, b = Conv(8, 8, 1), Conv(8, 8, 1)
    assert Chained((a,)) == Chained((a,), None, None, False, None) and ops.Chain(1, 2, 3, 4, 5) == ops.Chain(1, 2, 3, 4, 5, False, None)
    rec = ops.Chain.of(dict(w=1, kp=2, bias=3, y=4, cout=5, x2=6))           # the kernel tests' spelling of a chain= argument
    assert rec == ops.Chain(1, 2, 3, 4, 5, False, 6) and ops.Chain.of(rec) is rec and ops.Chain.of(None) is None
    assert rec["y"] == rec.y == rec[3] == 4 and list(rec) == [1, 2, 3, 4, 5, False, 6]
    assert not Lead(a).from_image and not Lead(a, b).from_image and Lead(a, b, a, b).from_image
    assert Lead(a, b, a, b) == (a, b, a, b) and Lead(a) == (a, None, None, None)
