"""The validation loss on the MI355X (csrc/loss.hip, icaf_loss) against everything recorded from the reference's ComputeLoss
(tests/golden/loss) and the CPU statement pinned to the same recordings (tests/loss_ref.py, tests/test_loss_host.py).
Exact: the slot table read in slot order is build_targets' rows, values and order; the per-level counts; tobj for gr = 0.
Values: the four outputs against the reference's fp64 run within 4 x the reference's own fp32-vs-fp64 deviation (test_loss_host.ITEM_RTOL =
4 x 9.815938459275245e-08, README_loss.md); tobj for gr > 0 against the reference's fp64 map (TOBJ_ATOL)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import REPO, load_cfg                                                   # noqa: E402
import loss_ref                                                                      # noqa: E402
from numerics import F32, INF_BITS, NAN_BITS, PoisonedFlat, bits                     # noqa: E402
from test_loss_host import CASES, GOLDEN, ITEM_RTOL, check_items, check_rows, check_tobj, load_case      # noqa: E402
from icafusion_amd import ops                                                        # noqa: E402
from icafusion_amd.synth import synth_state_dict                                     # noqa: E402
from icafusion_amd.utils import loss as L                                            # noqa: E402

DEV = "cuda:0"
ERR_ARG, ERR_UNSUPPORTED = -1, -3
_RUNS = {}


class Launch:
    """One icaf_loss call on a recorded case with every buffer in the middle of a poisoned one: inputs (maps, targets) with their content,
    outputs (out, counts) and the workspace filled with `fill` (a NaN or an infinity pattern) beforehand."""

    def __init__(self, name, fill=NAN_BITS[F32], **override):
        c = load_case(name)
        self.c, self.name = c, name
        self.shapes = [(m.shape[2], m.shape[3]) for m in c["maps"]]
        self.B, self.na, self.nc, self.nt = c["maps"][0].shape[0], c["maps"][0].shape[1], c["maps"][0].shape[4] - 5, c["targets"].shape[0]
        self.nbytes, self.tobj_off, self.slots_off = ops.loss_workspace(self.shapes, self.B, self.na, self.nt)
        self.maps = [PoisonedFlat(tuple(m.shape), F32, DEV, fill, content=m.to(DEV)) for m in c["maps"]]
        targets = override.pop("targets", c["targets"])
        self.targets = PoisonedFlat(tuple(targets.shape), F32, DEV, fill, content=targets.to(DEV))
        self.out, self.counts = PoisonedFlat((4,), F32, DEV, fill), PoisonedFlat((c["nl"],), F32, DEV, fill)
        self.ws = PoisonedFlat((self.nbytes // 4,), F32, DEV, fill)
        assert self.ws.view.data_ptr() % 256 == 0
        prm = dict(c["prm"], **override.pop("prm", {}))
        ptrs = [m.view.data_ptr() for m in self.maps]
        for i in override.pop("null_maps", ()):
            ptrs[i] = 0
        self.status = ops.loss_launch(ptrs, self.shapes, self.B, override.pop("na", self.na), self.nc, c["anchors"].numpy(), self.targets.view, prm,
                                      self.out.view, self.counts.view.view(torch.int32), self.ws.view.view(torch.uint8), **override)
        torch.cuda.synchronize()

    def tobj(self, i):
        ny, nx = self.shapes[i]
        o = self.tobj_off[i] // 4
        return self.ws.view[o:o + self.B * self.na * ny * nx].view(self.B, self.na, ny, nx)

    def slots(self, i):
        o = self.slots_off[i] // 4
        return self.ws.view[o:o + 5 * self.na * self.nt * ops.LOSS_SLOT_INTS].view(torch.int32).view(5 * self.na * self.nt, ops.LOSS_SLOT_INTS)

    def guards_intact(self):
        for p in self.maps + [self.targets, self.out, self.counts, self.ws]:
            p.assert_outside_intact(self.name)

    def untouched(self):
        """outputs and workspace still hold the poison"""
        return all(bool((bits(p.view) == bits(p.before[p.g:p.g + p.n].view(p.view.shape))).all()) for p in (self.out, self.counts, self.ws))


def run(name):
    """the case's two launches (NaN-poisoned, then infinity-poisoned buffers), made once and shared by the tests"""
    if name not in _RUNS:
        _RUNS[name] = (Launch(name), Launch(name, fill=INF_BITS[F32]))
        assert _RUNS[name][0].status == 0 and _RUNS[name][1].status == 0, ops.lib().icaf_last_error()
    return _RUNS[name]


@pytest.mark.parametrize("name", CASES)
def test_assignment_counts_and_tobj_equal_the_reference(name):
    r, _ = run(name)
    c = r.c
    assert r.counts.view.view(torch.int32).tolist() == c["counts"]
    for i in range(c["nl"]):
        rec = r.slots(i).cpu().numpy()
        valid = rec[:, 0] == 1
        assert set(np.unique(rec[:, 0]).tolist()) <= {0, 1} and not rec[~valid].any()            # a slot is valid or all zero: no poison is left
        rows = rec[valid]                                                                        # slot order IS the reference's row order
        check_rows(name, i, rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5:9].copy().view(np.float32), rows[:, 9])
        check_tobj(name, i, r.tobj(i).cpu().numpy())


@pytest.mark.parametrize("name", CASES)
def test_loss_items_against_the_fp64_reference(name):
    r, _ = run(name)
    check_items(r.out.view.cpu().numpy(), r.c["items64"], name)


@pytest.mark.parametrize("name", CASES)
def test_two_launches_give_the_same_bits_and_stay_inside_their_buffers(name):
    a, b = run(name)
    assert torch.equal(bits(a.out.view), bits(b.out.view)) and torch.equal(bits(a.counts.view), bits(b.counts.view))
    for i in range(a.c["nl"]):
        assert torch.equal(bits(a.tobj(i)), bits(b.tobj(i))) and torch.equal(a.slots(i), b.slots(i))
    for r in (a, b):
        r.guards_intact()
        assert not torch.isnan(r.out.view).any() and not torch.isinf(r.out.view).any()
        for p, m in zip(r.maps, r.c["maps"]):                                                   # the inputs are read only
            assert torch.equal(bits(p.view), bits(m.to(DEV)))
        assert torch.equal(bits(r.targets.view), bits(r.c["targets"].to(DEV)))


@pytest.mark.parametrize("what, kw, code, words", [
    ("nl = 6", {"nl": 6}, ERR_UNSUPPORTED, "nl must be in [1, 5]"),
    ("na = 9", {"na": 9}, ERR_UNSUPPORTED, "na must be in [1, 8]"),
    ("nt = 4097", {"targets": torch.zeros((4097, 6))}, ERR_UNSUPPORTED, "at most 4096 targets"),
    ("null map", {"null_maps": (1,)}, ERR_ARG, "null map of level 1"),
    ("gr above 1", {"prm": {"gr": 1.5}}, ERR_ARG, "gr must be in [0, 1]"),
    ("gr below 0", {"prm": {"gr": -0.25}}, ERR_ARG, "gr must be in [0, 1]"),
    ("gr NaN", {"prm": {"gr": float("nan")}}, ERR_ARG, "gr must be in [0, 1]"),
    ("short workspace", {"ws_bytes": 256}, ERR_ARG, "workspace needs"),
])
def test_refusals_come_before_any_launch(what, kw, code, words):
    r = Launch("nc1", **kw)
    assert r.status == code and words in ops.lib().icaf_last_error().decode(), (what, r.status, ops.lib().icaf_last_error())
    assert r.untouched(), what
    r.guards_intact()


def kaist_model():
    from icafusion_amd.models.yolo import Model
    m = Model(load_cfg("yolov5s_Transfusion_kaist.yaml")).eval()
    m.load_state_dict(synth_state_dict(m, 0))
    m = m.to(DEV)
    m.compute_dtype, m.autotune, m.use_graph = torch.bfloat16, False, True
    return m


def statement(model, maps, targets):
    """tests/loss_ref.py on host copies of the maps, with the model's own parameters"""
    det = model.model[-1]
    got = loss_ref.compute([m.float().cpu() for m in maps], targets.float().cpu(), det.anchors.detach().float().cpu(),
                           L.loss_params(model.hyp, model.gr, det.nl))
    return got["items"].numpy()


def test_compute_loss_on_the_maps_of_a_forward():
    """yolov5s_Transfusion_kaist, synthetic weights, B = 2 at 320 x 352 — the smallest H != W input the model takes: its DMFF blocks pool to
    20 x 20 / 16 x 16 / 10 x 10 tokens at strides 8 / 16 / 32 and refuse smaller maps, so 128 x 160 cannot run —: ComputeLoss(model)(out[2],
    targets) against the CPU statement on the same maps; the runner is reused for the next call and a batch without labels takes the
    nt = 0 branch"""
    import yaml
    model = kaist_model()
    model.hyp = L.scale_hyp(yaml.safe_load(open(os.path.join(GOLDEN, "hyp.scratch.yaml"))), 3, 1, 352)
    model.gr = 1.0
    g = torch.Generator().manual_seed(4)
    img = torch.randint(0, 256, (2, 6, 320, 352), generator=g, dtype=torch.uint8).to(DEV)
    targets = torch.tensor([[0, 0, 0.3, 0.4, 0.2, 0.5], [0, 0, 0.7, 0.55, 0.1, 0.3], [1, 0, 0.5, 0.5, 0.4, 0.6], [1, 0, 0.52, 0.5, 0.35, 0.7]]).to(DEV)
    cl = L.ComputeLoss(model)
    out = model.forward_u8(img)
    total, items = cl(out[2], targets)
    assert items.shape == (4,) and items.is_cuda and total.shape == (1,) and float(total) == pytest.approx(float(items.sum()) * 2, rel=1e-6)
    check_items(items.cpu().numpy(), statement(model, out[2], targets), "forward")
    assert all(float(v) > 0 for v in items[:2]) and float(items[2]) == 0.0 and float(items[3]) == 0.0        # nc = 1: no class loss
    runners = dict(cl._runners)
    total0, items0 = cl(out[2], targets[:0])
    assert cl._runners == runners and float(items0[0]) == 0.0 and float(items0[1]) > 0
    check_items(items0.cpu().numpy(), statement(model, out[2], targets[:0]), "no labels")


@pytest.mark.parametrize("device_letterbox", [False, True], ids=["host-loader", "device-letterbox"])
def test_validation_loop_reports_the_loss(tmp_path, device_letterbox):
    """root test() over four 120 x 128 / 128 x 120 pairs at img-size 320 (batches of 320 x 352 and 352 x 320, the smallest the model's DMFF
    blocks take) with the loss built as `--hyp` builds it: the three trailing values are non-zero and
    equal the mean over the batches of the CPU statement on the maps each batch produced; precision, recall, mAP and maps are those of a
    run without the loss"""
    from test_frontends import make_dataset
    from helpers import val_module
    val = val_module()
    rgb_dir, ir_dir = make_dataset(str(tmp_path / "set"), n=4, size=(120, 128), nc=1, seed=3)
    data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 1, "names": ["person"]}
    model = kaist_model()
    plain = val.test(data, batch_size=2, imgsz=320, conf_thres=0.05, model=model, device_letterbox=device_letterbox)
    assert plain[0][4:] == (0.0, 0.0, 0.0)
    cl = val.loss_from_hyp(os.path.join(GOLDEN, "hyp.scratch.yaml"), model, 1, 320)
    seen = []

    def spy(p, targets):
        seen.append(statement(model, p, targets)[:3])
        assert float(targets[:, 2:].max()) <= 1.0                  # normalised: before the labels are scaled to pixels
        return cl(p, targets)
    res = val.test(data, batch_size=2, imgsz=320, conf_thres=0.05, model=model, device_letterbox=device_letterbox, compute_loss=spy)
    assert res[0][:4] == plain[0][:4] and np.array_equal(res[1], plain[1]) and len(res) == 3 and len(res[0]) == 7
    assert len(seen) == 2
    want = np.mean(seen, 0)
    print("loss", res[0][4:], "statement", want.tolist())
    assert want[0] > 0 and want[1] > 0 and want[2] == 0.0 and res[0][4] > 0 and res[0][5] > 0
    # the loop sums fp32 items of two batches: one fp32 rounding each on top of the kernel's budget
    assert np.allclose(res[0][4:6], want[:2], rtol=ITEM_RTOL + 3 * 2.0 ** -24, atol=0.0) and res[0][6] == 0.0
