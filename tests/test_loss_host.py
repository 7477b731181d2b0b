"""The validation loss without a GPU: the CPU statement of the rules (tests/loss_ref.py) against everything recorded from the reference's
ComputeLoss (tests/golden/loss, README_loss.md) — assignment and tobj exactly, the loss items against the reference's fp64 run —, the C ABI's
declaration, the refusals of ComputeLoss before any device call, the `--hyp` scaling, and root test.py's loop with the forward, NMS,
matching and the loss replaced by their CPU statements."""
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from helpers import REPO, val_module
import loss_ref
from icafusion_amd import _lib, ops
from icafusion_amd.utils import loss as L

GOLDEN = os.path.join(REPO, "tests", "golden", "loss")
CASES = ("empty", "lattice", "many", "nc1", "nl2_na2", "random_nc3_gr05", "random_nc3_gr1")
HYP_KEYS = ("box", "obj", "cls", "cls_pw", "obj_pw", "anchor_t", "label_smoothing")
# Tolerance of the loss items, relative to the reference's fp64 run (README_loss.md): the largest relative deviation of the reference's OWN
# fp32 run from its fp64 run over all cases and components is 9.815938459275245e-08 (summary.json, random_nc3_gr1 / lobj); the device and the
# CPU statement get 4 x that, for another exp / log1p / atan and another order of summation.  All terms are non-negative: nothing cancels.
REF_FP32_DEV = 9.815938459275245e-08
ITEM_RTOL = 4 * REF_FP32_DEV
# tobj where gr > 0, against the reference's fp64 map: 4 x the largest absolute deviation of its own fp32 map (6.331092486933088e-07, many)
REF_TOBJ_DEV = 6.331092486933088e-07
TOBJ_ATOL = 4 * REF_TOBJ_DEV

_CACHE = {}


def load_case(name):
    """One recorded case as torch tensors: maps, targets, anchors, prm (the parameter dict), gr, per level indices / tbox / anch / tcls /
    tobj / tobj64, items32, items64, counts.  Loaded once and shared: nobody writes into it."""
    if name not in _CACHE:
        g = np.load(os.path.join(GOLDEN, name + ".npz"))
        nl = sum(1 for k in g.files if k.startswith("map"))
        hyp = dict(zip(HYP_KEYS, g["hyp"].tolist()))
        c = {"nl": nl, "maps": [torch.from_numpy(g[f"map{i}"]) for i in range(nl)], "targets": torch.from_numpy(g["targets"]),
             "anchors": torch.from_numpy(g["anchors"]), "hyp": hyp, "gr": float(g["gr"]), "prm": L.loss_params(hyp, float(g["gr"]), nl),
             "items32": g["items32"], "items64": g["items64"], "counts": g["counts"].tolist()}
        for k in ("indices", "tbox", "anch", "tcls", "tobj", "tobj64_"):
            c[k.rstrip("_")] = [g[f"{k}{i}"] for i in range(nl)]
        _CACHE[name] = c
    return _CACHE[name]


def check_items(got, want64, what=""):
    """got (4,) against the reference's fp64 items: each figure is printed before it is judged"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    for k, n in enumerate(("box", "obj", "cls", "rank")):
        rel = abs(got[k] - want64[k]) / abs(want64[k]) if want64[k] != 0 else abs(got[k])
        print(f"{what} {n}: got {got[k]!r} want {want64[k]!r} rel {rel:.3e} (budget {ITEM_RTOL:.3e})")
    for k in range(4):
        assert (got[k] == 0.0) if want64[k] == 0 else abs(got[k] - want64[k]) <= ITEM_RTOL * abs(want64[k]), (what, k, got[k], want64[k])


def check_rows(name, level, b, a, gj, gi, tbox, tcls):
    """the valid slots of one level, in slot order, against the reference's build_targets rows: values and order"""
    c = load_case(name)
    idx = np.stack([np.asarray(v, np.int64) for v in (b, a, gj, gi)], 1).reshape(-1, 4)
    assert idx.tolist() == c["indices"][level].tolist(), (name, level)
    assert np.asarray(tbox, np.float32).reshape(-1, 4).tobytes() == c["tbox"][level].tobytes(), (name, level)
    assert np.asarray(tcls, np.int64).tolist() == c["tcls"][level].tolist(), (name, level)
    assert c["anchors"][level].numpy()[idx[:, 1]].tobytes() == c["anch"][level].tobytes(), (name, level)


def check_tobj(name, level, tobj):
    c = load_case(name)
    tobj = np.asarray(tobj, np.float32)
    if c["gr"] == 0.0:
        assert tobj.tobytes() == c["tobj"][level].tobytes(), (name, level)
    else:
        dev = float(np.abs(tobj.astype(np.float64) - c["tobj64"][level]).max())
        print(f"{name} level {level}: tobj deviation from the fp64 map {dev:.3e} (budget {TOBJ_ATOL:.3e})")
        assert dev <= TOBJ_ATOL and ((tobj != 0) == (c["tobj"][level] != 0)).all(), (name, level, dev)


def test_fixture_set_is_complete_and_the_budget_is_the_recorded_one():
    with open(os.path.join(GOLDEN, "summary.json")) as f:
        summary = json.load(f)
    assert set(summary["cases"]) == set(CASES) and all(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) < 1 << 20 for n in CASES)
    assert summary["max_rel_dev_fp32_vs_fp64"] == REF_FP32_DEV and summary["max_abs_dev_tobj_fp32_vs_fp64"] == REF_TOBJ_DEV
    worst = max(abs(float(a) - b) / abs(b) for n in CASES for a, b in zip(load_case(n)["items32"][:3], load_case(n)["items64"][:3]) if b != 0)
    assert worst == REF_FP32_DEV
    lat, rnd = load_case("lattice"), load_case("random_nc3_gr1")
    assert lat["gr"] == 0.0 and all(m.shape[2] != m.shape[3] for n in CASES for m in load_case(n)["maps"])
    assert (lat["tbox"][0][:, 0] == 1.0).any() and (lat["tbox"][0][:, 1] == 1.0).any()                        # the clamp trap is in the recording
    assert summary["cases"]["random_nc3_gr1"]["duplicate_rows"] > 0 and not (rnd["targets"][:, 0] == 1).any()
    assert load_case("random_nc3_gr05")["gr"] == 0.5 and rnd["hyp"]["label_smoothing"] == 0.1 and rnd["prm"]["cls_pw"] == 0.7 and rnd["prm"]["obj_pw"] == 1.3
    assert load_case("nc1")["items64"][2] == 0.0 and load_case("empty")["counts"] == [0, 0, 0] and len(load_case("many")["targets"]) == 600
    assert load_case("nl2_na2")["nl"] == 2 and load_case("nl2_na2")["maps"][0].shape[1] == 2 and load_case("nl2_na2")["prm"]["balance"] == [4.0, 1.0]
    with open(os.path.join(GOLDEN, "hyp.scratch.yaml")) as f:
        hyp = yaml.safe_load(f)
    assert all(isinstance(v, float) for v in hyp.values()) and {"box", "obj", "cls", "cls_pw", "obj_pw", "anchor_t", "fl_gamma"} <= set(hyp)


@pytest.mark.parametrize("name", CASES)
def test_cpu_statement_equals_the_reference(name):
    c = load_case(name)
    got = loss_ref.compute(c["maps"], c["targets"], c["anchors"], c["prm"])
    assert got["counts"] == c["counts"]
    for i in range(c["nl"]):
        b, a, gj, gi, tbox, tcls = loss_ref.rows(got["levels"][i])
        check_rows(name, i, b.numpy(), a.numpy(), gj.numpy(), gi.numpy(), tbox.numpy(), tcls.numpy())
        check_tobj(name, i, got["tobj"][i].numpy())
    check_items(got["items"].numpy(), c["items64"], name)


def test_header_declares_the_entry_points_with_their_citations():
    with open(os.path.join(REPO, "include", "icaf.h")) as f:
        header = f.read()
    assert "int icaf_loss_workspace_bytes(int nl, ICAF_HOST const int* ny, ICAF_HOST const int* nx, int B, int na, int nt, ICAF_HOST size_t* bytes, ICAF_HOST size_t* tobj_off, ICAF_HOST size_t* slots_off);" in header
    assert "int icaf_loss(ICAF_HOST const float* const* maps, ICAF_HOST const int* ny, ICAF_HOST const int* nx, int nl, int B, int na, int nc, ICAF_HOST const float* anchors," in header
    assert "double box, obj, cls, cls_pw, obj_pw, anchor_t, gr, cp, cn, balance[5];" in header
    block = header[header.index("---- Validation loss"):header.index("int icaf_loss_workspace_bytes(")]
    for cite in ("utils/loss.py:325-463", ":409-463", ":362-388", ":379-382", ":457", ":458", "utils/general.py:410-452", "SLOT LAYOUT", "(off * na + a) * nt + t",
                 "DUPLICATE RULE", "CLAMP TRAP", "REFUSALS", "ICAF_LOSS_MAX_TARGETS = 4096", "no gradient", "gr outside [0, 1]"):
        assert cite in block, cite
    assert len(_lib.SIGNATURES["icaf_loss"][1]) == 16 and len(_lib.SIGNATURES["icaf_loss_workspace_bytes"][1]) == 9
    fields = [n for n, _ in _lib.LossParams._fields_]
    assert fields == ["box", "obj", "cls", "cls_pw", "obj_pw", "anchor_t", "gr", "cp", "cn", "balance"] and ctypes.sizeof(_lib.LossParams) == 14 * 8
    assert (ops.LOSS_MAX_LEVELS, ops.LOSS_MAX_ANCHORS, ops.LOSS_MAX_TARGETS, ops.LOSS_SLOT_INTS) == (5, 8, 4096, 10)
    assert "ICAF_LOSS_MAX_LEVELS = 5, ICAF_LOSS_MAX_ANCHORS = 8, ICAF_LOSS_MAX_TARGETS = 4096, ICAF_LOSS_SLOT_INTS = 10" in header
    from icafusion_amd import build
    assert build.PER_FILE["loss.hip"] == ["-ffp-contract=off"] and build.NO_SCRATCH.search("icaf::loss_assign_kernel(")
    blk = ops.loss_params_block(load_case("random_nc3_gr05")["prm"])
    assert (blk.gr, blk.cls_pw, blk.cp, blk.cn, list(blk.balance)) == (0.5, 0.7, 0.95, 0.05, [4.0, 1.0, 0.4, 0.0, 0.0])


class FakeDetect:
    na, nc, nl = 3, 1, 3
    anchors = torch.ones((3, 3, 2))


class FakeLossModel:
    def __init__(self, gr=1.0, **hyp):
        self.hyp = dict({"box": 0.05, "obj": 1.0, "cls": 0.5, "cls_pw": 1.0, "obj_pw": 1.0, "anchor_t": 4.0, "fl_gamma": 0.0}, **hyp)
        self.gr, self.model = gr, [FakeDetect()]


def test_compute_loss_refusals_come_before_any_device_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device call")
    monkeypatch.setattr(ops, "LossRunner", boom)
    monkeypatch.setattr(ops, "loss_launch", boom)
    monkeypatch.setattr(ops, "lib", boom)
    with pytest.raises(NotImplementedError, match="focal"):
        L.ComputeLoss(FakeLossModel(fl_gamma=1.5))
    with pytest.raises(NotImplementedError, match="autobalance"):
        L.ComputeLoss(FakeLossModel(), autobalance=True)
    for gr in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"gr must be in \[0, 1\]"):
            L.ComputeLoss(FakeLossModel(gr=gr))
    cl = L.ComputeLoss(FakeLossModel())
    assert (cl.na, cl.nc, cl.nl, cl.gr, cl.cp, cl.cn, cl.balance) == (3, 1, 3, 1.0, 1.0, 0.0, [4.0, 1.0, 0.4])
    maps = [torch.zeros((1, 3, 2, 3, 6))] * 3
    with pytest.raises(RuntimeError, match=r"MI355X only \(no CPU fallback"):
        cl(maps, torch.zeros((2, 6)))
    with pytest.raises(ValueError, match="4097 targets exceed the cap of 4096"):
        cl(maps, torch.zeros((4097, 6)))
    with pytest.raises(ValueError, match=r"\(nt, 6\)"):
        cl(maps, torch.zeros((2, 5)))
    with pytest.raises(ValueError, match="2 maps for a head of 3 levels"):
        cl(maps[:2], torch.zeros((2, 6)))
    assert L.smooth_BCE(0.1) == (0.95, 0.05) and L.smooth_BCE(0.0) == (1.0, 0.0)
    assert L.loss_params(FakeLossModel().hyp, 1.0, 2)["balance"] == [4.0, 1.0] and len(L.loss_params(FakeLossModel().hyp, 1.0, 5)["balance"]) == 5


def test_hyp_flag_and_its_scaling():
    val = val_module()
    assert val.parse_opt([]).hyp is None and val.parse_opt(["--hyp", "h.yaml"]).hyp == "h.yaml"
    assert inspect.signature(val.test).parameters["compute_loss"].default is None
    with open(os.path.join(GOLDEN, "hyp.scratch.yaml")) as f:
        hyp = yaml.safe_load(f)
    before = dict(hyp)
    got = L.scale_hyp(hyp, nl=3, nc=1, imgsz=640)
    assert hyp == before                                            # the caller's dict is left alone
    assert got["box"] == 0.05 * (3.0 / 3) and got["cls"] == 0.5 * (1 / 80.0 * 3.0 / 3) and got["obj"] == 1.0 * ((640 / 640) ** 2 * 3.0 / 3)
    assert got["label_smoothing"] == 0.0 and got["anchor_t"] == 4.0
    got = L.scale_hyp(hyp, nl=2, nc=3, imgsz=512)
    assert got["box"] == 0.05 * (3.0 / 2) and got["cls"] == 0.5 * (3 / 80.0 * 3.0 / 2) and got["obj"] == 1.0 * ((512 / 640) ** 2 * 3.0 / 2)

    class M:
        model = [FakeDetect()]
    m = M()
    cl = val.loss_from_hyp(os.path.join(GOLDEN, "hyp.scratch.yaml"), m, nc=1, imgsz=320)
    assert m.gr == 1.0 and m.hyp["obj"] == 0.25 and m.hyp["cls"] == 0.5 * (1 / 80.0 * 3.0 / 3) and cl.params["obj"] == 0.25 and cl.params["gr"] == 1.0


def test_validation_loop_on_cpu_reports_the_loss_of_the_cpu_statement(tmp_path, monkeypatch):
    """Root test.py's loop with the forward, NMS and TP matching replaced by their CPU oracle statements (the pattern of
    test_result_files.test_validation_loop_on_cpu_with_the_oracle_behind_it) and the loss by tests/loss_ref.py: the three trailing values are the
    mean over the batches of the statement's items on the very maps and (still normalised) targets of each batch; without compute_loss they
    are 0.0 and the metrics are the same."""
    from test_frontends import make_dataset
    from icafusion_amd.models.yolo import Model
    from icafusion_amd.synth import synth_state_dict
    from icafusion_amd.utils import datasets as D
    from icafusion_amd.utils.general import scale_coords
    from icafusion_amd.utils.metrics import match_predictions
    sys.path.insert(0, REPO)
    from oracle import icaf_oracle as oracle
    val = val_module()
    rgb_dir, ir_dir = make_dataset(str(tmp_path / "set"), n=3, size=(120, 128), nc=3, seed=5)
    cfg = yaml.safe_load(open(os.path.join(REPO, "models", "transformer", "yolov5s_Transfusion_FLIR.yaml")))
    model = Model(cfg)
    om = oracle.OracleModel(cfg, synth_state_dict(model, seed=0))
    det = model.model[-1]
    anchors = det.anchors.detach().float().clone()
    hyp = L.scale_hyp(yaml.safe_load(open(os.path.join(GOLDEN, "hyp.scratch.yaml"))), det.nl, 3, 320)
    prm = L.loss_params(hyp, 1.0, det.nl)
    calls = []

    class FakeModel:
        stride = torch.tensor([8.0, 16.0, 32.0])

        def parameters(self):
            yield torch.zeros(1)

        def forward_u8(self, img6):
            f = img6.float() / 255.0
            return om.forward(f[:, :3].contiguous(), f[:, 3:].contiguous())

    def cpu_loss(p, targets):
        got = loss_ref.compute([m.float() for m in p], targets, anchors, prm)
        calls.append((targets.clone(), got["items"].clone(), p[0].shape[0]))
        return got["items"].sum().view(1) * p[0].shape[0], got["items"].float()

    def fake_nms(out, conf_thres, iou_thres, multi_label=False, agnostic=False, **kw):
        dets = oracle.non_max_suppression(out.numpy(), conf_thres, iou_thres, multi_label=multi_label, agnostic=agnostic)
        det_ = torch.zeros((len(dets), 300, 6))
        for i, d in enumerate(dets):
            det_[i, :len(d)] = torch.from_numpy(d)
        return det_, torch.tensor([len(d) for d in dets], dtype=torch.int32), None

    def fake_match(det_, count, labels, label_off, iouv, scale=None, predn=None, stream_ptr=None):
        correct = torch.zeros((det_.shape[0], 300, iouv.numel()), dtype=torch.uint8)
        for b in range(det_.shape[0]):
            n = int(count[b])
            d = det_[b, :n].clone()
            gain, px, py, w0, h0 = scale[b].tolist()
            scale_coords(None, d[:, :4], (h0, w0), ((gain, gain), (px, py)))
            lab = labels[int(label_off[b]):int(label_off[b + 1])]
            correct[b, :n] = torch.from_numpy(match_predictions(d.numpy(), lab.numpy(), iouv.numpy()).astype(np.uint8))
        return correct

    monkeypatch.setattr(val, "nms_device", fake_nms)
    monkeypatch.setattr(val.ops, "match_predictions", fake_match)
    data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 3, "names": ["person", "car", "bicycle"]}
    plain = val.test(data, batch_size=2, imgsz=320, conf_thres=0.3, model=FakeModel())
    assert plain[0][4:] == (0.0, 0.0, 0.0) and not calls
    res = val.test(data, batch_size=2, imgsz=320, conf_thres=0.3, model=FakeModel(), compute_loss=cpu_loss)
    assert res[0][:4] == plain[0][:4] and np.array_equal(res[1], plain[1]) and len(res) == 3 and len(res[0]) == 7
    loader, _ = D.create_dataloader_rgb_ir(rgb_dir, ir_dir, 320, 2, 32, None, pad=0.5, rect=True)
    batches = [t for _, t, _, _ in loader]
    assert len(calls) == len(batches) == 2
    for (seen, _, _), want in zip(calls, batches):
        assert torch.equal(seen, want) and float(want[:, 2:].max()) <= 1.0          # the loader's normalised labels: before the pixel scaling
    want = torch.stack([c[1][:3].float() for c in calls]).sum(0) / len(batches)
    assert all(w > 0 for w in want.tolist()) and res[0][4:] == pytest.approx(tuple(want.tolist()), rel=1e-6)
