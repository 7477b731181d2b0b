"""icaf_nms_ex on the device — apriori labels (test.py --save-hybrid) and merge-NMS — against the numpy restatement tests/nms_modes_ref.py,
which tests/test_nms_modes_host.py pins to the reference's own results: det and count bit for bit, keep_idx exactly, the rows behind count as
the call without merge leaves them.  The cases are nms_modes_ref.cases(): B = 3 (5 for the candidate counts), rows = 4096 + 37."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import REPO, load_cfg                                          # noqa: E402
import nms_modes_ref as R                                                   # noqa: E402
from icafusion_amd import _lib, ops                                         # noqa: E402
from icafusion_amd.utils.general import nms_device, non_max_suppression    # noqa: E402

DEV = "cuda:0"
CASES = R.cases()
_WANT = {}
SENTINEL = -77.25                                                           # what the output block holds before a launch


def want(name, redundant=True):
    """the restatement's answer, computed once per (case, redundant)"""
    if (name, redundant) not in _WANT:
        _WANT[name, redundant] = R.run_case(CASES[name], redundant=redundant)
    return _WANT[name, redundant]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def launch(c, merge=None, redundant=True, max_labels=None, poison=False, runner=None):
    """One NmsRunner of its own per call, output block pre-filled -> (det, count, keep) as numpy, the runner"""
    pred, labels, kw = c["pred"], c["labels"], dict(c["kw"])
    B, rows, no = pred.shape
    merge = c["merge"] if merge is None else merge
    table = off = None
    if labels is not None:
        table, off, most = ops.nms_label_table(labels, B, no - 5, max_labels, device=DEV)
        max_labels = most if max_labels is None else max_labels
    if runner is None:
        runner = ops.NmsRunner(B, rows, no - 5, DEV, kw.get("multi_label", False), max_labels=max_labels or 0, merge=merge)
    runner.det.fill_(SENTINEL); runner.count.fill_(-5); runner.keep.fill_(-9)
    if poison:                                                              # NaN bytes everywhere the call may read before it writes
        runner.ws.fill_(0xFF); runner.det.view(torch.int32).fill_(-1); runner.count.fill_(-1); runner.keep.fill_(-1)
    det, count, keep = runner.launch(torch.from_numpy(pred).to(DEV), kw["conf_thres"], kw["iou_thres"], kw.get("agnostic", False),
                                     kw.get("classes"), labels=table, label_off=off, redundant=redundant)
    torch.cuda.synchronize()
    return det.cpu().numpy(), count.cpu().numpy(), keep.cpu().numpy(), runner


def check(name, got, redundant=True):
    det, count, keep, _ = got
    rows, idx, ns = want(name, redundant)
    for b in range(len(rows)):
        n = int(count[b])
        assert n == len(rows[b]), (name, b, n, len(rows[b]), ns[b])
        assert np.array_equal(bits(det[b, :n]), bits(rows[b])), (name, b)
        assert keep[b, :n].tolist() == idx[b].tolist(), (name, b)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_restatement(name):
    """every case the fixtures were recorded for: bit-exact rows, exact indices; behind count the rows of the same call without merge (which,
    like icaf_nms, leaves the block untouched behind ITS count); a second launch and a launch into poisoned buffers give the same bits"""
    c = CASES[name]
    got = launch(c)
    check(name, got)
    det, count, keep, runner = got
    base = launch(c, merge=False)
    for b in range(c["pred"].shape[0]):
        n, nb = int(count[b]), int(base[1][b])
        assert n <= nb
        assert np.array_equal(bits(det[b, n:]), bits(base[0][b, n:])) and np.array_equal(keep[b, n:], base[2][b, n:])
        assert (base[0][b, nb:] == SENTINEL).all() and (base[2][b, nb:] == -9).all()
    again = launch(c, runner=runner)
    assert np.array_equal(bits(again[0]), bits(det)) and np.array_equal(again[1], count) and np.array_equal(again[2], keep)
    check(name, launch(c, poison=True))


def test_redundant_off_keeps_the_isolated_boxes():
    """redundant = 0: every kept box stays, merged; the zero-area box comes out as 0 / 0 = NaN"""
    for name in ("merge_nc1", "merge_nc3_agnostic", "merge_labels"):
        got = launch(CASES[name], redundant=False)
        check(name, got, redundant=False)
        plain = launch(CASES[name], merge=False)
        assert np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])
    det, count, _, _ = launch(CASES["merge_nc1"], redundant=False)
    assert np.isnan(det[2, :count[2], :4]).any(1).sum() == 1 and not np.isnan(det[0, :count[0]]).any()


def test_counts_on_both_sides_of_the_merge_limit():
    """n = 0, 1, 2, 2999, 3000: at 3000 (and at 1) the output is plain NMS bit for bit, at 2999 it is not"""
    c = CASES["merge_counts"]
    det, count, keep, _ = launch(c)
    plain = launch(c, merge=False)
    assert want("merge_counts")[2] == [0, 1, 2, 2999, 3000]
    for b in (0, 1, 4):
        assert count[b] == plain[1][b] and np.array_equal(bits(det[b]), bits(plain[0][b])) and np.array_equal(keep[b], plain[2][b])
    assert count[4] == 300 and not np.array_equal(bits(det[3, :count[3]]), bits(plain[0][3, :count[3]]))


def test_max_labels_exactly_met_and_label_rows_in_keep_idx():
    """the runner's room is the longest list (4 rows); a label's index lies behind the prediction rows of its image"""
    c = CASES["labels_nc3_multi"]
    det, count, keep, runner = launch(c, max_labels=4)
    assert runner.max_labels == 4
    check("labels_nc3_multi", (det, count, keep, runner))
    n_pred = [len(R.candidates(x, c["kw"]["conf_thres"], None, True)) for x in c["pred"]]
    assert n_pred[1] == 0 and count[1] == 3 and keep[1, :3].tolist() == [0, 1, 2]          # labels only; of the identical pair the first wins
    assert (det[1, :3, 4] == 1).all() and (keep[2, :count[2]] >= n_pred[2]).sum() == 3
    with pytest.raises(ValueError, match="max_labels is 3"):
        launch(c, max_labels=3)


def test_reference_signature_and_shared_runners():
    """non_max_suppression(labels=..., merge=...) and nms_device through the shared runner cache"""
    for name in ("labels_nc1", "merge_nc3_multi", "merge_labels"):
        c = CASES[name]
        t = torch.from_numpy(c["pred"]).to(DEV)
        lab = [torch.from_numpy(np.asarray(l, np.float32)) for l in c["labels"]] if c["labels"] is not None else ()
        out = non_max_suppression(t, labels=lab, merge=c["merge"], **c["kw"])
        for b, o in enumerate(out):
            assert np.array_equal(bits(o.cpu().numpy()), bits(want(name)[0][b])), (name, b)
    c = CASES["labels_nc1"]
    plain = non_max_suppression(torch.from_numpy(c["pred"]).to(DEV), **c["kw"])
    ref = R.non_max_suppression(c["pred"], **c["kw"])[0]
    assert all(np.array_equal(bits(o.cpu().numpy()), bits(r)) for o, r in zip(plain, ref))


def _ex(runner, pred, conf, iou, agnostic=False, classes=None, max_nms=30000, max_wh=4096.0):
    """icaf_nms_ex itself, no labels, merge = 0"""
    a = _lib.NmsArgs()
    arr = (C.c_int * max(len(classes or ()), 1))(*[int(v) for v in classes or ()])
    a.pred, a.B, a.rows, a.nc = pred.data_ptr(), runner.B, runner.rows, runner.nc
    a.conf_thres, a.iou_thres, a.multi_label, a.agnostic = conf, iou, int(runner.multi_label), int(agnostic)
    a.classes, a.n_classes = (C.addressof(arr) if classes is not None else None), len(classes or ())
    a.max_det, a.max_nms, a.max_wh = runner.max_det, max_nms, max_wh
    a.det, a.count, a.keep_idx = runner.det.data_ptr(), runner.count.data_ptr(), runner.keep.data_ptr()
    a.workspace, a.workspace_bytes = runner.ws.data_ptr(), runner.ws.numel()
    _lib.check(_lib.lib().icaf_nms_ex(C.byref(a), ops.current_stream_ptr()), "icaf_nms_ex")
    torch.cuda.synchronize()
    return runner.det.clone(), runner.count.clone(), runner.keep.clone()


def test_plain_path_equals_icaf_nms_bit_for_bit():
    """icaf_nms_ex without labels and with merge = 0 on the inputs of test_nms_bit_exact: every output byte equals icaf_nms'"""
    from test_gpu_kernels import NMS_CASES, _rand_pred
    for case in NMS_CASES:
        c = dict(case)
        B, rows, nc = c.pop("B"), c.pop("rows"), c.pop("nc")
        conf, iou, ties, near = c.pop("conf"), c.pop("iou"), c.pop("ties", False), c.pop("near", False)
        pred = _rand_pred(B, rows, nc, seed=rows + nc, ties=ties)
        if near:
            g = np.random.default_rng(9)
            pred[..., 4] = 1.0
            pred[..., 5:] = (0.5 + g.uniform(0, 2.0 ** -9, pred[..., 5:].shape)).astype(np.float32)
        t = torch.from_numpy(pred).to(DEV)
        outs = []
        for ex in (False, True):
            r = ops.NmsRunner(B, rows, nc, DEV, c.get("multi_label", False))
            r.det.fill_(SENTINEL); r.count.fill_(-5); r.keep.fill_(-9)
            if ex:
                outs.append(_ex(r, t, conf, iou, c.get("agnostic", False), c.get("classes")))
            else:
                r.launch(t, conf, iou, c.get("agnostic", False), c.get("classes"))
                torch.cuda.synchronize()
                outs.append((r.det.clone(), r.count.clone(), r.keep.clone()))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*outs)), case


def test_library_refusals():
    r = ops.NmsRunner(1, 64, 1, DEV, merge=True)
    with pytest.raises(ValueError, match="max_nms >= 3000"):
        r.launch(torch.zeros((1, 64, 6), device=DEV), 0.1, 0.5, max_nms=100)
    a = _lib.NmsArgs()
    a.pred = a.det = a.count = a.workspace = r.ws.data_ptr()
    a.B, a.rows, a.nc, a.max_det, a.max_nms, a.merge, a.workspace_bytes = 1, 64, 1, 300, 2999, 1, r.ws.numel()
    assert _lib.lib().icaf_nms_ex(C.byref(a), ops.current_stream_ptr()) != 0 and b"merge needs max_nms" in _lib.lib().icaf_last_error()


def _label_boxes(root, stem, w0, h0):
    lab = np.loadtxt(os.path.join(root, "labels", "test", stem + ".txt"), ndmin=2)
    xywh = lab[:, 1:] * [w0, h0, w0, h0]
    return lab[:, 0], np.concatenate((xywh[:, :2] - xywh[:, 2:] / 2, xywh[:, 2:]), 1)


def test_validation_loop_with_save_hybrid_and_merge(tmp_path, monkeypatch):
    """test(save_hybrid=True) on two 96 x 128 pairs: the result files hold every label box at conf 1 and every label is matched at IoU 0.5
    (recall 1.0 by construction: no two labels of a class overlap beyond the NMS threshold); test(merge_nms=True) returns finite metrics"""
    from helpers import val_module
    from test_frontends import make_dataset
    from icafusion_amd.models.yolo import Model
    from icafusion_amd.synth import synth_state_dict
    from oracle import icaf_oracle as oracle
    val = val_module()
    root = str(tmp_path / "set")
    rgb_dir, ir_dir = make_dataset(root, n=2, size=(96, 128), nc=1, seed=7, mixed=False)          # five labels, IoU up to 0.33 between two of an image
    labels = {}
    for stem in ("im000", "im001"):
        cls, tlwh = _label_boxes(root, stem, 128, 96)
        xyxy = np.concatenate((tlwh[:, :2], tlwh[:, :2] + tlwh[:, 2:]), 1)
        iou = oracle.box_iou(xyxy, xyxy) * (cls[:, None] == cls[None]) - np.eye(len(cls))
        assert iou.max() < 0.5, "the data set must not hold two labels of a class that suppress each other"
        labels[stem] = (cls, tlwh)
    data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 1, "names": ["person"]}
    model = Model(load_cfg("yolov5s_Add_kaist.yaml")).eval()
    model.load_state_dict(synth_state_dict(model, 0))
    model = model.to(DEV)
    model.compute_dtype, model.autotune, model.use_graph = torch.bfloat16, False, True
    stats, run = [], tmp_path / "hybrid"
    real = val.nms_device

    def halved(out, *a, **kw):
        """the synthetic weights saturate: many predictions reach conf 1.0 exactly, tie with the labels and, lower in candidate order, win.  With
        their objectness halved every label is the best box on its spot, which is the situation the assertions below are stated for."""
        out = out.clone()
        out[..., 4] *= 0.5
        return real(out, *a, **kw)
    monkeypatch.setattr(val, "nms_device", halved)
    res = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, save_hybrid=True, save_dir=run, stats_out=stats)
    n_labels = sum(len(c) for c, _ in labels.values())
    assert len(stats) == 2 and sum(len(s[3]) for s in stats) == n_labels
    for correct, conf, pcls, tcls in stats:                                 # every label: a detection at conf 1 that is a TP at IoU 0.5
        assert int(correct[conf == 1][:, 0].sum()) == len(tcls) == int((conf == 1).sum())
    assert res[0][1] > 0.99 and all(np.isfinite(v) for v in res[0])
    for stem, (cls, tlwh) in labels.items():                               # save_hybrid forces save_txt: frame, x, y, w, h, conf
        rows = np.loadtxt(run / "labels" / (stem + ".txt"), delimiter=",", ndmin=2)
        ones = rows[rows[:, 5] == 1][:, 1:5]
        assert len(ones) == len(tlwh)
        for box in tlwh:
            assert np.abs(ones - box).max(1).min() < 0.05, (stem, box, ones)
    monkeypatch.setattr(val, "nms_device", real)
    merged = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, merge_nms=True)
    assert len(merged) == 3 and len(merged[0]) == 7 and all(np.isfinite(v) for v in merged[0]) and np.isfinite(merged[1]).all()
    with pytest.raises(ValueError, match="confluence"):
        val.test(data, batch_size=2, imgsz=64, model=model, merge_nms=True, confluence=0.5)
