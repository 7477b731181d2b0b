"""Confluence on the MI355X against the results recorded from the reference (tests/golden/confluence) and the CPU statement of the rules
(tests/confluence_ref.py, pinned to the same recordings by tests/test_confluence_host.py).  Exactness is the criterion throughout: kept
indices are equal, rows are bit-equal; there is no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import REPO, load_cfg, val_module                             # noqa: E402
import confluence_ref                                                      # noqa: E402
from test_confluence_host import process_cases, select_cases  # noqa: E402
from icafusion_amd import ops                                              # noqa: E402
from icafusion_amd.synth import synth_crowd_prediction, synth_state_dict   # noqa: E402
from icafusion_amd.utils import confluence as cf                           # noqa: E402

DEV = "cuda:0"
SELECT, PROCESS = select_cases(), process_cases()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def padded(cases, max_cand, poison=True):
    """Select cases side by side: cand (B, max_cand, 6) with NaN beyond every image's rows, n (B,)"""
    cand = np.full((len(cases), max_cand, 6), np.nan if poison else 0.0, np.float32)
    for b, d in enumerate(cases):
        cand[b, :len(d)] = d
    return torch.from_numpy(cand).to(DEV), torch.tensor([len(d) for d in cases], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("name", sorted(SELECT))
def test_confluence_returns_the_reference_indices(name):
    dets, nc, p, keep = SELECT[name]
    got = cf.confluence(dets, nc, p)
    assert got.dtype == np.int64 and got.tolist() == keep.tolist()
    if name == "chain":                                 # a tensor on the device is taken as it is
        assert cf.confluence(torch.from_numpy(dets).to(DEV), nc, p).tolist() == keep.tolist()


@pytest.mark.parametrize("name", ["process_nc1", "process_nc3"])
def test_confluence_process_rows_are_bit_equal(name):
    pred, conf, p, want = PROCESS[name]
    for t in (torch.from_numpy(pred).to(DEV), torch.from_numpy(pred).to(DEV).double()):      # other dtypes are converted to fp32 first
        got = cf.confluence_process(t, conf, p)
        assert [o is None for o in got] == [o is None for o in want]
        for a, b in zip(got, want):
            assert a is None or (a.dtype == torch.float32 and tuple(a.shape) == b.shape and np.array_equal(bits(a.cpu().numpy()), bits(b)))


def test_half_precision_input_is_widened_first():
    pred = torch.from_numpy(PROCESS["process_nc3"][0]).to(DEV).half()
    got = cf.confluence_process(pred, 0.1, 0.6)
    want = confluence_ref.confluence_process(pred.float().cpu().numpy(), 0.1, 0.6)
    assert [o is None for o in got] == [o is None for o in want]
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(want[0]))


def test_batch_of_unequal_images_poisoned_slack_and_optional_keep_idx():
    """B = 3 with 64 / 256 / 6 candidates of three classes in one launch (max_cand 300: slack behind every image), NaN in every slack row of cand
    and all over det / keep_idx beforehand: per image the reference's indices, det = the kept rows then zeros, no NaN anywhere; the same det
    without keep_idx."""
    names = ["crowd_n64_nc3", "crowd_n256_nc3", "classes_gap"]
    cand, n = padded([SELECT[k][0] for k in names], 300)
    outs = []
    for want_keep in (True, False):
        det = torch.full((3, 300, 6), float("nan"), device=DEV)
        count = torch.full((3,), -7, dtype=torch.int32, device=DEV)
        keep = torch.full((3, 300), 12345, dtype=torch.int32, device=DEV) if want_keep else None
        ops.confluence_select(cand, n, 3, 0.6, det=det, count=count, keep_idx=keep, want_keep=want_keep)
        outs.append((det.cpu().numpy(), count.cpu().numpy(), keep.cpu().numpy() if want_keep else None))
    (det, count, keep), (det2, count2, _) = outs
    assert np.array_equal(bits(det), bits(det2)) and np.array_equal(count, count2)
    assert not np.isnan(det).any()
    for b, k in enumerate(names):
        dets, _, _, want = SELECT[k]
        c = int(count[b])
        assert c == len(want) and keep[b, :c].tolist() == want.tolist() and (keep[b, c:] == -1).all()
        assert np.array_equal(bits(det[b, :c]), bits(dets[want])) and not bits(det[b, c:]).any()


def test_out_of_range_counts_stay_inside_the_buffers():
    """n[b] < 0 counts as no candidate, n[b] > max_cand refuses the image (count = -n, rows zero); guard rows around the buffers stay NaN"""
    dets = SELECT["crowd_n63_nc1"][0]
    cand, _ = padded([dets, dets, dets], 64)
    n = torch.tensor([-3, 63, 1000], dtype=torch.int32, device=DEV)
    block = torch.full((5, 64, 6), float("nan"), device=DEV)
    det, count, _ = ops.confluence_select(cand, n, 1, 0.6, det=block[1:4], want_keep=False)
    assert count.tolist() == [0, len(SELECT["crowd_n63_nc1"][3]), -1000]
    assert torch.isnan(block[0]).all() and torch.isnan(block[4]).all() and not det[0].any() and not det[2].any()


def test_image_above_the_cap_is_refused_not_truncated():
    pred, conf, p, want = PROCESS["refusal_cap64"]
    t = torch.from_numpy(pred).to(DEV)
    runner = ops.ConfluenceRunner(3, pred.shape[1], 1, DEV, max_cand=64)
    runner.det.fill_(float("nan"))
    det, count, keep = runner.launch(t, conf, p)
    assert count.tolist() == [len(want[0]), -65, len(want[2])]
    assert not det[1].any() and not torch.isnan(det).any()
    for b in (0, 2):
        assert np.array_equal(bits(det[b, :len(want[b])].cpu().numpy()), bits(want[b])) and not det[b, len(want[b]):].any()
    with pytest.raises(ValueError, match="image 1: 65 confluence candidates exceed the cap of 64"):
        cf.confluence_process(t, conf, p, max_cand=64)
    got = cf.confluence_process(t, conf, p, max_cand=65)                   # one more row of room: the reference's result
    assert all(np.array_equal(bits(a.cpu().numpy()), bits(b)) for a, b in zip(got, want))


def test_argument_errors_carry_a_message():
    cand, n = padded([SELECT["n1"][0]], 8)
    with pytest.raises(RuntimeError, match="max_cand must be in"):
        ops.ConfluenceRunner(1, 16, 1, DEV, max_cand=4097)
    runner = ops.ConfluenceRunner(1, 16, 1, DEV, max_cand=8)
    with pytest.raises(RuntimeError, match="conf_thres must be at least 2e-4"):
        runner.launch(torch.zeros((1, 16, 6), device=DEV), 1e-4, 0.6)
    with pytest.raises(RuntimeError, match="p_thres is NaN"):
        ops.confluence_select(cand, n, 1, float("nan"))


def test_whole_path_equals_select_and_the_cpu_statement_across_blocks():
    """600 candidates per image among 2000 rows (two images, two classes): the candidate stage compacts over two chunks of rows, the chip-wide
    sweep feeds the picks; the same candidates through the select alone (the workgroup sweeps its own rows) and through the CPU statement"""
    pred = synth_crowd_prediction(2, 2000, 600, nc=2, seed=3)
    t = torch.from_numpy(pred).to(DEV)
    got = cf.confluence_process(t, 0.1, 0.6)
    cands = [confluence_ref.candidates(x, 0.1) for x in pred]
    assert [len(c) for c in cands] == [600, 600]
    cand, n = padded(cands, 640)
    det, count, keep = ops.confluence_select(cand, n, 2, 0.6)
    for b in range(2):
        want = confluence_ref.confluence(cands[b], 2, 0.6)
        assert keep[b, :int(count[b])].tolist() == want.tolist()
        assert np.array_equal(bits(got[b].cpu().numpy()), bits(cands[b][want]))


def test_the_cap_itself_4096_candidates_of_one_class():
    """max_cand = 4096: the 140 KiB LDS plan.  The picks fed by the chip-wide sweep against the picks of a workgroup sweeping its own rows"""
    pred = synth_crowd_prediction(1, 4096, 4096, nc=1, seed=5)
    t = torch.from_numpy(pred).to(DEV)
    det, count, keep = cf.confluence_device(t, 0.1, 0.6)
    cand, n = padded([confluence_ref.candidates(pred[0], 0.1)], 4096)
    assert int(n[0]) == 4096
    det2, count2, keep2 = ops.confluence_select(cand, n, 1, 0.6)
    c = int(count[0])
    assert 256 < c < 4096 and c == int(count2[0]) and torch.equal(keep, keep2) and torch.equal(det.view(torch.int32), det2.view(torch.int32))
    k = keep[0, :c].cpu().numpy()
    assert (np.diff(k) > 0).all()
    P = confluence_ref.proximity(cand[0, k[:512], :4].cpu().numpy())       # no two kept boxes are closer than the bound
    assert not (P < 0.6).any()


def test_launch_replays_under_graph_capture():
    pred, conf, p, want = PROCESS["process_nc3"]
    t = torch.from_numpy(pred).to(DEV)
    runner = ops.ConfluenceRunner(3, pred.shape[1], 3, DEV)
    det, count, keep = runner.launch(t, conf, p)                           # warm-up outside the capture
    first = (det.clone(), count.clone(), keep.clone())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        runner.launch(t, conf, p)
    for _ in range(2):
        det.fill_(float("nan")); count.fill_(-9); keep.fill_(77)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(det.view(torch.int32), first[0].view(torch.int32)) and torch.equal(count, first[1]) and torch.equal(keep, first[2])
    assert count.tolist() == [len(want[0]), 0, 0]


def test_validation_loop_with_confluence(tmp_path, monkeypatch):
    """test(confluence=0.5) on five 96 x 128 pairs at img-size 64: the tuple shape of the plain call, and per image the detections the loop
    matched equal the CPU statement applied to the decoded rows of the same forward"""
    from test_frontends import make_dataset
    from icafusion_amd.models.yolo import Model
    val = val_module()
    rgb_dir, ir_dir = make_dataset(str(tmp_path / "set"), n=5, size=(96, 128), nc=2, seed=3)
    data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 2, "names": ["person", "car"]}
    model = Model(load_cfg("yolov5s_Add_kaist.yaml")).eval()
    model.load_state_dict(synth_state_dict(model, 0))
    model = model.to(DEV)
    model.compute_dtype, model.autotune, model.use_graph = torch.bfloat16, False, True
    seen, real = [], val.confluence_device

    def spy(out, conf_thres, p_thres):
        det, count, keep = real(out, conf_thres, p_thres)
        seen.append((out.float().cpu().numpy(), det.cpu().numpy(), count.cpu().numpy(), conf_thres, p_thres))
        return det, count, keep
    monkeypatch.setattr(val, "confluence_device", spy)
    plain = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model)
    assert not seen
    res = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, confluence=0.5)
    assert len(res) == len(plain) == 3 and len(res[0]) == len(plain[0]) == 7 and res[1].shape == plain[1].shape
    assert len(seen) == 3 and sum(len(s[2]) for s in seen) == 5
    kept = 0
    for z, det, count, conf, p in seen:
        assert (conf, p) == (0.05, 0.5)
        want = confluence_ref.confluence_process(z, conf, p)
        for b, w in enumerate(want):
            c = int(count[b])
            assert c == (0 if w is None else len(w)) and (w is None or np.array_equal(bits(det[b, :c]), bits(w)))
            kept += c
    assert kept > 0
