"""KAIST log-average miss rate on the MI355X: icaf_missrate_match against the reference evaluator's recorded per-image results (exact) and
numbers (1e-12), icaf_missrate_stage + match against the file route, poisoned stores and outputs, the refusals, and
test(miss_rate=...) against the result file of the same run."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import missrate_ref                                                        # noqa: E402
from icafusion_amd import _lib, ops                                        # noqa: E402
from icafusion_amd.utils import missrate                                   # noqa: E402
from helpers import val_module                                             # noqa: E402
from missrate_helpers import MR_DIR, assert_matches_golden, assert_numbers, case, table      # noqa: E402

DEV = "cuda:0"
GUARD = 4096


def sync():
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["synth", "MLPD", "MBNet", "MSDS-RCNN"])
def test_match_equals_the_reference_evaluator(name):
    """One launch over the synthetic corner set (14 images; 1,003 detections in one, 256 labels in another) and over each detector output
    the reference ships (2,252 images; MLPD 5,939 rows, MBNet 12,937, MSDS-RCNN 13,547): sorted order, matched annotation ids and both ignore masks equal the recorded results exactly, the ten numbers are
    within 1e-12."""
    c = case(name)
    res = ops.missrate_evaluate(c["table"], c["dt"], c["count"], device=DEV)
    assert_matches_golden(c, res["order"], res["dt_gt"], res["dt_ignore"], res["gt_ignore"])
    got = missrate.summarize(c["table"], c["count"], missrate.sorted_scores(c["dt"], res["order"], c["count"]), res["dt_gt"], res["dt_ignore"],
                             res["gt_ignore"])
    print(name, got)
    assert_numbers(got, c["numbers"])
    assert_numbers(missrate.kaist_miss_rate(c["table"], (c["image"], c["rows"]), device=DEV), c["numbers"])


def test_arrival_order_does_not_matter_beyond_ties():
    """The synthetic store with every image's rows shuffled (the recorded files arrive score-sorted, so only this exercises the rank sort
    on unsorted input): equal to the scalar restatement of the rules on the same shuffled store, ties in the new arrival order."""
    c = case("synth")
    rng = np.random.default_rng(5)
    dt = c["dt"].copy()
    for i, n in enumerate(c["count"]):
        dt[i, :n] = dt[i, rng.permutation(n)]
    res = ops.missrate_evaluate(c["table"], dt, c["count"], device=DEV)
    order, dt_gt, dt_ignore, gt_ignore = missrate_ref.match_all(c["table"], dt, c["count"])
    sel = c["sel"]
    assert np.array_equal(res["order"][sel], order[sel]) and np.array_equal(res["dt_gt"][sel], dt_gt[sel])
    assert np.array_equal(res["dt_ignore"][sel], dt_ignore[sel]) and np.array_equal(res["gt_ignore"], gt_ignore)
    assert not np.array_equal(order[sel], c["order"][sel])


def guarded(shape, dtype, fill):
    """A contiguous tensor of `shape` between two guard zones of one flat allocation, everything pre-filled with `fill`."""
    n = int(np.prod(shape))
    item = torch.empty((), dtype=dtype).element_size()
    flat = torch.full((2 * GUARD // item + n,), fill, dtype=dtype, device=DEV)
    return flat, flat[GUARD // item:GUARD // item + n].view(shape)


def guards_intact(flat, n, fill):
    item = flat.element_size()
    g = GUARD // item
    return bool((flat[:g] == fill).all()) and bool((flat[g + n:] == fill).all())


def test_poisoned_rows_and_outputs_change_nothing():
    """Store rows at or beyond dt_count hold NaN / huge values, the outputs start as poison between guard zones: rows below the count equal
    the clean run, rows beyond it keep the poison, the guards are untouched."""
    c = case("synth")
    clean = ops.missrate_evaluate(c["table"], c["dt"], c["count"], device=DEV)
    I, cap = c["dt"].shape[:2]
    cap2 = 1024                                                                  # the widest store the kernel takes
    dt = np.full((I, cap2, 5), np.nan)
    dt[:, :, 4] = 1e300                                                          # a poisoned score would win every sort
    dt[:, :cap][np.arange(cap)[None, :] < c["count"][:, None]] = c["dt"][np.arange(cap)[None, :] < c["count"][:, None]]
    tab = ops.missrate_table(c["table"], DEV)
    fo, order = guarded((I, cap2), torch.int32, -7)
    fg, dt_gt = guarded((I, cap2, 7), torch.int32, -7)
    fi, dt_ignore = guarded((I, cap2), torch.uint8, 0xA5)
    fq, gt_ignore = guarded((tab.labels,), torch.uint8, 0xA5)
    ops.missrate_match(tab, torch.from_numpy(dt).to(DEV), torch.from_numpy(c["count"].copy()).to(DEV), order, dt_gt, dt_ignore, gt_ignore)(
        ops.current_stream_ptr())
    sync()
    sel = np.zeros((I, cap2), bool)
    sel[:, :cap] = np.arange(cap)[None, :] < np.minimum(c["count"], 1000)[:, None]
    csel = sel[:, :cap]
    assert np.array_equal(order.cpu().numpy()[sel], clean["order"][csel]) and np.array_equal(dt_gt.cpu().numpy()[sel], clean["dt_gt"][csel])
    assert np.array_equal(dt_ignore.cpu().numpy()[sel], clean["dt_ignore"][csel]) and np.array_equal(gt_ignore.cpu().numpy(), clean["gt_ignore"])
    beyond = np.arange(cap2)[None, :] >= c["count"][:, None]
    assert (order.cpu().numpy()[beyond] == -7).all() and (dt_gt.cpu().numpy()[beyond] == -7).all() and (dt_ignore.cpu().numpy()[beyond] == 0xA5).all()
    assert guards_intact(fo, I * cap2, -7) and guards_intact(fg, I * cap2 * 7, -7) and guards_intact(fi, I * cap2, 0xA5)
    assert guards_intact(fq, tab.labels, 0xA5)


def test_stage_then_match_equals_the_file_route(tmp_path):
    """Two uneven batches (counts 0 and 300, then 1) staged into a poisoned, guarded store and matched, against the file route fed the same
    fp32 values printed with %.17g: the same store rows, the same match arrays, the same ten numbers."""
    c = case("synth")
    tab_h = c["table"]
    I, cap, max_det = len(tab_h["image_id"]), 300, 300
    rng = np.random.default_rng(11)
    boxes = tab_h["box"][tab_h["off"][11]:tab_h["off"][12]]                       # detections scattered over the 256-label image
    pick = rng.integers(0, len(boxes), 300)
    xy = (boxes[pick, :2] + rng.integers(-6, 7, (300, 2)) / 4).astype(np.float32)
    wh = (boxes[pick, 2:] + rng.integers(-4, 5, (300, 2)) / 4).astype(np.float32)
    batches = []
    for index, counts in (([4, 11], [0, 300]), ([10], [1])):
        B = len(index)
        predn = rng.uniform(0, 600, (B, max_det, 4)).astype(np.float32)          # rows beyond the count: junk that must not arrive
        det = rng.uniform(0, 1, (B, max_det, 6)).astype(np.float32)
        predn[-1, :, :2], predn[-1, :, 2:] = xy, xy + wh
        if counts[-1] == 1:
            b10 = tab_h["box"][tab_h["off"][10]]
            predn[0, 0] = np.array([b10[0], b10[1], b10[0] + b10[2], b10[1] + b10[3]], dtype=np.float32)
        batches.append((index, np.array(counts, dtype=np.int32), predn, det))
    flat, dt = guarded((I, cap, 5), torch.float64, float("nan"))
    fc, dt_count = guarded((I,), torch.int32, 0)
    image, rows = [], []
    for index, counts, predn, det in batches:
        ops.missrate_stage(torch.from_numpy(predn).to(DEV), torch.from_numpy(det).to(DEV), torch.from_numpy(counts).to(DEV), index,
                           torch.tensor(index, dtype=torch.int32, device=DEV), dt, dt_count)(ops.current_stream_ptr())
        for b, i in enumerate(index):
            n = int(counts[b])
            p = predn[b, :n]
            image += [i] * n
            rows.append(np.concatenate((p[:, :2], p[:, 2:] - p[:, :2], det[b, :n, 4:5]), 1).astype(np.float64))      # the subtraction in fp32
    sync()
    image, rows = np.array(image, dtype=np.int64), np.concatenate(rows)
    path = tmp_path / "result.txt"
    missrate.write_result_txt(path, image, rows)
    want_dt, want_count = missrate.pack_detections(I, *missrate.read_result_txt(path), cap=cap)
    got_dt, got_count = dt.cpu().numpy(), dt_count.cpu().numpy()
    sel = np.arange(cap)[None, :] < want_count[:, None]
    assert np.array_equal(got_count, want_count) and sorted(want_count[want_count > 0]) == [1, 300]
    assert np.array_equal(got_dt[sel], want_dt[sel]) and np.isnan(got_dt[~sel]).all()
    assert bool(torch.isnan(flat[:GUARD // 8]).all()) and bool(torch.isnan(flat[GUARD // 8 + I * cap * 5:]).all()) and guards_intact(fc, I, 0)
    tab = ops.missrate_table(tab_h, DEV)
    outs = ops.missrate_outputs(tab, cap, DEV)
    ops.missrate_match(tab, dt, dt_count, *outs)(ops.current_stream_ptr())
    order, dt_gt, dt_ignore, gt_ignore = (o.cpu().numpy() for o in outs)
    want = ops.missrate_evaluate(tab_h, want_dt, want_count, device=DEV)
    assert np.array_equal(order[sel], want["order"][sel]) and np.array_equal(dt_gt[sel], want["dt_gt"][sel])
    assert np.array_equal(dt_ignore[sel], want["dt_ignore"][sel]) and np.array_equal(gt_ignore, want["gt_ignore"])
    assert (dt_gt[sel][:, 0] >= 0).sum() > 20                                   # the scattered boxes do match labels
    ref = missrate_ref.match_all(tab_h, want_dt, want_count)                     # and the rules say the same about these fp32 boxes
    assert np.array_equal(order[sel], ref[0][sel]) and np.array_equal(dt_gt[sel], ref[1][sel]) and np.array_equal(dt_ignore[sel], ref[2][sel])
    got = missrate.summarize(tab_h, got_count, missrate.sorted_scores(got_dt, order, got_count), dt_gt, dt_ignore, gt_ignore)
    assert got == missrate.kaist_miss_rate(tab_h, str(path), device=DEV)


def test_refusals_come_before_any_launch():
    """257 labels in an image, a store of 1025 rows, null pointers and non-finite scores are refused by the wrappers (ValueError) and by the
    C entry (ICAF_ERR_UNSUPPORTED / ICAF_ERR_ARG) without a launch: the outputs keep their poison."""
    wide = missrate.load_annotations(os.path.join(MR_DIR, "synth257_annotation.json.gz"))
    with pytest.raises(ValueError, match="257 labels"):
        ops.missrate_table(wide, DEV)
    tab_h = table("synth_annotation.json.gz")
    I = len(tab_h["image_id"])
    with pytest.raises(ValueError, match="257 labels"):
        ops.missrate_evaluate(wide, np.zeros((I, 4, 5)), np.zeros(I, dtype=np.int32), device=DEV)
    tab = ops.missrate_table(tab_h, DEV)
    dt, cnt = torch.zeros((I, 1025, 5), dtype=torch.float64, device=DEV), torch.ones((I,), dtype=torch.int32, device=DEV)
    order = torch.full((I, 1025), -7, dtype=torch.int32, device=DEV)
    dt_gt = torch.full((I, 1025, 7), -7, dtype=torch.int32, device=DEV)
    dt_ignore, gt_ignore = torch.full((I, 1025), 0xA5, dtype=torch.uint8, device=DEV), torch.full((tab.labels,), 0xA5, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="cap must be in"):
        ops.missrate_match(tab, dt, cnt, order, dt_gt, dt_ignore, gt_ignore)
    with pytest.raises(ValueError, match="cap must be in"):
        ops.missrate_stage(torch.zeros((1, 8, 4), device=DEV), torch.zeros((1, 8, 6), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), [0],
                           torch.zeros(1, dtype=torch.int32, device=DEV), dt, cnt)
    with pytest.raises(ValueError, match="non-finite"):
        ops.missrate_evaluate(tab_h, np.full((I, 2, 5), np.inf), np.ones(I, dtype=np.int32), device=DEV)
    with pytest.raises(ValueError, match="distinct rows"):
        ops.missrate_stage(torch.zeros((2, 8, 4), device=DEV), torch.zeros((2, 8, 6), device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), [0, I],
                           torch.zeros(2, dtype=torch.int32, device=DEV), dt[:, :8].contiguous(), cnt)
    lib, s = _lib.lib(), ops.current_stream_ptr()
    args = (tab.box.data_ptr(), tab.height.data_ptr(), tab.occlusion.data_ptr(), tab.ignore.data_ptr(), tab.off.data_ptr(), I)
    outs = (order.data_ptr(), dt_gt.data_ptr(), dt_ignore.data_ptr(), gt_ignore.data_ptr())
    assert lib.icaf_missrate_match(*args, 257, dt.data_ptr(), cnt.data_ptr(), 1024, *outs, s) == -3 and b"256 labels" in lib.icaf_last_error()
    assert lib.icaf_missrate_match(*args, 256, dt.data_ptr(), cnt.data_ptr(), 1025, *outs, s) == -3 and b"1024" in lib.icaf_last_error()
    assert lib.icaf_missrate_match(*args, 256, None, cnt.data_ptr(), 1024, *outs, s) == -1
    assert lib.icaf_missrate_match(*args, 256, dt.data_ptr(), cnt.data_ptr(), 1024, order.data_ptr(), None, dt_ignore.data_ptr(), gt_ignore.data_ptr(), s) == -1
    assert lib.icaf_missrate_stage(None, dt.data_ptr(), cnt.data_ptr(), cnt.data_ptr(), 1, 8, dt.data_ptr(), cnt.data_ptr(), I, 8, s) == -1
    assert lib.icaf_missrate_stage(dt.data_ptr(), dt.data_ptr(), cnt.data_ptr(), cnt.data_ptr(), 1, 8, dt.data_ptr(), cnt.data_ptr(), I, 1025, s) == -3
    sync()
    assert bool((order == -7).all()) and bool((dt_gt == -7).all()) and bool((dt_ignore == 0xA5).all()) and bool((gt_ignore == 0xA5).all())
    assert bool((dt == 0).all()) and bool((cnt == 1).all())


def test_validation_loop_reports_the_miss_rate_of_its_own_result_file(tmp_path, capsys):
    """test(..., miss_rate=...) on four pairs (two batch shapes, so the loader's order differs from the label directory's): the returned
    dict equals kaist_miss_rate on the detections the same run handed to its result writer, written with full-precision lines (result.txt
    itself is %g text); without the option the return value is what it was."""
    import json
    from test_frontends import make_dataset
    from test_gpu_val_frames import build
    val = val_module()
    rgb_dir, ir_dir = make_dataset(str(tmp_path / "set"), n=4, size=(96, 128), nc=1, seed=3)
    data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 1, "names": ["person"]}
    seen = {"image": [], "rows": []}

    class Recorder(val.ResultWriter):                                            # the writer's own rows, kept at full precision
        def add(self, path, predn, conf, cls):
            super().add(path, predn, conf, cls)
            predn = np.asarray(predn, dtype=np.float32).reshape(-1, 4)
            seen["image"] += [val.frame_index(self.label_names, os.path.splitext(os.path.basename(str(path)))[0])] * len(predn)
            seen["rows"].append(np.concatenate((predn[:, :2], predn[:, 2:] - predn[:, :2], np.asarray(conf, dtype=np.float32).reshape(-1, 1)), 1))

    val.ResultWriter = Recorder
    model = build("yolov5s_Add_kaist.yaml", torch.bfloat16)
    model.use_graph = True
    plain = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, save_txt=True, save_dir=tmp_path / "plain")
    # annotations that this model's detections can hit: every third detection of the first run becomes a label, cut back to the inside of
    # the evaluator's border (x, y >= 5: boxes clipped to the frame start at 0 and would all be ignored)
    names = sorted(os.listdir(tmp_path / "set" / "labels" / "test"))
    first = np.concatenate(seen["rows"]).astype(np.float64)
    anns = []
    for k, (i, r) in enumerate(zip(seen["image"][::3], first[::3])):
        x, y = max(float(r[0]), 6.0), max(float(r[1]), 6.0)
        anns.append({"id": k, "image_id": int(i), "category_id": 1, "bbox": [x, y, float(r[0] + r[2]) - x, float(r[1] + r[3]) - y],
                     "height": 60, "occlusion": k % 3, "ignore": 0})
    print("detections of the first run:", np.bincount(seen["image"]).tolist(), "labels:", len(anns))
    ann = tmp_path / "ann.json"
    ann.write_text(json.dumps({"images": [{"id": i, "im_name": n[:-4]} for i, n in enumerate(names)], "annotations": anns}))
    seen["image"], seen["rows"] = [], []
    out = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, save_txt=True, save_dir=tmp_path / "run", miss_rate=str(ann))
    print(out[3])
    assert len(out) == 4 and set(out[3]) == set(missrate.KEYS)
    printed = capsys.readouterr().out
    assert "MR-all" in printed and "Recall-all" in printed and missrate.format_lines(out[3])[1] in printed
    rows = np.concatenate(seen["rows"]).astype(np.float64)
    assert len(rows) > 4 and len(set(seen["image"])) >= 2
    full = tmp_path / "full.txt"
    missrate.write_result_txt(full, seen["image"], rows)
    assert out[3] == missrate.kaist_miss_rate(str(ann), str(full), day_images=1455, device=DEV)
    assert 0 < out[3]["all"] < 1 and out[3]["recall_all"] > 0                   # labels are hit and missed
    assert len(plain) == 3 and plain[0] == out[0] and plain[1].tolist() == out[1].tolist()


def test_tool_prints_the_ten_numbers(capsys):
    """tools/kaist_mr.py ANNOTATIONS RESULT_TXT: the file route stand-alone, on the reference's MLPD file."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("icaf_tool_kaist_mr", os.path.join(os.path.dirname(MR_DIR), "..", "..", "tools", "kaist_mr.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got = tool.main([os.path.join(MR_DIR, "KAIST_annotation.json.gz"), os.path.join(MR_DIR, "MLPD_result.txt.gz")])
    assert_numbers(got, case("MLPD")["numbers"])
    lines = capsys.readouterr().out.split()
    assert lines[:6] == ["MR_all:", "7.58", "MR_day:", "7.96", "MR_night:", "6.95"] and lines[-2:] == ["recall_all:", "96.70"] and len(lines) == 20
