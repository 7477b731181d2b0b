"""Apriori labels and merge-NMS without a GPU: the numpy restatement (tests/nms_modes_ref.py, the device tests' oracle) against the fixtures the
reference itself produced (tests/golden/nms_modes/, made by make_golden_nms_modes.py), the derived binding of the new struct, and every refusal
that is decided on the host."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import nms_modes_ref as R                                                   # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "nms_modes")
with open(os.path.join(GOLDEN, "summary.json")) as _f:
    SUMMARY = json.load(_f)


def load_case(name):
    """fixture -> (case dict as nms_modes_ref.cases() builds them, the npz): the sparse input becomes the dense prediction again"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    s = SUMMARY[name]
    B, rows, no = (int(v) for v in g["shape"])
    pred = np.broadcast_to(g["filler"], (B, rows, no)).copy()
    for b in range(B):
        pred[b, g[f"at{b}"]] = g[f"rows{b}"]
    labels = [g[f"labels{b}"] for b in range(B)] if s["labels"] else None
    return dict(pred=pred, labels=labels, kw=dict(s["kw"]), merge=s["merge"]), g


def _root(name):
    spec = importlib.util.spec_from_file_location("icaf_root_" + name, os.path.join(REPO, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_fixtures_are_the_cases_the_device_tests_run():
    """the generator and the device tests share nms_modes_ref.cases(): the committed inputs must still be those"""
    cases = R.cases()
    assert sorted(cases) == sorted(SUMMARY)
    for name, c in cases.items():
        got, _ = load_case(name)
        np.testing.assert_array_equal(got["pred"], c["pred"])
        assert got["kw"] == c["kw"] and got["merge"] == c["merge"] and (got["labels"] is None) == (c["labels"] is None)
        if c["labels"] is not None:
            for a, b in zip(got["labels"], c["labels"]):
                np.testing.assert_array_equal(a, np.asarray(b, np.float32).reshape(-1, 5))


@pytest.mark.parametrize("name", sorted(SUMMARY))
def test_restatement_against_the_reference(name):
    """Kept indices, confidences and classes exactly; rows that no summation touched bit for bit; merged coordinates within 4 x the reference's
    own fp32-against-fp64 deviation of the case (summary.json), floored at one fp32 ulp of the coordinate."""
    c, g = load_case(name)
    s = SUMMARY[name]
    rows, idx, ns = R.run_case(c)
    plain_idx = R.non_max_suppression(c["pred"], labels=c["labels"], **c["kw"])[1]
    assert ns == s["candidates"]
    for b in range(c["pred"].shape[0]):
        ref = g[f"out32_{b}"]
        np.testing.assert_array_equal(plain_idx[b], g[f"keep{b}"])              # what the reference's greedy core returned
        assert len(rows[b]) == len(ref) == s["kept"][b]
        np.testing.assert_array_equal(rows[b][:, 4:], ref[:, 4:])
        assert set(idx[b].tolist()) <= set(plain_idx[b].tolist())
        if not (c["merge"] and 1 < ns[b] < R.MERGE_LIMIT):
            np.testing.assert_array_equal(rows[b], ref)
            continue
        bound = np.maximum(4.0 * s["merged_fp32_vs_fp64_max_abs"], np.spacing(np.abs(ref[:, :4])).astype(np.float64))
        err = np.abs(rows[b][:, :4].astype(np.float64) - ref[:, :4].astype(np.float64))
        print(name, b, "max error", err.max() if err.size else 0.0, "bound", bound.min() if bound.size else 0.0)
        assert (err <= bound).all()
        # the exact quotient of the fp64 sums lies inside the same bound, and the fp32 rule within three ulps of it (three roundings of at most 2^-24 relative each)
        exact = R.run_case(c, exact=True)[0][b]
        assert (np.abs(exact[:, :4] - ref[:, :4].astype(np.float64)) <= bound).all()
        assert (np.abs(exact[:, :4] - rows[b][:, :4].astype(np.float64)) <= 3.0 * np.spacing(np.abs(ref[:, :4])).astype(np.float64)).all()


def test_merge_changes_the_boxes_and_redundant_drops_the_isolated_ones():
    c, _ = load_case("merge_nc1")
    merged, idx, ns = R.run_case(c)
    plain, pidx, _ = R.non_max_suppression(c["pred"], **c["kw"])
    loose, lidx, _ = R.run_case(c, redundant=False)
    for b in range(3):
        assert len(merged[b]) < len(plain[b]) == len(loose[b]) and lidx[b].tolist() == pidx[b].tolist()
        both = np.isin(pidx[b], idx[b])
        np.testing.assert_array_equal(loose[b][both], merged[b])
        assert not np.array_equal(loose[b][both][:, :4], plain[b][both][:, :4])
    assert np.isnan(loose[2][:, :4]).any(1).sum() == 1                          # the zero-area box: 0 / 0, kept only without `redundant`


def test_header_binding_round_trip():
    from icafusion_amd import _lib
    h = _lib.HEADER
    fields = [f[0] for f in h.structs["icaf_nms_args"]]
    assert fields == ["pred", "classes", "labels", "label_off", "det", "count", "keep_idx", "workspace", "workspace_bytes", "rows", "B", "nc",
                      "conf_thres", "iou_thres", "multi_label", "agnostic", "n_classes", "max_det", "max_nms", "max_labels", "max_wh", "merge",
                      "redundant", "reserved"]
    assert ctypes.sizeof(_lib.NmsArgs) == 8 * 10 + 4 * 14 and _lib.NmsArgs.rows.offset == 72 and _lib.NmsArgs.merge.offset == 124
    assert _lib.NMS_MERGE_LIMIT == 3000 == R.MERGE_LIMIT
    res, args = _lib.SIGNATURES["icaf_nms_ex"]
    assert res is ctypes.c_int and args == [ctypes.POINTER(_lib.NmsArgs), ctypes.c_void_p]
    res, args = _lib.SIGNATURES["icaf_nms_ex_workspace_bytes"]
    assert args == [ctypes.POINTER(_lib.NmsArgs), ctypes.POINTER(ctypes.c_size_t)]
    assert len(_lib.SIGNATURES["icaf_nms"][1]) == 19                            # the old entry point keeps its signature
    a = _lib.NmsArgs()
    a.rows, a.max_labels, a.merge = 1 << 40, 7, 1
    assert (a.rows, a.max_labels, a.merge, a.labels) == (1 << 40, 7, 1, None)


def test_argument_refusals_are_decided_on_the_host():
    from icafusion_amd import ops
    from icafusion_amd.utils.general import nms_device, non_max_suppression
    pred = torch.zeros((2, 8, 8))
    with pytest.raises(ValueError, match="max_nms >= 3000"):
        nms_device(pred, merge=True, max_nms=2999)
    good = [torch.tensor([[2.0, 10, 10, 4, 4]]), torch.zeros((0, 5))]
    with pytest.raises(ValueError, match=r"class ids must be in \[0, 3\)"):
        nms_device(pred, labels=[torch.tensor([[3.0, 10, 10, 4, 4]]), torch.zeros((0, 5))])
    with pytest.raises(ValueError, match=r"class ids must be in \[0, 3\)"):
        nms_device(pred, labels=[torch.zeros((0, 5)), torch.tensor([[-1.0, 10, 10, 4, 4]])])
    with pytest.raises(ValueError, match="max_labels is 2"):
        ops.nms_label_table([torch.ones((3, 5)), torch.zeros((0, 5))], 2, 3, max_labels=2)
    with pytest.raises(ValueError, match="the batch holds 2"):
        ops.nms_label_table(good[:1], 2, 3)
    table, off, most = ops.nms_label_table(good[::-1] + good[::-1], 4, 3, max_labels=1)      # an empty image first and in the middle; max_labels met
    assert table.shape == (2, 5) and table.dtype == torch.float32 and off.dtype == torch.int32 and off.tolist() == [0, 0, 1, 1, 2] and most == 1
    # accepted arguments reach the device check: no NotImplementedError any more, and still no CPU fallback
    for kw in (dict(labels=good), dict(merge=True), dict(labels=good, merge=True), {}):
        with pytest.raises(RuntimeError, match="MI355X only"):
            non_max_suppression(pred, **kw)


def test_scripts_accept_and_refuse_the_flags():
    val, det = _root("test"), _root("detect_twostream")
    o = val.parse_opt(["--save-hybrid", "--merge-nms"])
    assert o.save_hybrid and o.merge_nms and not val.parse_opt([]).merge_nms and not val.parse_opt([]).save_hybrid
    d = det.parse_opt(["--source1", "a", "--source2", "b", "--merge-nms"])
    assert d.merge_nms and not det.parse_opt(["--source1", "a", "--source2", "b"]).merge_nms
    for kw in (dict(merge_nms=True), dict(save_hybrid=True)):
        with pytest.raises(ValueError, match="confluence"):
            val.test({"nc": 1}, confluence=0.6, **kw)
    d.confluence = 0.6
    with pytest.raises(ValueError, match="--merge-nms .* --confluence"):
        det.detect(d)
    with pytest.raises(NotImplementedError):                                    # unchanged: test() still refuses augment
        val.test({"nc": 1}, augment=True, merge_nms=True)
