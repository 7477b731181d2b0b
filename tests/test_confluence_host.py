"""Confluence without a GPU: the CPU statement of the rules (tests/confluence_ref.py) against every result recorded from the reference
(tests/golden/confluence, README_confluence.md), the C ABI's declaration, the wrapper's refusals before any device call and the opt-in flag
of test.py (without it the loop still calls nms_device)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import REPO, val_module
import confluence_ref
from icafusion_amd import _lib, ops
from icafusion_amd.utils import confluence as cf

GOLDEN = os.path.join(REPO, "tests", "golden", "confluence")


def select_cases():
    g = np.load(os.path.join(GOLDEN, "select_cases.npz"))
    names = sorted(k[:-len("__dets")] for k in g.files if k.endswith("__dets"))
    return {n: (g[n + "__dets"], int(g[n + "__nc"]), float(g[n + "__p"]), g[n + "__keep"]) for n in names}


def process_cases():
    g = np.load(os.path.join(GOLDEN, "process_cases.npz"))
    names = sorted(k[:-len("__pred")] for k in g.files if k.endswith("__pred"))
    out = {}
    for n in names:
        none = g[n + "__none"]
        out[n] = (g[n + "__pred"], float(g[n + "__conf"]), float(g[n + "__p"]), [None if none[i] else g[f"{n}__out{i}"] for i in range(len(none))])
    return out


def test_fixture_set_is_complete():
    sel, proc = select_cases(), process_cases()
    for name in ("n1", "n2_overlap", "n2_far", "cluster_isolated", "duplicates", "lattice_on_bound", "lattice_above_bound", "p_equals_two",
                 "nan_pair", "chain", "classes_gap"):
        assert name in sel
    assert {len(v[0]) for k, v in sel.items() if k.startswith("crowd")} >= {63, 64, 65, 255, 256, 257, 600}
    assert set(proc) == {"process_nc1", "process_nc3", "refusal_cap64"}
    with open(os.path.join(GOLDEN, "summary.json")) as f:
        summary = json.load(f)
    assert set(summary["select"]) == set(sel) and all(v["reference_seconds"] >= 0 for v in summary["select"].values())
    assert sel["lattice_on_bound"][3].tolist() == [0, 1] and sel["lattice_above_bound"][3].tolist() == [0]
    assert sel["chain"][3].tolist() == [0, 3] and 3 not in sel["classes_gap"][3].tolist()


@pytest.mark.parametrize("name", sorted(select_cases()))
def test_cpu_statement_equals_the_reference_select(name):
    dets, nc, p, keep = select_cases()[name]
    got = confluence_ref.confluence(dets, nc, p)
    assert got.dtype == np.int64 and got.tolist() == keep.tolist()


@pytest.mark.parametrize("name", sorted(process_cases()))
def test_cpu_statement_equals_the_reference_process(name):
    pred, conf, p, want = process_cases()[name]
    got = confluence_ref.confluence_process(pred, conf, p)
    assert [o is None for o in got] == [o is None for o in want]
    for a, b in zip(got, want):
        assert a is None or (a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes())


def test_proximity_is_bitwise_symmetric_and_exact_on_the_lattice():
    P = confluence_ref.proximity(np.array([[0, 0, 6, 8], [2, 0, 8, 8], [0, 0, 4, 4], [4, 4, 8, 8]], np.float32))
    assert P[0, 1] == 0.5 and P[2, 3] == 2.0
    Q = confluence_ref.proximity(select_cases()["crowd_n65_nc1"][0][:, :4])
    assert np.array_equal(Q, Q.T, equal_nan=True)


def test_header_declares_the_entry_points_with_their_citations():
    with open(os.path.join(REPO, "include", "icaf.h")) as f:
        header = f.read()
    assert "int icaf_confluence_select(const float* cand, const int* n, int B, int max_cand, int nc, double p_thres, float* det" in header
    assert "int icaf_confluence(const float* pred, int B, long long rows, int nc, float conf_thres, double p_thres, int max_cand" in header
    assert "int icaf_confluence_workspace_bytes(" in header
    block = header[header.index("---- Confluence suppression"):header.index("int icaf_confluence_select(")]
    for cite in ("utils/confluence.py:50-193", ":109-193", ":50-106", "test.py:139-140", "ICAF_CONFLUENCE_MAX_CAND = 4096", "2e-4", "REFUSED"):
        assert cite in block, cite
    assert len(_lib.SIGNATURES["icaf_confluence_select"][1]) == 10 and len(_lib.SIGNATURES["icaf_confluence"][1]) == 13
    import ctypes
    assert _lib.SIGNATURES["icaf_confluence_select"][1][5] is ctypes.c_double and _lib.SIGNATURES["icaf_confluence"][1][5] is ctypes.c_double
    assert ops.CONFLUENCE_MAX_CAND == _lib.CONFLUENCE_MAX_CAND == 4096
    from icafusion_amd import build
    assert build.PER_FILE["confluence.hip"] == ["-ffp-contract=off"] and build.NO_SCRATCH.search("icaf::confluence_pick_kernel(")


def test_wrapper_refuses_cpu_tensors_and_small_conf_before_any_device_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("device call")
    monkeypatch.setattr(ops, "ConfluenceRunner", boom)
    monkeypatch.setattr(ops, "confluence_select", boom)
    monkeypatch.setattr(ops, "lib", boom)
    pred = torch.zeros((1, 8, 6))
    with pytest.raises(RuntimeError, match="confluence_process runs on the MI355X only"):
        cf.confluence_process(pred)
    with pytest.raises(RuntimeError, match="MI355X only"):
        cf.confluence_device(pred.half(), 0.1, 0.6)

    class OnDevice:                                    # a tensor that claims to live on the device: the conf check comes next
        is_cuda = True
    with pytest.raises(ValueError, match="conf_thres >= 0.0002"):
        cf.confluence_device(OnDevice(), 1e-4, 0.6)
    with pytest.raises(ValueError, match="every conf must exceed"):
        cf.confluence(np.array([[0, 0, 4, 4, 1e-4, 0]], np.float32), 1)
    with pytest.raises(ValueError, match=r"\(n, 6\)"):
        cf.confluence(np.zeros((3, 5), np.float32), 1)
    with pytest.raises(ValueError, match="exceed the cap of 4096"):
        cf.confluence(np.ones((4097, 6), np.float32), 1)
    assert cf.confluence(np.zeros((0, 6), np.float32), 1).tolist() == []
    with pytest.raises(ValueError, match="image 1: 65 confluence candidates exceed the cap of 64"):
        cf.refused([3, -65, 0], 64)


def test_front_ends_parse_the_flag():
    val = val_module()
    assert val.parse_opt([]).confluence is None and val.parse_opt(["--confluence", "0.5"]).confluence == 0.5
    import inspect
    assert inspect.signature(val.test).parameters["confluence"].default is None
    import detect_twostream as dt
    base = ["--source1", "a", "--source2", "b"]
    assert dt.parse_opt(base).confluence is None and dt.parse_opt(base + ["--confluence", "0.6"]).confluence == 0.6


class FakeModel:
    stride = torch.tensor([8.0, 16.0, 32.0])

    def parameters(self):
        return iter([torch.zeros(1)])

    def forward_u8(self, img):
        return [torch.zeros((img.shape[0], 12, 6))]


@pytest.mark.parametrize("flag", [None, 0.5])
def test_validation_loop_calls_nms_unless_the_flag_is_given(monkeypatch, flag):
    val = val_module()
    calls = {"nms": 0, "confluence": 0}

    def fake_nms(out, conf_thres, iou_thres, **kw):
        calls["nms"] += 1
        return torch.zeros((out.shape[0], 300, 6)), torch.zeros((out.shape[0],), dtype=torch.int32), None

    def fake_confluence(out, conf_thres, p_thres):
        calls["confluence"] += 1
        assert p_thres == 0.5
        return torch.zeros((out.shape[0], 4096, 6)), torch.zeros((out.shape[0],), dtype=torch.int32), None

    def fake_match(det, count, labels, off, iouv, scale=None, predn=None):
        assert det.shape[1] == (300 if flag is None else 1024) and det.is_contiguous()
        return torch.zeros((det.shape[0], det.shape[1], 10), dtype=torch.uint8)
    monkeypatch.setattr(val, "nms_device", fake_nms)
    monkeypatch.setattr(val, "confluence_device", fake_confluence)
    monkeypatch.setattr(val.ops, "match_predictions", fake_match)
    batch = (torch.zeros((2, 6, 32, 32), dtype=torch.uint8), torch.zeros((0, 6)), ["a.png", "b.png"], [((32, 32), ((1.0, 1.0), (0.0, 0.0)))] * 2)
    res = val.test({"nc": 1, "names": ["person"]}, model=FakeModel(), dataloader=[batch, batch], conf_thres=0.05, confluence=flag)
    assert calls == ({"nms": 2, "confluence": 0} if flag is None else {"nms": 0, "confluence": 2})
    assert len(res) == 3 and len(res[0]) == 7


def test_validation_loop_names_the_image_it_refuses(monkeypatch):
    val = val_module()
    for bad, words in ((-5000, "met 5000 candidates"), (1025, "kept 1025 detections")):
        def fake_confluence(out, conf_thres, p_thres, bad=bad):
            return torch.zeros((2, 4096, 6)), torch.tensor([3, bad], dtype=torch.int32), None
        monkeypatch.setattr(val, "confluence_device", fake_confluence)
        batch = (torch.zeros((2, 6, 32, 32), dtype=torch.uint8), torch.zeros((0, 6)), ["a.png", "dir/b.png"], [((32, 32), ((1.0, 1.0), (0.0, 0.0)))] * 2)
        with pytest.raises(ValueError, match="dir/b.png: confluence " + words):
            val.test({"nc": 1, "names": ["person"]}, model=FakeModel(), dataloader=[batch], conf_thres=0.05, confluence=0.6)
