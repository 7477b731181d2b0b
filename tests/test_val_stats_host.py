"""The CPU side of the device validation statistics: the scalar restatements (tests/ap_ref.py, tests/confusion_ref.py) against the
reference's recorded outputs (tests/golden/stats/), the new test.py flags, and the C ABI of the new entry points.  No GPU."""
import numpy as np
import pytest

import ap_ref
import confusion_ref
import val_stats_helpers as H
from icafusion_amd import _lib
from icafusion_amd.utils.metrics import ap_per_class
from helpers import val_module


@pytest.mark.parametrize("name", H.names("ap"))
def test_ap_ref_equals_the_recorded_reference(name):
    """Distinct confidences: the stable order IS the reference's order, so everything it returns is reproduced — integers, classes and the
    P / R / F1 / TP / FP / FN columns at the best-F1 index exactly, ap within 1e-12 (only np.trapz's summation order differs)."""
    g = H.golden("ap", name)
    uc, n_l = H.labels_of(g["target_cls"])
    assert np.array_equal(uc.astype("int32"), g["classes"])
    res = ap_ref.ap_per_class(g["tp_in"], g["conf"], g["pred_cls"], uc, n_l)
    H.assert_equals_reference_tuple(res, (g["tp"], g["fp"], g["fn"], g["p"], g["r"], g["ap"], g["f1"]), name)
    # the project's numpy function is the reference on such input: same bar, and the same best index
    mine = ap_per_class(np.array(g["tp_in"]), np.array(g["conf"]), np.array(g["pred_cls"]), np.array(g["target_cls"]))
    H.assert_equals_reference_tuple(res, mine, name + " (numpy)")


def test_ap_ref_cases_cover_the_corners():
    g = H.golden("ap", "labels_no_predictions")
    assert 1 in g["classes"] and not (g["pred_cls"] == 1).any() and (g["ap"][list(g["classes"]).index(1)] == 0).all()
    g = H.golden("ap", "predictions_no_labels")
    assert 2 not in g["classes"] and (g["pred_cls"] == 2).any()
    g = H.golden("ap", "last_class_gap")
    assert g["classes"].tolist() == [0, 1, 3] and (g["tp"] + g["fn"] == 2).all()      # the leaked n_l: the LAST class's two labels
    g = H.golden("ap", "all_tp_all_fp")
    assert (g["ap"][1] == 0).all() and g["ap"][0, 0] > 0.5


def test_ap_ref_interp_is_np_interp_with_ties():
    g = np.random.default_rng(1)
    for _ in range(40):
        n = int(g.integers(1, 200))
        conf = np.sort(g.integers(1, 30, n).astype(np.float32) / np.float32(30))[::-1].astype(np.float64)
        tpc = g.integers(0, 2, n).cumsum()
        rec, pre = tpc / (37 + 1e-16), tpc / np.arange(1, n + 1)
        px = np.linspace(0, 1, 1000)
        assert all(ap_ref.linspace(k, 1000) == px[k] for k in range(1000))
        for fp, left in ((rec, 0.0), (pre, 1.0)):
            want = np.interp(-px, -conf, fp, left=left)
            got = [ap_ref.interp(-ap_ref.linspace(k, 1000), list(-conf), list(fp), left=left) for k in range(1000)]
            assert np.array_equal(np.array(got), want)


def test_stable_order_breaks_ties_by_arrival():
    conf = np.array([0.5, 0.25, 0.5, 0.5, 0.25], np.float32)
    cls = np.array([1, 0, 0, 1, 0])
    assert ap_ref.stable_order(conf, cls).tolist() == [2, 1, 4, 0, 3]


@pytest.mark.parametrize("name", H.names("cm"))
def test_confusion_ref_equals_the_recorded_reference(name):
    g = H.golden("cm", name)
    nc = int(g["nc"])
    total = np.zeros((nc + 1, nc + 1), np.int64)
    for k in range(int(g["images"])):
        m = np.zeros((nc + 1, nc + 1), np.int64)
        if len(g[f"det{k}"]) and len(g[f"lab{k}"]):                   # test.py never calls process_batch otherwise
            confusion_ref.process_batch(m, nc, g[f"det{k}"], g[f"lab{k}"])
        assert np.array_equal(m, g[f"delta{k}"]), (name, k)
        total += m
    assert np.array_equal(total, g["matrix"])


def test_confusion_quirk_cases_are_what_they_claim():
    assert H.golden("cm", "no_match")["matrix"].tolist() == [[0, 0, 0, 0]] * 3 + [[1, 1, 0, 0]]          # no unmatched detection counted
    assert H.golden("cm", "below_conf")["matrix"][3].tolist() == [1, 1, 0, 0]
    m = H.golden("cm", "match_and_unmatched")["matrix"]
    assert m[1, 0] == 1 and m[3, 1] == 1 and m[0, 3] == 1 and m.sum() == 3


def test_new_flags_default_to_off():
    o = val_module().parse_opt([])
    assert o.plots is False and o.device_stats is False
    o = val_module().parse_opt(["--plots", "--device-stats"])
    assert o.plots is True and o.device_stats is True


def test_new_entry_points_are_in_the_header():
    for name in ("icaf_stats_stage", "icaf_ap_workspace_bytes", "icaf_ap_per_class", "icaf_confusion_matrix"):
        assert name in _lib.SIGNATURES
    assert _lib.STATS_MAX_T == 16 and _lib.STATS_MAX_ROWS == 1 << 24 and _lib.STATS_MAX_CLASSES == 256 and _lib.STATS_SORT_TILE >= 256
