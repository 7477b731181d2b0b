"""Shared loading of the validation-statistics fixtures (tests/golden/stats/, written by tests/golden/make_golden_stats.py) and the
comparison every test of ap_per_class uses: read once per session, handed out read-only."""
import functools
import glob
import os

import numpy as np

STATS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats")
AP_TOL = 1e-12          # ap: values in [0, 1], sums of at most 101 fp64 terms (error near 1e-14); only the summation order of np.trapz may differ


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def names(kind):
    return tuple(sorted(os.path.basename(f)[len(kind) + 1:-4] for f in glob.glob(os.path.join(STATS_DIR, kind + "_*.npz"))))


@functools.lru_cache(maxsize=None)
def golden(kind, name):
    return _freeze(dict(np.load(os.path.join(STATS_DIR, f"{kind}_{name}.npz"))))


def labels_of(target_cls):
    """(unique_classes, n_l) as the host has them from the labels"""
    return np.unique(np.asarray(target_cls), return_counts=True)


def assert_same(got, want, what=""):
    """Two result dicts of ap_per_class (tests/ap_ref.py or ops.ap_per_class_device): everything exact, ap within AP_TOL."""
    for k in ("p", "r", "f1", "tp", "fp", "fn"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)
    assert int(got["best"]) == int(want["best"]), (what, "best")
    assert np.asarray(got["ap"]).shape == np.asarray(want["ap"]).shape
    assert np.abs(np.asarray(got["ap"]) - np.asarray(want["ap"])).max(initial=0.0) <= AP_TOL, (what, "ap")
    for k in ("perm", "tpc"):
        if k in got and k in want:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def assert_equals_reference_tuple(res, ref_tuple, what=""):
    """A result dict against the tuple of the reference's / the project's numpy ap_per_class: (tp, fp, fn, p, r, ap, f1, classes)."""
    tpn, fpn, fnn, p, r, ap, f1 = ref_tuple[:7]
    i = int(res["best"])
    for got, want, k in ((res["tp"], tpn, "tp"), (res["fp"], fpn, "fp"), (res["fn"], fnn, "fn"), (res["p"][:, i], p, "p"), (res["r"][:, i], r, "r"),
                         (res["f1"][:, i], f1, "f1")):
        assert np.array_equal(np.asarray(got), np.asarray(want)), (what, k)
    assert np.abs(np.asarray(res["ap"]) - np.asarray(ap)).max(initial=0.0) <= AP_TOL, (what, "ap")
