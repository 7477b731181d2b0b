"""Shared loading of the KAIST miss-rate fixtures (tests/golden/kaist_mr/, written by tests/golden/make_golden_mr.py): every table,
store and recorded result is read once per session and handed out read-only."""
import functools
import json
import os

import numpy as np

from icafusion_amd.utils import missrate

MR_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kaist_mr")
SETS = {"MLPD": "KAIST_annotation.json.gz", "MBNet": "KAIST_annotation.json.gz", "MSDS-RCNN": "KAIST_annotation.json.gz",
        "synth": "synth_annotation.json.gz"}


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def table(ann):
    return {k: _freeze(v) for k, v in missrate.load_annotations(os.path.join(MR_DIR, ann)).items()}


@functools.lru_cache(maxsize=None)
def summary():
    with open(os.path.join(MR_DIR, "summary.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: table, image / rows (file order), dt / count (the packed store), golden (the recorded arrays) and their (I, cap) forms
    score / order / dt_id (I, cap, 7) / dt_ignore (I, cap) mask / gt_ignore (G,) mask, gt_seen."""
    tab = table(SETS[name])
    image, rows = missrate.read_result_txt(os.path.join(MR_DIR, name + "_result.txt.gz"))
    dt, count = missrate.pack_detections(len(tab["image_id"]), image, rows)
    g = dict(np.load(os.path.join(MR_DIR, name + "_match.npz")))
    I, cap = dt.shape[:2]
    sel = np.arange(cap)[None, :] < g["count"][:, None]
    score, order = np.zeros((I, cap)), np.full((I, cap), -1, dtype=np.int32)
    dt_id, dt_ignore = np.zeros((I, cap, 7), dtype=np.int64), np.zeros((I, cap), dtype=np.uint8)
    score[sel], order[sel], dt_id[sel] = g["score"], g["order"], g["dtm"]
    dt_ignore[sel] = (g["dtig"].astype(np.uint8) << np.arange(7, dtype=np.uint8)).sum(1).astype(np.uint8)
    gt_ignore = (g["gtig"].astype(np.uint8) << np.arange(7, dtype=np.uint8)).sum(1).astype(np.uint8)
    out = {"table": tab, "image": image, "rows": rows, "dt": dt, "count": count, "kept": g["count"], "sel": sel, "score": score, "order": order,
           "dt_id": dt_id, "dt_ignore": dt_ignore, "gt_ignore": gt_ignore, "gt_seen": g["gt_seen"], "numbers": summary()[name]["numbers"]}
    return {k: _freeze(v) for k, v in out.items()}


def assert_matches_golden(c, order, dt_gt, dt_ignore, gt_ignore):
    """order / dt_gt / dt_ignore / gt_ignore (the arrays of ops.missrate_match or tests/missrate_ref.match_all) equal the reference's
    recorded results EXACTLY: sorted order, matched annotation ids and both ignore masks, for every set-up."""
    sel, tab = c["sel"], c["table"]
    assert (c["kept"] == np.minimum(c["count"], 1000)).all()
    assert np.array_equal(np.asarray(order)[sel], c["order"][sel])
    assert np.array_equal(missrate.matched_ids(np.asarray(dt_gt)[sel], tab["id"]), c["dt_id"][sel])
    assert np.array_equal(np.asarray(dt_ignore)[sel], c["dt_ignore"][sel])
    assert np.array_equal(np.asarray(gt_ignore)[c["gt_seen"]], c["gt_ignore"][c["gt_seen"]])


def assert_numbers(got, want, tol=1e-12):
    assert set(got) == set(missrate.KEYS)
    for k in missrate.KEYS:
        assert abs(got[k] - want[k]) <= tol, (k, got[k], want[k])
