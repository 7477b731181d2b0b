"""The builders, references and checkers of tests/detect_nms_ref.py, shown to work and shown to fail (CPU only).

A numpy restatement of the device's arithmetic stands in for the kernels: emulate_decode32 for the three decode kernels of detect.hip,
emulate_nms (iou_gt with its band, candidates by score rank and slot) for the walk of nms.hip.  Faithful, it must pass every check the
device tests apply — the float64 decode reference, the exact values, the sentinel rows, the oracle's non_max_suppression on every case of
nms_cases().  With a defect planted it must be rejected by a named case.  The reach conditions of the builders are asserted here too, so
that a change which empties the band of the IoU ladders fails without a GPU.

One plausible defect cannot be caught by anything: a contracted fma(sg, 2, -0.5).  The doubling is exact in binary
floating point, so sg * 2 - 0.5 has one rounding either way and the bits are the same; test_contracted_doubling_is_bit_identical states
that instead."""
import numpy as np
import pytest

import detect_nms_ref as R
from oracle import icaf_oracle as oracle

CASES = R.nms_cases()
_ORACLE = {}


def want(name):
    if name not in _ORACLE:
        build, kw = CASES[name]
        pred = build()
        _ORACLE[name] = (pred, oracle.non_max_suppression(pred, return_indices=True, **kw))
    return _ORACLE[name]


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------------------------------------------
def emulated_level(p, nc, pos, sentinel, defect=None, fma=False):
    na, no = 3, nc + 5
    B, ny, nx, _ = p.shape
    stride, anchors = R.LEVELS[pos]
    rows_total, off = R.three_levels(pos, na, ny, nx)
    zbuf = np.full((B, rows_total, no), sentinel, np.uint32).view(np.float32)
    R.write_level(zbuf, R.emulate_decode32(p, na, no, stride, anchors, defect, fma), off, defect)
    return zbuf, off


@pytest.mark.parametrize("pos", [0, 1, 2])
@pytest.mark.parametrize("nc", R.SWEEP_NC)
def test_logit_sweep_through_the_emulation(nc, pos):
    """1c: every listed logit at every o index and anchor; the faithful emulation passes, each planted decode defect is rejected"""
    na, no = 3, nc + 5
    p = R.sweep_map(*R.SWEEP_SHAPE, na, no)
    raw = R.to_raw(p, na, no)
    for v in R.LOGIT_VALUES:
        hit = raw.view(np.uint32) == v.view(np.uint32)
        assert all(hit[:, a, :, :, o].any() for a in range(na) for o in range(no)), f"{v!r} does not meet every (anchor, o)"
    stride, anchors = R.LEVELS[pos]
    for sentinel in R.SENTINELS:
        zbuf, off = emulated_level(p, nc, pos, sentinel)
        assert not np.isnan(zbuf[:, off:off + raw[0, ..., 0].size]).any()
        ratio = R.check_level(zbuf, sentinel, off, p, na, no, stride, anchors, f"sweep nc {nc} level {pos}")
        print(f"sweep nc {nc} level {pos}: largest err / tolerance {ratio:.3f}")
        zs, _ = emulated_level(p, nc, pos, sentinel, "anchor_swap")
        assert rejected(lambda: R.check_level(zs, sentinel, off, p, na, no, stride, anchors)), "swapped anchor w / h accepted"
        if pos < 2:                                        # behind the last level lies the guard, which the device test checks
            zp, _ = emulated_level(p, nc, pos, sentinel, "row_past")
            assert rejected(lambda: R.check_level(zp, sentinel, off, p, na, no, stride, anchors)), "a row past the level accepted"


def test_contracted_doubling_is_bit_identical():
    p = np.concatenate([R.sweep_map(*R.SWEEP_SHAPE, 3, 14), R.random_map(2, 5, 7, 3, 14, 5)])
    for stride, anchors in R.LEVELS:
        a, b = R.emulate_decode32(p, 3, 14, stride, anchors), R.emulate_decode32(p, 3, 14, stride, anchors, fma=True)
        assert np.array_equal(R.u32(a), R.u32(b))


def test_nan_logits_stay_where_they_are():
    na, no = 3, 8
    p, m = R.nan_map(2, 5, 7, na, no)
    stride, anchors = R.LEVELS[2]
    for sentinel in R.SENTINELS:
        zbuf, off = emulated_level(p, 3, 2, sentinel)
        R.check_level(zbuf, sentinel, off, p, na, no, stride, anchors, "nan")             # NaN in z exactly where the logit is NaN
    z64, lg, raw = R.decode64(p, na, no, stride, anchors)
    assert np.array_equal(np.isnan(raw), R.to_raw(m.astype(np.float32), na, no) > 0) and int(np.isnan(z64).sum()) == int(m.sum())
    assert int(np.isnan(lg).sum()) == int(R.to_raw(m.astype(np.float32), na, no)[..., 5:].sum())


# ------------------------------------------------------------------------------------------------------------------------------------
# NMS
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_faithful_walk_agrees_with_the_oracle(name):
    pred, ref = want(name)
    assert R.same_result(ref, R.emulate_nms(pred, **CASES[name][1])), name


@pytest.mark.parametrize("nc,agnostic", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("thr", R.LADDER_THR)
def test_ladders_reach_the_band(thr, nc, agnostic):
    """2a: >= 100 points inside the band, >= 30 on each side of the oracle's decision, >= 10 with fl(inter / union) == thr"""
    lad = R.ladder(thr, nc, agnostic)
    print(f"ladder thr {thr} nc {nc} agnostic {agnostic}: {R.assert_ladder_reach(lad, f'thr {thr} nc {nc}')}")
    assert np.array_equal(R.ladder_decisions(lad), lad["suppressed"])
    kept = [len(i) for i in want(f"ladder-{thr}-split-nc{nc}" + ("-agnostic" if agnostic else ""))[1][1]]
    assert max(kept) <= 1024 and len(lad["a"]) % R.PAIRS_PER_IMAGE == 0


def test_score_arrangements():
    lo, _ = R.same_step_share(R.PAIRS_PER_IMAGE, "adjacent")
    _, hi = R.same_step_share(R.PAIRS_PER_IMAGE, "split")
    assert lo >= 0.9 and hi == 0.0 and R.PAIRS_PER_IMAGE >= 128
    pred = R.ladder_pred(R.ladder(0.45), "adjacent")
    sc = pred[..., 4] * pred[..., 5]
    assert all(len(np.unique(s)) == len(s) for s in sc) and float(sc.min()) > R.LADDER_CONF


def test_decision_defects_differ_on_the_ladders():
    """>= for >: >= 10 points per threshold (the exact-equality points); the compare without the division and the contracted union: >= 1
    over all thresholds (at 0.5 the product thr * union is exact and the naive compare is right)"""
    total = {"naive": 0, "fused_union": 0}
    for thr in R.LADDER_THR:
        lad = R.ladder(thr)
        diff = {d: int((R.ladder_decisions(lad, d) != lad["suppressed"]).sum()) for d in R.DECISION_DEFECTS}
        print(f"thr {thr}: {diff}")
        assert diff["ge"] >= 10
        for d in total:
            total[d] += diff[d]
    assert total["naive"] >= 1 and total["fused_union"] >= 1, total


@pytest.mark.parametrize("defect,name", [("ge", "ladder-0.45-adjacent-nc1"), ("ge", "ladder-0.6-split-nc1"), ("naive", "ladder-0.6-adjacent-nc1"),
                                         ("fused_union", "ladder-0.6-split-nc1"), ("offset_after_area", "ladder-0.45-adjacent-nc3"),
                                         ("offset_after_area", "ladder-0.6-split-nc3"), ("cut_by_slot", "max_nms-single-9000"),
                                         ("cut_by_slot", "max_nms-multi-5001"), ("rank_edge", "tail-spread-4097"), ("rank_edge", "tail-onebin-1025"),
                                         ("rank_edge", "tail-ties-5121")])
def test_planted_walk_defect_is_caught(defect, name):
    pred, ref = want(name)
    assert not R.same_result(ref, R.emulate_nms(pred, defect=defect, **CASES[name][1])), f"{defect} passes {name}"


@pytest.mark.parametrize("kind", ["spread", "onebin", "ties"])
def test_tail_cases_keep_every_distinct_box(kind):
    """2c: the oracle keeps the first duplicate and the box at every chosen rank, in rank order"""
    for n in R.TAIL_N:
        pred, info = R.tail_case(n, kind)
        rows, idx = want(f"tail-{kind}-{n}")[1]
        m = len(info["distinct"])
        assert len(idx[0]) == m + (1 if n > m else 0), (kind, n)
        assert set(info["cand_of_rank"][info["distinct"]]) <= set(idx[0].tolist())
        if kind == "ties" and n >= 5000:
            assert len(np.unique(pred[0, :, 4] * pred[0, :, 5])) == 2           # 0 (no candidate) and one score
        if kind == "onebin":
            s = (pred[0, :, 4] * pred[0, :, 5])
            assert len(set((s[s > 0].view(np.uint32) >> 16).tolist())) == 1


@pytest.mark.parametrize("multi", [False, True])
def test_max_nms_cuts_by_rank(multi):
    """2d: rank max_nms - 1 is kept, rank max_nms is not, and the indices are ranks exactly when n > max_nms"""
    for n in R.MAX_NMS_N:
        pred, info = R.max_nms_case(n, multi)
        rows, idx = want(f"max_nms-{'multi' if multi else 'single'}-{n}")[1]
        boxes = R.xywh2xyxy(info["box_of_rank"])
        has = lambda r: bool((rows[0][:, :4] == boxes[r]).all(1).any())
        assert has(0) and (n < R.MAX_NMS or has(R.MAX_NMS - 1)) and (n <= R.MAX_NMS or not has(R.MAX_NMS))
        assert info["cand_of_rank"][0] != 0
        assert int(idx[0][0]) == (0 if n > R.MAX_NMS else int(info["cand_of_rank"][0]))


def test_max_det_counts():
    for md in R.MAX_DET:
        pred, (rows, idx) = want(f"max_det-{md}")
        assert len(rows[0]) == min(1000, md)
        assert np.array_equal(rows[0][:, 4], np.sort(pred[0, :, 5])[::-1][:len(rows[0])])


def test_threshold_equality_and_bin_edges():
    pred, ok = R.threshold_pred()
    rows = want("threshold")[1][0][0]
    assert sorted(rows[:, 0].tolist()) == sorted(R.xywh2xyxy(pred[0, ok, :4])[:, 0].tolist())
    (p, info), counts = R.bin_edge_case()
    assert counts["ones"] >= 5000 and counts["tiny"] >= 5000 and counts["subnormal"] >= 100 and counts["above_one"] >= 1
    assert len(want("bin-edges")[1][1][0]) == len(info["distinct"]) + 1
    s = p[0, :, 4] * p[0, :, 5]
    assert (s == np.float32(2.0 ** -17)).sum() == 1 and ((s > 0) & (s < np.float32(2.0 ** -17))).sum() >= 5000
