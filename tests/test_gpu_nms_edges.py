"""The NMS walk (icaf_nms, nms.hip) where its claim "bit-identical to the CPU algorithm" could break, against
oracle.non_max_suppression(..., return_indices=True): det rows bit for bit, count, keep_idx exactly, and the rows at or behind count as the
test left them.  Every case is one of tests/detect_nms_ref.py nms_cases(), which tests/test_detect_nms_edges_host.py runs on the CPU
through a restatement of the device's decision and shows to catch planted defects:

(a) IoU ulp ladders: isolated pairs whose B is moved ulp by ulp across the place where inter / union > thr flips, so that iou_gt's division
    (inside its +-2^-20 band) decides on both sides and at exact equality — adjacent scores (the 64 x 64 relation inside a step decides)
    and split scores (the kept list of phase A decides), nc = 1 and nc = 3 with and without the class offset;
(b) degenerate boxes (zero width, 0 / 0, negative w, w = inf, inf - inf, subnormal areas, identical boxes), thr = 0 and thr = 1;
(c) a distinct box at the ranks around every round boundary (64, 1024, 4096) with scores over many bins, inside one bin, and all equal;
(d) max_nms by score rank, (e) max_det inside a 64-candidate step, (f) strict > at conf_thres, histogram bin 0 and the top bins."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import detect_nms_ref as R                              # noqa: E402
from icafusion_amd import ops                           # noqa: E402
from oracle import icaf_oracle as oracle                # noqa: E402

DEV = "cuda:0"
CASES = R.nms_cases()
DET_SENTINEL, COUNT_SENTINEL, KEEP_SENTINEL = -77.25, -5, -9


def device_nms(pred, conf_thres, iou_thres, agnostic=False, multi_label=False, max_det=300, max_nms=30000, max_wh=4096.0):
    """one NmsRunner per call, its output block pre-filled -> det, count, keep as numpy"""
    B, rows, no = pred.shape
    runner = ops.NmsRunner(B, rows, no - 5, DEV, multi_label, max_det=max_det)
    runner.det.fill_(DET_SENTINEL); runner.count.fill_(COUNT_SENTINEL); runner.keep.fill_(KEEP_SENTINEL)
    det, count, keep = runner.launch(torch.from_numpy(pred).to(DEV), conf_thres, iou_thres, agnostic, None, max_nms, max_wh)
    torch.cuda.synchronize()
    return det.cpu().numpy(), count.cpu().numpy(), keep.cpu().numpy()


def run_case(name):
    build, kw = CASES[name]
    pred = build()
    rows, idx = oracle.non_max_suppression(pred, return_indices=True, **kw)
    det, count, keep = device_nms(pred, **kw)
    for b in range(pred.shape[0]):
        n = int(count[b])
        assert n == len(idx[b]), f"{name} image {b}: {n} kept, the oracle keeps {len(idx[b])}"
        same = R.u32(det[b, :n]) == R.u32(rows[b])
        assert same.all(), f"{name} image {b}: row {int(np.argwhere(~same)[0][0])} differs: {det[b, :n][~same.all(1)][0]} != {rows[b][~same.all(1)][0]}"
        assert keep[b, :n].tolist() == idx[b].tolist(), f"{name} image {b}: keep_idx differs"
        assert (det[b, n:] == DET_SENTINEL).all() and (keep[b, n:] == KEEP_SENTINEL).all(), f"{name} image {b}: rows behind count were written"
    return pred, rows, idx, count


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_oracle(name):
    run_case(name)


@pytest.mark.parametrize("nc,agnostic", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("thr", R.LADDER_THR)
def test_ladders_reach_the_band(thr, nc, agnostic):
    """the conditions under which (a) tests the division at all, on the data this run used (`-s` prints the counts)"""
    print(f"\n[ladder] thr {thr} nc {nc} agnostic {agnostic}: {R.assert_ladder_reach(R.ladder(thr, nc, agnostic))}")
    assert R.same_step_share(R.PAIRS_PER_IMAGE, "adjacent")[0] >= 0.9 and R.same_step_share(R.PAIRS_PER_IMAGE, "split")[1] == 0.0


@pytest.mark.parametrize("md", R.MAX_DET)
def test_max_det_inside_a_step(md):
    pred, rows, idx, count = run_case(f"max_det-{md}")
    assert int(count[0]) == min(pred.shape[1], md)


@pytest.mark.parametrize("multi", [False, True])
def test_keep_idx_switches_to_ranks_beyond_max_nms(multi):
    for n in R.MAX_NMS_N:
        _, info = R.max_nms_case(n, multi)
        build, kw = CASES[f"max_nms-{'multi' if multi else 'single'}-{n}"]
        det, count, keep = device_nms(build(), **kw)
        boxes = R.xywh2xyxy(info["box_of_rank"])
        has = lambda r: bool((det[0, :count[0], :4] == boxes[r]).all(1).any())
        assert int(keep[0, 0]) == (0 if n > R.MAX_NMS else int(info["cand_of_rank"][0]))
        assert (n < R.MAX_NMS or has(R.MAX_NMS - 1)) and (n <= R.MAX_NMS or not has(R.MAX_NMS))
