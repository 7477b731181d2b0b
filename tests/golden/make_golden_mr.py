#!/usr/bin/env python3
"""Fixtures of the KAIST miss-rate tests (tests/golden/kaist_mr/), recorded from the reference evaluator.

    python tests/golden/make_golden_mr.py /path/to/reference

The reference's `evaluation_script` package is imported at generation time only; what is stored is data:
Every text fixture is stored byte for byte inside a gzip container (load_annotations / read_result_txt read a .gz): the annotation JSON is
1.6 MB, above the 1 MiB limit of a committed file, and the result files are 34,000 lines of numbers.
  KAIST_annotation.json.gz      the reference's annotation file
  {MLPD,MBNet,MSDS-RCNN}_result.txt.gz   the three detector outputs the reference ships
  synth_annotation.json.gz, synth_result.txt.gz   a synthetic set of 14 images on a dyadic lattice (every IoU is exact in fp64) that
                                contains each corner of the matching rules; this script ASSERTS on the reference's own output that
                                each case occurs.  One exception, explained in main(): the reference cannot evaluate an image with
                                more than 1000 detections (IndexError), so it is given the stable top 1000 of the 1,003-detection image
  synth257_annotation.json.gz   the synthetic set with a 257th label in its 256-label image (the device refuses it)
  <name>_match.npz              per result file, from KAISTPedEval driven as evaluate() drives it, all images concatenated in id order:
                                count (I,) kept detections per image; score (N,) sorted scores; order (N,) sorted position -> arrival
                                index within the image; dtm (N, 7) dtMatches (annotation ids) and dtig (N, 7) dtIgnore per set-up;
                                gtig (G, 7) gtIgnore per label row of load_annotations and set-up, gt_seen (G,) = the evaluator
                                returned the label's image (images without detections return None)
  summary.json                  per result file the ten numbers evaluate() prints and the evaluator's wall time on the generating CPU
"""
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kaist_mr")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
os.environ.setdefault("MPLBACKEND", "Agg")

from icafusion_amd.utils.missrate import KEYS, load_annotations  # noqa: E402

SETUP_OF = {"all": 0, "near": 1, "medium": 2, "far": 3, "none": 4, "partial": 5, "heavy": 6}


def synthetic():
    """-> (images, per-image labels, detections (frame0, x, y, w, h, score) in file order, the image whose label gets annotation id 0)"""
    labels = {i: [] for i in range(14)}                     # image -> [x, y, w, h, height, occlusion, ignore or None]
    dets = []

    def lab(i, x, y, w, h, height=60, occ=0, ignore=0):
        labels[i].append([x, y, w, h, height, occ, ignore])

    def det(i, x, y, w, h, score):
        dets.append((i, x, y, w, h, score))

    # 0: two regular labels at exactly equal IoU (0.6): the later label wins, the next detection gets the earlier one
    lab(0, 100, 100, 32, 64); lab(0, 116, 100, 32, 64)
    det(0, 108, 100, 32, 64, 0.75); det(0, 108, 100, 32, 64, 0.625)
    # 1: IoU exactly 0.5 matches
    lab(1, 100, 100, 32, 64)
    det(1, 100, 100, 32, 32, 0.875)
    # 2: two ignored labels (occlusion 2), both >= 0.5, the better one second: the first wins and is never consumed
    lab(2, 100, 100, 32, 64, occ=2); lab(2, 104, 100, 32, 64, occ=2)
    det(2, 104, 100, 32, 64, 0.5); det(2, 104, 100, 32, 64, 0.4375)
    # 3: the label with annotation id 0, matched perfectly: counted as unmatched
    lab(3, 200, 200, 32.5, 64.25)
    det(3, 200, 200, 32.5, 64.25, 0.9375)
    # 4: labels, no detections (its labels do not count)
    lab(4, 50, 50, 32, 64); lab(4, 150, 50, 32, 64)
    # 5: detections, no labels; the best score of the set is a false positive: fppi starts at 1/14 > 0.01 (the -1 wrap)
    det(5, 10, 10, 20, 40, 0.998046875); det(5, 300, 300, 20, 40, 0.5)
    # 6, 7: equal scores within an image and across images
    lab(6, 100, 100, 32, 64); lab(6, 300, 100, 32, 64)
    det(6, 300, 100, 32, 64, 0.5); det(6, 100, 100, 32, 64, 0.5); det(6, 400, 300, 32, 64, 0.5)
    lab(7, 100, 100, 32, 64)
    det(7, 100, 104, 32, 64, 0.5); det(7, 100, 100, 32, 64, 0.5)
    # 8: 1,003 detections with many equal scores (the stable top 1000), a few labels under them
    for j in range(6):
        lab(8, 16 + 96 * j, 24, 16, 32, height=40 + 20 * j, occ=j % 3)
    for k in range(1003):
        det(8, 8 + (k % 50) * 12, 8 + (k // 50) * 16, 16, 32, (k * 37 % 200) / 256 + 1 / 1024)
    # 9: labels on each border of bndRng and one unit over it
    for j, (x, y, w, h) in enumerate([(5, 100, 32, 64), (4, 200, 32, 64), (100, 5, 32, 64), (200, 4, 32, 64), (603, 300, 32, 64),
                                      (604, 400, 32, 64), (300, 443, 32, 64), (400, 444, 32, 64)]):
        lab(9, x, y, w, h)
        det(9, x, y, w, h, 0.25 + j / 64)
    # 10: every height boundary and its neighbours, every occlusion value, a base ignore flag and a label without one
    for j, height in enumerate([0, 1, 2, 44, 45, 46, 54, 55, 56, 114, 115, 116]):
        lab(10, 8 + 48 * j, 16, 32, 64, height=height)
        det(10, 8 + 48 * j, 16, 32, 64, 0.125 + j / 128)
    for j, occ in enumerate([0, 1, 2, 3]):
        lab(10, 8 + 48 * j, 200, 32, 64, occ=occ)
        det(10, 8 + 48 * j, 200, 32, 64, 0.0625 + j / 128)
    lab(10, 300, 200, 32, 64, ignore=1)
    det(10, 300, 200, 32, 64, 0.3125)
    lab(10, 400, 200, 32, 64, ignore=None)
    det(10, 400, 200, 32, 64, 0.34375)
    # 11: 256 labels (the device's limit; four labels per lane), heights and occlusions mixed so that every set-up orders them
    # differently; labels 0 and 200 coincide: a tie between labels four chunks apart
    for j in range(256):
        c, r = (0, 0) if j == 200 else (j % 16, j // 16)
        lab(11, 8 + c * 36, 8 + r * 30, 32, 28, height=30 + (j * 7) % 100, occ=(j // 5) % 3)
    for k in range(96):
        j = (k * 11) % 256
        det(11, 8 + (j % 16) * 36 + (k % 3) * 4, 8 + (j // 16) * 30 + (k % 2) * 2, 32, 28, 0.03125 + (k * 5 % 96) / 128)
    # 12, 13: plain images
    lab(12, 100, 100, 32, 64); det(12, 102, 100, 32, 64, 0.8125); det(12, 500, 100, 32, 64, 0.0078125)
    lab(13, 100, 100, 32, 64, occ=1); det(13, 100, 102, 32, 64, 0.6875)
    return labels, dets, 3


def synthetic_json(labels, id0_image, extra=None):
    order = [id0_image] + [i for i in sorted(labels, reverse=True) if i != id0_image]     # annotation order differs from image order
    anns = []
    for i in order:
        rows = labels[i] + (extra if extra and i == 11 else [])
        for x, y, w, h, height, occ, ignore in rows:
            a = {"id": len(anns), "image_id": i, "category_id": 1, "bbox": [x, y, w, h], "height": height, "occlusion": occ}
            if ignore is not None:
                a["ignore"] = ignore
            anns.append(a)
    return {"images": [{"id": i, "im_name": "set00/V000/I%05d" % i, "height": 512, "width": 640} for i in sorted(labels)],
            "annotations": anns, "categories": [{"id": 0, "name": "__ignore__"}, {"id": 1, "name": "person"}]}


def record(evaluate, ann_path, txt_path, name):
    """Run the reference on one result file -> (match arrays, summary entry, the reference's result objects)."""
    cwd, tmp = os.getcwd(), tempfile.mkdtemp()
    os.chdir(tmp)                                           # loadRes drops a temporary JSON into the working directory
    try:
        t0 = time.perf_counter()
        res = evaluate(os.path.abspath(ann_path), os.path.abspath(txt_path))
        wall = time.perf_counter() - t0
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp)
    table = load_annotations(ann_path)
    I, G = len(table["image_id"]), len(table["id"])
    row_of = {int(v): r for r, v in enumerate(table["id"])}
    numbers = {}
    for k in KEYS[:-1]:
        numbers[k] = float(res[k].summarize(SETUP_OF.get(k, 0)))
    numbers["recall_all"] = float(1 - res["all"].eval["yy"][0][-1])
    # arrival index of every detection id inside its image (ids are file line numbers, 1-based)
    dt_anns = res["all"].cocoDt.dataset["annotations"]
    arrival, seen_n = {}, {}
    for a in dt_anns:
        arrival[a["id"]] = seen_n.get(a["image_id"], 0)
        seen_n[a["image_id"]] = arrival[a["id"]] + 1
    count = np.zeros(I, dtype=np.int32)
    score, order = [], []
    dtm, dtig = [[] for _ in range(7)], [[] for _ in range(7)]
    gtig, gt_seen = np.zeros((G, 7), dtype=np.uint8), np.zeros(G, dtype=bool)
    for k, s in SETUP_OF.items():
        imgs = [e for e in res[k].evalImgs]
        assert len(imgs) == I
        for i, e in enumerate(imgs):
            if e is None:
                continue
            assert e["image_id"] == table["image_id"][i]
            if s == 0:
                count[i] = len(e["dtScores"])
                score.append(np.asarray(e["dtScores"], dtype=np.float64))
                order.append(np.array([arrival[d] for d in e["dtIds"]], dtype=np.int32))
            else:
                assert len(e["dtScores"]) == count[i]
            dtm[s].append(np.asarray(e["dtMatches"][0], dtype=np.int64))
            dtig[s].append(np.asarray(e["dtIgnore"][0], dtype=np.uint8))
            rows = [row_of[g] for g in e["gtIds"]]
            gtig[rows, s] = np.asarray(e["gtIgnore"], dtype=np.uint8)
            gt_seen[rows] = True
    arrays = {"count": count, "score": np.concatenate(score), "order": np.concatenate(order),
              "dtm": np.stack([np.concatenate(v) for v in dtm], 1), "dtig": np.stack([np.concatenate(v) for v in dtig], 1),
              "gtig": gtig, "gt_seen": gt_seen}
    assert len(arrays["score"]) == count.sum() == len(arrays["dtm"])
    np.savez_compressed(os.path.join(OUT, name + "_match.npz"), **arrays)
    print(name, {k: round(v * 100, 4) for k, v in numbers.items()}, "%.2f s" % wall)
    return arrays, {"numbers": numbers, "evaluator_wall_s": wall, "detections": int(len(dt_anns)), "images": I}, res


def check_synthetic(res, table, arrays, labels):
    """Every case the synthetic set exists for really occurs in the reference's output."""
    ev = res["all"]
    E = {e["image_id"]: e for e in ev.evalImgs if e is not None}
    ids_of = {i: [int(v) for v in table["id"][table["off"][i]:table["off"][i + 1]]] for i in range(len(table["image_id"]))}
    iou = lambda i: np.asarray(ev.ious[(i, 1)])                                  # noqa: E731  (detections sorted, labels in annotation order)
    assert iou(0)[0, 0] == iou(0)[0, 1] == 0.6 and list(E[0]["dtMatches"][0]) == [ids_of[0][1], ids_of[0][0]]       # tie -> the later label
    assert iou(1)[0, 0] == 0.5 and E[1]["dtMatches"][0][0] == ids_of[1][0]                                          # IoU exactly 0.5
    assert 0.5 <= iou(2)[0, 0] < iou(2)[0, 1] and list(E[2]["dtMatches"][0]) == [ids_of[2][0]] * 2                  # first ignored label, twice
    assert list(E[2]["dtIgnore"][0]) == [1, 1]
    assert ids_of[3] == [0] and iou(3)[0, 0] == 1.0 and E[3]["dtMatches"][0][0] == 0 and E[3]["gtMatches"][0][0] > 0   # matched to id 0
    assert 4 not in E and len(ids_of[4]) == 2 and 5 in E and len(ids_of[5]) == 0
    assert len(set(E[6]["dtScores"])) == 1 and E[7]["dtScores"][0] == E[6]["dtScores"][0]                           # equal scores
    assert list(arrays["order"][arrays["count"][:6].sum():][:3]) == [0, 1, 2]
    assert len(E[8]["dtScores"]) == 1000 and E[8]["dtMatches"][0].any()      # the stable top 1000 of 1,003 (see main)
    assert list(E[9]["gtIgnore"]) == [0, 0, 0, 0, 1, 1, 1, 1] and sorted(E[9]["gtIds"][:4]) == ids_of[9][0::2]      # on the border / over it
    heights = [l[4] for l in labels[10][:12]]
    for k, s in SETUP_OF.items():
        lo, hi = ev.params.HtRng[s]
        got = dict(zip(res[k].evalImgs[10]["gtIds"], res[k].evalImgs[10]["gtIgnore"]))
        for h, g in zip(heights, ids_of[10][:12]):
            assert got[g] == int(h < lo or h > hi or 0 not in ev.params.OccRng[s]), (k, h)
        assert [got[g] for g in ids_of[10][12:16]] == [int(o not in ev.params.OccRng[s] or 60 < lo or 60 > hi) for o in (0, 1, 2, 3)]
        assert got[ids_of[10][16]] == 1 and got[ids_of[10][17]] == int(0 not in ev.params.OccRng[s] or 60 < lo or 60 > hi)
    assert len(ids_of[11]) == 256 and E[11]["dtMatches"][0].any()
    assert ev.eval["xx"][0][0] > 0.01                                            # the smallest fppi is above the first threshold
    assert not res["night"].evalImgs and res["night"].summarize(0) == -1         # empty night subset
    for k in SETUP_OF:                                                           # every subset matches something and ignores something
        assert arrays["dtm"][:, SETUP_OF[k]].any() and arrays["dtig"][:, SETUP_OF[k]].any(), k


def store_gz(src, name):
    """src (a file) -> OUT/name.gz, the same bytes, a reproducible container."""
    with open(src, "rb") as f, open(os.path.join(OUT, name + ".gz"), "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as g:
            g.write(f.read())


def main(ref_root):
    sys.path.insert(0, ref_root)
    from evaluation_script.evaluation_script import evaluate
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ref_root, "evaluation_script")
    work = tempfile.mkdtemp()                               # the reference reads plain files
    store_gz(os.path.join(src, "KAIST_annotation.json"), "KAIST_annotation.json")
    summary = {}
    for name in ("MLPD", "MBNet", "MSDS-RCNN"):
        txt = os.path.join(src, "state_of_arts", name + "_result.txt")
        store_gz(txt, name + "_result.txt")
        _, summary[name], _ = record(evaluate, os.path.join(src, "KAIST_annotation.json"), txt, name)
    labels, dets, id0 = synthetic()
    ann, ann257 = os.path.join(work, "synth_annotation.json"), os.path.join(work, "synth257_annotation.json")
    with open(ann, "w") as f:
        json.dump(synthetic_json(labels, id0), f)
    with open(ann257, "w") as f:
        json.dump(synthetic_json(labels, id0, extra=[[560, 470, 32, 28, 60, 0, 0]]), f)
    store_gz(ann, "synth_annotation.json")
    store_gz(ann257, "synth257_annotation.json")
    # Every image's detections go into the file in descending score order (equal scores as generated), as in the three shipped files and
    # in what NMS hands to test.py: evaluateImg applies its score permutation to IoU rows that computeIoU has ALREADY sorted (:214), so
    # the reference pairs detections with their own IoUs only when that permutation is the identity.
    dets.sort(key=lambda d: (d[0], -d[5]))
    txt = os.path.join(work, "synth_result.txt")
    # The same line (:214) indexes the 1000 kept IoU rows with the permutation of ALL detections: the reference raises IndexError on any
    # image with more than maxDets detections.  It is therefore fed the stable top 1000 of image 8 (what maxDets intends, :131-132 and
    # :208); synth_result.txt.gz holds all 1,003 and the tests expect the same result from it.
    with open(txt, "w") as f, tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as cut:
        n8 = 0
        for i, x, y, w, h, sc in dets:
            line = "%d,%r,%r,%r,%r,%r\n" % (i + 1, float(x), float(y), float(w), float(h), float(sc))
            f.write(line)
            n8 += i == 8
            if i != 8 or n8 <= 1000:
                cut.write(line)
    assert n8 == 1003
    store_gz(txt, "synth_result.txt")
    arrays, summary["synth"], res = record(evaluate, ann, cut.name, "synth")
    os.remove(cut.name)
    summary["synth"]["detections"] = len(dets)
    check_synthetic(res, load_annotations(ann), arrays, labels)
    assert int(np.diff(load_annotations(os.path.join(OUT, "synth257_annotation.json.gz"))["off"]).max()) == 257
    shutil.rmtree(work)
    with open(os.path.join(OUT, "summary.json"), "w") as f:
        json.dump(summary, f, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
