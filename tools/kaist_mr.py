#!/usr/bin/env python3
"""KAIST log-average miss rate of a result file — the reference's `evaluate(KAIST_annotation.json, result.txt)` stand-alone.

    python tools/kaist_mr.py ANNOTATIONS RESULT_TXT [--day-images 1455]

ANNOTATIONS: the evaluator's annotation JSON; RESULT_TXT: `frame,x,y,w,h,score` lines, frame 1-based (what
`test.py --save-txt --save-conf` leaves as labels/result.txt); a .gz of either is read too.  The matching runs on the GPU (icaf_missrate_match), the FPPI sweep in
numpy; the ten numbers are printed in percent, in the reference's order."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from icafusion_amd.utils import missrate   # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(prog="kaist_mr.py")
    ap.add_argument("annotations")
    ap.add_argument("result_txt")
    ap.add_argument("--day-images", type=int, default=1455, help="the first N image ids are the day subset, the rest the night subset")
    o = ap.parse_args(argv)
    mr = missrate.kaist_miss_rate(o.annotations, o.result_txt, day_images=o.day_images)
    for k in missrate.KEYS:
        print(("recall_all" if k == "recall_all" else "MR_" + k) + ": %.2f" % (mr[k] * 100))
    return mr


if __name__ == "__main__":
    main()
