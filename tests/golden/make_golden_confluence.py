"""Record the reference's confluence results as fixtures:  python tests/golden/make_golden_confluence.py /path/to/reference

Loads the reference's utils/confluence.py (cv2 stubbed: only its drawing helpers use it; no bytecode is written beside it), runs its
`confluence` / `confluence_process` on the cases below and stores DATA only under tests/golden/confluence/: the inputs, the kept indices /
rows per case, and summary.json with the reference's wall time per case.  Every corner a case is there for is asserted on the reference's
own output before anything is written (README_confluence.md says what each file pins)."""
import importlib.util
import json
import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from icafusion_amd.synth import synth_crowd_dets, synth_crowd_prediction      # noqa: E402
import confluence_ref                                                          # noqa: E402


def load_reference(root):
    sys.dont_write_bytecode = True
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("reference_confluence", os.path.join(root, "utils", "confluence.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def D(rows):
    return np.asarray(rows, np.float32).reshape(-1, 6)


def select_cases():
    """name -> (dets, class_num, p_thres, check(keep, trace) or None)"""
    cases = {}
    cases["n1"] = (D([[10, 10, 50, 90, 0.9, 0]]), 1, 0.6, lambda k, t: k == [0])
    cases["n2_overlap"] = (D([[10, 10, 50, 90, 0.9, 0], [12, 11, 52, 92, 0.8, 0]]), 1, 0.6, lambda k, t: k == [0])
    cases["n2_far"] = (D([[0, 0, 10, 10, 0.5, 0], [100, 100, 110, 110, 0.9, 0]]), 1, 0.6, lambda k, t: k == [0, 1])
    # three overlapping boxes and one far away, LAST in candidate order and of the lowest conf: it has no neighbour, scores 0 and is picked first
    cases["cluster_isolated"] = (D([[100, 100, 140, 200, 0.9, 0], [102, 101, 142, 202, 0.8, 0], [98, 99, 139, 199, 0.7, 0],
                                    [400, 300, 440, 400, 0.2, 0]]), 1, 0.6, lambda k, t: len(k) == 2 and 3 in k and t[0] == 3)
    cases["duplicates"] = (D([[20, 30, 60, 130, 0.7, 0]] * 3), 1, 0.6, lambda k, t: k == [0])
    # dyadic lattice: x values 0, 6, 2, 8 normalise to 0, .75, .25, 1 exactly: p = 0.5 on the strict bound
    lattice = D([[0, 0, 6, 8, 0.9, 0], [2, 0, 8, 8, 0.8, 0]])
    cases["lattice_on_bound"] = (lattice, 1, 0.5, lambda k, t: k == [0, 1])
    cases["lattice_above_bound"] = (lattice, 1, 0.5000001, lambda k, t: k == [0])
    # p exactly 2: not a neighbour (strict).  Were it one, box 1 (higher conf) would score lower and win; as it is both score 0, box 0 is
    # picked first and removes box 1 (2 < 2.5)
    cases["p_equals_two"] = (D([[0, 0, 4, 4, 0.5, 0], [4, 4, 8, 8, 0.9, 0]]), 1, 2.5, lambda k, t: k == [0])
    # zero-width boxes sharing their x: hi == lo, 0 / 0 = NaN, every comparison false: both kept
    cases["nan_pair"] = (D([[5, 0, 5, 10, 0.9, 0], [5, 2, 5, 12, 0.8, 0]]), 1, 0.6, lambda k, t: k == [0, 1])
    # chain A B C D of equal boxes shifted along x (p = 2 s / (10 + s) for a shift s): A is picked and removes B, which attained C's minimum.
    # C's value must rise to p(C, D) / conf_C, above D's: D is picked and removes C.  With C's stale value C would win and remove D.
    cases["chain"] = (D([[0, 0, 10, 10, 0.95, 0], [1.5, 0, 11.5, 10, 0.5, 0], [3, 0, 13, 10, 0.85, 0], [4.6, 0, 14.6, 10, 0.88, 0]]), 1, 0.3,
                      lambda k, t: k == [0, 3] and t == [0, 3])
    # three classes, class 1 empty, one row of class 7 that no class loop visits
    cases["classes_gap"] = (D([[10, 10, 50, 90, 0.9, 0], [12, 11, 52, 92, 0.8, 2], [11, 10, 51, 91, 0.7, 0], [13, 12, 53, 93, 0.95, 7],
                               [300, 10, 340, 90, 0.6, 2], [14, 12, 54, 92, 0.5, 2]]), 3, 0.6, lambda k, t: k == [0, 1, 4])
    for n, nc in ((48, 1), (63, 1), (64, 3), (65, 1), (96, 3), (255, 1), (256, 3), (257, 1), (320, 1), (600, 1)):
        cases[f"crowd_n{n}_nc{nc}"] = (synth_crowd_dets(n, nc, seed=n), nc, 0.6, lambda k, t, n=n: 0 < len(k) < n)
    return cases


def process_cases():
    """name -> (pred, conf_thres, p_thres): image 1 entirely below conf_thres, image 2 above it in obj only (empty after the class-conf filter)"""
    out = {}
    for nc in (3, 1):
        pred = synth_crowd_prediction(3, 96, 40, nc, seed=7 + nc)
        pred[0, :, 4] = np.where(pred[0, :, 4] > 0, pred[0, :, 4], np.float32(0.05))      # the filler rows: below the threshold, not zero
        if nc > 1:
            pred[0, ::3, 6] = np.float32(0.8)                                               # a second label on every third box
        pred[1, :, 4] *= np.float32(0.1)                                                    # obj < 0.1 everywhere
        pred[2, :, 4] = np.where(pred[2, :, 4] > 0, np.float32(0.3), np.float32(0.0))      # obj passes,
        pred[2, :, 5:] = np.float32(0.3)                                                    # 0.3 * 0.3 does not
        out[f"process_nc{nc}"] = (pred, 0.1, 0.6)
    refusal = synth_crowd_prediction(3, 128, 40, 1, seed=11)
    refusal[1] = synth_crowd_prediction(1, 128, 65, 1, seed=12)[0]                          # 65 candidates against a cap of 64
    out["refusal_cap64"] = (refusal, 0.1, 0.6)
    return out


def main(root):
    ref = load_reference(root)
    outdir = os.path.join(HERE, "confluence")
    os.makedirs(outdir, exist_ok=True)
    summary, sel = {"select": {}, "process": {}}, {}
    for name, (dets, nc, p, check) in select_cases().items():
        t0 = time.perf_counter()
        keep = ref.confluence(dets.copy(), nc, p)
        dt = time.perf_counter() - t0
        trace = []
        mine = confluence_ref.confluence(dets, nc, p, trace=trace)
        assert keep.tolist() == mine.tolist(), name                  # the CPU statement (whose pick order the corner checks read) agrees
        assert check(keep.tolist(), trace), (name, keep.tolist(), trace)
        sel[name + "__dets"], sel[name + "__keep"] = dets, keep.astype(np.int64)
        sel[name + "__nc"], sel[name + "__p"] = np.int64(nc), np.float64(p)
        summary["select"][name] = {"n": len(dets), "nc": nc, "p_thres": p, "kept": len(keep), "picks": len(trace), "reference_seconds": round(dt, 6)}
        print(f"{name}: n {len(dets)} kept {len(keep)} in {dt:.3f} s")
    np.savez_compressed(os.path.join(outdir, "select_cases.npz"), **sel)
    proc = {}
    for name, (pred, conf, p) in process_cases().items():
        t0 = time.perf_counter()
        out = ref.confluence_process(torch.from_numpy(pred.copy()), conf, p)
        dt = time.perf_counter() - t0
        ncand = [len(confluence_ref.candidates(x, conf)) for x in pred]
        if name.startswith("process"):
            assert out[0] is not None and out[1] is None and out[2] is None and ncand[1] == 0 and ncand[2] == 0, (name, ncand)
            assert (pred[2, :, 4] > conf).any()
            assert ncand[0] > 40 if pred.shape[2] > 6 else ncand[0] == 40      # multi-label: more candidates than boxes
        else:
            assert ncand[1] == 65 and max(ncand[0], ncand[2]) <= 64 and all(o is not None for o in out), ncand
        proc[name + "__pred"], proc[name + "__conf"], proc[name + "__p"] = pred, np.float64(conf), np.float64(p)
        proc[name + "__none"] = np.array([o is None for o in out])
        for i, o in enumerate(out):
            proc[f"{name}__out{i}"] = np.zeros((0, 6), np.float32) if o is None else o.numpy().astype(np.float32)
        summary["process"][name] = {"shape": list(pred.shape), "candidates": ncand, "kept": [0 if o is None else len(o) for o in out],
                                    "reference_seconds": round(dt, 6)}
        print(f"{name}: candidates {ncand} kept {summary['process'][name]['kept']} in {dt:.3f} s")
    np.savez_compressed(os.path.join(outdir, "process_cases.npz"), **proc)
    with open(os.path.join(outdir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
