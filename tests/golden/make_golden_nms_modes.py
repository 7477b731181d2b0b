"""Record the reference's apriori-label and merge-NMS results as fixtures:  python tests/golden/make_golden_nms_modes.py /path/to/reference

Imports the reference's real utils.general with the stubs of make_golden.py (its stable torchvision.ops.nms stand-in included, wrapped here so
that the kept indices it returns are recorded) and runs non_max_suppression on the cases of tests/nms_modes_ref.py, in fp32 and on .double()
inputs.  merge-NMS is a constant of that function (`merge = False`, :536): its source is taken IN MEMORY with inspect.getsource, that one
line is replaced — exactly one replacement is asserted — and the result is executed in the module's namespace; nothing of it is written to
disk.  Stored under tests/golden/nms_modes/ is DATA only: the inputs sparsely (the rows with objectness above 0, their indices, the filler
row), the label tables, the indices the greedy core kept, the output rows of both precisions, and summary.json with the reference's own
fp32-against-fp64 deviation of the merged coordinates per case.  Every corner a case is there for is asserted on the reference's own output
before anything is written (README_nms_modes.md says what each case pins)."""
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.dont_write_bytecode = True


def load_reference(root):
    import make_golden                                                       # the stubs live there
    make_golden.REF = root
    general = make_golden.import_reference()[2]
    src = inspect.getsource(general.non_max_suppression)
    assert src.count("merge = False") == 1
    ns = general.__dict__
    plain = general.non_max_suppression
    exec(compile(src.replace("merge = False", "merge = True"), "<non_max_suppression with merge = True>", "exec"), ns)
    merged = ns["non_max_suppression"]
    ns["non_max_suppression"] = plain
    kept = []
    tv_nms = sys.modules["torchvision.ops"].nms

    def recording_nms(boxes, scores, thr):
        i = tv_nms(boxes, scores, thr)                                       # (fp32 inside for both precisions: the same decisions)
        kept.append(i.numpy().copy())
        return i
    general.torchvision.ops.nms = recording_nms
    return plain, merged, kept


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def main(root):
    plain, merged, kept = load_reference(root)
    import nms_modes_ref as R
    outdir = os.path.join(HERE, "nms_modes")
    os.makedirs(outdir, exist_ok=True)
    summary = {}
    for name, c in R.cases().items():
        pred, labels, kw = c["pred"], c["labels"], c["kw"]
        B = pred.shape[0]
        fn = merged if c["merge"] else plain
        runs = {}
        for prec in ("f32", "f64"):
            del kept[:]
            pt = torch.from_numpy(pred.copy())
            lt = [torch.from_numpy(np.asarray(l, np.float32)) for l in labels] if labels is not None else ()
            if prec == "f64":
                pt, lt = pt.double(), [l.double() for l in lt]
            out = fn(pt, labels=lt, **kw)
            runs[prec] = ([o.numpy().astype(np.float64 if prec == "f64" else np.float32) for o in out], [k.copy() for k in kept])
        out32, keep32 = runs["f32"]
        out64, _ = runs["f64"]
        mine, mine_idx, ns = R.run_case(c)
        plain_idx = R.non_max_suppression(pred, labels=labels, **kw)[1]
        # the greedy core ran once per image with candidates: its kept indices are the restatement's plain ones
        nz = [b for b in range(B) if ns[b] > 0]
        assert len(keep32) == len(nz), (name, len(keep32), nz)
        for k, b in zip(keep32, nz):
            assert k[:300].tolist() == plain_idx[b].tolist(), (name, b)
        dev, devulp = 0.0, 0.0
        for b in range(B):
            assert len(out32[b]) == len(mine[b]) == len(out64[b]), (name, b, len(out32[b]), len(mine[b]), len(out64[b]))
            assert np.array_equal(out32[b][:, 4:], mine[b][:, 4:]) and np.array_equal(out32[b][:, 4:], out64[b][:, 4:].astype(np.float32)), (name, b)
            if not (c["merge"] and 1 < ns[b] < 3000):
                assert np.array_equal(out32[b], mine[b]), (name, b)                       # no summation involved: bit for bit
            elif len(out32[b]):
                d = np.abs(out32[b][:, :4].astype(np.float64) - out64[b][:, :4])
                ok = np.isfinite(d)
                dev = max(dev, float(d[ok].max()) if ok.any() else 0.0)
                devulp = max(devulp, float((d / ulp(out32[b][:, :4]))[ok].max()) if ok.any() else 0.0)
        corners(name, c, out32, mine_idx, ns)
        z = {}
        for b in range(B):
            at = np.nonzero(pred[b, :, 4] > 0)[0]
            z[f"at{b}"], z[f"rows{b}"] = at.astype(np.int32), pred[b, at]
            z[f"out32_{b}"], z[f"out64_{b}"] = out32[b], out64[b]
            z[f"keep{b}"] = plain_idx[b].astype(np.int32)
            if labels is not None:
                z[f"labels{b}"] = np.asarray(labels[b], np.float32).reshape(-1, 5)
        filler = pred[0, np.nonzero(pred[0, :, 4] == 0)[0][0]]
        z["filler"], z["shape"] = filler, np.asarray(pred.shape, np.int64)
        np.savez_compressed(os.path.join(outdir, name + ".npz"), **z)
        summary[name] = {"shape": list(pred.shape), "kw": kw, "merge": bool(c["merge"]), "labels": labels is not None, "candidates": ns,
                         "kept": [len(o) for o in out32], "merged_fp32_vs_fp64_max_abs": dev, "merged_fp32_vs_fp64_max_ulp": devulp}
        print(name, summary[name]["candidates"], summary[name]["kept"], dev, devulp)
    with open(os.path.join(outdir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
        f.write("\n")


def corners(name, c, out, idx, ns):
    """what each case exists for, on the reference's own fp32 output"""
    def has(o, box, conf=None):
        m = np.all(np.abs(o[:, :4] - np.asarray(box, np.float32)) < 1e-3, 1)
        return bool((m & (o[:, 4] == np.float32(conf))).any() if conf is not None else m.any())
    if name.startswith("labels") or name == "merge_labels":
        only, both, none = {"labels_nc3_multi": (1, 2, 0), "labels_nc1": (2, 0, 1), "labels_nc3_agnostic_filter": (0, 1, 2), "merge_labels": (1, 2, 0)}[name]
        nc = c["pred"].shape[2] - 5
        if name != "merge_labels":
            assert (out[only][:, 4] == 1).all() and len(out[only]) == 3, (name, out[only])           # labels only; the identical pair kept once
            assert has(out[both], [1180, 250, 1220, 350], 1.0) and (out[both][:, 4] == np.float32(0.99 * 0.99)).sum() == 0      # the label beat the prediction
            assert int((out[both][:, 4] == 1).sum()) == (2 if "filter" in name else 3), name          # the filter removed the class-1 label
            assert (out[both][:, 5] == nc - 1).any() and (out[none][:, 4] < 1).all() and len(out[none])
            assert idx[only][0] < idx[only][1] if len(idx[only]) > 1 else True
        else:
            o = out[only]                           # the identical labels (two hits) and the label pair survive `redundant`; the pair is merged
            assert len(o) == 2 and sorted(o[:, 5].tolist()) == [0, 2] and 300 < o[o[:, 5] == 2][0, 0] + 15 < 301
    if name == "merge_nc1":
        assert not has(out[0], [1480, 250, 1520, 350])                                                 # isolated: dropped
        assert not has(out[1], [1024, 1024, 1028, 1028]) and not has(out[1], [1024, 1024, 1028, 1026])  # IoU exactly 0.5: no hit, both dropped
        assert not np.isnan(out[2]).any() and (out[2][:, 0] > 1400).sum() == 1                         # the zero-area box has no hit and goes; the pair merges
        assert all(0 < len(o) for o in out)
    if name == "merge_nc3_classoff":
        assert all((o[:, 0] > 1400).sum() == 0 for o in out)                                           # different classes: no overlap, both isolated
    if name == "merge_nc3_agnostic":
        assert all((o[:, 0] > 1400).sum() == 1 for o in out)                                           # merged into one
    if name == "merge_counts":
        assert ns == [0, 1, 2, 2999, 3000] and len(out[0]) == 0 and len(out[1]) == 1                   # n = 1: plain
        assert len(out[4]) == len(idx[4])                                                              # n = 3000: plain
    if name == "merge_maxdet":
        assert ns == [720] and len(out[0]) == 300


if __name__ == "__main__":
    main(sys.argv[1])
