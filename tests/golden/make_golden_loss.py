"""Record the reference's validation loss as fixtures:  python tests/golden/make_golden_loss.py /path/to/reference

Imports the reference's real utils.loss.ComputeLoss (cv2 / seaborn / thop / torchvision / timm stubbed: none of them is on the loss's path; no
bytecode is written beside it), runs it on the cases below and stores DATA only under tests/golden/loss/: per case the maps, targets,
anchors, hyp and gr, build_targets' five outputs per level, tobj per level (caught by a recorder put in the place of the object's BCEobj
criterion: the reference's files stay untouched and none of its statements is repeated here), and the four loss items of an fp32 run and of
an fp64 run (torch's default dtype switched, every input widened).  summary.json holds the largest relative deviation of the fp32 items from
the fp64 ones over all cases and components: the tolerance budget of the device tests is 4 x that figure (README_loss.md).
Every corner a case is there for is asserted on the reference's own output before anything is written."""
import json
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import loss_ref                                                                # noqa: E402

HYP = {"box": 0.05, "obj": 1.0, "cls": 0.5, "cls_pw": 1.0, "obj_pw": 1.0, "anchor_t": 4.0, "fl_gamma": 0.0, "label_smoothing": 0.0}
HYP_KEYS = ("box", "obj", "cls", "cls_pw", "obj_pw", "anchor_t", "label_smoothing")
YOLO_ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]
STRIDES = (8.0, 16.0, 32.0)


class _Dummy:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return None

    def __getattr__(self, k):
        return _Dummy()


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def load_reference(root):
    _stub("cv2", setNumThreads=lambda *a: None, ocl=_Dummy())
    _stub("seaborn")
    _stub("thop")
    _stub("timm"); _stub("timm.models"); _stub("timm.models.layers", DropPath=_Dummy)
    tv = _stub("torchvision")
    tv.ops = _stub("torchvision.ops", nms=None)
    tv.transforms = _stub("torchvision.transforms")
    tv.utils = _stub("torchvision.utils", save_image=None)
    tv.models = _stub("torchvision.models")
    sys.path.insert(0, root)
    for k in [k for k in sys.modules if k.split(".")[0] in ("models", "utils", "descriptor")]:
        del sys.modules[k]
    import utils.loss as ref_loss
    assert os.path.abspath(ref_loss.__file__).startswith(os.path.abspath(root))
    return ref_loss


def grid_anchors(nl=3):
    return (torch.tensor(YOLO_ANCHORS, dtype=torch.float32).view(3, 3, 2) / torch.tensor(STRIDES).view(3, 1, 1))[:nl].contiguous()


def random_maps(seed, B, na, shapes, nc):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn((B, na, ny, nx, 5 + nc), generator=g) * 1.5).contiguous() for ny, nx in shapes]


def random_targets(seed, images, n, nc, pairs=0):
    """n rows on the given images; the first `pairs` rows are repeated with the same centre and a slightly different size"""
    g = np.random.default_rng(seed)
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0] = g.choice(images, n)
    rows[:, 1] = g.integers(0, nc, n)
    rows[:, 2:4] = g.uniform(0.03, 0.97, (n, 2))
    rows[:, 4:6] = np.exp(g.uniform(np.log(0.03), np.log(0.6), (n, 2)))
    twins = rows[:pairs].copy()
    twins[:, 4:6] *= g.uniform(0.85, 1.2, (pairs, 2)).astype(np.float32)
    twins[:, 1] = g.integers(0, nc, pairs)
    out = np.concatenate((rows, twins)).astype(np.float32)
    return torch.from_numpy(out[np.argsort(out[:, 0], kind="stable")])            # the collate order: by image


def lattice_case():
    """dyadic coordinates, sizes and anchors: every product, ratio and remainder of the assignment is exact"""
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    t = torch.tensor([
        [0, 0, 0.5, 0.5, 0.25, 0.25],                 # gxy = (6, 4) on level 0: remainders 0 in both frames, all five offsets
        [0, 1, 0.53125, 0.5625, 0.25, 0.125],         # gy = 4.5: a remainder of exactly one half fails `< 0.5`, in gxy and in gxi
        [1, 2, 0.09375, 0.125, 0.125, 0.25],          # gx = 1.125 just above 1, gy = 1.0 exactly (fails `> 1.`)
        [1, 0, 0.90625, 0.875, 0.125, 0.25],          # the same from the far border: gxi = (1.125, 1.0)
        [0, 2, 1.0, 0.25, 0.125, 0.25],               # a centre at x = 1.0: gi = nx is clamped, tbox.x = 1.0 (the clamp trap)
        [1, 1, 0.25, 1.0, 0.125, 0.25],               # a centre at y = 1.0
        [0, 0, 0.375, 0.375, 0.25, 0.5],              # gh = 4.0 on level 0: the ratio to an anchor of height 1 is exactly anchor_t: no match
        [0, 0, 0.375, 0.375, 0.25, below],            # one step below: matches
        [1, 1, 0.6875, 0.3125, 1 / 256, 1 / 256],     # matches no anchor on any level
    ], dtype=torch.float32)
    anchors = torch.tensor([[[1, 1], [2, 2], [4, 1]], [[1, 2], [2, 1], [4, 4]], [[0.5, 1], [1, 1], [2, 2]]], dtype=torch.float32)
    return dict(maps=random_maps(11, 2, 3, [(8, 12), (4, 6), (2, 3)], 3), targets=t, anchors=anchors, hyp=dict(HYP), gr=0.0)


def cases():
    out = {"lattice": lattice_case()}
    hyp = dict(HYP, label_smoothing=0.1, cls_pw=0.7, obj_pw=1.3)
    for tag, gr in (("gr1", 1.0), ("gr05", 0.5)):
        out["random_nc3_" + tag] = dict(maps=random_maps(12, 3, 3, [(12, 20), (6, 10), (3, 5)], 3), targets=random_targets(21, [0, 2], 26, 3, pairs=14),
                                        anchors=grid_anchors(), hyp=hyp, gr=gr)
    out["nc1"] = dict(maps=random_maps(13, 2, 3, [(8, 10), (4, 5), (2, 3)], 1), targets=random_targets(22, [0, 1], 8, 1, pairs=2),
                      anchors=grid_anchors(), hyp=dict(HYP), gr=1.0)
    out["empty"] = dict(maps=random_maps(14, 2, 3, [(8, 12), (4, 6), (2, 3)], 2), targets=torch.zeros((0, 6)), anchors=grid_anchors(),
                        hyp=dict(HYP), gr=1.0)
    out["many"] = dict(maps=random_maps(15, 8, 3, [(16, 20), (8, 10), (4, 5)], 2), targets=random_targets(23, list(range(8)), 600, 2),
                       anchors=grid_anchors(), hyp=dict(HYP), gr=1.0)
    out["nl2_na2"] = dict(maps=random_maps(16, 2, 2, [(8, 12), (4, 6)], 2), targets=random_targets(24, [0, 1], 12, 2, pairs=3),
                          anchors=torch.tensor([[[1.5, 2.0], [3.5, 2.5]], [[2.0, 3.5], [4.0, 3.0]]], dtype=torch.float32), hyp=dict(HYP), gr=1.0)
    return out


class Recorder:
    """Stands where the object's BCEobj criterion stood: keeps the target map it is handed, then calls the criterion"""

    def __init__(self, inner):
        self.inner, self.seen = inner, []

    def __call__(self, pred, true):
        self.seen.append(true.detach().clone())
        return self.inner(pred, true)


def run_reference(ref_loss, case, dtype):
    """One run of the reference at `dtype`: (items (4,), build_targets' outputs, tobj per level)"""
    torch.set_default_dtype(dtype)
    try:
        maps = [m.to(dtype) for m in case["maps"]]
        nl, na = len(maps), maps[0].shape[1]
        det = types.SimpleNamespace(na=na, nc=maps[0].shape[4] - 5, nl=nl, anchors=case["anchors"].to(dtype), stride=torch.tensor(STRIDES[:nl]))
        model = types.SimpleNamespace(hyp=dict(case["hyp"]), gr=case["gr"], model=[det], parameters=lambda: iter([torch.zeros(1)]))
        cl = ref_loss.ComputeLoss(model)
        cl.BCEobj = Recorder(cl.BCEobj)
        targets = case["targets"].to(dtype)
        built = cl.build_targets(maps, targets)
        total, items = cl(maps, targets)
        assert torch.equal(total, items.sum() * maps[0].shape[0]) or torch.allclose(total, items.sum() * maps[0].shape[0])
        return items.detach().clone(), built, cl.BCEobj.seen
    finally:
        torch.set_default_dtype(torch.float32)


def prm_of(case, nl):
    from icafusion_amd.utils.loss import loss_params
    return loss_params(case["hyp"], case["gr"], nl)


def main(root):
    # one thread: the reference scatters tobj with duplicate indices (several rows on one cell) after sorting by iou so that the LAST, largest
    # write stays (utils/loss.py:379-382); torch's CPU scatter keeps that order only when it runs sequentially — with a thread pool the
    # `many` case left smaller values in 92 cells of level 0, differently in the fp32 and the fp64 run
    torch.set_num_threads(1)
    sys.path.insert(0, REPO)
    ref_loss = load_reference(root)
    outdir = os.path.join(HERE, "loss")
    os.makedirs(outdir, exist_ok=True)
    summary = {"cases": {}, "max_rel_dev_fp32_vs_fp64": 0.0, "max_abs_dev_tobj_fp32_vs_fp64": 0.0}
    for name, case in cases().items():
        i32, built, tobj32 = run_reference(ref_loss, case, torch.float32)
        i64, built64, tobj64 = run_reference(ref_loss, case, torch.float64)
        tcls, tbox, indices, anch, offsets = built
        nl = len(case["maps"])
        assert i32.dtype == torch.float32 and i64.dtype == torch.float64 and float(i64[3]) == 0.0
        for i in range(nl):                                          # the two runs assign alike: their items differ by rounding only
            assert all(torch.equal(x, y) for x, y in zip(indices[i], built64[2][i])) and torch.equal(tcls[i], built64[0][i]), name
        rel = [abs(float(i32[k]) - float(i64[k])) / abs(float(i64[k])) for k in range(3) if float(i64[k]) != 0.0]
        tdev = max(float((a.double() - b).abs().max()) for a, b in zip(tobj32, tobj64))
        summary["max_rel_dev_fp32_vs_fp64"] = max([summary["max_rel_dev_fp32_vs_fp64"]] + rel)
        summary["max_abs_dev_tobj_fp32_vs_fp64"] = max(summary["max_abs_dev_tobj_fp32_vs_fp64"], tdev)
        counts = [int(indices[i][0].shape[0]) for i in range(nl)]
        cells = [torch.stack(indices[i], 1) for i in range(nl)]
        dup = sum(int(len(c) - len(torch.unique(c, dim=0))) for c in cells)
        # the corners
        if name == "lattice":
            assert all(float(t[ix].min()) == 1.0 for t, ix in zip(tobj32, indices) if len(ix[0])) and min(counts) > 0
            nx0, ny0 = case["maps"][0].shape[3], case["maps"][0].shape[2]                                                   # the clamp trap
            assert ((indices[0][3] == nx0 - 1) & (tbox[0][:, 0] == 1.0)).any() and ((indices[0][2] == ny0 - 1) & (tbox[0][:, 1] == 1.0)).any()
            lvl0 = torch.stack(indices[0], 1).tolist()
            t7 = [r for r, b in zip(lvl0, tbox[0].tolist()) if b[3] == 4.0]
            assert all(case["anchors"][0][r[1]][1] != 1.0 for r in t7) and any(case["anchors"][0][r[1]][1] == 1.0 and b[3] < 4.0 and b[3] > 3.99
                                                                                for r, b in zip(lvl0, tbox[0].tolist()))
        if name.startswith("random_nc3"):
            assert dup > 0 and not (case["targets"][:, 0] == 1).any() and 35 <= len(case["targets"]) <= 45
        if name == "nc1":
            assert float(i32[2]) == 0.0 and float(i64[2]) == 0.0 and sum(counts) > 0
        if name == "empty":
            assert counts == [0] * nl and float(i32[0]) == 0.0 and float(i32[2]) == 0.0 and float(i32[1]) > 0 and not any(t.any() for t in tobj32)
        if name == "many":
            assert min(counts) > 256 and 5 * 3 * len(case["targets"]) > 2 * 2048 and case["maps"][0][..., 0].numel() > 2 * 2048     # several workgroups
        # the CPU statement agrees before anything is written
        mine = loss_ref.compute(case["maps"], case["targets"], case["anchors"], prm_of(case, nl))
        for i in range(nl):
            b, a, gj, gi, tb, tc = loss_ref.rows(mine["levels"][i])
            assert all(torch.equal(x, y) for x, y in zip((b, a, gj, gi), indices[i])) and torch.equal(tb, tbox[i]) and torch.equal(tc, tcls[i]), name
        rec = {"targets": case["targets"].numpy(), "anchors": case["anchors"].numpy(), "gr": np.float64(case["gr"]),
               "hyp": np.array([case["hyp"][k] for k in HYP_KEYS], np.float64), "items32": i32.numpy(), "items64": i64.numpy(),
               "counts": np.array(counts, np.int64)}
        for i in range(nl):
            rec[f"map{i}"] = case["maps"][i].numpy()
            rec[f"indices{i}"] = cells[i].numpy().astype(np.int32)                  # columns b, a, gj, gi
            rec[f"tbox{i}"], rec[f"anch{i}"], rec[f"tcls{i}"] = tbox[i].numpy(), anch[i].numpy(), tcls[i].numpy().astype(np.int32)
            off = offsets[i]
            rec[f"offsets{i}"] = np.zeros((0, 2), np.float32) if not torch.is_tensor(off) else off.numpy()
            rec[f"tobj{i}"], rec[f"tobj64_{i}"] = tobj32[i].numpy(), tobj64[i].numpy()
        path = os.path.join(outdir, name + ".npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < 1 << 20, (name, os.path.getsize(path))
        summary["cases"][name] = {"targets": len(case["targets"]), "counts": counts, "duplicate_rows": dup, "items_fp32": [float(v) for v in i32],
                                  "items_fp64": [float(v) for v in i64], "rel_dev": rel, "tobj_abs_dev": tdev, "bytes": os.path.getsize(path)}
        print(name, counts, "dup", dup, "rel dev", rel, "tobj dev", tdev, os.path.getsize(path), "bytes")
    with open(os.path.join(outdir, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1, sort_keys=True)
        f.write("\n")
    print("budget:", summary["max_rel_dev_fp32_vs_fp64"], "x 4 =", 4 * summary["max_rel_dev_fp32_vs_fp64"])


if __name__ == "__main__":
    main(sys.argv[1])
