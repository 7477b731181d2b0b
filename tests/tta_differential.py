#!/usr/bin/env python3
"""Differential run for test-time augmentation: the LIVE reference (imported from make_golden.REF, build container only) against the
oracle composition of tests/tta_helpers.py.  Executed as a subprocess by tests/test_tta_host.py (importing the reference re-binds the
`models` / `utils` package names).  The reference's own augment branch cannot run for the two-stream model (models/yolo_test.py:122-123
call forward_once(xi) without the second image), so its pieces are driven as it plainly means them: its scale_img on both images, its
forward_once(xi, xi2), and the de-scale / de-flip statements of its lines 125-130 exec'ed from its source, then torch.cat(y, 1).

    python tests/tta_differential.py
"""
import os
import sys
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.dont_write_bytecode = True

import numpy as np      # noqa: E402
import torch            # noqa: E402
import yaml             # noqa: E402

import make_golden as mg                                               # noqa: E402
import tta_helpers as T                                                # noqa: E402
from icafusion_amd.models import yolo as ours                          # noqa: E402
from icafusion_amd.synth import synth_images, synth_state_dict         # noqa: E402
from oracle import icaf_oracle as oracle                               # noqa: E402

# (config, batch, H, W): the two cases of the GPU parity test
CASES = [("yolov5s_Transfusion_kaist.yaml", 2, 448, 448), ("yolov5s_Transfusion_kaist.yaml", 1, 480, 640)]


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yt, common, general, metrics = mg.import_reference()
    import utils.torch_utils as tu
    assert tu.__file__.startswith(mg.REF)
    # the size table against the reference's own scale_img, on one-pixel-deep images
    for H in range(448, 1281, 96):
        for W in range(448, 1281, 160):
            probe = torch.zeros(1, 1, H, W)
            for p in ours.tta_sizes(H, W, 32):
                assert tuple(tu.scale_img(probe, p[0], gs=32).shape[2:]) == (p[4], p[5]), (H, W, p)
    print("size table equals scale_img's output shapes")
    # the reference's own merge statements (models/yolo_test.py:125-130), exec'ed from its source as reference_differential.match_sweep does
    with open(os.path.join(mg.REF, "models", "yolo_test.py")) as f:
        lines = f.read().splitlines()
    i0 = next(i for i, l in enumerate(lines) if "# de-scale" in l)
    i1 = next(i for i, l in enumerate(lines) if i > i0 and "y.append(yi)" in l)
    merge_lines = compile(textwrap.dedent("\n".join(lines[i0:i1 + 1])), "reference models/yolo_test.py:125-130", "exec")
    for k, (name, B, H, W) in enumerate(CASES):
        seed = 300 + k
        model = yt.Model(os.path.join(mg.REF, "models", "transformer", name)).eval()
        sd = synth_state_dict(model, seed)
        model.load_state_dict(sd)
        rgb, ir = synth_images(B, H, W, seed)
        gs = int(model.stride.max())
        y = []
        with torch.no_grad():
            for si, fi in zip([1, 0.83, 0.67], [None, 3, None]):
                xi = tu.scale_img(rgb.flip(fi) if fi else rgb, si, gs=gs)
                xi2 = tu.scale_img(ir.flip(fi) if fi else ir, si, gs=gs)
                assert torch.equal(xi, T.scale_img_cpu(rgb, si, fi == 3, gs)) and torch.equal(xi2, T.scale_img_cpu(ir, si, fi == 3, gs))
                ns = dict(yi=model.forward_once(xi, xi2)[0].clone(), si=si, fi=fi, img_size=rgb.shape[-2:], y=y)
                exec(merge_lines, ns)                                # de-scale, de-flip, y.append(yi)
        want = torch.cat(y, 1).numpy()
        cfg = yaml.safe_load(open(os.path.join(REPO, "models", "transformer", name)))
        got, zs = T.oracle_tta(oracle.OracleModel(cfg, sd), rgb, ir, gs)
        assert got.shape == want.shape and got.shape[1] == sum(z.shape[1] for z in zs)
        # the merge itself is exact: the reference's in-place `/=` and `W - x` on the ORACLE's rows give the helper's merge bit for bit
        again = []
        for z, si, fi in zip(zs, [1, 0.83, 0.67], [None, 3, None]):
            exec(merge_lines, dict(yi=torch.from_numpy(z.copy()), si=si, fi=fi, img_size=rgb.shape[-2:], y=again))
        assert np.array_equal(torch.cat(again, 1).numpy(), got)
        # forward error: the bounds of reference_differential.model_sweep (the same two implementations, the same operations after them)
        eb = float(np.abs(got[..., :4] - want[..., :4]).max()) / max(1.0, float(np.abs(want[..., :4]).max()))
        es = float(np.abs(got[..., 4:] - want[..., 4:]).max())
        print(f"{name} {B}x{H}x{W}: {got.shape[1]} rows, box error {eb:.2e} (relative), score error {es:.2e}")
        assert eb <= 2e-4 and es <= 2e-4, (name, H, W, eb, es)
    print("TTA_DIFFERENTIAL_OK")


if __name__ == "__main__":
    main()
