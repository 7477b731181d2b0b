#!/usr/bin/env python3
"""Generate the ResNet50-backbone fixtures by running the REAL reference on the CPU, next to make_golden_vgg.py (whose case function and
make_golden.py's import stubs are reused by import; none of the existing fixtures is touched):

    python tests/golden/make_golden_resnet.py [name ...]

    model_resnet50_kaist_320_b1.npz                  yolov5_ResNet50_Transfusion_kaist, seed 23
    model_resnet50_ninfusion_flir_320x352_b2.npz     yolov5_ResNet50_NiNfusion_FLIR, seed 24: rectangular input, nc = 3, logits sampled

Contents as the VGG fixtures (make_golden_vgg.py): z, logits, layer and raw samples, sd_keys / sd_shapes / n_params, z_bf16 / z_fp16 (the
reference's OWN 16-bit outputs: fuse() folds the head's Convs, a ResNetlayer keeps its BatchNorms) and dev_bf16 / dev_fp16.  The batch-2
file keeps 1024 of the 2048 samples of every layer output (sample_idx(numel, layer, n=1024), which is the first half of the 2048 draw): with
three full copies of z it would otherwise pass 1,000,000 bytes.  README_resnet50.md says how the synthetic weights were chosen.

    python tests/golden/make_golden_resnet.py --trim-only      # no reference run: apply the sample cut to the recorded files"""
import os
import sys

import numpy as np
import torch

import make_golden_vgg as mv                                                   # noqa: E402  (puts this directory and the stubs in place)

CASES = [("model_resnet50_kaist_320_b1", "yolov5_ResNet50_Transfusion_kaist.yaml", 1, 320, 320, 23, False),
         ("model_resnet50_ninfusion_flir_320x352_b2", "yolov5_ResNet50_NiNfusion_FLIR.yaml", 2, 320, 352, 24, True)]
LAYER_SAMPLES = {"model_resnet50_ninfusion_flir_320x352_b2": 1024}
LIMIT = 1_000_000                                                              # bytes, every fixture of this directory stays below


def trim_layer_samples(name, n):
    """keep the first n samples of every `layer<i>` array: sample_idx draws them in order, so they are sample_idx(numel, i, n=n)"""
    path = os.path.join(mv.HERE, name + ".npz")
    rec = dict(np.load(path))
    for k, v in rec.items():
        if k.startswith("layer") and not k.endswith("_shape"):
            i, numel = int(k[5:]), int(np.prod(rec[k + "_shape"]))
            assert np.array_equal(mv.mg.sample_idx(numel, i)[:n], mv.mg.sample_idx(numel, i, n=n))
            rec[k] = v[:n]
    np.savez_compressed(path, **rec)
    print(name, "layer samples cut to", n, "bytes", os.path.getsize(path))


def main():
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--trim-only" not in sys.argv[1:]:
        torch.set_num_threads(os.cpu_count())
        yt, _, _, _ = mv.mg.import_reference()
    for case in CASES:
        if not names or case[0] in names:
            if "--trim-only" not in sys.argv[1:]:
                mv.vgg_case(yt, *case)
            if case[0] in LAYER_SAMPLES:
                trim_layer_samples(case[0], LAYER_SAMPLES[case[0]])
            size = os.path.getsize(os.path.join(mv.HERE, case[0] + ".npz"))
            assert size < LIMIT, f"{case[0]}.npz: {size} bytes"


if __name__ == "__main__":
    main()
