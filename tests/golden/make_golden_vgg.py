#!/usr/bin/env python3
"""Generate the VGG16-backbone fixtures by running the REAL reference on the CPU, next to make_golden.py (whose import stubs and
model_case are reused by import; none of the existing fixtures is touched):

    python tests/golden/make_golden_vgg.py

    model_vgg16_kaist_320_b1.npz                  yolov5_VGG16_Transfusion_kaist, seed 21
    model_vgg16_ninfusion_flir_320x352_b2.npz     yolov5_VGG16_NiNfusion_FLIR, seed 22: rectangular input, nc = 3, logits sampled

Besides what model_case records (z, logits, 2048 samples of every layer output, the raw maps' samples) both files carry
    sd_keys / sd_shapes / n_params    the reference model's state_dict key names, their shapes (rows padded with -1) and parameter count
    z_bf16 / z_fp16                   the reference's OWN output after .to(dtype), on the CPU, made as make_golden.py --half-only makes
                                      reference_16bit.npz (fuse() folds nothing here: a VGGblock has no BatchNorm, the head's Convs do)
    dev_bf16 / dev_fp16               [box max, box mean, conf max, conf mean] of |z_16 - z_32|
oracle/ does not know VGGblock, so these recorded 16-bit outputs are the yardstick of the HIP path's 16-bit runs.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                                      # noqa: E402
from icafusion_amd.synth import synth_images, synth_state_dict                 # noqa: E402

CASES = [("model_vgg16_kaist_320_b1", "yolov5_VGG16_Transfusion_kaist.yaml", 1, 320, 320, 21, False),
         ("model_vgg16_ninfusion_flir_320x352_b2", "yolov5_VGG16_NiNfusion_FLIR.yaml", 2, 320, 352, 22, True)]


def vgg_case(yt, name, yaml_name, batch, h, w, seed, sample_logits):
    z32 = mg.model_case(yt, name, yaml_name, batch, h, w, seed, sample_logits=sample_logits)
    path = os.path.join(HERE, name + ".npz")
    rec = dict(np.load(path))
    ref_cfg = os.path.join(mg.REF, "models", "transformer", yaml_name)
    model = yt.Model(ref_cfg).eval()
    sd = model.state_dict()
    rec["sd_keys"] = np.asarray(list(sd))
    shapes = np.full((len(sd), 6), -1, np.int64)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = list(v.shape)
    rec["sd_shapes"] = shapes
    rec["n_params"] = np.asarray(sum(p.numel() for p in model.parameters()), np.int64)
    rgb, ir = synth_images(batch, h, w, seed)
    for dn, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        model = yt.Model(ref_cfg).eval()
        model.load_state_dict(synth_state_dict(model, seed))
        model = model.fuse().eval()
        with torch.no_grad():
            z16 = model.to(dt)(rgb.to(dt), ir.to(dt))[0]
        d = (z16.float() - z32).abs()
        # the 16-bit values themselves: fp16 as such, bf16 as its bit pattern (numpy has no bfloat16)
        rec[f"z_{dn}"] = z16.numpy() if dt is torch.float16 else z16.view(torch.int16).numpy()
        rec[f"dev_{dn}"] = np.asarray([d[..., :4].max(), d[..., :4].mean(), d[..., 4:].max(), d[..., 4:].mean()], np.float64)
        print(name, dn, "box max / mean, conf max / mean:", rec[f"dev_{dn}"].tolist())
    np.savez_compressed(path, **rec)
    print(name, "keys", len(sd), "params", int(rec["n_params"]), "bytes", os.path.getsize(path))


def main():
    torch.set_num_threads(os.cpu_count())
    yt, _, _, _ = mg.import_reference()
    for case in CASES:
        vgg_case(yt, *case)


if __name__ == "__main__":
    main()
