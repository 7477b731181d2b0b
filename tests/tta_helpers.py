"""CPU statements of test-time augmentation for the tests (test infrastructure): scale_img by torch's own operators, the merge of the
reference's models/yolo_test.py:125-131 in numpy, and the oracle composition both the GPU parity test and the live differential test
compare against."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SCALES = (1, 0.83, 0.67)          # models/yolo_test.py:118-119
FLIPS = (None, 3, None)
PAD = 0.447                       # utils/torch_utils.py:267


def sizes(H, W, ratio, gs=32):
    """(Hr, Wr, Hp, Wp) of scale_img (utils/torch_utils.py:262-266), in Python double arithmetic."""
    return int(H * ratio), int(W * ratio), math.ceil(H * ratio / gs) * gs, math.ceil(W * ratio / gs) * gs


def scale_img_cpu(x, ratio, flip, gs=32):
    """scale_img of `x.flip(3) if flip else x` with torch's CPU operators (the expected value of the staging kernel)."""
    x = x.flip(3) if flip else x
    if ratio == 1.0:
        return x
    H, W = x.shape[2:]
    hr, wr, hp, wp = sizes(H, W, ratio, gs)
    y = F.interpolate(x, size=(hr, wr), mode="bilinear", align_corners=False)
    return F.pad(y, [0, wp - wr, 0, hp - hr], value=PAD)


def merge_cpu(zs, W):
    """yi[..., :4] /= si (a correctly rounded fp32 division by float32(si)); fi == 3: yi[..., 0] = W - yi[..., 0]; cat along rows."""
    out = []
    for z, s, f in zip(zs, SCALES, FLIPS):
        z = np.array(z, dtype=np.float32, copy=True)
        z[..., :4] = z[..., :4] / np.float32(s)
        if f == 3:
            z[..., 0] = np.float32(W) - z[..., 0]
        out.append(z)
    return np.concatenate(out, 1)


def oracle_tta(model, rgb, ir, gs=32):
    """The oracle composition: OracleModel.forward on the CPU-resized image pair of every pass, merged on the CPU.  Returns (merged z,
    [z of each pass])."""
    zs = []
    with torch.no_grad():
        for s, f in zip(SCALES, FLIPS):
            zs.append(model.forward(scale_img_cpu(rgb, s, f == 3, gs), scale_img_cpu(ir, s, f == 3, gs))[0].numpy())
    return merge_cpu(zs, rgb.shape[3]), zs
