"""CPU statement of the validation loss (include/icaf.h, the validation-loss block), written from the rules and not from the kernel: the
target assignment as whole-tensor fp32 torch operations over the (offset, anchor, target) slot grid, the loss terms in fp64 on the matched
rows, the duplicate rule as a scatter with `amax`.  The host tests pin it to what the reference recorded (tests/golden/loss: assignment and
tobj exactly, the loss items against the reference's fp64 run); the GPU tests may then use it for inputs that have no recording (the maps
of a forward).  It takes tensors on any device, so tools/val_loss_bench.py also times it as "the same loss written with torch ops"."""
import math

import torch

OFFSETS = ((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (-0.5, 0.0), (0.0, -0.5))
EPS = 1e-7
PARAM_KEYS = ("box", "obj", "cls", "cls_pw", "obj_pw", "anchor_t", "gr", "cp", "cn")


def _near_low_edge(v):
    """fractional part below one half, and more than one cell away from the border the value is measured from"""
    return ((v - torch.floor(v)) < 0.5) & (v > 1.0)


def assign_level(targets, anchors, ny, nx, anchor_t, B):
    """targets (nt, 6) fp32 [image, class, x, y, w, h], anchors (na, 2) fp32 in grid units -> the slot grid of one level: a dict of
    (5, na, nt) tensors valid / b / a / gj / gi / tcls and tbox (5, na, nt, 4) fp32."""
    t = targets.to(torch.float32)
    anchors = anchors.to(torch.float32)
    nt, na, dev = t.shape[0], anchors.shape[0], t.device
    fx, fy = torch.tensor(float(nx), dtype=torch.float32, device=dev), torch.tensor(float(ny), dtype=torch.float32, device=dev)
    gx, gy, gw, gh = t[:, 2] * fx, t[:, 3] * fy, t[:, 4] * fx, t[:, 5] * fy
    rw, rh = gw[None, :] / anchors[:, 0:1], gh[None, :] / anchors[:, 1:2]                                  # (na, nt)
    worst = torch.maximum(torch.maximum(rw, 1.0 / rw), torch.maximum(rh, 1.0 / rh))
    joined = worst < torch.tensor(anchor_t, dtype=torch.float32, device=dev)
    side = torch.stack((torch.ones_like(gx, dtype=torch.bool), _near_low_edge(gx), _near_low_edge(gy), _near_low_edge(fx - gx),
                        _near_low_edge(fy - gy)))                                                            # (5, nt)
    b, c = t[:, 0].trunc().long(), t[:, 1].trunc().long()
    valid = side[:, None, :] & joined[None, :, :] & ((b >= 0) & (b < B))[None, None, :]
    off = torch.tensor(OFFSETS, dtype=torch.float32, device=dev)
    gi = (gx[None, :] - off[:, 0:1]).trunc().long().clamp(0, nx - 1)                                        # (5, nt)
    gj = (gy[None, :] - off[:, 1:2]).trunc().long().clamp(0, ny - 1)
    box = torch.stack((gx[None, :] - gi.float(), gy[None, :] - gj.float(), gw[None, :].expand(5, nt), gh[None, :].expand(5, nt)), -1)
    shape = (5, na, nt)
    return {"valid": valid, "b": b[None, None, :].expand(shape), "a": torch.arange(na, device=dev)[None, :, None].expand(shape),
            "gj": gj[:, None, :].expand(shape), "gi": gi[:, None, :].expand(shape), "tcls": c[None, None, :].expand(shape),
            "tbox": box[:, None, :, :].expand(5, na, nt, 4)}


def rows(level):
    """The valid slots of a level in slot order: (b, a, gj, gi, tbox, tcls)"""
    keep = level["valid"].reshape(-1).nonzero()[:, 0]
    return tuple(level[k].reshape(-1)[keep] for k in ("b", "a", "gj", "gi")) + (level["tbox"].reshape(-1, 4)[keep], level["tcls"].reshape(-1)[keep])


def bce_logits(x, t, pos_weight):
    return (1.0 - t) * x + (1.0 + (pos_weight - 1.0) * t) * (torch.log1p(torch.exp(-x.abs())) + torch.relu(-x))


def ciou(p, t):
    """(n, 4) centre boxes -> (n,) complete IoU, the fp64 statement of the header's formula"""
    px1, px2, py1, py2 = p[:, 0] - p[:, 2] / 2, p[:, 0] + p[:, 2] / 2, p[:, 1] - p[:, 3] / 2, p[:, 1] + p[:, 3] / 2
    tx1, tx2, ty1, ty2 = t[:, 0] - t[:, 2] / 2, t[:, 0] + t[:, 2] / 2, t[:, 1] - t[:, 3] / 2, t[:, 1] + t[:, 3] / 2
    inter = (torch.minimum(px2, tx2) - torch.maximum(px1, tx1)).clamp(min=0) * (torch.minimum(py2, ty2) - torch.maximum(py1, ty1)).clamp(min=0)
    w1, h1, w2, h2 = px2 - px1, py2 - py1 + EPS, tx2 - tx1, ty2 - ty1 + EPS
    iou = inter / (w1 * h1 + w2 * h2 - inter + EPS)
    cw, ch = torch.maximum(px2, tx2) - torch.minimum(px1, tx1), torch.maximum(py2, ty2) - torch.minimum(py1, ty1)
    rho2 = ((tx1 + tx2 - px1 - px2) ** 2 + (ty1 + ty2 - py1 - py2) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    alpha = v / (v - iou + (1 + EPS))
    return iou - (rho2 / (cw ** 2 + ch ** 2 + EPS) + v * alpha)


def compute(maps, targets, anchors, prm):
    """maps: nl raw Detect maps (B, na, ny, nx, 5 + nc) fp32, targets (nt, 6), anchors (nl, na, 2), prm: PARAM_KEYS + balance -> a dict with
    items (4,) fp64 [lbox * box, lobj * obj, lcls * cls, 0], counts [nl], tobj (nl fp32 maps) and levels (the slot grids)."""
    dev = maps[0].device
    lbox = lobj = lcls = torch.zeros((), dtype=torch.float64, device=dev)
    counts, tobjs, levels = [], [], []
    for i, p in enumerate(maps):
        B, na, ny, nx, no = p.shape
        level = assign_level(targets, anchors[i], ny, nx, prm["anchor_t"], B)
        b, a, gj, gi, tbox, tcls = rows(level)
        tobj = torch.zeros((B, na, ny, nx), dtype=torch.float32, device=dev)
        n = b.shape[0]
        if n:
            q = p[b, a, gj, gi].double()
            s = torch.sigmoid(q[:, :4]) * 2.0
            pbox = torch.cat((s[:, :2] - 0.5, s[:, 2:] ** 2 * anchors[i].double()[a]), 1)
            iou = ciou(pbox, tbox.double())
            lbox = lbox + (1.0 - iou).mean()
            value = ((1.0 - prm["gr"]) + prm["gr"] * iou.clamp(min=0)).float()
            cell = ((b * na + a) * ny + gj) * nx + gi
            tobj.view(-1).scatter_reduce_(0, cell, value, "amax", include_self=True)          # the largest value of a cell stays
            if no > 6:
                want = torch.full_like(q[:, 5:], prm["cn"])
                want[torch.arange(n, device=dev), tcls] = prm["cp"]
                lcls = lcls + bce_logits(q[:, 5:], want, prm["cls_pw"]).mean()
        lobj = lobj + bce_logits(p[..., 4].double(), tobj.double(), prm["obj_pw"]).mean() * prm["balance"][i]
        counts.append(n)
        tobjs.append(tobj)
        levels.append(level)
    items = torch.stack((lbox * prm["box"], lobj * prm["obj"], lcls * prm["cls"], torch.zeros_like(lbox)))
    return {"items": items, "counts": counts, "tobj": tobjs, "levels": levels}
