"""Validation loss with the reference's names (utils/loss.py:15-17, 325-463): smooth_BCE and ComputeLoss, the box / objectness / class loss
the reference's test() reports beside mAP (test.py:132-133, 364-367).  FORWARD VALUE ONLY: the arithmetic runs in HIP kernels
(csrc/loss.hip, icaf_loss), no gradient is computed and the returned tensors carry no autograd graph — this is what validation needs and
the first brick of any later training work, not a training loss.

Not carried over: focal loss (fl_gamma > 0) and autobalance (training-time state) raise NotImplementedError; the ranking / similarity /
varifocal losses of the file are never reached by ComputeLoss.__call__.  At most ops.LOSS_MAX_TARGETS targets per call: more raise, nothing
is truncated."""
import torch

from .. import ops


def smooth_BCE(eps=0.1):
    """positive, negative label-smoothing BCE targets (utils/loss.py:15-17)"""
    return 1.0 - 0.5 * eps, 0.5 * eps


def loss_params(hyp, gr, nl):
    """The parameter block of icaf_loss from a hyp dict, model.gr and the level count (utils/loss.py:334-349): a plain dict of floats."""
    cp, cn = smooth_BCE(eps=hyp.get("label_smoothing", 0.0))
    balance = {3: [4.0, 1.0, 0.4]}.get(nl, [4.0, 1.0, 0.25, 0.06, 0.02])
    return {"box": float(hyp["box"]), "obj": float(hyp["obj"]), "cls": float(hyp["cls"]), "cls_pw": float(hyp["cls_pw"]),
            "obj_pw": float(hyp["obj_pw"]), "anchor_t": float(hyp["anchor_t"]), "gr": float(gr), "cp": cp, "cn": cn,
            "balance": [float(b) for b in balance[:nl]]}


def scale_hyp(hyp, nl, nc, imgsz):
    """train.py:238-241 — the gains as training scales them to the head and the image size; label smoothing off (the CLI's default)."""
    hyp = dict(hyp)
    hyp["box"] *= 3.0 / nl
    hyp["cls"] *= nc / 80.0 * 3.0 / nl
    hyp["obj"] *= (imgsz / 640) ** 2 * 3.0 / nl
    hyp["label_smoothing"] = 0.0
    return hyp


class ComputeLoss:
    """ComputeLoss(model)(p, targets) -> (loss * bs, cat(lbox, lobj, lcls, lrk)) as device tensors, forward value only (no gradients).
    Reads model.hyp, model.gr and the Detect layer's na / nc / nl / anchors as utils/loss.py:327-352 does.  p: the nl raw maps
    (B, na, ny, nx, 5 + nc) fp32 of a forward (out[2]); targets (nt, 6) [image, class, x, y, w, h] on the same device.  No host sync."""

    def __init__(self, model, autobalance=False):
        if autobalance:
            raise NotImplementedError("ComputeLoss(autobalance=True) is training-time state (utils/loss.py:395-399); only the forward value is built")
        h = model.hyp
        if h.get("fl_gamma", 0.0) > 0:
            raise NotImplementedError("focal loss (fl_gamma > 0, utils/loss.py:342-344) is not built")
        parallel = type(model) in (torch.nn.parallel.DataParallel, torch.nn.parallel.DistributedDataParallel)
        det = (model.module if parallel else model).model[-1]                       # Detect() module
        self.gr, self.hyp, self.autobalance = float(model.gr), h, False
        for k in "na", "nc", "nl", "anchors":
            setattr(self, k, getattr(det, k))
        if not 0.0 <= self.gr <= 1.0:
            raise ValueError(f"ComputeLoss: model.gr must be in [0, 1] (got {self.gr:g}): the duplicate rule of tobj needs non-negative values")
        self.params = loss_params(h, self.gr, self.nl)
        self.cp, self.cn, self.balance = self.params["cp"], self.params["cn"], self.params["balance"]
        self._anchors = self.anchors.detach().float().cpu().contiguous()          # host copy, once: icaf_loss takes the anchors from the host
        self._runners = {}

    def __call__(self, p, targets):
        if len(p) != self.nl:
            raise ValueError(f"ComputeLoss: {len(p)} maps for a head of {self.nl} levels")
        if targets.dim() != 2 or targets.shape[1] != 6:
            raise ValueError(f"ComputeLoss: targets must be (nt, 6), got {tuple(targets.shape)}")
        if targets.shape[0] > ops.LOSS_MAX_TARGETS:
            raise ValueError(f"ComputeLoss: {targets.shape[0]} targets exceed the cap of {ops.LOSS_MAX_TARGETS} per call (nothing is truncated)")
        if not targets.is_cuda or not all(t.is_cuda for t in p):
            raise RuntimeError("ComputeLoss runs on the MI355X only (no CPU fallback; see tests/loss_ref.py for the CPU statement used by the tests)")
        B = p[0].shape[0]
        key = (B, tuple(tuple(t.shape[2:4]) for t in p), self.na, self.nc, p[0].device)
        runner = self._runners.pop(key, None)
        if runner is None:
            while len(self._runners) >= 8:                    # rectangular validation batches meet a handful of shapes
                self._runners.pop(next(iter(self._runners)))
            runner = ops.LossRunner(B, key[1], self.na, self.nc, self._anchors, p[0].device)
        self._runners[key] = runner
        items, _ = runner.launch(p, targets.to(torch.float32).contiguous(), self.params)
        items = items.clone()                                 # the runner's output buffer is static
        return items.sum().view(1) * B, items
