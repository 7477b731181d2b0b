"""Confluence suppression with the reference's function names (utils/confluence.py:50-193): the alternative to NMS that picks boxes by a
normalised Manhattan proximity instead of IoU.  Everything runs on the device in HIP kernels (csrc/confluence.hip).

Two stated departures from the reference:
  * the cap — an image with more than `max_cand` (at most ops.CONFLUENCE_MAX_CAND) candidates is refused with a ValueError, never truncated:
    the reference has no cap, and a silent top-k would be another algorithm;
  * the conf precondition — the reference crashes when no value p / conf falls below 10000, i.e. for conf <= 2e-4; here conf_thres < 2e-4
    (confluence_process) or a candidate with conf <= 2e-4 (confluence) raises a ValueError before any launch."""
import numpy as np
import torch

from .. import ops

_RUNNERS = {}          # small LRU of ConfluenceRunners for the stand-alone entry points
_MAX_RUNNERS = 4
MIN_CONF = 2e-4        # p < 2 and conf > 2e-4 keep every value p / conf below the reference's starting minimum of 10000


def confluence_device(prediction, conf_thres=0.1, p_thres=0.6, max_cand=ops.CONFLUENCE_MAX_CAND, stream_ptr=None, runner=None):
    """Device-resident confluence: returns (det (B, max_cand, 6), count (B,), keep_idx (B, max_cand)) without any host sync.  det holds the
    kept candidates in ascending candidate order (not by score) and zeros behind them; count[b] < 0 marks an image refused for having
    -count[b] > max_cand candidates.  The three tensors are the runner's STATIC output buffers, as with nms_device."""
    if not prediction.is_cuda:
        raise RuntimeError("confluence_process runs on the MI355X only (no CPU fallback; see tests/confluence_ref.py for the "
                           "CPU statement used by the tests)")
    if conf_thres < MIN_CONF:
        raise ValueError(f"confluence needs conf_thres >= {MIN_CONF:g} (got {conf_thres:g}): with a smaller conf no value p / conf is sure to "
                         "fall below the reference's starting minimum of 10000")
    pred = prediction.float().contiguous()                 # fp16 / bf16 widened first (utils/confluence.py:57-58)
    B, rows, no = pred.shape
    nc = no - 5
    if runner is None:
        key = (B, rows, nc, int(max_cand), pred.device)
        runner = _RUNNERS.pop(key, None)
        if runner is None:
            while len(_RUNNERS) >= _MAX_RUNNERS:
                _RUNNERS.pop(next(iter(_RUNNERS)))
            runner = ops.ConfluenceRunner(B, rows, nc, pred.device, max_cand)
        _RUNNERS[key] = runner
    elif (runner.B, runner.rows, runner.nc) != (B, rows, nc):
        raise ValueError("confluence_device: the runner was built for another (B, rows, nc)")
    return runner.launch(pred, conf_thres, p_thres, stream_ptr)


def refused(counts, cap, what="image"):
    """ValueError for the first negative count of a confluence launch (the image's candidate number, negated)."""
    for i, n in enumerate(counts):
        if n < 0:
            raise ValueError(f"{what} {i}: {-n} confluence candidates exceed the cap of {cap}; raise conf_thres (nothing is truncated)")


def confluence_process(prediction, conf_thres=0.1, p_thres=0.6, max_cand=ops.CONFLUENCE_MAX_CAND):
    """Drop-in for the reference's confluence_process (utils/confluence.py:50-106): per image a (k, 6) tensor [x1, y1, x2, y2, conf, cls] of
    the kept candidates in ascending candidate order, or None for an image without candidates."""
    det, count, _ = confluence_device(prediction, conf_thres, p_thres, max_cand)
    counts = count.tolist()                                # the one device->host sync
    refused(counts, det.shape[1])
    return [det[i, :n].clone() if n else None for i, n in enumerate(counts)]


def confluence(dets, class_num, p_thres=0.6):
    """Drop-in for the reference's confluence (utils/confluence.py:109-193): dets (n, 6) array or tensor [x1, y1, x2, y2, conf, cls] -> the
    kept indices, a sorted int64 array."""
    if isinstance(dets, torch.Tensor):
        d = dets.detach().to(dtype=torch.float32)
    else:
        d = torch.from_numpy(np.ascontiguousarray(np.asarray(dets, dtype=np.float32)))
    if d.dim() != 2 or d.shape[1] != 6:
        raise ValueError(f"confluence: dets must be (n, 6), got {tuple(d.shape)}")
    n = d.shape[0]
    if n == 0:
        return np.zeros((0,), np.int64)
    if n > ops.CONFLUENCE_MAX_CAND:
        raise ValueError(f"confluence: {n} candidates exceed the cap of {ops.CONFLUENCE_MAX_CAND} (nothing is truncated)")
    if not bool((d[:, 4] > MIN_CONF).all()):
        raise ValueError(f"confluence: every conf must exceed {MIN_CONF:g} (the reference crashes otherwise)")
    if not d.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("confluence runs on the MI355X only (no CPU fallback; see tests/confluence_ref.py for the CPU statement "
                               "used by the tests)")
        d = d.cuda()
    cand = d.contiguous().view(1, n, 6)
    _, count, keep = ops.confluence_select(cand, torch.tensor([n], dtype=torch.int32, device=d.device), int(class_num), p_thres)
    return keep[0, :int(count.item())].cpu().numpy().astype(np.int64)
