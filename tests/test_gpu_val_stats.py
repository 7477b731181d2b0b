"""Validation statistics on the MI355X: icaf_ap_per_class (stable radix sort, integer scans, fp64 curves) against the scalar restatement
tests/ap_ref.py (exact; ap within 1e-12) and the reference's recorded outputs, icaf_stats_stage against the host concatenation between guard
zones, icaf_confusion_matrix against tests/confusion_ref.py, the refusals, and test(device_stats=True, plots=True) against the host path of
the same run."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ap_ref                                                              # noqa: E402
import confusion_ref                                                       # noqa: E402
import val_stats_helpers as H                                              # noqa: E402
from helpers import load_cfg, val_module                                   # noqa: E402
from icafusion_amd import _lib, ops                                        # noqa: E402
from icafusion_amd.synth import synth_state_dict                           # noqa: E402
from icafusion_amd.utils import metrics                                    # noqa: E402

DEV = "cuda:0"
GUARD = 4096
TILE = _lib.STATS_SORT_TILE
T = 10


def pack(tp):
    tp = np.asarray(tp).astype(bool)
    return (tp.astype(np.uint16) << np.arange(tp.shape[1], dtype=np.uint16)[None, :]).sum(1).astype(np.uint16).view(np.int16)


def upload(tp, conf, cls):
    return (torch.from_numpy(pack(tp)).to(DEV), torch.from_numpy(np.array(conf, np.float32)).to(DEV),          # copies: the fixtures are read-only
            torch.from_numpy(np.array(cls, np.int32)).to(DEV), len(conf))


@functools.lru_cache(maxsize=None)
def synth(n, nc, pattern, seed=0):
    """(tp (n, T) bool, conf (n,) fp32, cls (n,) int32, unique_classes, n_l): class 1 (nc >= 3) has predictions and no labels"""
    g = np.random.default_rng(1000 * seed + 7 * n + nc)
    tp = np.logical_and.accumulate(g.random((n, T)) < np.linspace(0.7, 0.2, T)[None, :], 1)
    if pattern == "lattice":
        conf = (g.integers(1, 64, n) / 64.0).astype(np.float32)            # many ties
    elif pattern == "equal":
        conf = np.full(n, 0.5, np.float32)
    else:                                                                  # already sorted, ascending: the worst arrival order
        conf = np.sort((g.integers(1, 4096, n) / 4096.0).astype(np.float32))
    cls = g.integers(0, nc, n).astype(np.int32)
    tcls = g.integers(0, nc, 40 + 3 * nc)
    if nc >= 3:
        tcls = tcls[tcls != 1]
    uc, n_l = np.unique(tcls, return_counts=True)
    out = (tp, conf, cls, uc, n_l)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synth_ref(n, nc, pattern, seed=0):
    tp, conf, cls, uc, n_l = synth(n, nc, pattern, seed)
    return ap_ref.ap_per_class(tp, conf, cls, uc, n_l)


def labelled_rows(want, cls, uc, n_l):
    """Sorted positions whose class has labels: only there is tpc defined"""
    ok = np.isin(cls[want["perm"]], np.asarray(uc)[np.asarray(n_l) > 0])
    return ok


SIZES = [0, 1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 70001]
CASES = [(n, nc, "lattice") for n in SIZES for nc in (1, 3, 80)] + [(n, 3, pat) for n in (TILE + 1, 3 * TILE + 17) for pat in ("equal", "ascending")]


@pytest.mark.parametrize("n,nc,pattern", CASES)
def test_sort_and_ap_equal_the_scalar_restatement(n, nc, pattern):
    """Permutation, tpc, p / r / f1 curves, best index, TP / FP / FN exact; ap within 1e-12.  Sizes around the sort tile, several tiles, many
    ties (a 1/64 lattice, all-equal), ascending arrival order; 1, 3 and 80 classes; a class with predictions and no labels."""
    tp, conf, cls, uc, n_l = synth(n, nc, pattern)
    want = synth_ref(n, nc, pattern)
    got = ops.ap_per_class_device(upload(tp, conf, cls), uc, n_l, T=T, want_perm=True, want_tpc=True)
    ok = labelled_rows(want, cls, uc, n_l)
    got["tpc"], ref = got["tpc"][:, ok], dict(want, tpc=want["tpc"][:, ok])
    H.assert_same(got, ref, (n, nc, pattern))


@pytest.mark.parametrize("name", H.names("ap"))
def test_golden_cases_on_the_device(name):
    """The reference's recorded outputs (distinct confidences) through the same call"""
    g = H.golden("ap", name)
    uc, n_l = H.labels_of(g["target_cls"])
    got = ops.ap_per_class_device(upload(g["tp_in"], g["conf"], g["pred_cls"]), uc, n_l, T=10)
    H.assert_equals_reference_tuple(got, (g["tp"], g["fp"], g["fn"], g["p"], g["r"], g["ap"], g["f1"]), name)
    H.assert_same(got, ap_ref.ap_per_class(g["tp_in"], g["conf"], g["pred_cls"], uc, n_l), name)


def test_distinct_confidences_equal_the_numpy_function():
    """utils.metrics.ap_per_class_device (the reference's signature) against the project's numpy ap_per_class, the reference on well-defined input"""
    g = np.random.default_rng(3)
    n = 5000
    conf = ((g.permutation(n) + 1) / (n + 1)).astype(np.float32)
    assert len(np.unique(conf)) == n
    tp = np.logical_and.accumulate(g.random((n, T)) < 0.5, 1)
    pcls, tcls = g.integers(0, 3, n).astype(np.float64), g.integers(0, 3, 900).astype(np.float64)
    want = metrics.ap_per_class(tp, conf, pcls, tcls)
    for args in ((tp, conf, pcls, tcls), (torch.from_numpy(tp).to(DEV), torch.from_numpy(conf).to(DEV), torch.from_numpy(pcls).to(DEV), tcls)):
        got = metrics.ap_per_class_device(*args)
        for k in (0, 1, 2, 3, 4, 6):
            assert np.array_equal(got[k], want[k]), k
        assert np.abs(got[5] - want[5]).max() <= H.AP_TOL
        assert np.array_equal(got[7], want[7]) and got[7].dtype == want[7].dtype


def test_two_calls_give_the_same_bits_and_arrival_order_only_decides_ties():
    n, nc = 3 * TILE + 17, 3
    tp, conf, cls, uc, n_l = synth(n, nc, "lattice")
    a = ops.ap_per_class_device(upload(tp, conf, cls), uc, n_l, T=T, want_perm=True)
    b = ops.ap_per_class_device(upload(tp, conf, cls), uc, n_l, T=T, want_perm=True)
    for k in ("ap", "p", "r", "f1", "perm", "tp", "fp", "fn"):
        assert np.array_equal(a[k].view(np.int64) if a[k].dtype == np.float64 else a[k], b[k].view(np.int64) if b[k].dtype == np.float64 else b[k]), k
    sh = np.random.default_rng(9).permutation(n)
    c = ops.ap_per_class_device(upload(tp[sh], conf[sh], cls[sh]), uc, n_l, T=T, want_perm=True)
    H.assert_same(c, {k: v for k, v in ap_ref.ap_per_class(tp[sh], conf[sh], cls[sh], uc, n_l).items() if k != "tpc"}, "shuffled")
    # the same multiset of rows: sorted keys agree, the order inside ties (hence the curves) does not
    assert np.array_equal(conf[sh][c["perm"]], conf[a["perm"]]) and np.array_equal(cls[sh][c["perm"]], cls[a["perm"]])
    assert not np.array_equal(a["ap"], c["ap"])


# ---- icaf_stats_stage --------------------------------------------------------------------------------------------------------------------------
def guarded(shape, dtype, fill):
    """A contiguous tensor of `shape` between two guard zones of one flat allocation, everything pre-filled with `fill`."""
    n = int(np.prod(shape))
    item = torch.empty((), dtype=dtype).element_size()
    flat = torch.full((2 * GUARD // item + n,), fill, dtype=dtype, device=DEV)
    return flat, flat[GUARD // item:GUARD // item + n].view(shape)


def guards_intact(flat, n, fill):
    g = GUARD // flat.element_size()
    return bool((flat[:g] == fill).all()) and bool((flat[g + n:] == fill).all())


def stage_batches(seed=4):
    """Three batches (B, max_det 300): correct uint8 (0xFF beyond the count), det fp32 (NaN beyond the count), count"""
    g = np.random.default_rng(seed)
    out = []
    for counts in ([0, 300, 1, 0, 299], [7], [300, 0, 0, 150]):
        B = len(counts)
        correct = np.full((B, 300, T), 0xFF, np.uint8)
        det = np.full((B, 300, 6), np.nan, np.float32)
        for b, c in enumerate(counts):
            correct[b, :c] = np.logical_and.accumulate(g.random((c, T)) < 0.6, 1)
            det[b, :c] = np.concatenate((g.uniform(0, 600, (c, 4)), g.uniform(0.001, 1, (c, 1)), g.integers(0, 3, (c, 1))), 1)
        out.append((correct, det, np.array(counts, np.int32)))
    return out


def host_concat(batches):
    tp = np.concatenate([c[b, :n].astype(bool) for c, d, cnt in batches for b, n in enumerate(cnt)])
    conf = np.concatenate([d[b, :n, 4] for c, d, cnt in batches for b, n in enumerate(cnt)])
    cls = np.concatenate([d[b, :n, 5].astype(np.int32) for c, d, cnt in batches for b, n in enumerate(cnt)])
    return tp, conf, cls


@pytest.mark.parametrize("capacity", [1057, 2000, 700])
def test_stage_equals_the_host_concatenation(capacity):
    """Counts [0, 300, 1, 0, 299] / [7] / [300, 0, 0, 150] (1,057 rows): the store equals the host loop's concatenation, rows beyond every
    count are poison and never read, nothing outside the store, the cursor or the flag is written.  A store of 700 rows takes the first 700
    rows, writes nothing at or beyond its capacity and reports the overflow."""
    batches = stage_batches()
    tp, conf, cls = host_concat(batches)
    total = len(conf)
    fm, mask = guarded((capacity,), torch.int16, 0x5A5A)
    fc, sconf = guarded((capacity,), torch.float32, -7.0)
    fk, scls = guarded((capacity,), torch.int32, -77)
    fs, state = guarded((2,), torch.int32, -5)
    state.zero_()
    for i, (c, d, cnt) in enumerate(batches):
        ops.stats_stage(torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV), torch.from_numpy(cnt).to(DEV), mask, sconf, scls,
                        state[0:1], state[1:2])(ops.current_stream_ptr())
    torch.cuda.synchronize()
    k = min(total, capacity)
    assert total == 1057 and state.tolist() == [total, 1]                             # the cursor counts every row, stored or not
    assert np.array_equal(mask[:k].cpu().numpy(), pack(tp)[:k]) and np.array_equal(sconf[:k].cpu().numpy(), conf[:k])
    assert np.array_equal(scls[:k].cpu().numpy(), cls[:k])
    assert bool((mask[k:] == 0x5A5A).all()) and bool((sconf[k:] == -7.0).all()) and bool((scls[k:] == -77).all())
    assert guards_intact(fm, capacity, 0x5A5A) and guards_intact(fc, capacity, -7.0) and guards_intact(fk, capacity, -77) and guards_intact(fs, 2, -5)
    if capacity == 700:
        assert state[0].item() > capacity and state[1].item() == 1


@functools.lru_cache(maxsize=None)
def wide_batch(B, max_det=3):
    """One batch of B images, max_det 3, counts in [0, 3] with runs of zeros (up to 40 images, so whole threads' shares are empty); poison
    beyond the counts.  Returns the batch and its host concatenation."""
    g = np.random.default_rng(100 + B)
    counts = g.integers(0, max_det + 1, B)
    for start in g.integers(0, B, B // 64):
        counts[start:start + g.integers(1, 41)] = 0
    counts[-1] = max_det                                                              # the last image of the last thread's share stores rows
    correct = np.full((B, max_det, T), 0xFF, np.uint8)
    det = np.full((B, max_det, 6), np.nan, np.float32)
    for b, c in enumerate(counts):
        correct[b, :c] = np.logical_and.accumulate(g.random((c, T)) < 0.6, 1)
        det[b, :c] = np.concatenate((g.uniform(0, 600, (c, 4)), g.uniform(0.001, 1, (c, 1)), g.integers(0, 3, (c, 1))), 1)
    batch = (correct, det, counts.astype(np.int32))
    return batch, host_concat([batch])


@pytest.mark.parametrize("B", [1025, _lib.STATS_MAX_BATCH])
def test_stage_at_batch_counts_where_a_thread_owns_several_images(B):
    """B = 1025 (two images a thread, half the threads without any) and B = 4096 (four a thread, the limit): the prefix of the counts runs
    inside a thread's share and across the workgroup.  The store equals the host concatenation, the cursor the total, nothing else is written."""
    (c, d, cnt), (tp, conf, cls) = wide_batch(B)
    total = len(conf)
    assert total == int(cnt.sum()) and 0 < total < 3 * B and (cnt == 0).sum() > B // 8
    capacity = total + 5
    fm, mask = guarded((capacity,), torch.int16, 0x5A5A)
    fc, sconf = guarded((capacity,), torch.float32, -7.0)
    fk, scls = guarded((capacity,), torch.int32, -77)
    fs, state = guarded((2,), torch.int32, -5)
    state.zero_()
    ops.stats_stage(torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV), torch.from_numpy(cnt).to(DEV), mask, sconf, scls,
                    state[0:1], state[1:2])(ops.current_stream_ptr())
    torch.cuda.synchronize()
    assert state.tolist() == [total, 1]
    assert np.array_equal(mask[:total].cpu().numpy(), pack(tp)) and np.array_equal(sconf[:total].cpu().numpy(), conf)
    assert np.array_equal(scls[:total].cpu().numpy(), cls)
    assert bool((mask[total:] == 0x5A5A).all()) and bool((sconf[total:] == -7.0).all()) and bool((scls[total:] == -77).all())
    assert guards_intact(fm, capacity, 0x5A5A) and guards_intact(fc, capacity, -7.0) and guards_intact(fk, capacity, -77) and guards_intact(fs, 2, -5)


def test_store_object_round_trip_and_any_tp():
    batches = stage_batches(seed=6)
    tp, conf, cls = host_concat(batches)
    store = ops.StatsStore(3 * 5 * 300, T, DEV)
    assert store.rows() == 0 and store.any_tp() is False
    for c, d, cnt in batches:
        c = c.copy()
        c[:, :, :] = np.where(c == 0xFF, 0xFF, 0)                                     # no TP anywhere below the counts
        store.stage(torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV), torch.from_numpy(cnt).to(DEV))
    assert store.rows() == len(conf) and store.any_tp() is False                     # the poison beyond the counts is never read
    got = store.to_host()
    assert not got[0].any() and np.array_equal(got[1], conf) and np.array_equal(got[2], cls)
    c, d, cnt = batches[1]
    store.stage(torch.from_numpy(c).to(DEV), torch.from_numpy(d).to(DEV), torch.from_numpy(cnt).to(DEV))
    assert store.rows() == len(conf) + 7 and store.any_tp() == bool(c[0, :7].any())
    assert np.array_equal(store.to_host()[0][-7:], c[0, :7].astype(bool))


# ---- icaf_confusion_matrix -----------------------------------------------------------------------------------------------------------------
def cm_batch(images, max_det, poison=True):
    """[(det (N, 6), labels (M, 5))] -> predn, det, count, labels, label_off as test.py hands them over (NaN beyond every count)"""
    B = len(images)
    predn = np.full((B, max_det, 4), np.nan if poison else 0.0, np.float32)
    det = np.full((B, max_det, 6), np.nan if poison else 0.0, np.float32)
    off = [0]
    for b, (d, lab) in enumerate(images):
        predn[b, :len(d)], det[b, :len(d)] = d[:, :4], d
        det[b, :len(d), :4] = np.nan if poison else 0.0                               # the boxes are read from predn only
        off.append(off[-1] + len(lab))
    labels = np.concatenate([lab for _, lab in images]).astype(np.float32).reshape(-1, 5)
    return predn, det, np.array([len(d) for d, _ in images], np.int32), labels, np.array(off, np.int32)


def run_cm(nc, images, max_det, group):
    m = torch.zeros((nc + 1, nc + 1), dtype=torch.int32, device=DEV)
    for i in range(0, len(images), group):
        predn, det, count, labels, off = cm_batch(images[i:i + group], max_det)
        lab = torch.from_numpy(labels).to(DEV) if len(labels) else torch.zeros((0, 5), dtype=torch.float32, device=DEV)
        ops.confusion_matrix(torch.from_numpy(predn).to(DEV), torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV), lab,
                             torch.from_numpy(off).to(DEV), m)(ops.current_stream_ptr())
    return m.cpu().numpy().astype(np.int64)


def random_images(seed, count, nc):
    g = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        L, D = int(g.integers(0, 12)), int(g.integers(0, 40))
        lc, lw = g.uniform(50, 450, (L, 2)), g.uniform(20, 120, (L, 2))
        lab = np.concatenate([g.integers(0, nc, (L, 1)), lc - lw / 2, lc + lw / 2], 1).astype(np.float32)
        box = (lab[g.integers(0, L, D), 1:] if L else g.uniform(0, 400, (D, 4))) + g.normal(0, 15, (D, 4))
        if D > 3:
            box[1] = box[0]                                                           # an exact duplicate: an IoU tie between detections
        out.append((np.concatenate([box, g.uniform(0, 1, (D, 1)), g.integers(0, nc, (D, 1))], 1).astype(np.float32), lab))
    return out


@functools.lru_cache(maxsize=None)
def cm_reference(seed, count, nc):
    images = random_images(seed, count, nc)
    m = np.zeros((nc + 1, nc + 1), np.int64)
    for det, lab in images:
        if len(det) and len(lab):
            confusion_ref.process_batch(m, nc, det, lab)
    return images, m


@pytest.mark.parametrize("group", [1, 32])
def test_confusion_matrix_equals_the_restatement(group):
    """The recorded images of the reference (quirk cases included) and 200 random ones (images without labels / detections, duplicate boxes),
    one image or 32 images a launch, NaN in every row beyond the counts"""
    for name in H.names("cm"):
        g = H.golden("cm", name)
        images = [(g[f"det{k}"], g[f"lab{k}"]) for k in range(int(g["images"]))]
        assert np.array_equal(run_cm(int(g["nc"]), images, 64, group), g["matrix"]), name
    images, want = cm_reference(11, 200, 3)
    assert want.sum() > 1000 and want[3].sum() > 0 and want[:, 3].sum() > 0
    assert np.array_equal(run_cm(3, images, 40, group), want)


def test_confusion_matrix_object():
    """utils.metrics.ConfusionMatrix: process_batch (one image, the reference's signature) and process_images give the same float64 matrix"""
    images, want = cm_reference(11, 200, 3)
    a = metrics.ConfusionMatrix(3, device=DEV)
    for det, lab in images[:40]:
        if len(det) and len(lab):
            a.process_batch(torch.from_numpy(det), torch.from_numpy(lab))
    m = np.zeros((4, 4), np.int64)
    for det, lab in images[:40]:
        if len(det) and len(lab):
            confusion_ref.process_batch(m, 3, det, lab)
    assert a.matrix.dtype == np.float64 and np.array_equal(a.matrix, m.astype(np.float64))
    b = metrics.ConfusionMatrix(3, device=DEV)
    predn, det, count, labels, off = cm_batch(images[:40], 40)
    b.process_images(*(torch.from_numpy(x).to(DEV) for x in (predn, det, count, labels, off)))
    assert np.array_equal(b.matrix, a.matrix)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_the_library_text():
    tp, conf, cls, uc, n_l = synth(TILE + 1, 3, "lattice")
    with pytest.raises(_lib.IcafError, match="at most 256 classes"):
        ops.ap_per_class_device(upload(tp, conf, cls), np.arange(257), np.ones(257, int), T=T)
    with pytest.raises(_lib.IcafError, match=r"T must be in \[1, 16\]"):
        ops.ap_per_class_device(upload(tp, conf, cls), uc, n_l, T=17)
    B, md = 2, 8
    det, count = torch.zeros((B, md, 6), device=DEV), torch.full((B,), md, dtype=torch.int32, device=DEV)
    state = torch.zeros((2,), dtype=torch.int32, device=DEV)

    def stores(cap):
        return torch.full((cap,), 3, dtype=torch.int16, device=DEV), torch.zeros((cap,), device=DEV), torch.zeros((cap,), dtype=torch.int32, device=DEV)
    m, c, k = stores(64)
    with pytest.raises(_lib.IcafError, match=r"T must be in \[1, 16\]"):
        ops.stats_stage(torch.ones((B, md, 17), dtype=torch.uint8, device=DEV), det, count, m, c, k, state[0:1], state[1:2])(ops.current_stream_ptr())
    big = stores((1 << 24) + 1)
    with pytest.raises(_lib.IcafError, match="capacity must be in"):
        ops.stats_stage(torch.ones((B, md, T), dtype=torch.uint8, device=DEV), det, count, *big, state[0:1], state[1:2])(ops.current_stream_ptr())
    torch.cuda.synchronize()
    assert state.tolist() == [0, 0] and bool((m == 3).all()) and bool((big[0][:64] == 3).all())          # nothing was launched
    with pytest.raises(_lib.IcafError, match="capacity"):
        ops.StatsStore((1 << 24) + 1, T, DEV)
    with pytest.raises(_lib.IcafError, match="T must be"):
        ops.StatsStore(64, 17, DEV)


# ---- test.py -----------------------------------------------------------------------------------------------------------------------------------
def test_validation_loop_on_the_device(tmp_path, monkeypatch, capsys):
    """test(device_stats=True, plots=True) on five 96 x 128 pairs: the store equals the host path's statistics row for row, the reported
    numbers equal ap_ref on those rows (and the default path's when no confidence is tied), the confusion matrix equals confusion_ref over
    the detections the loop handed over, and the matrix file exists."""
    from test_frontends import make_dataset
    from icafusion_amd.models.yolo import Model
    val = val_module()
    rgb_dir, ir_dir = make_dataset(str(tmp_path / "set"), n=5, size=(96, 128), nc=2, seed=3)
    data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 2, "names": ["person", "car"]}
    model = Model(load_cfg("yolov5s_Add_kaist.yaml")).eval()
    model.load_state_dict(synth_state_dict(model, 0))
    model = model.to(DEV)
    model.compute_dtype, model.autotune, model.use_graph = torch.bfloat16, False, True
    handed, made = [], []

    class Spy(metrics.ConfusionMatrix):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

        def process_images(self, predn, det, count, labels, label_off):
            handed.append(tuple(x.cpu().numpy() for x in (predn, det, count, labels, label_off)))
            super().process_images(predn, det, count, labels, label_off)
    monkeypatch.setattr(val, "ConfusionMatrix", Spy)
    real_match = ops.match_predictions

    def match_with_hits(*a, **k):
        """Seeded weights hit no label: every third row becomes a TP at the first four thresholds, for both paths alike, so that the
        statistics downstream of the matching have something to count"""
        correct = real_match(*a, **k)
        correct[:, ::3, :4] = 1
        return correct
    monkeypatch.setattr(val.ops, "match_predictions", match_with_hits)
    host = []
    plain = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, stats_out=host)
    text_plain = capsys.readouterr().out
    assert not made                                                                  # the default call builds no matrix
    again = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model)
    text_again = capsys.readouterr().out
    strip = lambda s: [l for l in s.splitlines() if not l.startswith("Speed:")]       # noqa: E731
    assert plain[0] == again[0] and strip(text_plain) == strip(text_again)
    out = []
    res = val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, device_stats=True, plots=True, save_dir=tmp_path / "run", stats_out=out)
    text_dev = capsys.readouterr().out
    assert len(res) == 3 and len(res[0]) == 7 and res[1].shape == plain[1].shape and len(res[2]) == 6 and res[2][3:] == plain[2][3:]
    store = out[0]
    tp, conf, cls = store.to_host()
    cat = [np.concatenate([np.asarray(s[k]) for s in host], 0) for k in range(4)]
    assert len(conf) > 0 and np.array_equal(tp, cat[0].astype(bool)) and np.array_equal(conf, cat[1].astype(np.float32))
    assert np.array_equal(cls, cat[2].astype(np.int32))
    tied = len(conf) - len(np.unique(conf))
    print(f"rows {len(conf)}, tied {tied}, any TP {bool(tp.any())}")
    if tp.any():
        uc, n_l = np.unique(cat[3], return_counts=True)
        want = ap_ref.ap_per_class(tp, conf, cls, uc, n_l)
        i = want["best"]
        for got, ref in zip(res[0][:4], (want["p"][:, i].mean(), want["r"][:, i].mean(), want["ap"][:, 0].mean(), want["ap"].mean())):
            assert abs(got - ref) <= H.AP_TOL
    else:
        assert res[0][:4] == (0.0, 0.0, 0.0, 0.0)
    if tied == 0:
        assert all(abs(a - b) <= H.AP_TOL for a, b in zip(res[0][:4], plain[0][:4]))
        assert strip(text_dev)[:len(strip(text_plain))] == strip(text_plain)          # the same table, then the matrix
    assert len(made) == 1 and len(handed) == 3
    m = np.zeros((3, 3), np.int64)
    for predn, det, count, labels, off in handed:
        confusion_ref.process_images(m, 2, predn, det, count, labels, off)
    assert np.array_equal(made[0].matrix, m.astype(np.float64))
    assert (tmp_path / "run" / "confusion_matrix.txt").exists() or (tmp_path / "run" / "confusion_matrix.png").exists()


def test_result_files_are_the_same_bytes_with_and_without_device_stats(tmp_path):
    """test(save_txt, save_conf, save_json) with device_stats off and on, on the inputs of test_validation_loop_on_the_device: both write
    the same set of files — every per-image label file, result.txt, the predictions JSON — with the same bytes, and result.txt is not
    empty (equal empty files would prove nothing)."""
    from test_frontends import make_dataset
    from icafusion_amd.models.yolo import Model
    val = val_module()
    rgb_dir, ir_dir = make_dataset(str(tmp_path / "set"), n=5, size=(96, 128), nc=2, seed=3)
    data = {"val_rgb": rgb_dir, "val_ir": ir_dir, "nc": 2, "names": ["person", "car"]}
    model = Model(load_cfg("yolov5s_Add_kaist.yaml")).eval()
    model.load_state_dict(synth_state_dict(model, 0))
    model = model.to(DEV)
    model.compute_dtype, model.autotune, model.use_graph = torch.bfloat16, False, True
    files = {}
    for device_stats in (False, True):
        run = tmp_path / ("device" if device_stats else "host")
        val.test(data, batch_size=2, imgsz=64, conf_thres=0.05, model=model, save_txt=True, save_conf=True, save_json=True, save_dir=run,
                 device_stats=device_stats)
        files[device_stats] = {str(f.relative_to(run)): f.read_bytes() for f in sorted(run.rglob("*")) if f.is_file()}
    host, dev = files[False], files[True]
    print({k: len(v) for k, v in host.items()})
    assert len(host["labels/result.txt"]) > 0 and "_predictions.json" in host and len(host) >= 3
    assert sorted(host) == sorted(dev)
    for name in host:
        assert host[name] == dev[name], name
