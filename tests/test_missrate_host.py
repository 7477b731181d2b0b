"""KAIST log-average miss rate, host side (no GPU): the numpy FPPI sweep against the reference evaluator's recorded numbers, the scalar
restatement of the matching rules against its recorded per-image results (three shipped detector outputs + the synthetic corner set of
tests/golden/make_golden_mr.py), the file parsers, the C ABI surface and test.py's option."""
import inspect
import os
import re
import types

import numpy as np
import pytest

import missrate_ref
from helpers import REPO, val_module
from icafusion_amd import _lib
from icafusion_amd.utils import missrate
from missrate_helpers import MR_DIR, SETS, assert_matches_golden, assert_numbers, case, table

NAMES = sorted(SETS)


@pytest.mark.parametrize("name", NAMES)
def test_accumulate_reproduces_the_reference_numbers(name):
    """accumulate / summarize fed the reference's own per-image results give its ten numbers within 1e-12 (the same numpy fp64
    operations; the margin covers another libm's log / exp)."""
    c = case(name)
    dt_id, day = c["dt_id"], min(1455, len(c["kept"]))
    got = {}
    for key, setup, subset in missrate.SUBSETS:
        first, last = {"all": (0, None), "day": (0, day), "night": (day, None)}[subset]
        got[key], rec = missrate.accumulate(c["kept"], c["score"], dt_id, c["dt_ignore"], c["gt_ignore"], c["table"]["off"], setup, first, last)
        if key == "all":
            got["recall_all"] = rec
    print(name, {k: got[k] for k in missrate.KEYS})
    assert_numbers(got, c["numbers"])
    if name == "MLPD":                                       # the figures the reference prints for its own MLPD file
        assert [round(got[k] * 100, 2) for k in ("all", "day", "night")] == [7.58, 7.96, 6.95]
    if name == "synth":
        assert got["night"] == -1.0                          # no image in the night subset


def test_accumulate_corner_cases():
    """The -1 wrap (first fppi above the first threshold reads the LAST recall), images without detections not counting their labels, the
    id-0 match counting as unmatched, all-ignored detections leaving zeros, and the empty subsets."""
    off = np.array([0, 1, 2, 3])
    gt_ignore = np.zeros(3, dtype=np.uint8)
    count = np.array([2, 0, 1])
    score = np.array([[0.9, 0.8], [0, 0], [0.7, 0]])
    dt_id = np.zeros((3, 2, 7), dtype=np.int64)
    dt_id[0, 1, :], dt_id[2, 0, :] = 5, 7                    # image 0: FP then TP; image 2: TP
    dt_ignore = np.zeros((3, 2), dtype=np.uint8)
    mr, rec = missrate.accumulate(count, score, dt_id, dt_ignore, gt_ignore, off, 0)
    # npig = 2 (image 1 has no detections); fppi = [1/3, 1/3, 1/3], recall = [0, .5, 1]: thresholds below 1/3 wrap to recall[-1] = 1, the
    # others read the last index at fppi <= thr, also 1
    assert rec == 1.0 and mr == pytest.approx(1e-5, rel=1e-9)
    dt_id[2, 0, :] = 0                                       # the match of image 2 is to annotation id 0: a false positive
    mr, rec = missrate.accumulate(count, score, dt_id, dt_ignore, gt_ignore, off, 0)
    q = np.array([0.5] * 8 + [0.5])                          # fppi = [1/3, 1/3, 2/3]: wrap -> .5; thr .5623 -> index 1 -> .5; thr 1 -> .5
    assert rec == 0.5 and mr == pytest.approx(float(np.exp(np.mean(np.log(1 - q + 1e-5)))), abs=1e-15)
    dt_ignore[:] = 1                                         # every detection ignored: the recalls stay 0
    mr, rec = missrate.accumulate(count, score, dt_id, dt_ignore, gt_ignore, off, 0)
    assert mr == pytest.approx(1 + 1e-5, abs=1e-15)
    assert missrate.accumulate(count, score, dt_id, dt_ignore, gt_ignore, off, 0, 1, 2) == (-1.0, -1.0)      # no evaluated image
    assert missrate.accumulate(count, score, dt_id, dt_ignore, gt_ignore, off, 0, 3, 3) == (-1.0, -1.0)      # empty subset
    assert missrate.accumulate(count, score, dt_id, dt_ignore, gt_ignore | 1, off, 0) == (-1.0, -1.0)        # npig == 0


@pytest.mark.parametrize("name", NAMES)
def test_scalar_restatement_equals_the_reference_exactly(name):
    """tests/missrate_ref.py (the matching rules of include/icaf.h, one label at a time) reproduces every recorded dtMatches / dtIgnore /
    gtIgnore and the sorted order exactly."""
    c = case(name)
    order, dt_gt, dt_ignore, gt_ignore = missrate_ref.match_all(c["table"], c["dt"], c["count"])
    assert_matches_golden(c, order, dt_gt, dt_ignore, gt_ignore)
    got = missrate.summarize(c["table"], c["count"], missrate.sorted_scores(c["dt"], order, np.minimum(c["count"], 1000)), dt_gt, dt_ignore,
                             gt_ignore)
    assert_numbers(got, c["numbers"])


def test_synthetic_set_holds_its_corner_cases():
    """What the generator asserted on the reference's output is visible in the fixtures: an image of 1,003 detections cut to the stable top
    1000, one of 256 labels, a match to annotation id 0, rows that differ from ids, labels without detections and the reverse."""
    c = case("synth")
    tab = c["table"]
    assert len(tab["image_id"]) <= 64 and np.bincount(c["image"]).max() == 1003 and c["count"].max() == 1000
    assert np.diff(tab["off"]).max() == 256 and not np.array_equal(tab["id"], np.arange(len(tab["id"])))
    n_lab = np.diff(tab["off"])
    n_det = np.bincount(c["image"], minlength=len(n_lab))
    assert ((n_lab > 0) & (n_det == 0)).any() and ((n_lab == 0) & (n_det > 0)).any()
    order, dt_gt, _, _ = missrate_ref.match_all(tab, c["dt"], c["count"])
    hit = dt_gt[:, :, 0][c["sel"]]
    assert (tab["id"][hit[hit >= 0]] == 0).any()                                 # matched to id 0 ...
    assert (c["dt_id"][:, :, 0][c["sel"]][hit >= 0] == 0).any()                  # ... and recorded as unmatched by the reference
    wide = missrate.load_annotations(os.path.join(MR_DIR, "synth257_annotation.json.gz"))
    assert np.diff(wide["off"]).max() == 257 == _lib.MISSRATE_MAX_LABELS + 1


def test_result_txt_round_trip(tmp_path):
    c = case("MLPD")
    p = tmp_path / "result.txt"
    missrate.write_result_txt(p, c["image"], c["rows"])
    image, rows = missrate.read_result_txt(p)
    assert np.array_equal(image, c["image"]) and np.array_equal(rows, c["rows"])
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((50, 5)) * np.array([300, 300, 40, 80, 1])        # arbitrary fp64: %.17g reads back to the same bits
    image = rng.integers(0, 7, 50)
    missrate.write_result_txt(p, image, rows)
    image2, rows2 = missrate.read_result_txt(p)
    assert np.array_equal(image2, image) and np.array_equal(rows2, rows)
    dt, count = missrate.pack_detections(7, image, rows)
    assert count.sum() == 50 and all(np.array_equal(dt[i, :count[i]], rows[image == i]) for i in range(7))       # arrival order kept
    p.write_text("1,2,3,4,5\n")
    with pytest.raises(ValueError):
        missrate.read_result_txt(p)
    with pytest.raises(ValueError):
        missrate.pack_detections(7, [7], [[0, 0, 1, 1, 0.5]])
    with pytest.raises(ValueError):
        missrate.pack_detections(7, [0], [[0, 0, 1, 1, float("nan")]])


def test_pack_keeps_the_stable_top_1000():
    scores = (np.arange(1100) * 37 % 100) / 128.0                                # many ties
    rows = np.concatenate([np.tile([1.0, 2.0, 3.0, 4.0], (1100, 1)), scores[:, None]], 1)
    rows[:, 0] = np.arange(1100)                                                 # x = arrival index
    dt, count = missrate.pack_detections(2, np.ones(1100, dtype=np.int64), rows)
    keep = np.sort(np.argsort(-scores, kind="mergesort")[:1000])
    assert list(count) == [0, 1000] and dt.shape == (2, 1000, 5) and np.array_equal(dt[1, :, 0], keep)


def test_annotation_table():
    tab = table("KAIST_annotation.json.gz")
    assert len(tab["image_id"]) == 2252 and len(tab["id"]) == 4254 and tab["off"][-1] == 4254 and tab["im_name"][0] == "set06/V000/I00019"
    assert tab["box"].dtype == np.float64 and set(np.unique(tab["occlusion"])) == {0, 1, 2}
    syn = table("synth_annotation.json.gz")
    for i in range(len(syn["image_id"])):                                        # rows are grouped by image, ids are kept
        assert (np.diff(syn["id"][syn["off"][i]:syn["off"][i + 1]]) > 0).all()


def test_abi_surface_and_citations():
    header = open(os.path.join(REPO, "include", "icaf.h")).read()
    for name, nargs in (("icaf_missrate_stage", 11), ("icaf_missrate_match", 15)):
        assert re.search(rf"\bint {name}\s*\(", header) and len(_lib.SIGNATURES[name][1]) == nargs
    block = header[header.index("KAIST log-average miss rate"):header.index("int icaf_missrate_stage(")]
    for cite in ("evaluation_script/evaluation_script.py", "46-79", "119-179", "181-294", "478-497", ":229-250", "mergesort"):
        assert cite in block, cite
    assert f"ICAF_MISSRATE_MAX_DET = {_lib.MISSRATE_MAX_DET}" in block and f"ICAF_MISSRATE_MAX_LABELS = {_lib.MISSRATE_MAX_LABELS}" in block
    assert f"ICAF_MISSRATE_KEEP = {_lib.MISSRATE_KEEP}" in block and f"ICAF_MISSRATE_SETUPS = {_lib.MISSRATE_SETUPS}" in block
    from icafusion_amd import build
    assert build.PER_FILE["missrate.hip"] == ["-ffp-contract=off"] and build.NO_SCRATCH.search("icaf::missrate_match_kernel(")


def test_built_kernels_use_no_scratch():
    import json
    from icafusion_amd import build
    rep = json.load(open(build.RESOURCES))
    mine = {k: v for k, v in rep.items() if "missrate_" in k}
    assert len(mine) == 2 and all(v["scratch"] == 0 and v.get("vgpr_spill", 0) == 0 and v["file"] == "missrate.hip" for v in mine.values())


def test_option_and_signature():
    val = val_module()
    assert val.parse_opt([]).miss_rate is None and val.parse_opt(["--miss-rate", "a.json"]).miss_rate == "a.json"
    params = list(inspect.signature(val.test).parameters)
    assert params[-1] == "device_letterbox" and params[-2] == "miss_rate" and inspect.signature(val.test).parameters["miss_rate"].default is None


def test_value_errors(tmp_path):
    """nc > 1 without single_cls; an image count that differs from the annotation file's; label files that are all im_names of the file
    but in other positions — each before any device call (no GPU here)."""
    val = val_module()
    with pytest.raises(ValueError, match="single-cls"):
        val.test({"nc": 2}, miss_rate="unused.json")
    ann = os.path.join(MR_DIR, "synth_annotation.json.gz")
    names = table("synth_annotation.json.gz")["im_name"]
    labels = tmp_path / "labels"
    labels.mkdir()

    def dataset(stems):
        for f in labels.iterdir():
            f.unlink()
        files = []
        for s in stems:
            (labels / (s + ".txt")).write_text("")
            files.append(str(labels / (s + ".txt")))
        return types.SimpleNamespace(label_files=files)

    with pytest.raises(ValueError, match="describes 14 images"):
        val.MissRate(ann, dataset([n.replace("/", "_") for n in names[:-1]]), "cpu")
    moved = list(names)
    moved[3], moved[4] = moved[4], moved[3]
    import json
    import gzip
    with gzip.open(ann, "rt") as f:
        data = json.load(f)
    for im, n in zip(data["images"], moved):
        im["im_name"] = n
    other = tmp_path / "moved.json"
    other.write_text(json.dumps(data))
    with pytest.raises(ValueError, match="frame 4 is"):
        val.MissRate(str(other), dataset([n.replace("/", "_") for n in names]), "cpu")
    with pytest.raises(ValueError, match="no CPU fallback"):                     # names agree: only the missing device stops it
        val.MissRate(ann, dataset([n.replace("/", "_") for n in names]), "cpu")
