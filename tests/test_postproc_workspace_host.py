"""Workspace sizes of the post-processing entry points (icaf_nms_workspace_bytes, icaf_nms_ex_workspace_bytes, icaf_confluence_workspace_bytes,
icaf_ap_workspace_bytes with its tpc offset) — host code of the library, asked without a GPU.  Callers allocate by these numbers and read the
tpc table at the offset, so a change of the layout code must leave every one of them as it was: the expectation is the recorded answer of the
library before its three layout functions shared one arena (tests/golden/postproc_workspace_bytes.json)."""
import ctypes as C
import itertools
import json
import os

from helpers import GOLDEN
from icafusion_amd import _lib
from icafusion_amd._lib import lib

TILE = _lib.STATS_SORT_TILE
# (B, rows, nc): every row count around the 4096-row chunk, the 640 x 640 head, one and many classes, one and many images
NMS_SHAPES = [(B, rows, nc) for B, (rows, nc) in itertools.product((1, 32), ((1, 1), (4095, 3), (4096, 1), (4096, 80), (4097, 3), (25200, 1),
                                                                             (25200, 3), (25200, 80)))]
MAX_LABELS = (0, 1, 100)
CF_SHAPES = [(1, 1, 1, 1), (1, 4095, 3, 1000), (32, 4096, 80, 4096), (1, 4097, 3, 4095), (32, 25200, 1, 4096), (1, 25200, 80, 17)]
AP_SHAPES = list(itertools.product((0, 1, TILE - 1, TILE, TILE + 1, 70001), (1, 10, 16)))


def answers():
    """{query: bytes (or [bytes, tpc_off])} of the loaded library"""
    out, L = {}, lib()
    for B, rows, nc in NMS_SHAPES:
        for multi in (0, 1):
            sz = C.c_size_t(0)
            assert L.icaf_nms_workspace_bytes(B, rows, nc, multi, C.byref(sz)) == 0
            out[f"nms,{B},{rows},{nc},{multi}"] = sz.value
            for ml in MAX_LABELS:
                a = _lib.NmsArgs()
                a.B, a.rows, a.nc, a.multi_label, a.max_labels = B, rows, nc, multi, ml
                assert L.icaf_nms_ex_workspace_bytes(C.byref(a), C.byref(sz)) == 0
                out[f"nms_ex,{B},{rows},{nc},{multi},{ml}"] = sz.value
    for B, rows, nc, max_cand in CF_SHAPES:
        sz = C.c_size_t(0)
        assert L.icaf_confluence_workspace_bytes(B, rows, nc, max_cand, C.byref(sz)) == 0
        out[f"confluence,{B},{rows},{nc},{max_cand}"] = sz.value
    for n, T in AP_SHAPES:
        sz, off = C.c_size_t(0), C.c_size_t(0)
        assert L.icaf_ap_workspace_bytes(n, T, C.byref(sz), C.byref(off)) == 0
        out[f"ap,{n},{T}"] = [sz.value, off.value]
    return out


def test_workspace_queries_answer_as_before():
    with open(os.path.join(GOLDEN, "postproc_workspace_bytes.json")) as f:
        want = json.load(f)
    got = answers()
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, f"{len(bad)} queries differ, first (got, recorded): {list(bad.items())[:5]}"


def test_the_sizes_are_consistent():
    """what the recorded numbers themselves must satisfy: 256-byte granules, the ex query without labels equals the plain one, labels and
    classes only add, and the tpc table ends the AP workspace"""
    got = answers()
    for k, v in got.items():
        for x in (v if isinstance(v, list) else [v]):
            assert x % 256 == 0, k
    for B, rows, nc in NMS_SHAPES:
        for multi in (0, 1):
            assert got[f"nms_ex,{B},{rows},{nc},{multi},0"] == got[f"nms,{B},{rows},{nc},{multi}"]
            assert got[f"nms_ex,{B},{rows},{nc},{multi},100"] > got[f"nms_ex,{B},{rows},{nc},{multi},0"]
        assert got[f"nms,{B},{rows},{nc},1"] >= got[f"nms,{B},{rows},{nc},0"]
    for n, T in AP_SHAPES:
        size, off = got[f"ap,{n},{T}"]
        assert off + (max(n, 1) * 4 * T + 255) // 256 * 256 == size
