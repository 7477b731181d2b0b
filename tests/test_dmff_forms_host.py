"""Which forms of a DMFF block iteration are built (icaf.h: icaf_dmff_block_forms) — host code of the library, asked without a GPU.  The query runs
the resolve (dmff_fused.hip) and the table lookup (dmff_wide.hip) of the launches themselves; the expectation below is written out as literal
rules and shares nothing with them."""
import ctypes as C
import itertools
import json
import os

import torch

from helpers import GOLDEN
from icafusion_amd import ops
from icafusion_amd._lib import lib

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
CS, HEADS, NS, KSPLITS = (64, 128, 192, 256, 384, 512, 1024), (4, 8, 16), (64, 100, 400, 1600), (1, 2, 4)
# the three-launch instantiations: (C, 16-bit type?, ksplit) -> the token-stream settings built (False: 16-bit, True: fp32)
THREE = {(128, True, 1): (False, True), (128, False, 1): (False,),
         (256, True, 1): (False, True), (256, True, 2): (False, True), (256, True, 4): (False,),
         (512, True, 1): (False,), (512, True, 2): (False, True), (512, True, 4): (False,)}

with open(os.path.join(GOLDEN, "dmff_attn_mlp_lds_bytes.json")) as f:
    LDS = json.load(f)          # icaf_dmff_attn_mlp_lds_bytes before the resolve function existed; -1 = not covered


def hiddens(Cc):
    return (4 * Cc, 2 * Cc, 4 * Cc + 128)


def expect_three(dn, Cc, heads, hidden, ks, stream):
    dk = Cc // heads
    return (stream in THREE.get((Cc, dn != "f32", ks), ()) and hidden % ((128 if Cc == 128 else 256) * ks) == 0
            and Cc % heads == 0 and dk % 8 == 0)


def expect_two(dn, Cc, N, heads, hidden):
    """fill, icaf_dmff_attn_mlp, dispatch_attn_mlp / dispatch_np2 / dispatch_attn_mlp_f32 and launch_attn_mlp's 160 KiB limit as they stood"""
    dk = Cc // heads
    if Cc % 64 or Cc % heads or dk % 8 or hidden % 128 or hidden < 128:
        return False
    if dn == "f32":
        if Cc > 128 or dk > 32:
            return False
    elif Cc > 512 or dk > 128:
        return False
    return 0 < LDS[f"{dn},{Cc},{heads},{N}"] <= 160 * 1024


def test_block_forms_query_over_the_grid():
    bad, counts = [], [0, 0]
    for (dn, dt), Cc, heads, N, ks, stream in itertools.product(DTYPES.items(), CS, HEADS, NS, KSPLITS, (False, True)):
        for hidden in hiddens(Cc):
            got = ops.dmff_block_forms(dt, Cc, N, heads, hidden, ks, stream)
            want = (expect_two(dn, Cc, N, heads, hidden), expect_three(dn, Cc, heads, hidden, ks, stream))
            counts[0] += want[0]
            counts[1] += want[1]
            if got != want:
                bad.append((dn, Cc, heads, N, hidden, ks, stream, got, want))
    assert not bad, f"{len(bad)} points differ, first (dtype, C, heads, N, hidden, ksplit, stream, got, expected): {bad[:5]}"
    assert counts[0] > 500 and counts[1] > 500          # both verdicts occur on both sides: the grid tests something


def test_attn_mlp_lds_bytes_answers_as_before():
    fn, none = lib().icaf_dmff_attn_mlp_lds_bytes, C.c_size_t(-1).value
    for dn, Cc, heads, N in itertools.product(DTYPES, CS, HEADS, NS):
        sz = C.c_size_t(0)
        assert fn(Cc, N, heads, ops.dtype_code(DTYPES[dn]), C.byref(sz)) == 0
        assert (-1 if sz.value == none else sz.value) == LDS[f"{dn},{Cc},{heads},{N}"], (dn, Cc, heads, N)
    assert fn(128, 64, 3, ops.dtype_code(torch.bfloat16), C.byref(sz)) != 0           # C % heads != 0 stays an argument error
