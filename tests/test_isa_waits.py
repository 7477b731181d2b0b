"""tools/isa_waits.py on hand-written assembly text (no compiler, no GPU): a serial load -> wait -> store loop is listed under (a), an
LDS-DMA loop and a loop whose wait is counted are not; a register-ring loop reports the vmcnt immediates in front of its MFMAs under
(b), waits behind the last MFMA and LDS-only waits left out; an enclosing loop is reported as not innermost."""
import io
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_waits                                         # noqa: E402

SERIAL = """
_Z6serialv:
        s_load_dwordx2 s[0:1], s[4:5], 0x0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
        global_load_dwordx4 v[2:5], v1, s[0:1]
        v_add_u32_e32 v0, 0x200, v0
        s_waitcnt vmcnt(0)
        ds_write_b128 v6, v[2:5]
        s_cbranch_execnz .LBB0_1
; %bb.2:
        s_endpgm
.Lfunc_end0:
"""

DMA_AND_COUNTED = """
_Z3dmav:
.LBB1_1:
        buffer_load_dword v1, s[8:11], 0 offen lds
        s_waitcnt vmcnt(0)
        s_cbranch_scc1 .LBB1_1
.LBB1_2:
        global_load_dwordx4 v[2:5], v1, s[0:1]
        s_waitcnt vmcnt(1)
        ds_write_b128 v6, v[8:11]
        s_cbranch_scc1 .LBB1_2
.LBB1_3:
        global_load_dwordx4 v[2:5], v1, s[0:1]
        s_cbranch_vccz .LBB1_4
        s_waitcnt vmcnt(0)
.LBB1_4:
        s_cbranch_scc1 .LBB1_3
        s_endpgm
"""

RING = """
_Z4ringv:
.LBB2_1:                                ; outer
        v_mov_b32_e32 v9, 0
.LBB2_2:                                ; ring
        s_waitcnt vmcnt(15)
        v_mfma_f32_32x32x16_bf16 v[16:31], v[0:3], v[8:11], v[16:31]
        s_waitcnt vmcnt(14) lgkmcnt(0)
        v_mfma_f32_32x32x16_bf16 v[16:31], v[4:7], v[8:11], v[16:31]
        global_load_dwordx4 v[0:3], v12, s[0:1]
        global_load_dwordx4 v[4:7], v12, s[0:1] offset:1024
        s_waitcnt lgkmcnt(0)
        s_waitcnt vmcnt(12)
        v_mfma_f32_32x32x16_bf16 v[16:31], v[32:35], v[8:11], v[16:31]
        s_waitcnt vmcnt(0)
        s_cbranch_scc1 .LBB2_2
; %bb.3:
        s_waitcnt vmcnt(3)
        v_mfma_f32_32x32x16_bf16 v[16:31], v[32:35], v[8:11], v[16:31]
        s_cbranch_scc0 .LBB2_1
        s_endpgm
"""


def test_serial_loop_is_listed_and_counted_or_dma_loops_are_not():
    serial, rings = isa_waits.analyse(SERIAL.split("\n"))
    assert serial == [dict(label=".LBB0_1", loads=1, insts=5)] and rings == []
    serial, rings = isa_waits.analyse(DMA_AND_COUNTED.split("\n"))
    # .LBB1_1: LDS-DMA only; .LBB1_2: counted wait; .LBB1_3: not a self-loop (a label inside)
    assert serial == [] and rings == []


def test_ring_loop_reports_the_waits_in_front_of_its_mfmas():
    serial, rings = isa_waits.analyse(RING.split("\n"))
    assert serial == [dict(label=".LBB2_2", loads=2, insts=11)]          # (a ring that drains to vmcnt(0) once per trip is a serial loop as well)
    by = {r["label"]: r for r in rings}
    assert by[".LBB2_2"] == dict(label=".LBB2_2", mfma=3, loads=2, waits=[15, 14, 12], min=12, innermost=True)
    assert by[".LBB2_1"]["innermost"] is False and by[".LBB2_1"]["min"] == 0 and by[".LBB2_1"]["waits"] == [15, 14, 12, 0, 3]


def test_report_prints_both_parts():
    out = io.StringIO()
    isa_waits.report({"k_serial": SERIAL.split("\n"), "k_ring": RING.split("\n")}, {}, out)
    text = out.getvalue()
    assert "(a) serial load loops: 1" in text and ".LBB0_1: 1 load(s)" in text
    assert "(b) .LBB2_2 innermost: 3 MFMAs, 2 loads, vmcnt before an MFMA: 15 14 12; min 12" in text
