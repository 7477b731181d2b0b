"""The four kinds of frame table (ops.KINDS: plain, yuv, align, y16) against rows recorded from commit 422f75a, the last one with a
separate host path per kind (no GPU): the bytes its pack_frames / pack_yuv_frames / pack_warp_frames / pack_y16_frames gave for one
two-modality B = 2 table each, the arena offsets its DetectionPipeline._frame_table / _yuv_rows / _warp_rows / _y16_rows gave for one
contiguous and one ragged batch each (run there on CPU arrays), and the text of every refusal of a combination, which ops.frame_kind
now states once.  Every comparison is exact."""
import re

import numpy as np
import pytest

from icafusion_amd import ops

H, W, B = 64, 96, 2
RAGGED, UNIFORM = [(48, 80), (60, 44)], [(44, 60), (44, 60)]
M = np.array([[0.6 * np.cos(0.1), -0.6 * np.sin(0.1), 3.0], [0.6 * np.sin(0.1), 0.6 * np.cos(0.1), 1.5], [0.0, 0.0, 1.0]], np.float32)
OPTS = {"matrix": 1, "clip": (100, 250), "border": 7}

# recorded from commit 422f75a: (first free byte, the rows' bytes) of the calls in packed()
PACKED = {
    "plain": (25936,
              "00000000000000003000000050000000f0000000030000003a0000006000000003000000000000005555553fb1dc533f002d0000000000003c0000002c000000"
              "8400000003000000400000002f0000000000000018000000daa86f3f0000703f004c000000000000300000005000000050000000010000003a00000060000000"
              "03000000000000005555553fb1dc533f005b0000000000003c0000002c0000002c00000001000000400000002f0000000000000018000000daa86f3f0000703f"),
    "yuv": (32192,
              "0000000000000000300000005000000060000000010000003a0000006000000003000000000000005555553fb1dc533f00120000000000000112000000000000"
              "60000000020000000100000001000000001b0000000000003c0000002c0000003000000001000000400000002f0000000000000018000000daa86f3f0000703f"
              "4026000000000000412600000000000030000000020000000100000001000000002c000000000000300000005000000000010000030000003a00000060000000"
              "03000000000000005555553fb1dc533f0000000000000000000000000000000000000000000000000000000000000000005c0000000000003c0000002c000000"
              "9000000003000000400000002f0000000000000018000000daa86f3f0000703f0000000000000000000000000000000000000000000000000000000000000000"),
    "align": (23304,
              "00000000000000003000000050000000f0000000030000003a0000006000000003000000000000005555553fb1dc533f00000000000000000000000000000000"
              "00000000000000000000000000000000000000000000000000000000000000000000000000000000002d0000000000003c0000002c0000008400000003000000"
              "400000002f0000000000000018000000daa86f3f0000703f00000000000000000000000000000000000000000000000000000000000000000000000000000000"
              "00000000000000000000000000000000004c000000000000300000005000000032000000010000003a0000006000000003000000000000005555553fb1dc533f"
              "0100000024000000320000000700000028d5183fc15975bd00004040c159753d28d5183f0000c03f00000000000000000000803f000000000054000000000000"
              "3c0000002c0000003200000001000000400000002f0000000000000018000000daa86f3f0000703f0100000024000000320000000700000028d5183fc15975bd"
              "00004040c159753d28d5183f0000c03f00000000000000000000803f00000000"),
    "y16": (32416,
              "00000000000000003000000050000000f0000000030000003a0000006000000003000000000000005555553fb1dc533f00000000000000000000000000000000"
              "0000000000000000002d0000000000003c0000002c0000008400000003000000400000002f0000000000000018000000daa86f3f0000703f0000000000000000"
              "00000000000000000000000000000000004c0000000000003000000050000000a0000000010000003a0000006000000003000000000000005555553fb1dc533f"
              "0100000000000000e80300003075000064000000fa000000006a0000000000003c0000002c0000005800000001000000400000002f0000000000000018000000"
              "daa86f3f0000703f0100000001000000000000000000000064000000fa000000"),
}
LAYOUTS = {       # kind: {contiguous: (capacities, offsets, cb_offset, cr_offset)}
    "plain": {True: ([29184, 9728], [0, 7920, 29184, 31824], None, None),
             False: ([29184, 9728], [0, 11520, 29184, 33024], None, None)},
    "yuv": {True: ([14848, 9728], [0, 3960, 14848, 17488], [2640, 6600, 0, 0], [2641, 6601, 0, 0]),
           False: ([14848, 9728], [0, 5888, 14848, 18688], [3840, 8528, 0, 0], [3841, 8529, 0, 0])},
    "align": {True: ([29184, 4096], [0, 7920, 29184, 30984], None, None),
             False: ([29184, 4096], [0, 11520, 29184, 31232], None, None)},
    "y16": {True: ([29184, 19456], [0, 7920, 29184, 34464], None, None),
           False: ([29184, 19456], [0, 11520, 29184, 36864], None, None)},
}


def table(shapes):
    g, _ = ops.frame_geometry(shapes, (H, W))
    return np.concatenate((g, g))


def packed(kind):
    """(rows, end) of the kind's public pack function on the recorded inputs: ragged 48x80 and 60x44 frames into 64x96, two modalities."""
    if kind == "plain":
        g = table(RAGGED)
        return g, ops.pack_frames(g, [3, 3, 1, 1])
    if kind == "yuv":                    # nv12 beside a 3-channel modality, explicit pitches
        return ops.pack_yuv_frames(table(RAGGED), ["nv12", "nv12", 3, 3], pitch=[96, 48, 256, 144], c_pitch=[96, 48, None, None], matrix="bt709")
    if kind == "align":                  # a 36x50 grey source through a rotation, border 7
        return ops.pack_warp_frames(table(RAGGED), [3, 3, (36, 50, 1), (36, 50, 1)], [None, None, M, M], [0, 0, 7, 7])
    return ops.pack_y16_frames(table(RAGGED), [3, 3, "y16", "y16"], clip=(100, 250), window=[None, None, (1000, 30000), None])


@pytest.mark.parametrize("kind", list(PACKED))
def test_packed_rows_equal_the_recorded_bytes(kind):
    rows, end = packed(kind)
    want_end, want = PACKED[kind]
    assert rows.dtype == ops.KINDS[kind].dtype and len(rows) == 2 * B
    assert end == want_end and rows.tobytes().hex() == want
    assert ops.frame_rows(rows).dtype == ops.GEOM_DTYPE and np.array_equal(ops.frame_rows(rows)["h0"], [48, 60, 48, 60])
    ops.KINDS[kind].validate(rows, end, H, W)
    assert sum(ops.KINDS[kind].read(q) for q in rows) > 0


def modality_specs(kind, contiguous):
    """What the recorded pipelines packed per modality: frame_channels (3, 1), the second modality in the kind's own format."""
    src = [(36, 50), (36, 50)] if contiguous else [(36, 50), (30, 40)]
    second = {"plain": [1] * B, "yuv": ["nv12"] * B, "align": [(hs, ws, 1) for hs, ws in src], "y16": ["y16"] * B}[kind]
    return ([3] * B, second) if kind != "yuv" else (second, [1] * B)


@pytest.mark.parametrize("contiguous", [True, False])
@pytest.mark.parametrize("kind", list(LAYOUTS))
def test_layout_equals_the_recorded_offsets(kind, contiguous):
    cap, offsets, cb, cr = LAYOUTS[kind][contiguous]
    geom1, _ = ops.frame_geometry(UNIFORM if contiguous else RAGGED, (H, W))
    halves = []
    for m, base in ((0, 0), (1, cap[0])):
        rows, end = ops.KINDS[kind].pack(geom1.copy(), modality_specs(kind, contiguous)[m], base=base, **OPTS)
        halves.append(ops.layout_modality(rows, end, base, cap[m], contiguous, m))
    rows = np.concatenate(halves)
    assert ops.frame_rows(rows)["offset"].tolist() == offsets
    if cb is not None:
        assert rows["cb_offset"].tolist() == cb and rows["cr_offset"].tolist() == cr
    if not contiguous:                   # frames on FRAME_ALIGN starts pass the validator and must fit the modality's share of the arena
        ops.KINDS[kind].validate(rows, sum(cap), H, W)
        rows, end = ops.KINDS[kind].pack(geom1.copy(), modality_specs(kind, contiguous)[1], base=cap[0], **OPTS)
        with pytest.raises(ValueError, match=f"the frames of modality 1 need {end - cap[0]} bytes of the arena's {end - cap[0] - 1}"):
            ops.layout_modality(rows, end, cap[0], end - cap[0] - 1, False, 1)


def test_capacity_of_one_frame():
    assert [ops.frame_bytes(s, 60, 80) for s in (3, 1, "y16", "nv12", "i420", (36, 50, 1))] == [14400, 4800, 9600, 7200, 7200, 1800]
    assert ops.frame_bytes("nv21", 5, 7) == 35 + 2 * 3 * 4            # odd sizes: chroma rounded up


def test_kind_chooser_and_its_refusals():
    one = np.eye(3, dtype=np.float32)
    for formats, align, name in ((None, None, "plain"), ((None, None), None, "plain"), (("nv12", None), None, "yuv"), ((None, "i420"), None, "yuv"),
                                 ((None, "y16"), None, "y16"), (("y16", "y16"), None, "y16"), (None, (None, one), "align"),
                                 ((None, None), ("stretch", None), "align")):
        assert ops.frame_kind(formats, align) is ops.KINDS[name]
    assert ops.frame_kind(None, None, val_size=320) is ops.KINDS["plain"]
    for formats, align, val_size, msg in (
            (("nv12", None), None, 320, "forward_frames: YUV 4:2:0 frames have no validation geometry (val_size); the area down-scale reads interleaved frames"),
            ((None, "y16"), None, 320, "forward_frames: 16-bit thermal frames ('y16') have no validation geometry (val_size); the validation sets are 8-bit"),
            (None, (None, one), 320, "forward_frames: align= has no validation geometry (val_size); validation sets are registered offline"),
            ((None, "y16"), (one, None), None,
             "forward_frames: align= takes interleaved 8-bit frames; a 16-bit thermal modality ('y16') cannot be combined with it yet"),
            (("nv12", "y16"), None, None, "a 16-bit thermal modality ('y16') beside a YUV 4:2:0 modality is not supported yet: one table holds one kind of row"),
            (("nv12", None), (None, one), None, "forward_frames: align= takes interleaved frames; a YUV 4:2:0 modality (formats) cannot be combined with it yet"),
            (None, (one, one), None, "align=(A_rgb, A_ir): both modalities carry an alignment; one of them defines the aligned space and stays None"),
            (None, (None, None), None, "align=(A_rgb, A_ir): neither modality carries an alignment (plain pairs: leave align=None)"),
            (None, one[0], None, "align=(A_rgb, A_ir): one entry per modality, None for the modality that is not warped")):
        with pytest.raises(ValueError, match="^" + re.escape(msg) + "$"):
            ops.frame_kind(formats, align, val_size)
    # the pipeline's names for the same arguments
    for formats, msg in (((None, "y16"), "frame_align takes interleaved 8-bit frames; a 16-bit thermal modality ('y16') cannot be combined with it yet"),
                         (("nv21", None), "frame_align takes interleaved frames; a YUV 4:2:0 modality (frame_formats) cannot be combined with it yet")):
        with pytest.raises(ValueError, match="^" + re.escape(msg) + "$"):
            ops.frame_kind(formats, (None, True), who="", align_arg="frame_align", formats_arg="frame_formats")


def test_per_call_fields():
    """The fields a call rewrites: matrices and border of the aligned modality, clip and windows of the 16-bit modalities; the rest of
    the rows stays."""
    rows, _ = packed("align")
    before = rows.copy()
    mats = np.stack([M, 2 * M])
    ops.KINDS["align"].update(rows, B, (None, None), 1, mats=mats, border=9)
    assert np.array_equal(rows["m"][B:], mats.reshape(B, 9)) and rows["border"].tolist() == [0, 0, 9, 9]
    rows["m"], rows["border"] = before["m"], before["border"]
    assert rows.tobytes() == before.tobytes()
    rows, end = packed("y16")
    ops.KINDS["y16"].update(rows, B, (None, "y16"), None, clip=(5, 6), wins=[None, (7, 8)])
    assert (rows["mode"].tolist(), rows["lo"].tolist(), rows["hi"].tolist()) == ([0, 0, 1, 0], [0, 0, 0, 7], [0, 0, 0, 8])
    assert rows["clip_lo"].tolist() == [0, 0, 5, 5] and rows["clip_hi"].tolist() == [0, 0, 6, 6]
    ops.KINDS["y16"].validate(rows, end, H, W)
    assert ops.KINDS["plain"].update is None and ops.KINDS["yuv"].update is None
