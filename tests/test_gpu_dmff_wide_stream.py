"""The weight stream and the batched prologue / epilogue loads of the DMFF token kernels (dmff_wide.hip: icaf_dmff_wide_ln_qkv,
icaf_dmff_wide_proj_mlp, icaf_dmff_wide_proj_mlp_split + icaf_dmff_wide_reduce) at the row counts where a clamped address or a
refill past the end of the stream could leak: 1 row per modality (a lone tile, 63 of its 64 rows clamped), 63 / 64 / 65 (one row short
of a tile, a full tile, one row over) and 129 (a ragged third tile).  Operands and references are those of tests/test_gpu_exact_dmff.py
(exact LayerNorm rows, lattice weights: tests/numerics.py), shared with that module when both run in one process.

  * LayerNorm + QKV, both forms (three passes per workgroup, one): the whole qkv tensor bit for bit.
  * out-projection + MLP (unsplit; the two-way hidden split with its reduce launch at C = 512; one fp32-stream build per width):
    (a) W2 = 0: y (and y32) bit for bit; (b) W_o = 0: the counted bound of numerics.dmff_ref_b.
  * Every output (qkv; y in a strided NaN-filled buffer; y32; the partial sums) is NaN-prefilled and must be untouched outside its valid rows;
    every token input (x, att, x32) lies between NaN guard rows, so a value fetched through a row index that was not clamped shows.
  * Every fragment-major weight tensor [2][Np / 32][Kp / 16][64][8] is the front of a tensor whose third block is NaN: well over
    WDEPTH slices behind the last valid one, so a refill past the end of a stream that were CONSUMED shows (that it stays inside the
    matrix in the first place is what tests/test_wide_cursor_host.py checks, under AddressSanitizer, on the host)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm                                   # noqa: E402
from numerics import BF16, F16, F32                     # noqa: E402
import test_gpu_exact_dmff as xd                        # noqa: E402  (its operand cache and launch helpers; nothing of it is collected here)
from icafusion_amd import ops                           # noqa: E402

DEV = xd.DEV
ROWS = (1, 63, 64, 65, 129)
WIDTHS = [(C, dt) for C in (128, 256, 512) for dt in (BF16, F16)]
# (C, dtype, ksplit, fp32 stream): every unsplit build, the split + reduce at C = 512, one fp32-stream build per width
CELLS = ([(C, dt, 1, False) for C, dt in WIDTHS] + [(512, BF16, 2, False), (512, F16, 2, False)] +
         [(128, BF16, 1, True), (256, F16, 1, True), (512, BF16, 2, True)])


def nan_tailed(packs, dt):
    """packs -> the same with every weight tensor replaced by its fragment-major copy at the front of a [3][...] tensor whose last block is NaN"""
    out = {}
    for k, (w, kp, b) in packs.items():
        f = ops.frag_weights(w)
        big = xd.nan_filled((3,) + tuple(f.shape[1:]), dt)
        big[:2].copy_(f)
        assert big[2].numel() * big.element_size() >= 4 * 4 * 64 * 16      # WDEPTH slices of four K steps
        out[k] = (big[:2], kp, b)
    return out


@pytest.fixture
def tailed(monkeypatch):
    """ops.dmff_wide_* take the weight tensors as given (already fragment-major, NaN behind them)"""
    monkeypatch.setattr(ops, "_wide_packs", lambda packs: packs)
    cache = {}

    def get(blk):
        if id(blk) not in cache:
            cache[id(blk)] = nan_tailed(blk.packs, blk.dt)
        return cache[id(blk)]
    return get


@pytest.mark.parametrize("C,dt", WIDTHS, ids=[f"C{C}-{nm.DT_NAME[dt]}" for C, dt in WIDTHS])
def test_ln_qkv_bit_for_bit_at_the_tile_edges(C, dt, tailed, monkeypatch):
    blk, zs = xd.case("qkv", C, dt)
    z = zs[False]
    nm.assert_lattice_condition(z, dt, 1.0, f"qkv C={C} {dt}")
    packs = tailed(blk)
    failures = []
    for rows in ROWS:
        want = nm.rne(z[:, :rows], dt) + 0.0
        x = nm.PoisonedFlat((2, rows, C), dt, DEV, nm.NAN_BITS[dt], blk.rows("x", rows), 2 * C)
        outs = []
        for npass in (0, 1):
            what = f"icaf_dmff_wide_ln_qkv C={C} {nm.DT_NAME[dt]} rows={rows} npass={npass or 3}"
            monkeypatch.setattr(ops.OPT, "dmff_qkv_npass", npass)
            qkv = nm.PoisonedFlat((2, rows, 3 * C), dt, DEV, nm.NAN_BITS[dt], None, 6 * C)
            ops.dmff_wide_ln_qkv(x.view, qkv.view, packs, blk.ln, blk.coef, blk.d["eps"], 1, rows, xd.HEADS)(ops.current_stream_ptr())
            torch.cuda.synchronize()
            outs.append(qkv.view.cpu())
            try:
                qkv.assert_outside_intact(what + ": qkv")
                x.assert_outside_intact(what + ": x")
                nm.assert_same_bits(outs[-1], want, what)
            except AssertionError as e:
                failures.append(str(e)[:400])
        if not nm.same_bits(outs[0], outs[1]):
            failures.append(f"C={C} rows={rows}: the one-pass and the three-pass form differ")
    assert not failures, f"{len(failures)} checks failed:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("cell", CELLS, ids=[nm.cell_id(c) for c in CELLS])
def test_proj_mlp_exact_at_the_tile_edges(cell, tailed):
    C, dt, ks, r32 = cell
    guard = 2 * C
    failures = []
    for kind in ("a", "b"):
        blk, refs = xd.case(kind, C, dt)
        packs = tailed(blk)
        shim = type("Shim", (), dict(dt=dt, C=C, packs=packs, ln=blk.ln, coef=blk.coef, d=blk.d, rows=blk.rows))()
        for use_x32 in ((False, True) if r32 else (False,)):
            if kind == "a":
                nm.assert_lattice_condition(refs[use_x32], dt, 1.0, f"(a) {nm.cell_id(cell)} x32={use_x32}")
            else:
                assert refs[use_x32]["share"] <= 0.05
            for rows in ROWS:
                what = f"({kind}) {nm.cell_id(cell)} rows={rows} x32={int(use_x32)}"
                x = nm.PoisonedFlat((2, rows, C), dt, DEV, nm.NAN_BITS[dt], blk.rows("x", rows), guard)
                att = nm.PoisonedFlat((2, rows, C), dt, DEV, nm.NAN_BITS[dt], blk.rows("att", rows), guard)
                x32 = nm.PoisonedFlat((2, rows, C), F32, DEV, nm.NAN_BITS[F32], blk.rows("x32", rows), guard) if use_x32 else None
                y = xd.StridedOut(rows, C, dt)
                y32 = nm.PoisonedFlat((2, rows, C), F32, DEV, nm.NAN_BITS[F32], None, guard) if r32 else None
                part = nm.PoisonedFlat((ks, 2, rows, C), F32, DEV, nm.NAN_BITS[F32], None, guard) if ks > 1 else None
                xd.run_proj_mlp(shim, rows, ks, r32, use_x32, x=x.view, att=att.view, x32=x32.view if use_x32 else None, y=y.view,
                                y32=y32.view if r32 else None, partial=part.view if part else None)
                try:
                    y.assert_gaps_intact(what + ": y")
                    for name, buf in (("y32", y32), ("partial", part), ("x", x), ("att", att), ("x32", x32)):
                        if buf is not None:
                            buf.assert_outside_intact(f"{what}: {name}")
                    yv, y32v = y.view.contiguous().cpu(), (y32.view.cpu() if r32 else None)
                    assert bool(torch.isfinite(yv.float()).all()), f"{what}: y holds unwritten or non-finite elements"
                    assert part is None or bool(torch.isfinite(part.view).all()), f"{what}: unwritten partial sums"
                    if kind == "a":
                        nm.check_proj_mlp_a(yv, y32v, refs[use_x32][:, :rows], dt, what)
                    else:
                        nm.check_proj_mlp_b(yv, y32v, refs[use_x32], dt, what)
                except AssertionError as e:
                    failures.append(f"{what}: {str(e)[:400]}")
    assert not failures, f"{len(failures)} launches failed:\n" + "\n".join(failures[:12])
