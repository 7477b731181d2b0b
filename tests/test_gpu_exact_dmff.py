"""Exact and poisoned-buffer tests of the DMFF block kernels (dmff_wide.hip: icaf_dmff_wide_ln_qkv, icaf_dmff_wide_proj_mlp,
icaf_dmff_wide_proj_mlp_split + icaf_dmff_wide_reduce; dmff_fused.hip: icaf_dmff_ln_qkv, icaf_dmff_attn_mlp), called through the `ops`
entry points — no Plan, no model.  tests/test_gpu_dmff_fused.py holds whole iterations to the oracle within a measured error on Gaussian data; this module says
WHICH element is wrong.  Operands are chosen so that everything up to a known point is exact in fp32 in any summation order
(tests/numerics.py, "DMFF block kernels"): rows m +- s with eps = 1 - s^2 make the LayerNorm exact (mean m, rstd 1), a zeroed GEMM isolates
the others, a sparse W2 keeps the fc2 accumulation error counted.

(a) out-projection + coefficient mix (W2 = 0): y == RNE(c_res x + c_acc (att W_o^T + b_o)) bit for bit, the fp32 stream y32 == the
    unrounded value bit for bit; x32 holds values no 16-bit type represents, so a kernel reading the 16-bit x instead fails.
(b) LayerNorm + MLP + final mix (W_o = 0): every element of y and y32 within a COUNTED bound of the fp64 reference (numerics.dmff_ref_b:
    the hidden roundings that the GELU budget leaves ambiguous, nnz - 1 roundings of the sparse fc2 sum, the final mix, the storage rounding).
    (a) and (b) run on every build of the instantiation table numerics.DMFF_CELLS at 64 / 33 / 154 / 321 rows; a closing test checks that
    every cell ran.
(c) a subset again with NaN-prefilled strided outputs (ldy > C, y_gs != rows * ldy), NaN-prefilled y32 / partial sums and NaN / Inf guard
    rows around x, att and x32; every launch twice, the two results bit-identical.
(d) icaf_dmff_ln_qkv and icaf_dmff_wide_ln_qkv on the exact-LayerNorm rows: the WHOLE qkv tensor — Q, K and V thirds — equals RNE(exact) bit
    for bit; the wide kernel in both forms (three passes per workgroup, and one: OPT.dmff_qkv_npass = 1), which must also agree with each other.
(e) the two-launch kernel icaf_dmff_attn_mlp with an attention output known exactly (K = 0, V with a representable per-image mean:
    numerics.attn_known_qkv), then (a) and (b) on it: all three softmax-denominator forms of attn_core.h (d_k = 16, 32, 64), N = 64 and
    N = 77 (a second tile of 13 rows per image), both workgroup placements (2 B a multiple of 8 or not).  The 16-bit builds again with
    the select family (numerics.attn_select_qkv: one winning key per query, the tile is V of that key), which moves under a wrong key
    order in V^T, a wrong Q offset, a wrong maximum and a denominator the cold path skipped — all of which leave the mean where it is.

Known limitation: on rows m +- s that a 16-bit type represents, x * x is exact as well, so this gate does not tell a one-pass variance
E[x^2] - mean^2 from the two-pass one.  In the fp32-stream builds it does: every fourth row of the x32 case of (b) lies around m = 4096, where
x * x is not an fp32 number.  For the 16-bit stream the protection is the `ln_rows` kinds of tests/test_gpu_exact.py (icaf_layernorm and the
identity-Q test of the fused LayerNorm + QKV kernels).

Every test prints the largest err / budget it saw before it asserts (`-s`); docs/HISTORY.md sections 20 and 22 record them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm                                   # noqa: E402
from numerics import BF16, F16, F32                     # noqa: E402
from icafusion_amd import ops                           # noqa: E402

DEV = "cuda:0"
HEADS = 4
RAN = {}                                                # cell -> set of (rows, x32) on which (a) and (b) both ran
RATIOS = {}                                             # (what, cell id) -> largest err / budget
SHARES = {}                                             # (C, dtype, x32) -> ambiguous-rounding share of (b)
_CASES = {}


def nan_filled(shape, dt):
    t = torch.empty(shape, dtype=dt, device=DEV)
    nm.bits(t).fill_(nm.NAN_BITS[dt])
    return t


class Block:
    """Device operands of one case: packed weights, LayerNorm parameters, coefficients, and the token tensors at numerics.DMFF_ROWS_MAX rows."""

    def __init__(self, d, dt):
        self.d, self.dt, self.C = d, dt, d["x"].shape[2]
        C, hid = self.C, d["hidden"]
        dev = lambda t: t.to(DEV).contiguous()
        zw, zb = (lambda n, k: torch.zeros((2, n, k))), (lambda n: torch.zeros((2, n)))
        pack = lambda w, b: ops.pack_streams([(dev(w[m]), dev(b[m])) for m in range(2)], dt)
        self.packs = dict(qkv=pack(d.get("wqkv", zw(3 * C, C)), d.get("bqkv", zb(3 * C))), out=pack(d.get("wo", zw(C, C)), d.get("bo", zb(C))),
                          fc1=pack(d.get("w1", zw(hid, C)), d.get("b1", zb(hid))), fc2=pack(d.get("w2", zw(C, hid)), d.get("b2", zb(C))))
        self.ln = {k: dev(v) for k, v in d["ln"].items()}
        self.coef = dict(hidden=hid, co=d["co"])
        self.tok = {k: dev(d[k].to(F32 if k == "x32" else dt)) for k in ("x", "att", "x32") if k in d}

    def rows(self, name, n):
        return self.tok[name][:, :n].contiguous()


def case(kind, C, dt):
    """(Block, CPU operands) of test (a) / (b) / (d) for (C, dtype), built once."""
    key = (kind, C, dt)
    if key not in _CASES:
        if kind == "qkv":
            d, z = nm.dmff_operands_qkv(C, dt)
            _CASES[key] = (Block(d, dt), {False: z})
        elif kind == "a":
            d = nm.dmff_operands_a(C, dt)
            _CASES[key] = (Block(d, dt), {x32: nm.dmff_xatt64(d, x32) for x32 in ((False, True) if dt != F32 else (False,))})
        else:
            d = nm.dmff_operands_b(C, dt)
            _CASES[key] = (Block(d, dt), {x32: nm.dmff_ref_b(d, dt, x32) for x32 in ((False, True) if dt != F32 else (False,))})
            for x32, ref in _CASES[key][1].items():
                SHARES[(C, nm.DT_NAME[dt], x32)] = ref["share"]
    return _CASES[key]


def run_proj_mlp(blk, rows, ks, r32, use_x32, x=None, att=None, x32=None, y=None, y32=None, partial=None):
    """One proj_mlp launch (ks > 1: split + reduce) on the first `rows` rows; outputs NaN-prefilled unless given.  Returns (y, y32, partial)."""
    dt, C = blk.dt, blk.C
    x = blk.rows("x", rows) if x is None else x
    att = blk.rows("att", rows) if att is None else att
    if use_x32 and x32 is None:
        x32 = blk.rows("x32", rows)
    y = nan_filled((2, rows, C), dt) if y is None else y
    if r32 and y32 is None:
        y32 = nan_filled((2, rows, C), F32)
    if ks > 1 and partial is None:
        partial = nan_filled((ks, 2, rows, C), F32)
    ls = ops.dmff_wide_proj_mlp(x, att, y, blk.packs, blk.ln, blk.coef, blk.d["eps"], 1, rows, HEADS, partial=partial, ksplit=ks,
                                x32=x32 if use_x32 else None, y32=y32 if r32 else None)
    assert isinstance(ls, list) == (ks > 1)
    for l in (ls if isinstance(ls, list) else [ls]):
        l(ops.current_stream_ptr())
    torch.cuda.synchronize()
    return y, (y32 if r32 else None), partial


def check_a(y, y32, z, rows, dt, what):
    nm.check_proj_mlp_a(y.cpu(), None if y32 is None else y32.cpu(), z[:, :rows], dt, what)


def check_b(y, y32, ref, dt, what, cell):
    yc, y32c = y.cpu(), None if y32 is None else y32.cpu()
    n = yc.shape[1]
    r = nm.budget_ratio(yc, ref["out"][:, :n], ref["by"][:, :n])
    r32 = nm.budget_ratio(y32c, ref["out"][:, :n], ref["b32"][:, :n]) if y32c is not None else 0.0
    for k, v in (("(b) y", r),) + ((("(b) y32", r32),) if y32c is not None else ()):
        RATIOS[(k, nm.cell_id(cell))] = max(RATIOS.get((k, nm.cell_id(cell)), 0.0), v)
    msg = ""
    if y32c is not None:                                 # where every hidden operand is known exactly the y32 bound is the fc2 accumulation + the mix
        k = ref["known"][:, :n]
        rk = nm.budget_ratio(y32c[k], ref["out"][:, :n][k], ref["b32"][:, :n][k])
        RATIOS[("(b) y32, h known", nm.cell_id(cell))] = max(RATIOS.get(("(b) y32, h known", nm.cell_id(cell)), 0.0), rk)
        msg = f", y32 {r32:.3f}, y32 where no hidden rounding is ambiguous ({float(k.double().mean()):.2f} of the outputs) {rk:.3f}"
    print(f"\n[dmff b] {what}: err / budget y {r:.3f}" + msg)
    nm.check_proj_mlp_b(yc, y32c, ref, dt, what)


@pytest.mark.parametrize("cell", nm.DMFF_CELLS, ids=[nm.cell_id(c) for c in nm.DMFF_CELLS])
def test_proj_mlp_exact_out_projection_and_counted_mlp(cell):
    """(a) and (b) on one build of the instantiation table, at every row count, on the first iteration's operands (x) and — fp32-stream
    builds — a later iteration's (x32)."""
    C, dt, ks, r32 = cell
    blk_a, zs = case("a", C, dt)
    blk_b, refs = case("b", C, dt)
    failures = []
    for use_x32 in ((False, True) if r32 else (False,)):
        assert refs[use_x32]["share"] <= 0.05, f"ambiguous-rounding share {refs[use_x32]['share']:.4f} of (b) exceeds 5 %"
        if dt != F32:
            nm.assert_lattice_condition(zs[use_x32], dt, 1.0, f"(a) {nm.cell_id(cell)} x32={use_x32}")
        for rows in nm.DMFF_ROWS:
            what = f"{nm.cell_id(cell)} rows={rows} x32={int(use_x32)}"
            try:
                y, y32, _ = run_proj_mlp(blk_a, rows, ks, r32, use_x32)
                check_a(y, y32, zs[use_x32], rows, dt, "(a) " + what)
                y, y32, _ = run_proj_mlp(blk_b, rows, ks, r32, use_x32)
                check_b(y, y32, refs[use_x32], dt, what, cell)
            except AssertionError as e:
                failures.append(f"{what}: {str(e)[:400]}")
                continue
            RAN.setdefault(cell, set()).add((rows, use_x32))
    assert not failures, f"{len(failures)} launches failed:\n" + "\n".join(failures[:12])


def test_every_cell_of_the_instantiation_table_ran():
    """Closing test of (a) / (b): every (C, dtype, ksplit, r32) build ran at every row count, the fp32-stream builds with and without x32."""
    if not RAN:
        pytest.fail("run together with test_proj_mlp_exact_out_projection_and_counted_mlp (same process): nothing was recorded")
    for cell in nm.DMFF_CELLS:
        want = {(rows, x32) for rows in nm.DMFF_ROWS for x32 in ((False, True) if cell[3] else (False,))}
        assert RAN.get(cell, set()) == want, f"{nm.cell_id(cell)}: ran {sorted(RAN.get(cell, set()))}"
    print("\n[cells] " + ", ".join(nm.cell_id(c) for c in nm.DMFF_CELLS))
    print("[ratios] " + "; ".join(f"{k[0]} {k[1]}: {v:.3f}" for k, v in sorted(RATIOS.items())))
    print("[ambiguous shares] " + "; ".join(f"C{k[0]} {k[1]} x32={int(k[2])}: {v:.4f}" for k, v in sorted(SHARES.items())))


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) poisoned buffers
# ------------------------------------------------------------------------------------------------------------------------------------
# parked builds (C = 512: x_att parked in y; every split: parked for the reduce launch; fp32 stream: parked in y32), one unparked of each kind
POISON_CELLS = [(512, BF16, 1, False), (512, F16, 4, False), (256, F16, 2, False), (512, BF16, 2, True), (256, BF16, 1, True), (128, F32, 1, False),
                (128, F16, 1, False)]


class StridedOut:
    """y as the plan hands it to a last iteration: a (2, rows, C) view with ldy = C + 16 and y_gs = (rows + 3) * ldy inside a NaN-filled buffer."""

    def __init__(self, rows, C, dt):
        self.buf = nan_filled((2, rows + 3, C + 16), dt)
        self.before = self.buf.clone()
        self.view = self.buf[:, 1:rows + 1, 8:8 + C]
        assert self.view.stride() == ((rows + 3) * (C + 16), C + 16, 1)

    def assert_gaps_intact(self, what):
        ne = nm.bits(self.buf) != nm.bits(self.before)
        ne[:, 1:self.view.shape[1] + 1, 8:8 + self.view.shape[2]] = False
        assert not bool(ne.any()), f"{what}: {int(ne.sum())} elements of the row padding / gap rows changed; first at {nm._first(ne)}"


@pytest.mark.parametrize("rows", [33, 154])
@pytest.mark.parametrize("cell", POISON_CELLS, ids=[nm.cell_id(c) for c in POISON_CELLS])
def test_proj_mlp_poisoned_buffers(cell, rows):
    """(c): the checks of (a) and (b) into a NaN-prefilled strided y whose gaps must stay bit-unchanged; y32 and the partial sums NaN-prefilled
    inside NaN guards; x, att, x32 between +Inf / NaN guard rows the clamped row indices must never reach (a value derived from one is not
    finite, or off its bound); each launch twice with identical bits (the reduce adds in slice order)."""
    C, dt, ks, r32 = cell
    use_x32 = r32
    guard = 2 * C
    for kind in ("a", "b"):
        blk, refs = case(kind, C, dt)
        what = f"poison ({kind}) {nm.cell_id(cell)} rows={rows}"
        x = nm.PoisonedFlat((2, rows, C), dt, DEV, nm.INF_BITS[dt], blk.rows("x", rows), guard)
        att = nm.PoisonedFlat((2, rows, C), dt, DEV, nm.NAN_BITS[dt], blk.rows("att", rows), guard)
        x32 = nm.PoisonedFlat((2, rows, C), F32, DEV, nm.INF_BITS[F32], blk.rows("x32", rows), guard) if use_x32 else None
        got = []
        for _ in range(2):
            y = StridedOut(rows, C, dt)
            y32 = nm.PoisonedFlat((2, rows, C), F32, DEV, nm.NAN_BITS[F32], None, guard) if r32 else None
            part = nm.PoisonedFlat((ks, 2, rows, C), F32, DEV, nm.NAN_BITS[F32], None, guard) if ks > 1 else None
            run_proj_mlp(blk, rows, ks, r32, use_x32, x=x.view, att=att.view, x32=x32.view if use_x32 else None, y=y.view,
                         y32=y32.view if r32 else None, partial=part.view if part else None)
            y.assert_gaps_intact(what + ": y")
            for name, buf in (("y32", y32), ("partial", part), ("x", x), ("att", att), ("x32", x32)):
                if buf is not None:
                    buf.assert_outside_intact(f"{what}: {name}")
            yv, y32v = y.view.contiguous(), (y32.view if r32 else None)
            assert bool(torch.isfinite(yv.float()).all()), f"{what}: y holds unwritten or non-finite elements"
            assert part is None or bool(torch.isfinite(part.view).all()), f"{what}: unwritten partial sums"
            if kind == "a":
                check_a(yv, y32v, refs[use_x32], rows, dt, what)
            else:
                nm.check_proj_mlp_b(yv.cpu(), None if y32v is None else y32v.cpu(), refs[use_x32], dt, what)
            got.append((yv.cpu(), None if y32v is None else y32v.cpu().clone()))
        assert nm.same_bits(got[0][0], got[1][0]), f"{what}: y differs between two runs"
        assert got[0][1] is None or nm.same_bits(got[0][1], got[1][1]), f"{what}: y32 differs between two runs"


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) all three thirds of the QKV kernels
# ------------------------------------------------------------------------------------------------------------------------------------
QKV_CASES = ([("fused", C, dt) for C in (64, 128) for dt in (BF16, F16, F32)] + [("wide", 128, dt) for dt in (BF16, F16, F32)] +
             [("wide", C, dt) for C in (256, 512) for dt in (BF16, F16)])


@pytest.mark.parametrize("kernel,C,dt", QKV_CASES, ids=[f"{k}-C{C}-{nm.DT_NAME[dt]}" for k, C, dt in QKV_CASES])
def test_layernorm_qkv_every_third_bit_for_bit(kernel, C, dt, monkeypatch):
    """(d): exact LayerNorm rows (eps_attn = 0.75), lattice W_qkv / bias different per modality, the two attention LayerNorms with different
    gamma / beta: the whole NaN-prefilled qkv tensor equals RNE(exact) bit for bit at every row count; icaf_dmff_wide_ln_qkv in both forms
    (three passes per workgroup, one pass per workgroup), bit-identical to each other."""
    blk, zs = case("qkv", C, dt)
    z = zs[False]
    if dt != F32:
        nm.assert_lattice_condition(z, dt, 1.0, f"qkv C={C} {dt}")
    failures = []
    for rows in nm.DMFF_ROWS:
        want = nm.rne(z[:, :rows], dt) + 0.0
        x = nm.PoisonedFlat((2, rows, C), dt, DEV, nm.INF_BITS[dt], blk.rows("x", rows), 2 * C)
        outs = []
        for npass in ((0, 1) if kernel == "wide" else (0,)):
            what = f"icaf_dmff_{'wide_' if kernel == 'wide' else ''}ln_qkv C={C} {nm.DT_NAME[dt]} rows={rows} npass={npass or 3}"
            monkeypatch.setattr(ops.OPT, "dmff_qkv_npass", npass)
            qkv = nm.PoisonedFlat((2, rows, 3 * C), dt, DEV, nm.NAN_BITS[dt], None, 6 * C)
            fn = ops.dmff_wide_ln_qkv if kernel == "wide" else ops.dmff_ln_qkv
            launch = fn(x.view, qkv.view, blk.packs, blk.ln, blk.coef, blk.d["eps"], 1, rows, HEADS)
            assert kernel != "wide" or launch.keep[0].reserved == npass
            launch(ops.current_stream_ptr())
            torch.cuda.synchronize()
            outs.append(qkv.view.cpu())
            try:
                qkv.assert_outside_intact(what + ": qkv")
                x.assert_outside_intact(what + ": x")
                for third, name in enumerate("QKV"):
                    nm.assert_same_bits(outs[-1][:, :, third * C:(third + 1) * C], want[:, :, third * C:(third + 1) * C], f"{what}: {name} third")
            except AssertionError as e:
                failures.append(str(e)[:400])
        if len(outs) == 2 and not nm.same_bits(outs[0], outs[1]):
            failures.append(f"C={C} rows={rows}: the one-pass and the three-pass form differ")
    assert not failures, f"{len(failures)} checks failed:\n" + "\n".join(failures[:12])


# ------------------------------------------------------------------------------------------------------------------------------------
# (e) the two-launch kernel
# ------------------------------------------------------------------------------------------------------------------------------------
# (C, heads): d_k = 16 (denominator from the free rows of the last O^T tile), 32 (one extra MFMA), 64 (VALU row sums)
ATTN_HEADS = [(64, 4), (128, 4), (128, 2)]
# (B, N): N = 64 — 1 / N exact, one tile per image, 2 B = 8 pairs dealt over the XCDs; N = 77 — 1 / N rounded, a second tile of 13 rows, pairs in order
ATTN_TOKENS = [(4, 64), (3, 77)]
# (the fp32 build: a power-of-two N only — it stores the attention tile unrounded — and head dims up to 32, all it is instantiated for)
ATTN_CASES = [(C, h, dt, B, N) for C, h in ATTN_HEADS for dt in (BF16, F16, F32) for B, N in ATTN_TOKENS
              if dt != F32 or (N & (N - 1) == 0 and C // h <= 32)]


@pytest.mark.parametrize("C,heads,dt,B,N", ATTN_CASES, ids=[f"C{C}-h{h}-{nm.DT_NAME[dt]}-B{B}-N{N}" for C, h, dt, B, N in ATTN_CASES])
def test_attn_mlp_with_known_attention_tile(C, heads, dt, B, N):
    """(e): K = 0 makes every probability 1 / N, so the attention tile is the mean of V over the image's keys — of the modality the
    direction reads, different per modality and image.  Stages A to B of dmff_attn_mlp_kernel: p = exp2(0) = 1 for the N keys and 0 for the
    padding, O^T = the exact key sum N * mean, l = N, and the tile is stored as RNE_dt(O * (1.0f / l)).  At N = 64 the reciprocal is exact;
    at N = 77 it carries one rounding and the product another, 2^-23 relative in all, which the 16-bit store absorbs because the mean
    itself is representable (tests/test_numerics_selftest.py checks both statements); the fp32 build stores the tile unrounded and is
    therefore run at the power-of-two count only.  With the tile known, (a) (W2 = 0: y == RNE(x_att) bit for bit) and (b) (W_o = 0: counted
    bound) run as for the three-launch kernels, into a NaN-prefilled strided y whose gaps must stay untouched."""
    attn_mlp_on_known_tile(*nm.attn_known_qkv(B, N, C, dt, 100 * C + N), "", C, heads, dt, B, N)


def attn_mlp_on_known_tile(qkv_c, att, tag, C, heads, dt, B, N):
    """One icaf_dmff_attn_mlp launch per check (a) / (b) on a qkv whose attention tile `att` is known exactly after the store to `dt`."""
    rows = B * N
    qkv = nm.PoisonedFlat((2, rows, 3 * C), dt, DEV, nm.NAN_BITS[dt], qkv_c.to(dt).to(DEV), 6 * C)
    failures = []
    for kind in ("a", "b"):
        d = (nm.dmff_operands_a if kind == "a" else nm.dmff_operands_b)(C, dt, rows)
        d["att"] = att
        want = nm.dmff_xatt64(d) if kind == "a" else nm.dmff_ref_b(d, dt)
        blk = Block(d, dt)
        x = nm.PoisonedFlat((2, rows, C), dt, DEV, nm.INF_BITS[dt], blk.tok["x"], 2 * C)
        y = StridedOut(rows, C, dt)
        what = f"icaf_dmff_attn_mlp{tag} ({kind}) C={C} heads={heads} {nm.DT_NAME[dt]} B={B} N={N}"
        ops.dmff_attn_mlp(x.view, qkv.view, y.view, blk.packs, blk.ln, blk.coef, d["eps"], B, N, heads)(ops.current_stream_ptr())
        torch.cuda.synchronize()
        try:
            y.assert_gaps_intact(what + ": y")
            x.assert_outside_intact(what + ": x")
            qkv.assert_outside_intact(what + ": qkv")
            got = y.view.contiguous().cpu()
            if kind == "a":
                nm.check_proj_mlp_a(got, None, want, dt, what)
            else:
                assert want["share"] <= 0.05
                r = nm.budget_ratio(got, want["out"], want["by"])
                RATIOS[("(e) y" + tag, f"C{C}-h{heads}-{nm.DT_NAME[dt]}-N{N}")] = r
                print(f"\n[dmff e] {what}: err / budget {r:.3f}, ambiguous share {want['share']:.4f}")
                nm.check_proj_mlp_b(got, None, want, dt, what)
        except AssertionError as e:
            failures.append(str(e)[:400])
    assert not failures, "\n".join(failures)


# The select family of tests/numerics.py ("cross attention"): one winning key per query, every other probability exactly 0, all scores
# negative — the attention tile is V[pi(i)] of the modality the direction reads, which a wrong key order in V^T, a wrong head or direction
# offset, an unmasked padding key or a skipped rescale of the denominator all change (the K = 0 mean above is invariant under a key
# permutation, under whatever Q holds and under a wrong maximum or rescale).  Stage A of dmff_attn_mlp_kernel stores the tile with pack4<DT>(o * inv): the bf16 and f16 builds round it to the storage type
# there, and RNE(v (1 + O(2^-13))) = v (numerics.attn_select_bound); the fp32 build stores o * inv unrounded, v (1 + 5 u) at best, so checks
# (a) and (b), which need the tile on the lattice, do not apply to it and it is left to the K = 0 cases.
SELECT_CASES = [(C, h, dt, B, N) for C, h in ATTN_HEADS for dt in (BF16, F16) for B, N in ATTN_TOKENS]


@pytest.mark.parametrize("C,heads,dt,B,N", SELECT_CASES, ids=[f"C{C}-h{h}-{nm.DT_NAME[dt]}-B{B}-N{N}" for C, h, dt, B, N in SELECT_CASES])
def test_attn_mlp_with_selected_attention_tile(C, heads, dt, B, N):
    """(e) with the select family (V = non-zero integers in [-8, 8], the lattice of (a)): d_k = 16 / 32 / 64, N = 64 / 77, the 16-bit builds."""
    qkv_c, att, _ = nm.attn_select_qkv(B, N, C // heads, 300 * C + N, heads=heads, vmax=8)
    attn_mlp_on_known_tile(qkv_c, att, " select", C, heads, dt, B, N)
