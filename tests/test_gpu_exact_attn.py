"""Exact and counted-budget tests of the cross-attention kernels (dmff.hip: cross_attn_kernel — K / V^T of a head resident in LDS — and
cross_attn_stream_kernel — key tiles streamed through LDS; attn_core.h: the inner loop AttnCore that dmff_attn_mlp_kernel shares), called
through ops.cross_attention.  tests/test_gpu_kernels.py and tests/test_gpu_resnet.py hold them to 4e-2 / 6e-3 / 4e-5 of the largest |ref|
of the tensor on Gaussian data and compare launch variants with each other; this module compares every element with an fp64 CPU
reference or a value known in closed form (tests/numerics.py, "cross attention"; the derivations are in the docstrings there).

select   one winning key pi(i) per query, every other probability exactly 0 in fp32 whatever maximum the deferred loop holds; all scores
         negative, so an unmasked padding key or a zero K row wins instead; V rows distinct.  Expected: V[pi(i)] of the modality the
         direction reads.  From attn_core.h (numerics.attn_select_bound): the held maximum IS the winner's score when its tile runs, P of
         the winner is exp2 of the rounding error of m * c, below 2^-13, and rounds to 1 in both 16-bit types — BIT FOR BIT in the free,
         xtra and valu denominator forms alike (valu divides by the unrounded 1 + O(2^-13), which the 16-bit store absorbs); fp32: 5 u |v|.
uniform  numerics.attn_known_qkv (K = 0): the mean over exactly N keys.  16 bit: bit for bit; fp32: 3 u |mean|.
graded   real softmax weights, Q / K small integers (exact integer scores), dominant keys late in the key order: a step below the
         deferral slack (no rescale, p up to 2^6), one just above it, steps far above it (O and the denominator rescaled), the last one on
         the last key of the ragged last tile.  Reference: fp64 softmax(q k^T / sqrt(d_k)) v with the true d_k; bound per element counted
         from the code (numerics.attn_graded_bound): exponent and exp2 terms times the weighted deviation of V around the reference, the
         rounding of P (numerator and denominator alike in free / xtra, numerator only in valu), the fp32 accumulation, 1 / l, half a unit
         of storage.  At the padded head dimensions (d_k = 40, 72, 192) c = log2e / sqrt(DKP) exceeds it more than tenfold
         (tests/test_numerics_selftest.py).

Cells: heads = 8; resident form d_k 16, 32, 40, 64, 72, 128 (free, xtra, free, valu, valu, valu); streaming form d_k 64, 128 (forced with
ops.attn_stream()), 192, 256; bf16, f16, fp32; (B, N) = (1, 77), (4, 77), (1, 130), (4, 130), (1, 32): a ragged last key / query tile of 13
and of 2, a fifth query tile (a wave's second), one tile without padding (the two-tiles-per-trip loop's odd exit), the plain grid and the
XCD-remapped one; query splits: the library's choice, 1 and 2.  B = 1 runs the first image of the B = 4 operands.  A closing test reads
the cells back from icaf_cross_attention_form / _config.  Poisoned buffers: qkv between +Inf rows in front and NaN rows behind, out
NaN-prefilled between NaN guards, the result bit-identical to a run whose guards hold ordinary numbers.

The exp2 term: EXP2_REL = 1 ulp is the accuracy the project's SiLU budget already takes from the ISA guide for v_exp_f32; the guide's text
is not at hand in this repository, so the fp32 rows of the table in docs/HISTORY.md section 22 — device against fp64, no other kernel
involved — are the record of the margin that figure leaves.

Known limitations.  uniform cannot see key order, a wrong maximum, a wrong rescale or a wrong scale (the mean is invariant under all of
them); select cannot see a wrong scale either (the winner still wins) — graded holds those.  select pins P = 1, so the half-unit-of-P
difference between the denominator forms is exercised by graded only, inside a budget, not bit for bit.  The graded budget is dominated
by half a unit of storage in 16 bit and by the accumulation term (3 u per key, no rounding mode assumed for the MFMA) in fp32, where the
device stays far inside it.  The cold-path vote is wave-wide, so which lanes take it depends on their neighbours; the emulation of the
self-test models that, the bound does not need to.

Every test prints the largest err / budget it saw before it asserts (`-s`); docs/HISTORY.md section 22 records them."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm                                   # noqa: E402
from numerics import BF16, F16, F32                     # noqa: E402
from helpers import lib_option                          # noqa: E402
from icafusion_amd import ops                           # noqa: E402

DEV = "cuda:0"
HEADS = nm.ATTN_HEADS
FAMILIES = ("select", "uniform", "graded")
SPLITS = (0, 1, 2)                                      # attn_qsplit: the library's choice, one split, two
DTYPES = (BF16, F16, F32)
CELLS = [(form, dk, dt) for form, dk in sorted(nm.ATTN_CELLS, key=lambda c: (c[1], c[0])) for dt in DTYPES]      # (by d_k: the operands are shared)
RAN = set()                                             # (form, dkp, dtype, remap, more than one split) of every launch that passed
RATIOS = {}                                             # (family, form, dkp, dtype) -> largest err / budget
_CASES = {}


def cell_id(form, dk, dt):
    return f"{'stream' if form else 'resident'}-dk{dk}-{nm.DT_NAME[dt]}"


def case(family, N, dk):
    """(qkv, reference) of one family on the CPU at the largest batch of this N, built once; only one d_k is kept."""
    if _CASES.get("dk") != dk:
        _CASES.clear()
        _CASES["dk"] = dk
    key = (family, N)
    if key not in _CASES:
        B, C = max(b for b, n in nm.ATTN_TOKENS if n == N), HEADS * dk
        if family == "select":
            qkv, want, _ = nm.attn_select_qkv(B, N, dk, 7000 + 10 * dk + N)
        elif family == "uniform":
            qkv, want = nm.attn_known_qkv(B, N, C, F16, 100 * C + N)
            assert torch.equal(qkv.to(BF16).float(), qkv)
        else:
            qkv = nm.attn_graded_qkv(B, N, dk, 9000 + 10 * dk + N)
            want = nm.attn_ref64(qkv, B, N, C)
        _CASES[key] = (qkv, want)
    return _CASES[key]


def first_images(qkv, ref, B, N):
    """The first B images of a case: rows [0, B * N) of either modality."""
    cut = lambda t: t[:, :B * N].contiguous() if torch.is_tensor(t) else t
    return cut(qkv), ({k: cut(v) for k, v in ref.items()} if isinstance(ref, dict) else cut(ref))


def forced_form(form, dk):
    """The streaming form is the library's own choice above d_k = 128 and forced through the knob below."""
    return ops.attn_stream() if form and dk <= 128 else contextlib.nullcontext()


def launch(qkv, out, B, N, form, dk, dt, forced):
    """One icaf_cross_attention launch under the cell's knobs (form: what numerics.attn_form expects for the shape); returns
    (dkp, qsplit, remap) as the library reports them."""
    C = HEADS * dk
    with lib_option("attn_qsplit", forced), forced_form(form, dk):
        assert ops.cross_attention_form(dt, B, N, C, HEADS) == form
        cfg = ops.cross_attention_config(dt, B, N, C, HEADS)
        ops.cross_attention(qkv, out, B, N, HEADS)(ops.current_stream_ptr())
        torch.cuda.synchronize()
    assert cfg[0] == nm.attn_dkp(dk, form) and cfg[2] == int((2 * B) % 8 == 0)
    return cfg


def note(family, form, dkp, dt, ratio):
    key = (family, "stream" if form else "resident", dkp, nm.DT_NAME[dt])
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)


@pytest.mark.parametrize("cell_form,dk,dt", CELLS, ids=[cell_id(*c) for c in CELLS])
def test_attention_families_against_fp64(cell_form, dk, dt):
    """select, uniform and graded on one (form, d_k, dtype) cell at every (B, N) and every split setting, into a NaN-prefilled output."""
    if dk % nm.VEC[dt]:
        pytest.skip("head dim not a multiple of the 16-byte vector for this dtype")
    C = HEADS * dk
    failures, worst = [], {}
    for B, N in nm.ATTN_TOKENS:
        form = nm.attn_form(dk, N, dt, cell_form)        # (fp32, d_k = 128, N = 130 does not fit the LDS: the library streams it)
        dkp = nm.attn_dkp(dk, form)
        for fam in FAMILIES:
            qkv, ref = first_images(*case(fam, N, dk), B, N)
            if fam == "graded":
                nm.assert_rounding_exercised(ref["out"], dt, f"graded dk={dk} N={N}")
            qg = qkv.to(dt).to(DEV)
            for forced in SPLITS:
                out = torch.empty((2, B * N, C), dtype=dt, device=DEV)
                nm.bits(out).fill_(nm.NAN_BITS[dt])
                _, qsplit, remap = launch(qg, out, B, N, form, dk, dt, forced)
                what = f"{fam} {cell_id(form, dk, dt)} B={B} N={N} qsplit={qsplit} remap={remap}"
                got = out.cpu()
                ratio = nm.attn_ratio(fam, got, ref, N, dk, form, dt)
                worst[fam] = max(worst.get(fam, 0.0), ratio)
                note(fam, form, dkp, dt, ratio)
                try:
                    nm.check_attention(fam, got, ref, N, dk, form, dt, what)
                except AssertionError as e:
                    failures.append(f"{what}: {str(e)[:300]}")
                    continue
                RAN.add((form, dkp, dt, remap, qsplit > 1))
    print(f"\n[attn] {cell_id(cell_form, dk, dt)} ({nm.attn_den(dk, cell_form, dt)}): largest err / budget " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not failures, f"{len(failures)} launches failed:\n" + "\n".join(failures[:12])


def test_every_attention_cell_ran():
    """Closing test: every (form, DKP, dtype, XCD remap, more than one split) cell that icaf_cross_attention_form / _config report for the
    lists above was run and passed; the lists reach both placements and both split classes of every instantiation."""
    if not RAN:
        pytest.fail("run together with test_attention_families_against_fp64 (same process): nothing was recorded")
    want = set()
    for cell_form, dk, dt in CELLS:
        C = HEADS * dk
        for B, N in nm.ATTN_TOKENS:
            for forced in SPLITS:
                with lib_option("attn_qsplit", forced), forced_form(cell_form, dk):
                    form = ops.cross_attention_form(dt, B, N, C, HEADS)
                    assert form == nm.attn_form(dk, N, dt, cell_form)
                    dkp, qsplit, remap = ops.cross_attention_config(dt, B, N, C, HEADS)
                want.add((form, dkp, dt, remap, qsplit > 1))
    full = {(form, nm.attn_dkp(dk, form), dt, r, s) for form, dk, dt in CELLS for r in (0, 1) for s in (False, True)}
    assert want == full, sorted(full - want, key=str)
    assert want <= RAN, f"unreached or failed cells: {sorted(want - RAN, key=str)}"
    print(f"\n[cells] {len(want)} (form, DKP, dtype, remap, split) cells ran")
    print("[ratios] " + "; ".join(f"{k[0]} {k[1]} DKP{k[2]} {k[3]}: {v:.3f}" for k, v in sorted(RATIOS.items())))


# ------------------------------------------------------------------------------------------------------------------------------------
# poisoned buffers
# ------------------------------------------------------------------------------------------------------------------------------------
class GuardedQkv:
    """qkv (2, B * N, 3C) inside a larger allocation: `guard` whole rows in front holding `front` bits and as many behind holding `back`
    bits (qkv has no leading-dimension argument, so the guards are whole rows)."""

    def __init__(self, qkv, dt, front, back, guard=4):
        rows, c3 = qkv.shape[0] * qkv.shape[1], qkv.shape[2]
        self.buf = torch.empty((rows + 2 * guard, c3), dtype=dt, device=DEV)
        b = nm.bits(self.buf)                            # (a view: the buffer is contiguous)
        b[:guard] = front
        b[guard + rows:] = back
        self.view = self.buf[guard:guard + rows].view(qkv.shape)
        self.view.copy_(qkv.to(dt))
        self.g, self.rows = guard, rows
        self.before = self.buf.clone()

    def assert_guards_intact(self, what):
        ne = nm.bits(self.buf) != nm.bits(self.before)
        assert not bool(ne.any()), f"{what}: {int(ne.sum())} elements of qkv or its guard rows changed; first at {nm._first(ne)}"


def plain_bits(dt):
    return int(nm.bits(torch.tensor([7.0], dtype=dt))[0])


POISON_CELLS = [(0, 40, dt) for dt in DTYPES] + [(0, 72, BF16), (0, 32, F16)] + [(1, 192, dt) for dt in DTYPES] + [(1, 64, BF16)]


@pytest.mark.parametrize("form,dk,dt", POISON_CELLS, ids=[cell_id(*c) for c in POISON_CELLS])
def test_attention_poisoned_buffers(form, dk, dt):
    """select and graded at N = 77, two images: qkv between +Inf rows in front and NaN rows behind, out NaN-prefilled between NaN guards.
    Every guard bitwise unchanged, no NaN left in out, the fp64 check passes, and the bits equal those of a run whose guards and prefill
    hold 7.0.  A staging read past row N of the last image or before the first, or past d_k into the neighbouring head, turns into NaN
    through 0 * Inf or into a wrong winner."""
    B, N, C = 2, 77, HEADS * dk
    for fam in ("select", "graded"):
        qkv, ref = first_images(*case(fam, N, dk), B, N)
        what = f"poison {fam} {cell_id(form, dk, dt)}"
        got = []
        for poisoned in (True, False):
            q = GuardedQkv(qkv, dt, nm.INF_BITS[dt] if poisoned else plain_bits(dt), nm.NAN_BITS[dt] if poisoned else plain_bits(dt))
            out = nm.PoisonedFlat((2, B * N, C), dt, DEV, nm.NAN_BITS[dt] if poisoned else plain_bits(dt), None, 4 * C)
            launch(q.view, out.view, B, N, form, dk, dt, 0)
            q.assert_guards_intact(what)
            out.assert_outside_intact(what + ": out")
            o = out.view.cpu()
            assert not bool(torch.isnan(o.float()).any()), f"{what}: NaN left in out (poisoned={poisoned})"
            if poisoned:
                r = nm.attn_ratio(fam, o, ref, N, dk, form, dt)
                print(f"\n[attn poison] {what}: err / budget {r:.3f}")
                nm.check_attention(fam, o, ref, N, dk, form, dt, what)
            got.append(o)
        assert nm.same_bits(got[0], got[1]), f"{what}: the poisoned run differs from the plain one"
