"""The checkers of tests/numerics.py, shown to fail (CPU only).

A torch emulation of one conv launch — fp32 convolution on lattice data, the device's activation expressions, RNE to the storage
type — stands in for the kernel.  The clean emulation must pass the bit-exact check and the counted budgets; each planted defect must
be rejected.  For every (shape, 16-bit type) that tests/test_gpu_exact.py checks bit for bit, the lattice must really exercise
rounding: >= 5 % inexact results and at least one exact tie, from the reference alone.

What the max-norm `close()` of tests/test_gpu_kernels.py (max |got - ref| / max |ref| <= 2e-2 bf16, 3e-3 fp16) makes of the same
defects is printed (`-s`) and not asserted; on these inputs it accepts: truncation (both types), the dropped bias of one channel
(both types), the changed erf coefficient, and -0 returned as a small positive number; it rejects the dropped 8-channel vector (lattice
sums are larger than Gaussian ones).  It cannot see the stray write at all (it never looks
outside the view), and sees the unwritten element only through the NaN prefill this suite adds."""
import pytest
import torch
import torch.nn.functional as F

import numerics as nm
from numerics import ACT_GELU, ACT_NONE, ACT_SILU, BF16, F16, F32

OLD_TOL = {F32: 2e-5, BF16: 2e-2, F16: 3e-3}


def old_close_accepts(got, ref, dt):
    scale = max(float(ref.abs().max()), 1e-6)
    return float((got.double() - ref).abs().max()) / scale <= OLD_TOL[dt]


def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def shape_operands(name, dt, g=0):
    if name in nm.PRE_SHAPES:
        B, H, W, cin, cout, phw, nearest = nm.PRE_SHAPES[name]
        k, s, p = 1, 1, 0
    else:
        B, H, W, cin, cout, k, s, p, _ = nm.EXACT_SHAPES[name]
        phw, nearest = None, False
    Ho, Wo = nm.out_hw(H, W, k, s, p)
    return nm.lattice(dt, B, H, W, cin, cout, k, Ho, Wo, nm.shape_seed(name, dt, g), pre_hw=phw), s, p, nearest


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("name", list(nm.EXACT_SHAPES) + list(nm.PRE_SHAPES))
def test_lattice_exercises_rounding_for_every_gpu_shape(name, dt):
    flags = nm.EXACT_SHAPES[name][8] if name in nm.EXACT_SHAPES else {}
    for g in range(2 if (flags.get("pair") or flags.get("groups2")) else 1):
        d, s, p, nearest = shape_operands(name, dt, g)
        z, _ = nm.ref64(d["x"], d["w"], d["bias"], s, p, ACT_NONE, pre=d["pre"], pre_nearest=nearest)
        aa = nm.ALPHAS_G2[g][0] if flags.get("groups2") else nm.ALPHA_ACC
        share, ties = nm.assert_lattice_condition(z, dt, aa, f"{name} group {g}")
        print(f"{name} {dt} g{g}: inexact share {share:.3f}, ties {ties}")


def test_fp32_accumulation_is_exact_in_any_order():
    """The premise: fp32 conv2d == fp64 on the lattice (ref64 asserts it), also with the channel order reversed and at the largest K."""
    d = nm.lattice(F16, 1, 6, 6, 512, 8, 3, 6, 6, 7)                    # K = 4608, the finest grid
    z, _ = nm.ref64(d["x"], d["w"], d["bias"], 1, 1, ACT_NONE)
    zr = F.conv2d(d["x"].flip(1), d["w"].flip(1), d["bias"], 1, 1)
    assert torch.equal(zr.double(), z)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("use_res", [False, True])
def test_clean_emulation_is_accepted(dt, use_res):
    d, s, p, _ = shape_operands("ragged3x3", dt)
    res = d["res"] if use_res else None
    for act in nm.A3:
        z, out = nm.ref64(d["x"], d["w"], d["bias"], s, p, act, res, nm.ALPHA_ACC, nm.ALPHA_RES)
        got = nm.emulate(d, s, p, act, dt, dt, use_res, nm.ALPHA_ACC, nm.ALPHA_RES)
        if act == ACT_NONE:
            nm.assert_same_bits(got, nm.expected_exact(z, dt, res, nm.ALPHA_ACC, nm.ALPHA_RES), f"clean {dt}")
        r = nm.assert_budget(got, out, nm.launch_bound(z, act, dt, dt, res, nm.ALPHA_ACC, nm.ALPHA_RES), f"clean act {act} {dt}", signed=not use_res)
        print(f"clean emulation act {act} {dt} res={use_res}: err / budget {r:.3f}")


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("defect", ["trunc", "vector", "bias"])
def test_linear_defects_are_rejected(defect, dt):
    """Truncation instead of RNE; one 8-channel vector of one tap dropped at a corner pixel; the bias of one channel dropped."""
    d, s, p, _ = shape_operands("ragged3x3", dt)
    if defect == "vector":
        assert bool((d["w"][:, 8:16, p, p] @ d["x"][0, 8:16, 0, 0] != 0).any()), "the dropped vector must contribute"
    for act in (ACT_NONE, ACT_SILU):
        z, out = nm.ref64(d["x"], d["w"], d["bias"], s, p, act, None, nm.ALPHA_ACC)
        got = nm.emulate(d, s, p, act, dt, dt, False, nm.ALPHA_ACC, defect=defect)
        bound = nm.launch_bound(z, act, dt, dt, None, nm.ALPHA_ACC)
        if act == ACT_NONE:
            assert rejected(lambda: nm.assert_same_bits(got, nm.expected_exact(z, dt, None, nm.ALPHA_ACC), defect))
        assert rejected(lambda: nm.assert_budget(got, out, bound, defect)), f"{defect} act {act}: the budget check accepted it"
        print(f"{defect} {dt} act {act}: err / budget {nm.budget_ratio(got, out, bound):.3g}; old close() accepts: {old_close_accepts(got, out, dt)}")


@pytest.mark.parametrize("in_dt", [BF16, F16], ids=["bf16", "f16"])
def test_changed_erf_coefficient_is_rejected(in_dt):
    """a3 = 1.421413741 -> 1.421513741 in gelu_fast_f, seen through the fp32 output of a 16-bit layer over every finite input pattern.
    (In a 16-bit OUTPUT the change — 1e-4 on erf at most — is below half a unit of the type except in the negative tail; the fp32-output
    configuration of the sweep is the one that pins the coefficients.)"""
    v = nm.all_finite_patterns(in_dt).float()
    ref = nm.act64(v.double(), ACT_GELU)
    bound = nm.launch_bound(v.double(), ACT_GELU, in_dt, F32)
    clean = nm.emulate(None, 1, 0, ACT_GELU, in_dt, F32, z=v)
    r = nm.assert_budget(clean, ref, bound, "clean fast GELU")
    bad = nm.emulate(None, 1, 0, ACT_GELU, in_dt, F32, z=v, defect="erf")
    assert rejected(lambda: nm.assert_budget(bad, ref, bound, "erf coefficient"))
    fin = v.abs() < 1e4
    print(f"fast GELU {in_dt}: clean err / budget {r:.3f}, changed coefficient {nm.budget_ratio(bad, ref, bound):.3g}; "
          f"old close() accepts (|v| < 1e4, fp16 out): {old_close_accepts(bad[fin].to(F16), ref[fin], F16)}")


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_negative_zero_as_small_positive_is_rejected(dt):
    v = nm.all_finite_patterns(dt).float()
    ref = nm.act64(v.double(), ACT_SILU)
    bound = nm.launch_bound(v.double(), ACT_SILU, dt, dt)
    clean = nm.emulate(None, 1, 0, ACT_SILU, dt, dt, z=v)
    assert bool(((clean == 0) & torch.signbit(clean.float())).any()), "the sweep must reach the -0 branch"
    r = nm.assert_budget(clean, ref, bound, "clean SiLU sweep")
    bad = nm.emulate(None, 1, 0, ACT_SILU, dt, dt, z=v, defect="negzero")
    assert rejected(lambda: nm.assert_budget(bad, ref, bound, "-0 as +1e-40"))
    print(f"SiLU sweep {dt}: clean err / budget {r:.3f}; -0 as +1e-40: old close() accepts: {old_close_accepts(bad, ref, dt)}")


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_unwritten_and_stray_elements_are_rejected(dt):
    """One output element left at its (NaN) prefill; one element written one vector past cout."""
    d, s, p, _ = shape_operands("ragged3x3s2", dt)
    z, out = nm.ref64(d["x"], d["w"], d["bias"], s, p, ACT_NONE)
    got = nm.emulate(d, s, p, ACT_NONE, dt, dt).permute(0, 2, 3, 1)                      # NHWC
    want = nm.expected_exact(z, dt).permute(0, 2, 3, 1)
    cout = got.shape[3]
    y = nm.Poisoned(got.shape[:3], cout, dt, "cpu", nm.NAN_BITS[dt])
    assert bool(torch.isnan(y.view.float()).all()) and bool(torch.isnan(y.buf.float()).all())
    y.view.copy_(got)
    nm.assert_same_bits(y.view, want, "clean")
    y.assert_outside_intact("clean")
    y.view[0, 3, 2, 5] = float("nan")                                                    # never written
    assert rejected(lambda: nm.assert_same_bits(y.view, want, "unwritten"))
    bound = nm.launch_bound(z, ACT_NONE, dt, dt).permute(0, 2, 3, 1)
    assert rejected(lambda: nm.assert_budget(y.view, out.permute(0, 2, 3, 1), bound, "unwritten", signed=False))
    y.view.copy_(got)
    y.buf[0, 1, 1, y.lo + cout + nm.VEC[dt] - 1] = 1.0                                   # the last lane of the vector behind the view
    nm.assert_same_bits(y.view, want, "stray write leaves the view alone")
    assert not y.outside_intact() and rejected(lambda: y.assert_outside_intact("stray"))
    y.buf.copy_(y.before)
    y.buf[0, 0, 0, y.lo - 1] = 1.0                                                       # ... and the element in front of it
    assert rejected(lambda: y.assert_outside_intact("stray in front"))


def test_ulp_and_rne():
    one = torch.tensor([1.0, 1.5, 0.99, 2.0 ** -14, 2.0 ** -20, 0.0, -3.0], dtype=torch.float64)
    assert nm.ulp(one, BF16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -21, 2.0 ** -27, 2.0 ** -133, 2.0 ** -6]
    assert nm.ulp(one, F16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -9]
    t = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8], dtype=torch.float64)       # ties: to even
    assert nm.rne(t, BF16).double().tolist() == [1.0, 1.0 + 2.0 ** -6]
    assert nm.truncate(t.float(), BF16).double().tolist() == [1.0, 1.0 + 2.0 ** -7]
    assert nm.truncate(-t.float(), F16).double().tolist() == [-(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8)]
    assert nm.all_finite_patterns(BF16).shape == (65536,) and nm.f32_sweep_grid().shape == (3 * 65536,)
