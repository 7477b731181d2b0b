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


# ====================================================================================================================================
# pooling, resize and merge: the helpers behind tests/test_gpu_exact_pool.py, shown to fail
# ====================================================================================================================================
# What close() made of each planted defect, on rnd() data of the same shape, is printed as `old close() accepts: ...` (docs/HISTORY.md section 19).
rnd_like = nm.rnd

D16 = [BF16, F16]
D16_IDS = ["bf16", "f16"]
VERDICTS = {}                                        # (defect, dtype) -> close() accepted it on rnd() data


def record(defect, dt, accepted):
    VERDICTS[(defect, str(dt).split(".")[1])] = accepted
    print(f"{defect} {dt}: rejected by the new checkers; old close() accepts: {accepted}")


def pool_case(name, dt, w, probes=False, g=0):
    B, H, W, C, geom, _, _ = nm.POOL_GEOMS[name]
    if probes:
        x, pos = nm.pool_probes(B, H, W, C, geom, g), torch.zeros((geom[0] * geom[1], C))
    else:
        x, pos = nm.pool_lattice(B, H, W, C, geom[0] * geom[1], nm.shape_seed(name, dt, g))
    avg, mx, ref = nm.pool64(x, geom, w, pos)
    return x, pos, geom, avg, mx, ref


pool_check = nm.check_pool


def old_pool_verdict(name, dt, w, defect):
    """close() on rnd() data of the same geometry: reference fp64 on the dt-rounded input, the defective emulation as `got`."""
    B, H, W, C, geom, _, _ = nm.POOL_GEOMS[name]
    x = rnd_like((B, H, W, C), 21).to(dt).float()
    pos = rnd_like((geom[0] * geom[1], C), 23, 0.3)
    _, _, ref = nm.pool64(x, geom, w, pos)
    got = nm.emulate_pool(x, geom, w, pos, dt, defect)
    got = torch.nan_to_num(got.float(), nan=0.0).to(dt)          # (close() ran on zero-filled outputs: an unwritten element reads 0)
    return old_close_accepts(got, ref, dt)


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", [n for n, g in nm.POOL_GEOMS.items() if not g[6].get("big")])
def test_pool_clean_emulation_is_accepted_on_every_geometry(name, dt):
    """Probes (max path: bits; sum path: bits at power-of-two areas, budget otherwise) and lattice data with both weight pairs."""
    for probes, w in ((True, (0.0, 1.0)), (True, (1.0, 0.0)), (False, nm.W_DYADIC), (False, nm.W_REAL)):
        x, pos, geom, avg, mx, ref = pool_case(name, dt, w, probes)
        if probes and w == (0.0, 1.0):
            assert nm.pool_is_exact(avg, mx, w, pos, geom[2] * geom[3])
            assert set(ref.unique().tolist()) <= {0.0, 0.25, 0.5, 1.0, 2.0, 4.0} and float(ref.max()) > 0
            assert bool((ref.reshape(x.shape[0], -1, x.shape[3]).amax(1) > 0).all()) or name == "ekw6", "a probe lies in no window"
        r = pool_check(nm.emulate_pool(x, geom, w, pos, dt), avg, mx, ref, w, pos, geom, dt, f"clean {name} {w}")
        if not probes:
            nm.assert_rounding_exercised(ref, dt, f"pool {name} w={w}")
            print(f"clean pool {name} {dt} w={w}: err / budget {r:.3f}")


POOL_DEFECTS = [("lastcol", "r12tr1"), ("row12", "chunks2"), ("duprow", "chunks2"), ("max0", "r8tr1"), ("short", "oddth"), ("pos_nb", "r4tr1"),
                ("trunc", "r8tr1")]


@pytest.mark.parametrize("dt", D16, ids=D16_IDS)
@pytest.mark.parametrize("defect,name", POOL_DEFECTS)
def test_pool_defects_are_rejected(defect, name, dt):
    """Each defect must fail at least one of the launches the GPU test makes for the geometry (probes on both paths, lattice data with both
    weight pairs)."""
    caught = []
    for probes, w in ((True, (0.0, 1.0)), (True, (1.0, 0.0)), (False, nm.W_DYADIC), (False, nm.W_REAL)):
        x, pos, geom, avg, mx, ref = pool_case(name, dt, w, probes)
        if not probes and defect == "pos_nb":
            assert not torch.equal(pos.roll(-1, 0), pos)
        got = nm.emulate_pool(x, geom, w, pos, dt, defect)
        if rejected(lambda: pool_check(got, avg, mx, ref, w, pos, geom, dt, defect)):
            caught.append((probes, w))
    assert caught, f"{defect}: no launch of the geometry rejects it"
    if defect in ("lastcol", "row12", "duprow"):
        assert any(p for p, _ in caught), f"{defect}: the membership probes must catch it on their own"
    if defect == "max0":
        assert (False, nm.W_REAL) in caught and (False, nm.W_DYADIC) in caught, "the all-negative channels must show a maximum that starts at 0"
    print(f"{defect} on {name} {dt}: rejected by {caught}")
    record("pool:" + defect, dt, old_pool_verdict(name, dt, nm.W_REAL, defect))


def merge_case(name, dt):
    B, H, W, C, th, tw, exact = nm.MERGE_GEOMS[name]
    tok, fea = nm.merge_lattice(dt, B, H, W, C, th, tw, nm.shape_seed("merge" + name, dt))
    ref, bound = nm.merge64(tok, fea, dt)
    return tok, fea, ref, bound, exact


merge_check = nm.check_merge


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", [n for n in nm.MERGE_GEOMS if n != "big"])
def test_merge_clean_emulation_is_accepted(name, dt):
    tok, fea, ref, bound, exact = merge_case(name, dt)
    interp = torch.stack([F.interpolate(tok[g].double().permute(0, 3, 1, 2), size=fea.shape[2:4], mode="bilinear", align_corners=False)
                          .permute(0, 2, 3, 1) + fea[g].double() for g in range(2)])
    assert float((torch.cat((interp[0], interp[1]), -1) - ref).abs().max()) < 1e-12, "merge64 disagrees with F.interpolate in fp64"
    r = merge_check(nm.emulate_merge(tok, fea, dt), ref, bound, exact, dt, f"clean merge {name}")
    share = nm.assert_rounding_exercised(ref, dt, f"merge {name}")
    print(f"clean merge {name} {dt}: err / budget {r:.3f}, not representable {share:.3f}")


@pytest.mark.parametrize("dt", D16, ids=D16_IDS)
@pytest.mark.parametrize("defect,name", [("swap", "x2"), ("swap", "16to40"), ("align", "x2"), ("align", "20to68x84"), ("noclamp", "x4"),
                                         ("noclamp", "7x9to30x33"), ("trunc", "identity"), ("trunc", "16to40")])
def test_merge_defects_are_rejected(defect, name, dt):
    tok, fea, ref, bound, exact = merge_case(name, dt)
    got = nm.emulate_merge(tok, fea, dt, defect)
    assert rejected(lambda: merge_check(got, ref, bound, exact, dt, defect)), f"{defect} on {name}: accepted"
    B, H, W, C, th, tw, _ = nm.MERGE_GEOMS[name]
    tk = rnd_like((2, B, th, tw, C), 25).to(dt).float()
    fe = rnd_like((2, B, H, W, C), 21).to(dt).float()
    record(f"merge:{defect}:{name}", dt, old_close_accepts(nm.emulate_merge(tk, fe, dt, defect), nm.merge64(tk, fe, dt)[0], dt))


@pytest.mark.parametrize("dt", D16, ids=D16_IDS)
def test_nearest_ceil_at_scale_3_is_rejected(dt):
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-8, 9, (2, 5, 7, 16), generator=g).float().to(dt)
    nm.assert_same_bits(nm.emulate_nearest(x, 3), nm.nearest64(x, 3), "clean nearest")
    assert torch.equal(nm.nearest64(x, 3).float().permute(0, 3, 1, 2), F.interpolate(x.float().permute(0, 3, 1, 2), scale_factor=3, mode="nearest"))
    assert rejected(lambda: nm.assert_same_bits(nm.emulate_nearest(x, 3, "ceil"), nm.nearest64(x, 3), "ceil"))
    xr = rnd_like((2, 5, 7, 16), 11).to(dt)
    record("nearest:ceil", dt, old_close_accepts(nm.emulate_nearest(xr, 3, "ceil"), nm.nearest64(xr, 3).double(), dt))


@pytest.mark.parametrize("dt", D16, ids=D16_IDS)
def test_axpby_clean_truncated_and_first_pass_only(dt):
    """axpby: (128, -127) on integers is exact (every product below 2^24); (0.4, 0.7) within the counted budget; truncation rejected by
    both; a grid-stride loop that stops after its first 2^20 vector items leaves NaN behind, which both checks reject."""
    rows, C = nm.STRIDE_ITEMS // 16 + 300, 128                                  # (rows * C / 8 > 2^20 vectors)
    x0, x1 = nm.axpby_lattice(dt, (rows, C), 6)
    ref, bound = nm.axpby64(x0, x1, 128.0, -127.0, dt)
    clean = nm.emulate_axpby(x0, x1, 128.0, -127.0, dt)
    nm.assert_same_bits(clean, nm.rne(ref, dt) + 0.0, "clean axpby")
    nm.assert_rounding_exercised(ref, dt, "axpby (128, -127)")
    assert rejected(lambda: nm.assert_same_bits(nm.emulate_axpby(x0, x1, 128.0, -127.0, dt, "trunc"), nm.rne(ref, dt) + 0.0, "trunc"))
    record("axpby:trunc", dt, old_close_accepts(nm.emulate_axpby(x0, x1, 128.0, -127.0, dt, "trunc"), ref, dt))
    half = nm.first_pass_only(clean, float("nan"), dt)
    assert rejected(lambda: nm.assert_same_bits(half, nm.rne(ref, dt) + 0.0, "first pass only"))
    assert rejected(lambda: nm.assert_budget(half, ref, bound, "first pass only", signed=False))
    zero = nm.first_pass_only(clean, 0.0, dt)                                   # what close() saw: outputs came from torch.zeros ...
    small = clean[:1000]                                                        # ... and no case was large enough to have a second pass
    record("stride:first_pass_only (at the old test's size: never reached)", dt, old_close_accepts(small, ref[:1000], dt))
    record("stride:first_pass_only (had the old test been this large)", dt, old_close_accepts(zero, ref, dt))
    ref2, bound2 = nm.axpby64(x0[:4096], x1[:4096], 0.4, 0.7, dt)
    r = nm.assert_budget(nm.emulate_axpby(x0[:4096], x1[:4096], 0.4, 0.7, dt), ref2, bound2, "clean axpby (0.4, 0.7)", signed=False)
    assert rejected(lambda: nm.assert_budget(nm.emulate_axpby(x0[:4096], x1[:4096], 0.4, 0.7, dt, "trunc"), ref2, bound2, "trunc", signed=False))
    print(f"axpby (0.4, 0.7) {dt}: clean err / budget {r:.3f}")


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_vector_written_past_C_is_rejected(dt):
    """One vector written behind the 2C channels of the merged map (ldo = 2C + one vector): the view is as expected, the padding is not."""
    tok, fea, ref, bound, exact = merge_case("x2", dt)
    got = nm.emulate_merge(tok, fea, dt)
    v = nm.VEC[dt]
    y = nm.Poisoned(got.shape[:3], got.shape[3], dt, "cpu", nm.NAN_BITS[dt], lo=0, hi=v)
    y.view.copy_(got)
    merge_check(y.view, ref, bound, exact, dt, "clean")
    y.assert_outside_intact("clean")
    y.buf[1, 2, 3, got.shape[3]:] = 1.0
    merge_check(y.view, ref, bound, exact, dt, "the view is still right")
    assert rejected(lambda: y.assert_outside_intact("past C"))
    f = nm.PoisonedFlat((3, 5), dt, "cpu", nm.NAN_BITS[dt], torch.ones((3, 5)))
    f.assert_outside_intact("clean flat")
    f.buf[f.g + f.n] = 1.0
    assert rejected(lambda: f.assert_outside_intact("behind the tensor"))


def test_staging_references():
    img = torch.arange(2 * 3 * 4 * 6, dtype=F32).reshape(2, 3, 4, 6)
    s0 = nm.stage64(img, 0, 8)
    assert s0.shape == (2, 4, 6, 8) and float(s0[1, 2, 3, 1]) == float(img[1, 1, 2, 3]) and float(s0[..., 3:].abs().max()) == 0
    s1 = nm.stage64(img, 1, 16)
    assert s1.shape == (2, 2, 3, 16) and float(s1[1, 1, 2, 2 * 3 + 1]) == float(img[1, 1, 2 * 1 + 1, 2 * 2 + 0]) and float(s1[..., 12:].abs().max()) == 0
    assert float(s1[0, 1, 1, 1 * 3 + 2]) == float(img[0, 2, 2, 3])               # sub = 1: dy 0, dx 1
    for dt in (F32, BF16, F16):
        e = nm.u8_expected(dt)
        assert float(e[0]) == 0.0 and float(e[255]) == 1.0 and bool((e[1:].float() > e[:-1].float()).all())


def test_pool_launch_choice_of_every_geometry():
    """icaf_dmff_pool_config is host code: the table of tests/test_gpu_exact_pool.py is checked here without a GPU — the instantiation each
    geometry names, all seven reached, both sides of the two-token-rows threshold, the fp32 LDS boundary, and the index64 knob."""
    from helpers import lib_option
    from icafusion_amd import ops
    seen = set()
    for name, (B, H, W, C, geom, want, _) in nm.POOL_GEOMS.items():
        for dt in (F32, BF16, F16):
            c = ops.dmff_pool_config(dt, B, H, W, C, *geom)
            assert (c["kernel"], c["R"], c["TR"]) == want[dt], f"{name} {dt}: {c}"
            assert c["index64"] == 0
            seen.add(want[dt])
    assert seen == {(nm.ELEM, 0, 0)} | {(nm.ROWS, r, t) for r in (4, 8, 12) for t in (1, 2)}
    for (B, H, W, C, geom), tr in nm.TR_THRESHOLD:
        assert 2 * B * ((geom[0] + 1) // 2) in (254, 256)
        for dt in (F32, BF16, F16):
            assert ops.dmff_pool_config(dt, B, H, W, C, *geom)["TR"] == tr
    with lib_option("index64", 1):
        assert ops.dmff_pool_config(BF16, 2, 16, 20, 32, 4, 5, 4, 4, 4, 4) == dict(kernel=0, R=0, TR=0, index64=1)
        assert ops.dmff_pool_config(BF16, 1, 9, 11, 32, 7, 9, 3, 3, 1, 1) == dict(kernel=1, R=4, TR=1, index64=0)      # the rows kernel has no flat index
    assert ops.dmff_pool_config(BF16, 2, 16, 20, 32, 4, 5, 4, 4, 4, 4)["index64"] == 0
    from icafusion_amd._lib import IcafError
    with pytest.raises(IcafError, match="window exceeds the feature map"):
        ops.dmff_pool_config(BF16, 1, 9, 11, 32, 7, 9, 4, 3, 1, 1)
    with pytest.raises(IcafError, match="multiples of 8"):
        ops.dmff_pool_config(BF16, 1, 9, 11, 36, 7, 9, 3, 3, 1, 1)


def test_close_verdicts_are_recorded():
    """Closing: prints what close() accepted (docs/HISTORY.md section 19); every planted defect above left its verdict."""
    if not VERDICTS:
        print("run with the defect tests of this file (same process): nothing was recorded")
    for k in sorted(VERDICTS):
        print(f"close() on {k[0]} {k[1]}: {'ACCEPTS' if VERDICTS[k] else 'rejects'}")


# ====================================================================================================================================
# DMFF block kernels: the helpers behind tests/test_gpu_exact_dmff.py, shown to fail
# ====================================================================================================================================
# A torch emulation of one icaf_dmff_wide_proj_mlp launch (nm.emulate_proj_mlp: fp32 arithmetic, the rounding points of dmff_wide.hip)
# stands in for the kernel.  What a max-norm tolerance makes of each planted defect on Gaussian data of the same shape is printed as
# `old close() accepts: ...` (docs/HISTORY.md section 20).
CPU_ROWS = 154                                       # three tiles, the last with an empty second half
_DMFF = {}


def dmff_case(kind, C, dt, use_x32=False):
    """(operands cut to CPU_ROWS, reference) of test (a) / (b), built once per (C, dtype)."""
    key = (kind, C, dt, use_x32)
    if key not in _DMFF:
        ops_key = (kind, C, dt)
        if ops_key not in _DMFF:
            _DMFF[ops_key] = nm.dmff_take_rows((nm.dmff_operands_a if kind == "a" else nm.dmff_operands_b)(C, dt, CPU_ROWS), CPU_ROWS)
        d = _DMFF[ops_key]
        _DMFF[key] = (d, nm.dmff_xatt64(d, use_x32) if kind == "a" else nm.dmff_ref_b(d, dt, use_x32))
    return _DMFF[key]


def dmff_checks(cell, use_x32, defect=None):
    """Run the emulation of one cell through the checks the GPU test makes; returns ({check name: error text or None}, ratios of (b))."""
    C, dt, ks, r32 = cell
    res = {}
    d, z = dmff_case("a", C, dt, use_x32)
    y, y32 = nm.emulate_proj_mlp(d, dt, ks, r32, use_x32, defect)
    try:
        nm.check_proj_mlp_a(y, y32, z, dt, "(a)")
        res["a"] = None
    except AssertionError as e:
        res["a"] = str(e)[:300]
    d, ref = dmff_case("b", C, dt, use_x32)
    y, y32 = nm.emulate_proj_mlp(d, dt, ks, r32, use_x32, defect)
    ratios = (nm.budget_ratio(y, ref["out"], ref["by"]), nm.budget_ratio(y32, ref["out"], ref["b32"]) if r32 else 0.0)
    try:
        nm.check_proj_mlp_b(y, y32, ref, dt, "(b)")
        res["b"] = None
    except AssertionError as e:
        res["b"] = str(e)[:300]
    return res, ratios, ref["share"]


@pytest.mark.parametrize("cell", nm.DMFF_CELLS, ids=[nm.cell_id(c) for c in nm.DMFF_CELLS])
def test_proj_mlp_clean_emulation_is_accepted_at_every_cell(cell):
    """The clean emulation passes (a) bit for bit and (b) within the counted bounds at every build of the instantiation table, with and
    without the fp32 stream of an earlier iteration; the ambiguous-rounding share of (b) is at most 5 %; (a) really exercises rounding."""
    C, dt, ks, r32 = cell
    for use_x32 in ((False, True) if r32 else (False,)):
        res, ratios, share = dmff_checks(cell, use_x32)
        assert res == {"a": None, "b": None}, f"{nm.cell_id(cell)} x32={use_x32}: {res}"
        assert share <= 0.05
        if dt != F32:
            nm.assert_lattice_condition(dmff_case("a", C, dt, use_x32)[1], dt, 1.0, f"(a) {nm.cell_id(cell)}")
        print(f"clean proj_mlp {nm.cell_id(cell)} x32={int(use_x32)}: (b) err / budget y {ratios[0]:.3f} y32 {ratios[1]:.3f}, ambiguous share {share:.4f}")


# defect -> the cells it is planted in (every one must reject it) — trunc has no x_att store to plant it in under the fp32 stream, b1off needs
# a split, erf is pinned by the UNROUNDED stream (in a 16-bit y a change of 1e-4 on erf is mostly below half a unit, as for the convolutions)
DEFECT_CELLS = {
    "trunc": [(256, 1, False), (512, 2, False)], "swap": [(128, 1, False), (512, 2, True)], "lastchunk": [(512, 1, False), (256, 4, False)],
    "b1off": [(256, 2, False), (512, 4, False), (256, 2, True)], "halfshift": [(128, 1, True), (512, 4, False)],
    "lnswap": [(256, 1, False), (512, 2, True)], "erf": [(256, 1, True), (512, 2, True)],
}
DEFECT_MUST = {"trunc": "a", "swap": "a", "lastchunk": "b", "b1off": "b", "halfshift": "a", "lnswap": "b", "erf": "b"}


@pytest.mark.parametrize("dt", D16, ids=D16_IDS)
@pytest.mark.parametrize("defect", nm.PROJ_MLP_DEFECTS)
def test_proj_mlp_defects_are_rejected(defect, dt):
    for C, ks, r32 in DEFECT_CELLS[defect]:
        cell = (C, dt, ks, r32)
        res, ratios, _ = dmff_checks(cell, False, defect)
        caught = sorted(k for k, v in res.items() if v is not None)
        assert DEFECT_MUST[defect] in caught, f"{defect} in {nm.cell_id(cell)}: check ({DEFECT_MUST[defect]}) accepted it ({res})"
        print(f"{defect} in {nm.cell_id(cell)}: rejected by {caught}; (b) err / budget y {ratios[0]:.3g} y32 {ratios[1]:.3g}")
        dr = nm.dmff_operands_rnd(C, CPU_ROWS)
        got, _ = nm.emulate_proj_mlp(dr, dt, ks, r32, False, defect)
        record(f"proj_mlp:{defect}:{nm.cell_id(cell)}", dt, old_close_accepts(got, nm.proj_mlp64(dr, dt), dt))
    if defect == "erf":                              # for the record: what the 16-bit y alone makes of it
        res, ratios, _ = dmff_checks((256, dt, 1, False), False, defect)
        print(f"erf in {nm.cell_id((256, dt, 1, False))} (no fp32 stream): rejected by {sorted(k for k, v in res.items() if v)}; err / budget y {ratios[0]:.3g}")


@pytest.mark.parametrize("dt", D16, ids=D16_IDS)
def test_one_pass_variance_shows_in_the_fp32_stream_only(dt):
    """The known limitation: on rows m +- s that a 16-bit type holds, E[x^2] - mean^2 is exact too; around m = 4096 (the x32 case) x * x
    is not an fp32 number and a one-pass variance leaves the lattice."""
    for use_x32, want_exact in ((False, True), (True, False)):
        d, _ = dmff_case("b", 256, dt, use_x32)
        x = (d["x32"] if use_x32 else d["x"])[0]
        var1 = (x * x).sum(1) / 256.0 - (x.sum(1) / 256.0) ** 2
        assert bool((var1 == 0.25).all()) == want_exact


@pytest.mark.parametrize("dt", D16, ids=D16_IDS)
@pytest.mark.parametrize("tpr", [4, 8])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_exact_layernorm_rows_stay_exact_under_partial_sums(C, tpr, dt):
    """Construction 1 through the tile LayerNorm's own association (4 / 8 threads per row, vectors dealt round-robin, xor-shuffle tree):
    mean = m, rstd = 1 and the output is +-s gamma + beta bit for bit, for s = 0.5 and for the scaled rows 2 (m +- 0.25)."""
    g = torch.Generator().manual_seed(C + tpr)
    gam, bet = nm._nonzero(g, 16, (C,)) / 8.0, nm._ri(g, -16, 16, (C,)) / 8.0
    for x in (nm.exact_ln_rows(64, C, 0.5, 40 + C), 2.0 * nm.exact_ln_rows(64, C, 0.25, 50 + C, kmax=8)):
        nm.assert_exact_ln(x, nm.LN_EPS_EXACT, dt)
        mean, rstd, out = nm.tile_layernorm32(x, gam, bet, nm.LN_EPS_EXACT, tpr, dt)
        m = (x.amax(1, keepdim=True) + x.amin(1, keepdim=True)) / 2.0
        assert torch.equal(mean, m) and bool((rstd == 1.0).all())
        nm.assert_same_bits(out, nm.rne(((x - m) * gam + bet).double(), dt), f"tile LayerNorm C={C} tpr={tpr}")
    assert rejected(lambda: nm.assert_exact_ln(x + 0.125 * (torch.arange(C) == 3), nm.LN_EPS_EXACT, dt))
    assert rejected(lambda: nm.assert_exact_ln(x, 1e-5, dt))


def test_rne64_and_sparse_w2():
    v = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).float()
    for dt in (BF16, F16):
        assert torch.equal(nm.rne64(v.double(), dt), v.to(dt).double())
        assert nm.rne64(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64), BF16).item() == 1.0 + 2.0 ** -7     # (through fp32 it would tie to 1.0)
    w = nm.sparse_w2(256, 1024, BF16, 3)
    assert bool(((w != 0).sum(2) == nm.W2_NNZ).all()) and bool(((w != 0).sum(1) == 8).all())


@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("B,N,C", [(4, 64, 64), (3, 77, 128)])
def test_known_attention_tile_and_the_two_launch_kernel_cases(B, N, C, dt):
    """Test (e)'s operands: with K = 0 the fp64 softmax attention over every image returns the recorded mean of V, which every type
    represents; for N = 77 the fp32 product (N mean) * fl(1 / N) lies within 2^-22 of the mean — far inside half a unit of either 16-bit
    type, where the attention tile is stored — while the fp32 build, which stores it unrounded, is only given power-of-two N.  The clean
    emulation passes (a) and (b) with that tile in place of att."""
    qkv, att = nm.attn_known_qkv(B, N, C, dt, 5)
    q, k, v = (qkv[:, :, i * C:(i + 1) * C].reshape(2, B, N, C).double() for i in range(3))
    for heads in (2, 4):
        dk = C // heads
        split = lambda t: t.reshape(2, B, N, heads, dk).transpose(2, 3)
        p = torch.softmax(split(q.flip(0)) @ split(k).transpose(-1, -2) / dk ** 0.5, -1)
        out = (p @ split(v)).transpose(2, 3).reshape(2, B * N, C)
        assert float((out - att.double()).abs().max()) < 1e-12
    assert torch.equal(att.to(dt).float(), att)
    dev = (att * N) * (torch.tensor(1.0) / torch.tensor(float(N))) - att
    assert float(dev.abs().max()) <= 8 * 2.0 ** -22 and (N & (N - 1) or not bool(dev.any()))
    for kind in ("a", "b"):
        d = (nm.dmff_operands_a if kind == "a" else nm.dmff_operands_b)(C, dt, B * N)
        d["att"] = att
        y, _ = nm.emulate_proj_mlp(d, dt)
        if kind == "a":
            nm.check_proj_mlp_a(y, None, nm.dmff_xatt64(d), dt, "(e, a)")
        else:
            nm.check_proj_mlp_b(y, None, nm.dmff_ref_b(d, dt), dt, "(e, b)")


def test_close_verdicts_of_the_block_defects_are_recorded():
    """Closing: what close() accepted among the proj_mlp defects above (docs/HISTORY.md section 20)."""
    mine = {k: v for k, v in VERDICTS.items() if k[0].startswith("proj_mlp:")}
    if not mine:
        print("run with test_proj_mlp_defects_are_rejected (same process): nothing was recorded")
    for k in sorted(mine):
        print(f"close() on {k[0]} {k[1]}: {'ACCEPTS' if mine[k] else 'rejects'}")


# ====================================================================================================================================
# cross attention: the helpers behind tests/test_gpu_exact_attn.py, shown to fail
# ====================================================================================================================================
# nm.emulate_attention (an fp32 restatement of the tile loop of attn_core.h) stands in for the kernels.  What close(factor=2) of
# tests/test_gpu_kernels.py makes of each planted defect on the Gaussian data of test_cross_attention is recorded beside the verdict of the
# new families (docs/HISTORY.md section 22).
D3 = [F32, BF16, F16]
D3_IDS = ["f32", "bf16", "f16"]
ATTN_FAMILIES = ("select", "uniform", "graded")
_ATTN = {}


def attn_case(family, B, N, dk):
    """(qkv, reference) of one family, built once per shape (every value is representable in all three types)."""
    key = (family, B, N, dk)
    if key not in _ATTN:
        C = nm.ATTN_HEADS * dk
        if family == "select":
            qkv, want, _ = nm.attn_select_qkv(B, N, dk, 7000 + 10 * dk + N)
        elif family == "uniform":
            qkv, want = nm.attn_known_qkv(B, N, C, F16, 100 * C + N)
        else:
            qkv = nm.attn_graded_qkv(B, N, dk, 9000 + 10 * dk + N)
            want = nm.attn_ref64(qkv, B, N, C)
        _ATTN[key] = (qkv, want)
    return _ATTN[key]


def attn_checks(form, dk, dt, B, N, defect=None, families=ATTN_FAMILIES):
    """The emulation of one cell through the check of every family: {family: (error text or None, err / budget)}."""
    res = {}
    for fam in families:
        qkv, want = attn_case(fam, B, N, dk)
        got = nm.emulate_attention(qkv, B, N, nm.ATTN_HEADS * dk, nm.ATTN_HEADS, dt, form, defect)
        ratio = nm.attn_ratio(fam, got, want, N, dk, form, dt)
        try:
            nm.check_attention(fam, got, want, N, dk, form, dt, fam)
            res[fam] = (None, ratio)
        except AssertionError as e:
            res[fam] = (str(e)[:200], ratio)
    return res


@pytest.mark.parametrize("dt", D3, ids=D3_IDS)
@pytest.mark.parametrize("form,dk", nm.ATTN_CELLS, ids=[f"{'stream' if f else 'resident'}-dk{d}" for f, d in nm.ATTN_CELLS])
def test_attention_clean_emulation_is_accepted_at_every_cell(form, dk, dt):
    """The clean emulation passes select, uniform and graded at N = 77, 130 and 32 in every (form, d_k, dtype) cell; graded really
    exercises rounding; at the power-of-two count the uniform family is exact in fp32 as well."""
    for N in (77, 130, 32):
        res = attn_checks(form, dk, dt, 1, N)
        assert all(v[0] is None for v in res.values()), f"N={N}: {res}"
        nm.assert_rounding_exercised(attn_case("graded", 1, N, dk)[1]["out"], dt, f"graded dk={dk} N={N}")
        print(f"clean attention form={form} dk={dk} N={N} {nm.DT_NAME[dt]} ({nm.attn_den(dk, form, dt)}): err / budget " +
              ", ".join(f"{k} {v[1]:.3f}" for k, v in res.items()))
        assert dt != F32 or N != 32 or res["uniform"][1] == 0.0


@pytest.mark.parametrize("N", [77, 130, 32])
@pytest.mark.parametrize("dk", sorted(set(nm.ATTN_RES_DK + nm.ATTN_STREAM_DK)))
def test_select_construction_holds_for_every_shape(dk, N):
    """attn_select_qkv asserts its own construction (negative integer scores below 2^24, every loser ATTN_UNDERFLOW below its winner in
    fp64, every key index somebody's winner, pi no bijection, distinct V rows, all three types hold every value); here for every
    (d_k, N) of the GPU module, at B = 1 and — the largest d_k of either form — B = 4, and against the fp64 softmax: the expected tensor IS
    the reference to 2^-150."""
    for B in ((1, 4) if dk in (128, 256) and N == 130 else (1,)):
        qkv, want, pi = nm.attn_select_qkv(B, N, dk, 7000 + 10 * dk + N)
        ref = nm.attn_ref64(qkv, B, N, nm.ATTN_HEADS * dk)
        assert float((ref["out"] - want.double()).abs().max()) <= 127.0 * N * 2.0 ** -150
        assert float(ref["dev"].max()) < 1e-9


# defect -> (the family that must reject it, the cells it is planted in: free, xtra, valu with a padded d_k, streaming with a padded d_k)
ATTN_DEFECT_CELLS = [(0, 16), (0, 32), (0, 72), (1, 192)]
ATTN_DEFECT_MUST = {"nomask": ("select", ATTN_DEFECT_CELLS), "vtperm": ("select", ATTN_DEFECT_CELLS), "scale_dkp": ("graded", [(0, 40), (0, 72), (1, 192)]),
                    "l_norescale": ("graded", ATTN_DEFECT_CELLS), "dirswap": ("select", ATTN_DEFECT_CELLS), "headoff": ("select", ATTN_DEFECT_CELLS),
                    "lastq": ("select", ATTN_DEFECT_CELLS)}


@pytest.mark.parametrize("dt", D3, ids=D3_IDS)
@pytest.mark.parametrize("defect", nm.ATTN_DEFECTS)
def test_attention_defects_are_rejected(defect, dt):
    """Every planted defect is rejected by the family built for it, in every denominator form; the wrong scale of a padded head dimension
    exceeds the graded budget by a wide factor (>= 10).  The same defect on the Gaussian data of test_cross_attention goes to
    close(factor=2) for the record."""
    must, cells = ATTN_DEFECT_MUST[defect]
    B, N = 1, 77
    for form, dk in cells:
        res = attn_checks(form, dk, dt, B, N, defect)
        caught = sorted(k for k, v in res.items() if v[0] is not None)
        assert must in caught, f"{defect} form={form} dk={dk}: {must} accepted it ({res})"
        assert defect != "scale_dkp" or res["graded"][1] >= 10.0, f"scale_dkp at dk={dk}: only {res['graded'][1]:.2f} x the budget"
        print(f"{defect} form={form} dk={dk} {nm.DT_NAME[dt]}: rejected by {caught}; err / budget " + ", ".join(f"{k} {v[1]:.3g}" for k, v in res.items()))
        C = nm.ATTN_HEADS * dk
        g = nm.attn_gauss_qkv(B, N, C).to(dt).float()
        got = torch.nan_to_num(nm.emulate_attention(g, B, N, C, nm.ATTN_HEADS, dt, form, defect).float(), nan=0.0)     # (close() ran on zero-filled outputs)
        ref = nm.attn_ref64(g, B, N, C)["out"]
        scale = max(float(ref.abs().max()), 1e-6)
        record(f"attention:{defect}:{'stream' if form else 'resident'}-dk{dk}", dt, float((got.double() - ref).abs().max()) / scale <= 2.0 * OLD_TOL[dt])


@pytest.mark.parametrize("dt", D16, ids=D16_IDS)
@pytest.mark.parametrize("C,heads,B,N", [(64, 4, 4, 64), (128, 4, 3, 77), (128, 2, 3, 77)])
def test_selected_attention_tile_of_the_two_launch_kernel_cases(C, heads, B, N, dt):
    """Test (e) of tests/test_gpu_exact_dmff.py with the select family: the operands build (their construction asserts hold at 2 and 4
    heads and V in [-8, 8]), the emulated attention returns the expected tile bit for bit, a wrong key order in V^T does not, and the
    clean block emulation passes (a) and (b) with that tile in place of att."""
    qkv, att, _ = nm.attn_select_qkv(B, N, C // heads, 300 * C + N, heads=heads, vmax=8)
    nm.assert_same_bits(nm.emulate_attention(qkv, B, N, C, heads, dt, 0), att.to(dt), "select tile")
    assert not nm.same_bits(nm.emulate_attention(qkv, B, N, C, heads, dt, 0, "vtperm"), att.to(dt))
    for kind in ("a", "b"):
        d = (nm.dmff_operands_a if kind == "a" else nm.dmff_operands_b)(C, dt, B * N)
        d["att"] = att
        y, _ = nm.emulate_proj_mlp(d, dt)
        if kind == "a":
            nm.check_proj_mlp_a(y, None, nm.dmff_xatt64(d), dt, "(e select, a)")
        else:
            nm.check_proj_mlp_b(y, None, nm.dmff_ref_b(d, dt), dt, "(e select, b)")


def test_close_verdicts_of_the_attention_defects_are_recorded():
    """Closing: what close(factor=2) accepted among the attention defects above (docs/HISTORY.md section 22)."""
    mine = {k: v for k, v in VERDICTS.items() if k[0].startswith("attention:")}
    if not mine:
        print("run with test_attention_defects_are_rejected (same process): nothing was recorded")
    for k in sorted(mine):
        print(f"close(factor=2) on {k[0]} {k[1]}: {'ACCEPTS' if mine[k] else 'rejects'}")
