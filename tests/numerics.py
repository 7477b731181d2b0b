"""Exact references, error budgets and poisoned buffers for the kernel tests (helpers only, CPU torch; no test lives here).

Three ideas, each closing a hole of a single max-norm tolerance on Gaussian data:

* LATTICE DATA.  x holds integers in [-8, 8], w integers / 2^s, bias / res / pre values on a finer dyadic grid, the alphas are powers
  of two.  Every product and every partial sum is then a dyadic rational of fewer than 2^24 units, so fp32 accumulation is exact in
  ANY order — on the MFMA as on the CPU — and the only inexact steps of a launch are the activation and the rounding(s) to the storage
  type.  Without an activation the expected output is known bit for bit.
* COUNTED BUDGETS.  With an activation the pre-activation is still exact, so the error of an element is the activation's fp32
  evaluation plus the storage rounding.  The budgets below count the roundings of the device expressions (icaf_common.h: silu_f,
  gelu_fast_f, gelu_f) with the accuracy the ISA documents for the hardware transcendentals; nothing is fitted to device output.
* POISON.  Outputs are pre-filled with NaN, every byte around a logical view with a NaN / Inf bit pattern, and compared bitwise
  afterwards: an element that is not written, or a byte written / read outside the view, cannot hide.
"""
import math
import zlib

import torch
import torch.nn.functional as F

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2          # icaf.h
MANT = {F32: 23, BF16: 7, F16: 10}              # stored mantissa bits
EMIN = {F32: -126, BF16: -126, F16: -14}        # exponent of the smallest normal number
U32 = 2.0 ** -24                                # unit roundoff of fp32: one correctly rounded fp32 operation has relative error <= U32
SUB32 = 2.0 ** -149                             # spacing of the fp32 subnormals: the absolute error floor of any fp32 operation
VEC = {F32: 4, BF16: 8, F16: 8}                 # elements per 16-byte vector


# ------------------------------------------------------------------------------------------------------------------------------------
# number formats
# ------------------------------------------------------------------------------------------------------------------------------------
def ulp(ref, dt):
    """Spacing of `dt` in the binade of |ref| (fp64 tensor), subnormal spacing below the smallest normal."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    _, e = torch.frexp(ref.abs())               # |ref| = m * 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, EMIN[dt]), torch.clamp(e - 1, min=EMIN[dt])) - MANT[dt]      # (frexp(0) = (0, 0))
    return torch.ldexp(torch.ones_like(ref), e)


def rne(x64, dt):
    """Round an fp64 tensor to `dt`, to nearest even.  torch converts double -> 16 bit through fp32, so the value must be an fp32
    number already (true for everything on the lattice, and asserted): fp32 -> `dt` is then ONE rounding."""
    x32 = x64.to(F32)
    assert torch.equal(x32.double(), x64), "rne(): the value is not representable in fp32 — the lattice is too fine for this shape"
    return x32.to(dt)


def bits(t):
    """Integer view of a float tensor (bitwise comparisons: NaN == NaN, -0 != +0)."""
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def all_finite_patterns(dt):
    """Every bit pattern of a 16-bit type as a (65536,) tensor, the non-finite ones (Inf, NaN) replaced by 1.0."""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt)
    return torch.where(torch.isfinite(v.float()), v, torch.ones_like(v))


def f32_sweep_grid():
    """fp32 sweep values: every finite bf16 value, every finite fp16 value, and the midpoint of every pair of adjacent bf16 values
    (196,608 values; a midpoint needs one more mantissa bit, so it is an fp32 number)."""
    b = all_finite_patterns(BF16).float()
    h = all_finite_patterns(F16).float()
    mid = (b.double() + 0.5 * ulp(b.double(), BF16) * torch.sign(b.double())).float()
    mid = torch.where(torch.isfinite(mid), mid, b)
    return torch.cat((b, h, mid))


# ------------------------------------------------------------------------------------------------------------------------------------
# lattice data
# ------------------------------------------------------------------------------------------------------------------------------------
# dtype -> (s_w, s_f): w = k / 2^s_w with |k| <= 2^s_w, bias / res / pre = j / 2^s_f.  bf16 keeps 8 significant bits, so eighths are
# fine enough: at K >= 32 the sums need 9+ bits.  fp16 keeps 11 bits and represents almost every such sum, so it gets the finer grids.
GRID = {BF16: (3, 4), F32: (3, 4), F16: (6, 8)}
KMAX = 4608                                       # largest K for which the worst-case sum stays below 2^24 units on the fp16 grid


def lattice(dt, B, H, W, cin, cout, k, Ho, Wo, seed, pre_hw=None):
    """CPU fp32 operands of one conv launch on the lattice of `dt`: dict(x NCHW, w, bias, res NCHW, pre NCHW or None)."""
    sw, sf = GRID[dt]
    K = cin * k * k
    # worst case of |sum| in units of 2^-s_f: K * 8 * 2^s_w (products) * 2^(s_f - s_w), plus bias and pre (<= 2 * 64)
    assert K <= KMAX and K * 8 * 2 ** sf + 128 < 2 ** 24, f"K = {K}: the lattice sums would not be exact in fp32"
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    d = dict(x=ri(-8, 8, (B, cin, H, W)), w=ri(-2 ** sw, 2 ** sw, (cout, cin, k, k)) / 2 ** sw,
             bias=ri(-64, 64, (cout,)) / 2 ** sf, res=ri(-64, 64, (B, cout, Ho, Wo)) / 2 ** sf, pre=None)
    if pre_hw:
        d["pre"] = ri(-64, 64, (B, cout, *pre_hw)) / 2 ** sf
    for name in ("x", "w", "res"):                 # the operands the kernel reads in `dt` must survive the conversion
        assert torch.equal(d[name].to(dt).float(), d[name]), f"lattice {name} is not representable in {dt}"
    return d


def act64(z, act):
    """The activation in fp64, evaluated so that neither tail cancels: SiLU as z / (1 + exp(-z)), GELU as 0.5 z erfc(-z / sqrt 2)."""
    if act == ACT_SILU:
        return z / (1.0 + torch.exp(-z))
    if act == ACT_GELU:
        return 0.5 * z * torch.special.erfc(-z * math.sqrt(0.5))
    return z


def interp64(pre, size, nearest):
    """The `pre` term of icaf_conv_args resized to the output map, fp64 (bilinear align_corners=False, or nearest = floor(dst * in / out))."""
    if pre is None:
        return 0.0
    p = pre.double()
    if not nearest:
        return F.interpolate(p, size=size, mode="bilinear", align_corners=False)
    iy = torch.arange(size[0]) * p.shape[2] // size[0]
    ix = torch.arange(size[1]) * p.shape[3] // size[1]
    return p[:, :, iy][:, :, :, ix]


def ref64(x, w, bias, stride, pad, act, res=None, alpha_acc=1.0, alpha_res=1.0, pre=None, pre_nearest=False):
    """fp64 (pre-activation, output) of one conv launch, NCHW: conv + bias [+ resized pre], activation, alpha_acc * act + alpha_res * res.
    On lattice data the pre-activation is EXACT: it is also computed by fp32 F.conv2d, which must agree bit for bit."""
    z = F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), stride, pad)
    z32 = F.conv2d(x, w, bias, stride, pad)
    assert torch.equal(z32.double(), z), "fp32 and fp64 convolution differ: the data is not on an exact lattice"
    z = z + interp64(pre, z.shape[-2:], pre_nearest)
    assert torch.equal(z.float().double(), z), "the pre-activation is not an fp32 number: the pre term is too fine for this shape"
    out = alpha_acc * act64(z, act)
    if res is not None:
        out = out + alpha_res * res.double()
    return z, out


def expected_exact(z, out_dt, res=None, alpha_acc=1.0, alpha_res=1.0):
    """Bit-exact expected output of a launch WITHOUT activation on lattice data.  The launch rounds twice when a residual is present,
    as the layer-by-layer reference does: the conv output is rounded to the output type (it is a tensor of that type), then the
    residual is added and the sum rounded again (icaf.h, `Rounding`).  Without a residual, or with fp32 output (where nothing on the
    lattice is inexact), this is RNE(alpha_res * res + alpha_acc * z).  `+ 0.0` turns a -0 of the reference into the +0 an
    accumulator that starts at +0 produces."""
    s = rne(alpha_acc * z, out_dt)
    if res is not None:
        s = rne(alpha_res * res.double() + s.double(), out_dt)
    return s + 0.0


def lattice_condition(z, out_dt, alpha_acc=1.0):
    """(inexact share, number of exact ties) of rounding the exact results alpha_acc * z to `out_dt`."""
    e = alpha_acc * z
    r = rne(e, out_dt).double()
    d = (e - r).abs()
    return float((d != 0).double().mean()), int((2.0 * d == ulp(e, out_dt)).sum())


def assert_lattice_condition(z, out_dt, alpha_acc=1.0, what=""):
    """A bit-exact test on a 16-bit type is worth something only if rounding happens: >= 5 % inexact results and at least one tie."""
    share, ties = lattice_condition(z, out_dt, alpha_acc)
    assert share >= 0.05 and ties >= 1, f"{what}: the lattice exercises no rounding in {out_dt}: inexact share {share:.4f}, {ties} ties"
    return share, ties


# ------------------------------------------------------------------------------------------------------------------------------------
# activation budgets: absolute bound on |device fp32 value - act64(v)|, BEFORE the rounding to the storage type
# ------------------------------------------------------------------------------------------------------------------------------------
def silu_budget32(v):
    """silu_f / silu4_f (icaf_common.h):  t = v * c;  e = exp2(t);  d = 1 + e;  r = rcp(d);  o = v * r,  c = fp32(-log2 e).
    With u = 2^-24 and E = exp(-v), first order:
      t   c carries the rounding of the constant (<= u), the product one more: t = t_true (1 + 2u).  An absolute error of t enters e
          relatively, times ln 2:  ln2 * |t_true| * 2u = 2u |v|.
      e   v_exp_f32 is accurate to 1 ulp = 2u (ISA guide)                               e = E (1 + 2u |v| + 2u)
      d   one add (u); the error of e enters with weight E / (1 + E) = sigmoid(-v) <= 1
      r   v_rcp_f32 is accurate to 1 ulp = 2u
      o   one product (u)
    Sum:  (2u |v| + 2u) sigmoid(-v) + u + 2u + u  <=  (6 + 2 |v| sigmoid(-v)) u.  c0 = 7: the six counted units plus one for every
    second-order product (they total < 0.01 u for |v| <= 104, where E stops being finite).
    Floor: fp32 results below 2^-126 are multiples of 2^-149 (SUB32).  For v < -87 the reciprocal itself falls below 2^-126 (d > 2^126): the
    hardware reciprocal returns such results as 0 and, once e overflows (v < -88.73), the product is -0 by construction; the true value there is
    at most |v| e^v <= 88.73 * 2^-126 (v e^v decreases in magnitude beyond), so 89 * 2^-126 = 1.05e-36 bounds the error of that branch."""
    v = v.double()
    ref = act64(v, ACT_SILU).abs()
    rel = (7.0 + 2.0 * v.abs() * torch.sigmoid(-v)) * U32
    rel = torch.where(torch.isfinite(rel), rel, torch.zeros_like(rel))          # (|v| sigmoid(-v) = inf * 0 at the positive end)
    floor = torch.where(v < -87.0, torch.full_like(v, 89.0 * 2.0 ** -126), torch.full_like(v, SUB32))
    return rel * ref + floor


A_S_ERF = 1.5e-7        # |erf(x) - formula 7.1.26| for x >= 0, Abramowitz & Stegun, Handbook of Mathematical Functions, p. 299


def gelu_fast_budget32(v):
    """gelu_fast_f (icaf_common.h), the 16-bit builds:  x = |v| c1;  t = rcp(fma(p, x, 1));  S = Horner(a5..a1; t) * t;
    e = exp2(x * x * c);  erf_abs = fma(-S, e, 1);  o = 0.5 v (1 +- erf_abs).   Write q = S e = 1 - erf_abs, so o = 0.5 v q for v < 0
    and 0.5 v (2 - q) for v > 0, and q <= 2 - q: a RELATIVE error of q is at most the same relative error of o.  Relative units (u = 2^-24):
      x          constant + product                                                        2u
      fma        one rounding, the constant p, and x's 2u, the latter two weighted px / (1 + px) < 1:  <= u + 3u px / (1 + px)
      t          + v_rcp_f32, 1 ulp = 2u: 3u at small x rising to 6u.  S depends on t with logarithmic slope L(t) = t S'(t) / S(t):
                 3.44 at t = 1 (x = 0) falling to 1.8 at x = 3; the product L * err(t) peaks at x -> 0:            <= 11u
      Horner     four fma on partial sums 0.39, 1.03, 0.75, 1.00 (t = 1; smaller elsewhere) relative to S / t = 1:     4u
      S          the product with t                                                                                     u
      a1..a5     each coefficient is an fp32 rounding of the published decimal: sum |a_i| t^i <= 4.5 at t = 1:         5u
      e          v_exp_f32, 1 ulp                                                                                       2u
      o          (1 +- erf_abs) and the product with v (0.5 v is exact)                                                 2u
    c0 = 25.  What is NOT relative to q goes into the absolute term 0.5 |v| (A&S + 2^-23):  the published bound of the formula; the
    rounding of erf_abs to the fp32 grid at 1 (2^-25); and the argument of e, x*x*c with 7u of relative error (x: 2u twice, two products,
    the constant), i.e. 7u x^2 relative in e and 7u x^2 q <= 7u * 0.16 = 1.1u absolute (x^2 erfc(x) <= 0.16) — together below 2^-23.
    In the tail v <= -3.5 this absolute term is many fp16 ulps of the (tiny) result: the fast GELU is an absolute approximation there."""
    v = v.double()
    ref = act64(v, ACT_GELU).abs()
    return 25.0 * U32 * ref + 0.5 * v.abs() * (A_S_ERF + 2.0 ** -23) + SUB32


def gelu_erff_budget32(v):
    """gelu_f (the fp32 build):  o = 0.5 v (1 + erff(v c1)).  Relative: the add (u), the product (u), and erff at the 4 ulp the HIP math
    API documents for it — relative to 1 + erf >= 1 for v >= 0 that is at most 8u erf / (1 + erf) <= 4u; the argument (constant +
    product, 2u) moves erf by at most 2u x erf'(x) <= u.  c0 = 2 + 4 + 1 + 3 for second order and the fp64 reference = 10.  For v < 0 the
    absolute error of erf survives the cancellation in 1 + erf: the same 0.5 |v| (1.5e-7 + 2^-23) term as the 16-bit builds carry."""
    v = v.double()
    ref = act64(v, ACT_GELU).abs()
    return 10.0 * U32 * ref + 0.5 * v.abs() * (A_S_ERF + 2.0 ** -23) + SUB32


def act_budget32(v, act, in_dt):
    """fp32 budget of the activation the conv kernels apply to pre-activation v for a layer whose storage type is `in_dt`."""
    if act == ACT_SILU:
        return silu_budget32(v)
    if act == ACT_GELU:
        return gelu_erff_budget32(v) if in_dt == F32 else gelu_fast_budget32(v)
    return torch.zeros_like(v.double())


def storage_bound(ref, b32, dt):
    """Bound on |RNE_dt(value) - ref| for a value within b32 of ref: half a unit of `dt` where the VALUE lies (it may sit one binade
    above ref) plus b32."""
    return 0.5 * ulp(ref.abs() + b32, dt) + b32


def launch_bound(z, act, in_dt, out_dt, res=None, alpha_acc=1.0, alpha_res=1.0):
    """Per-element bound on |got - ref64 output| of a launch with exact pre-activation z: the activation budget, the rounding of
    alpha_acc * act to the output type (alpha_acc is a power of two) and, with a residual, the fp32 fma and the second rounding."""
    a = alpha_acc * act64(z, act)
    bound = storage_bound(a, alpha_acc * act_budget32(z, act, in_dt), out_dt)
    if res is not None:
        out = a + alpha_res * res.double()
        bound = storage_bound(out, bound + U32 * out.abs() + SUB32, out_dt)
    return bound


def budget_ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound (fp64; inf for a non-finite result)."""
    g = got.double()
    err = (g - ref).abs() / bound
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    return float(err.max())


def assert_budget(got, ref, bound, what="", signed=True):
    """Every element of `got` within `bound` of the fp64 reference — no outlier allowance, no sampling — and finite.  signed: SiLU and GELU
    take the sign of their argument by construction (v times a non-negative factor), so a result on the wrong side of zero is an error
    however small it is.  Returns the largest err / bound."""
    g = got.double()
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} != {tuple(ref.shape)}"
    finite = torch.isfinite(g)
    assert bool(finite.all()), f"{what}: {int((~finite).sum())} non-finite results (first at {_first(~finite)})"
    err = (g - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements over budget; worst at {_first(err / bound == (err / bound).max())}: "
                                 f"got {float(g[bad][0]):.9g} ref {float(ref[bad][0]):.9g} err / budget {float((err / bound).max()):.3g}")
    if signed:
        wrong = ((ref <= 0) & (g > 0)) | ((ref >= 0) & (g < 0))
        assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} results on the wrong side of zero (first at {_first(wrong)})"
    return float((err / bound).max())


def assert_same_bits(got, want, what=""):
    """Bitwise equality of every element, with the coordinates of the first difference."""
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} != {want.dtype} {tuple(want.shape)}"
    ne = bits(got) != bits(want)
    assert not bool(ne.any()), (f"{what}: {int(ne.sum())} of {ne.numel()} elements differ; first at {_first(ne)}: "
                                f"got {float(got[ne][0])!r} want {float(want[ne][0])!r}")


def _first(mask):
    idx = torch.nonzero(mask)
    return tuple(int(i) for i in idx[0]) if len(idx) else None


# ------------------------------------------------------------------------------------------------------------------------------------
# poisoned buffers
# ------------------------------------------------------------------------------------------------------------------------------------
NAN_BITS = {F32: 0x7FC0BEEF, BF16: 0x7FC1, F16: 0x7E01}
INF_BITS = {F32: 0x7F800000, BF16: 0x7F80, F16: 0x7C00}


class Poisoned:
    """An act that is a channel slice [lo, lo + C) of a wider NHWC buffer (leading dims arbitrary: (B, H, W) or (2, B, H, W) for pair acts)
    whose every other byte — and, for outputs, the slice itself — holds a chosen bit pattern."""

    def __init__(self, lead, C, dt, device, fill_bits, content=None, lo=None, hi=None):
        v = VEC[dt]
        lo = v if lo is None else lo                                   # keeps the view 16-byte aligned
        hi = (v + (-(lo + C)) % v) if hi is None else hi               # >= one vector behind it, ld a multiple of the vector
        self.buf = torch.empty((*lead, lo + C + hi), dtype=dt, device=device)
        bits(self.buf).fill_(fill_bits)
        self.lo, self.C = lo, C
        self.view = self.buf[..., lo:lo + C]
        if content is not None:
            self.view.copy_(content)
        self.before = self.buf.clone()

    def outside_intact(self):
        """Every byte outside the logical view still holds what it held after construction."""
        now, was = bits(self.buf).clone(), bits(self.before).clone()
        now[..., self.lo:self.lo + self.C] = 0
        was[..., self.lo:self.lo + self.C] = 0
        return torch.equal(now, was)

    def assert_outside_intact(self, what=""):
        now, was = bits(self.buf), bits(self.before)
        ne = now != was
        ne[..., self.lo:self.lo + self.C] = False
        assert not bool(ne.any()), f"{what}: {int(ne.sum())} elements outside the view [{self.lo}, {self.lo + self.C}) changed; first at {_first(ne)}"


# ------------------------------------------------------------------------------------------------------------------------------------
# torch emulation of one launch (the self-test's stand-in for the device; defects are planted here)
# ------------------------------------------------------------------------------------------------------------------------------------
ERF_COEF = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def _silu32(v):
    e = torch.exp2(v * -1.4426950408889634)
    return v * (1.0 / (1.0 + e))


def _gelu_fast32(v, coef=ERF_COEF):
    a1, a2, a3, a4, a5 = (torch.tensor(c, dtype=F32) for c in coef)
    x = v.abs() * 0.70710678118654752440
    t = 1.0 / (0.3275911 * x + 1.0)
    poly = (((a5 * t + a4) * t + a3) * t + a2) * t + a1
    e = torch.exp2(x * x * -1.4426950408889634)
    erf_abs = 1.0 - poly * t * e
    return 0.5 * v * (1.0 + torch.where(v < 0, -erf_abs, erf_abs))


def truncate(x32, dt):
    """fp32 -> dt by dropping bits (round toward zero): the defect a missing RNE would be."""
    r = x32.to(dt)
    over = r.float().abs() > x32.abs()
    return torch.where(over, (bits(r) - 1).view(dt), r)        # one step towards zero (sign-magnitude bit patterns)


def emulate(d, stride, pad, act, in_dt, out_dt, use_res=False, alpha_acc=1.0, alpha_res=1.0, defect=None, z=None):
    """One conv launch in torch fp32 with the device's expressions and rounding points (NCHW result in out_dt).  d: lattice() operands.
    defect: None | "trunc" | "vector" | "bias" | "erf" | "negzero".  z: pre-activation to use instead of the convolution (sweeps)."""
    if z is None:
        z = F.conv2d(d["x"], d["w"], d["bias"], stride, pad)
        if defect == "vector":      # channels [8, 16) of tap (pad, pad) — the one that reads input pixel (0, 0) — at the corner output pixel (0, 0)
            z = z.clone()
            z[0, :, 0, 0] -= d["w"][:, 8:16, pad, pad] @ d["x"][0, 8:16, 0, 0]
        if defect == "bias":
            z = z.clone()
            z[:, 1] -= d["bias"][1]
    if act == ACT_SILU:
        a = _silu32(z)
        if defect == "negzero":
            tiny = 1e-7 if out_dt == F16 else 1e-40          # (survives the rounding to out_dt as a positive number)
            a = torch.where((a == 0) & torch.signbit(a), torch.full_like(a, tiny), a)
    elif act == ACT_GELU:
        coef = ERF_COEF if defect != "erf" else (ERF_COEF[0], ERF_COEF[1], 1.421513741, ERF_COEF[3], ERF_COEF[4])
        a = torch.erf(z * 0.70710678118654752440).add(1.0).mul(0.5 * z) if in_dt == F32 else _gelu_fast32(z, coef)
    else:
        a = z
    rnd = (lambda t: truncate(t, out_dt)) if defect == "trunc" else (lambda t: t.to(out_dt))
    s = rnd(a * alpha_acc)
    if use_res:
        s = rnd(torch.addcmul(s.float(), d["res"], torch.tensor(alpha_res)))
    return s


# ------------------------------------------------------------------------------------------------------------------------------------
# the layer shapes of tests/test_gpu_exact.py (here, so that the CPU self-test can check the lattice condition for each of them)
# ------------------------------------------------------------------------------------------------------------------------------------
# name: (B, H, W, cin, cout, k, stride, pad, dict(flags)).  flags: acts (default all three), pair (5-D acts, per-stream weights),
# groups2 (explicit group strides, different alphas per group), f32out (fp32 output from the 16-bit types too), extra (launch
# configurations conv_candidates never offers, passed as tile=), only16 (no fp32 run: the shape exists for 16-bit-only kernels)
A3 = (ACT_NONE, ACT_SILU, ACT_GELU)
EXACT_SHAPES = {
    "ragged3x3":   (2, 23, 29, 48, 160, 3, 1, 1, dict(extra=(29, 31, 32, 34))),            # M, N, K ragged; a K slice straddles taps (generic walk)
    "ragged3x3s2": (1, 13, 13, 72, 24, 3, 2, 1, dict(extra=(33,))),                        # stride 2, Cout <= 32: the 256 x 32 tile
    "conv5x5s2":   (1, 9, 7, 32, 32, 5, 2, 2, dict()),                                     # taps leave the image on all four sides by two pixels
    "wide1x1":     (2, 10, 12, 128, 512, 1, 1, 0, dict()),                                 # linear walk; wreg 61-66, stream 51 / 52, 25 / 26 / 28
    "pair3x3c64":  (2, 19, 21, 64, 64, 3, 1, 1, dict(pair=True)),                          # cstream 71, ctile 42 / 43, stream 52; both streams in one launch
    "c128":        (1, 13, 18, 128, 128, 3, 1, 1, dict()),                                 # cwide 81 / 82, ctile 45, wreg 61 / 66
    "c64s2":       (1, 21, 27, 64, 128, 3, 2, 1, dict()),                                  # cwide 83 / 85
    "c128s2":      (1, 17, 15, 128, 128, 3, 2, 1, dict()),                                 # cwide 84
    "c16":         (1, 15, 22, 16, 32, 3, 1, 1, dict()),                                   # ctile 41: 32 bytes per pixel, two taps per K slice
    "c32s2":       (1, 21, 19, 32, 64, 3, 2, 1, dict()),                                   # ctile 44
    "detect":      (2, 9, 11, 64, 18, 1, 1, 0, dict(f32out=True, acts=(ACT_NONE, ACT_GELU))),   # fp32 output from 16-bit inputs, Cout not a vector multiple
    "groups2":     (75, 2, 2, 64, 192, 1, 1, 0, dict(groups2=True)),                       # two problems in gridDim.z with their own weights and alphas
    # full-size maps: the persistent kernels walk several tiles per workgroup and the grids exceed one wave of workgroups — where
    # docs/HISTORY.md section 10 found wrong elements that every small shape passed.  16-bit types (the kernels these shapes exist for)
    "big1x1c64":   (16, 80, 80, 64, 64, 1, 1, 0, dict(only16=True, acts=(ACT_NONE, ACT_SILU))),            # 800 pixel tiles: stream 52
    "big3x3c64":   (4, 80, 80, 64, 64, 3, 1, 1, dict(only16=True, pair=True, acts=(ACT_SILU,))),           # cstream 71, ctile 42 / 43
    "bigc128":     (32, 40, 40, 128, 128, 3, 1, 1, dict(only16=True, acts=(ACT_SILU,))),                   # cwide 81 / 82, ctile 45
    "big1x1c256":  (8, 40, 40, 256, 512, 1, 1, 0, dict(only16=True, acts=(ACT_NONE, ACT_SILU))),           # wreg 61 - 66, stream 51 / 52, 26
}
ALPHA_ACC, ALPHA_RES = 0.5, 2.0                   # powers of two: scaling stays exact
ALPHAS_G2 = ((0.5, 2.0), (2.0, 0.5))              # (alpha_acc, alpha_res) per group of the groups2 shape
PRE_SHAPES = {
    # name: (B, H, W, cin, cout, (pre_h, pre_w), nearest).  Bilinear at power-of-two factors: the interpolation weights are k / 8 or k / 4 — dyadic
    "pre_bilinear_x4": (2, 16, 24, 64, 200, (4, 6), False),
    "pre_bilinear_x2": (1, 20, 12, 128, 128, (10, 6), False),
    "pre_nearest_x3":  (2, 9, 15, 64, 136, (3, 5), True),
    "pre_nearest_odd": (1, 14, 10, 128, 64, (5, 3), True),        # 14 / 5, 10 / 3: not integer factors
}


def out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def shape_seed(name, dt, g=0):
    """Seed of the lattice operands of (shape, dtype, group): a function of the NAME, so adding a shape leaves the others' data alone."""
    return zlib.crc32(name.encode()) % 100000 * 100 + 10 * [F32, BF16, F16].index(dt) + g
