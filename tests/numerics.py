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


# ====================================================================================================================================
# pooling, resize and merge kernels (dmff.hip: pool_tokens, upsample_merge; pool.hip: upsample_nearest, copy, axpby, staging).
# Everything below is NHWC on the CPU: features (B, H, W, C), tokens (B, th * tw, C), pairs with the modality in front.
# ====================================================================================================================================
SECOND = 1.0 + 2.0 ** -10        # every budget below is first order in u = 2^-24; the products of two roundings it drops are < 2^-20 of it
W_DYADIC, W_REAL = (0.5, 0.25), (0.4, 0.7)           # LearnableWeights pairs: exact in every type / what a checkpoint holds
GRID_MAX = 4096                                      # grid_for(): at most this many workgroups of 256 threads ...
STRIDE_ITEMS = GRID_MAX * 256                        # ... so vector items from 2^20 on belong to the second pass of the grid-stride loop
FEA_GRID = {BF16: 6, F32: 6, F16: 9}                 # residual features of the merge: j / 2^s with |j| <= 4 * 2^s — representable, and the
                                                     # sum with an interpolated integer needs more bits than the type keeps


def f32w(w):
    """The float the library receives for a Python weight, as an fp64 number."""
    return float(torch.tensor(w, dtype=F32))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(shape, seed, scale=1.0):
    """The Gaussian inputs of tests/test_gpu_kernels.py (same generator), for the self-test's record of what close() accepts on them."""
    import numpy as np
    return torch.from_numpy(np.random.default_rng(seed).normal(0, scale, shape).astype(np.float32))


def pool_lattice(B, H, W, C, N, seed):
    """Lattice operands of one pooling launch for ONE modality: x integers in [-8, 8] — channels c % 4 == 1 hold ONLY negative values
    (-8 .. -1), so a maximum that starts at 0 instead of -inf shows in every window — and pos = j / 1024, |j| <= 4096 (fp32, dyadic: ten fractional
    bits, more than either 16-bit type keeps beside an integer part, so the stored token is a rounded one also where the arithmetic is exact)."""
    g = _gen(seed)
    x = torch.randint(-8, 9, (B, H, W, C), generator=g).float()
    neg = torch.randint(-8, 0, (B, H, W, C), generator=g).float()
    x[..., 1::4] = neg[..., 1::4]
    pos = torch.randint(-4096, 4097, (N, C), generator=g).float() / 1024.0
    return x, pos


def _edges(n, t, k, s, R=12):
    """Rows (or columns) of an n-long axis on both sides of every window boundary of the first, second and last token row (t rows,
    window k, stride s), the two ends of the axis, and — for a window taller than the R rows a workgroup keeps in flight — both sides
    of every R-chunk boundary of the first and the last window.  The rows two consecutive token rows share ([s, k)) are among them."""
    out = {0, n - 1}
    for i in {0, min(1, t - 1), t - 1}:
        a, b = i * s, i * s + k - 1
        out |= {a - 1, a, b, b + 1}
        for c in range(R, k, R):
            out |= {a + c - 1, a + c}
    return sorted(v for v in out if 0 <= v < n)


def probe_pixels(H, W, th, tw, kh, kw, sh, sw):
    """The pixels a membership probe must sit on: the four corners, and every interesting row paired with every interesting column at
    least once (rows and columns cycled against each other)."""
    ry, cx = _edges(H, th, kh, sh), _edges(W, tw, kw, sw)
    px = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    px += [(ry[i % len(ry)], cx[i % len(cx)]) for i in range(max(len(ry), len(cx)))]
    px += [(ry[i % len(ry)], cx[(i + len(cx) // 2) % len(cx)]) for i in range(max(len(ry), len(cx)))]      # a second column per row
    return list(dict.fromkeys(px)), ry, cx


def pool_probes(B, H, W, C, geom, g):
    """Membership probes of modality g: channel c of image b is zero except at ONE pixel p(b, c), which holds a power of two
    (2^-2 .. 2^2).  The first len(probe_pixels) slots (b, c) take the listed pixels (rotated by modality), the others seeded ones.
    With w = (0, 1), pos = 0 a token is that power of two if its window covers the pixel and +0 otherwise — in every type."""
    px, ry, cx = probe_pixels(H, W, *geom)
    assert B * C >= len(px), f"{len(px)} probe pixels need more than {B * C} (image, channel) slots"
    gen = _gen(9000 + 10 * H + W + g)
    x = torch.zeros((B, H, W, C))
    where = []
    for i in range(B * C):
        b, c = divmod(i, C)
        y, xx = px[(i + 7 * g) % len(px)] if i < len(px) else (int(torch.randint(0, H, (1,), generator=gen)), int(torch.randint(0, W, (1,), generator=gen)))
        x[b, y, xx, c] = 2.0 ** (i % 5 - 2)
        where.append((y, xx))
    assert set(px) <= set(where)
    return x


def windows(x, geom):
    """(B, th, tw, C, kh, kw) view of the pooling windows of x (B, H, W, C)."""
    th, tw, kh, kw, sh, sw = geom
    assert (th - 1) * sh + kh <= x.shape[1] and (tw - 1) * sw + kw <= x.shape[2]
    return x[:, :(th - 1) * sh + kh, :(tw - 1) * sw + kw].unfold(1, kh, sh).unfold(2, kw, sw)


def pool_stats64(x, geom):
    """fp64 (mean, max) over the explicit windows of x (B, H, W, C), each (B, th * tw, C)."""
    win = windows(x.double(), geom)
    B, th, tw, C = win.shape[:4]
    avg = win.sum((-2, -1)) / float(geom[2] * geom[3])
    return avg.reshape(B, th * tw, C), win.amax((-2, -1)).reshape(B, th * tw, C)


def pool64(x, geom, w, pos, stats=None):
    """fp64 reference of pool_tokens for one modality: (avg, max, w1 * avg + w2 * max + pos), each (B, th * tw, C); w as the library
    receives it (fp32 values), windows explicit."""
    avg, mx = stats if stats is not None else pool_stats64(x, geom)
    return avg, mx, f32w(w[0]) * avg + f32w(w[1]) * mx + pos.double()


def is_f32(x64):
    return bool(torch.equal(x64.float().double(), x64))


def pool_is_exact(avg, mx, w, pos, area):
    """True when every step of the device expression (sum * inv_area) * w1 + mx * w2 + pos is exact in fp32 on this data, so that the
    expected tokens are RNE(reference) bit for bit: the window sums are integers / dyadic (exact in any order), 1 / area is exact for a
    power-of-two area or irrelevant when w1 = 0 (finite * 0 = 0), and each product and partial sum is an fp32 number."""
    w1, w2 = f32w(w[0]), f32w(w[1])
    if w1 != 0.0 and area & (area - 1):
        return False
    steps = ([avg, w1 * avg] if w1 != 0.0 else []) + [w2 * mx, w1 * avg + w2 * mx, w1 * avg + w2 * mx + pos.double()]
    return all(is_f32(s) for s in steps)


def pool_budget32(avg, mx, w, ref):
    """fp32 budget of pool_tokens' o = (sum * inv_area) * w1 + mx * w2 + pos on lattice data (the window sum is exact), u = 2^-24:
      inv_area = 1.0f / area        one rounding                                 u |w1 avg|
      sum * inv_area                one rounding                                 u |w1 avg|
      (..) * w1                     one rounding                                 u |w1 avg|
      mx * w2                       one rounding (mx itself is an input: exact)  u |w2 mx|
      (..) + (..)                   one rounding of the partial sum              u |w1 avg + w2 mx|
      (..) + pos                    one rounding of the result                   u |ref|
    A contraction to fma removes the rounding of the product it absorbs and adds none, so the count holds for either choice."""
    w1, w2 = f32w(w[0]), f32w(w[1])
    a, m = (w1 * avg).abs(), (w2 * mx).abs()
    return U32 * (3.0 * a + m + (w1 * avg + w2 * mx).abs() + ref.abs()) * SECOND + SUB32


def _axis64(n_out, n_in):
    """fp64 source coordinate of align_corners=False resizing along one axis: (unclamped f, i0, i1, fraction)."""
    fu = (torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5
    f = fu.clamp(min=0.0)
    i0 = f.floor().long().clamp(max=n_in - 1)
    return fu, i0, (i0 + 1).clamp(max=n_in - 1), f - i0


def merge64(tok, fea, dt, need_bound=True):
    """fp64 reference and per-element bound of upsample_merge.  tok (2, B, th, tw, C), fea (2, B, H, W, C) -> ref, bound (B, H, W, 2C):
    out[..., g*C + c] = bilinear(tok[g]) + fea[g], align_corners=False with clamped neighbours.

    Budget (device expression: top = a00 (1 - lx) + a01 lx, bot likewise, o = (top (1 - ly) + bot ly) + r; u = 2^-24; M = the largest
    magnitude among the four neighbours):
      1 - lx                        one rounding, times |a00|                              <= u M
      the two products and the sum  u (|a00| (1 - lx) + |a01| lx) + u |top|                <= 2u M        -> top, bot carry 3u M each
      the vertical lerp             the same three terms on top / bot, plus their own errors weighted (1 - ly) + ly = 1:  6u M in all
      + r                           one rounding of the result                             u |ref|
      coordinates                   fy = fl(fl((h + 0.5) fl(th / H)) - 0.5): the ratio and the product carry u each relative to
                                    (h + 0.5) th / H = f + 0.5, the subtraction u |f|:  |fy - f| <= dy = 3u (|f| + 1); fx likewise.  ly = fy - y0 is
                                    exact (fy < 2^24 and y0 = floor fy).  Bilinear interpolation is continuous and piecewise linear in (fy, fx),
                                    so the device value differs from the one at the true coordinate by at most slope * d, ALSO when fy lands on the
                                    other side of an integer (where the slope is that of the adjacent cell): slope_y = the largest
                                    |difference of vertically adjacent, horizontally interpolated rows| among rows y0 - 1 .. y1 + 1, slope_x likewise;
                                    the mixed term is bounded by 4 M dy dx.
    At dyadic ratios (identity, x2, x4, th = 1 with H a power of two) fy and every weight are exact and tests compare bits instead."""
    _, B, th, tw, C = tok.shape
    H, W = fea.shape[2], fea.shape[3]
    T, Fe = tok.double(), fea.double()
    fyu, y0, y1, ly = _axis64(H, th)
    fxu, x0, x1, lx = _axis64(W, tw)
    ly_, lx_ = ly.view(1, 1, H, 1, 1), lx.view(1, 1, 1, W, 1)
    at = lambda ys, xs: T[:, :, ys][:, :, :, xs]                                   # (2, B, H, W, C)
    hrow = lambda ys: at(ys, x0) * (1 - lx_) + at(ys, x1) * lx_                    # row ys interpolated horizontally
    vcol = lambda xs: at(y0, xs) * (1 - ly_) + at(y1, xs) * ly_
    v0, v1 = hrow(y0), hrow(y1)
    interp = v0 * (1 - ly_) + v1 * ly_
    ref = interp + Fe
    if not need_bound:                                                             # (exact-bits cases of tens of MB)
        return torch.cat((ref[0], ref[1]), -1), None
    ym, yp, xm, xp = (y0 - 1).clamp(min=0), (y1 + 1).clamp(max=th - 1), (x0 - 1).clamp(min=0), (x1 + 1).clamp(max=tw - 1)
    slope_y = torch.stack(((v1 - v0).abs(), (v0 - hrow(ym)).abs(), (hrow(yp) - v1).abs())).amax(0)
    u0, u1 = vcol(x0), vcol(x1)
    slope_x = torch.stack(((u1 - u0).abs(), (u0 - vcol(xm)).abs(), (vcol(xp) - u1).abs())).amax(0)
    M = torch.stack((at(y0, x0).abs(), at(y0, x1).abs(), at(y1, x0).abs(), at(y1, x1).abs())).amax(0)
    dy = (3.0 * U32 * (fyu.abs() + 1.0)).view(1, 1, H, 1, 1)
    dx = (3.0 * U32 * (fxu.abs() + 1.0)).view(1, 1, 1, W, 1)
    b32 = (U32 * (6.0 * M + ref.abs()) + slope_y * dy + slope_x * dx + 4.0 * M * dy * dx) * SECOND + SUB32
    cat = lambda t: torch.cat((t[0], t[1]), -1)
    ref, b32 = cat(ref), cat(b32)
    return ref, storage_bound(ref, b32, dt)


def merge_lattice(dt, B, H, W, C, th, tw, seed):
    """Lattice operands of one merge launch: tokens integers in [-8, 8] (2, B, th, tw, C), features j / 2^s on FEA_GRID (2, B, H, W, C)."""
    g = _gen(seed)
    s = FEA_GRID[dt]
    tok = torch.randint(-8, 9, (2, B, th, tw, C), generator=g).float()
    fea = torch.randint(-4 * 2 ** s, 4 * 2 ** s, (2, B, H, W, C), generator=g).float() / 2 ** s
    assert torch.equal(fea.to(dt).float(), fea) and torch.equal(tok.to(dt).float(), tok)
    return tok, fea


def nearest64(x, scale):
    """nn.Upsample(scale, 'nearest') of x (B, H, W, C): out[ho, wo] = x[ho // scale, wo // scale]."""
    B, H, W, C = x.shape
    return x[:, torch.arange(H * scale) // scale][:, :, torch.arange(W * scale) // scale]


def axpby_lattice(dt, shape, seed):
    """Two integer operands for y = 128 x0 - 127 x1: |x| <= 8 (fp16: <= 64, so that the sums need more than its 11 bits).  Every product
    and sum is an integer below 2^24: exact in fp32, so the stored bits are RNE of the true value."""
    g, hi = _gen(seed), 64 if dt == F16 else 8
    return tuple(torch.randint(-hi, hi + 1, shape, generator=g).float() for _ in range(2))


def axpby64(x0, x1, a, b, dt):
    """fp64 reference and bound of y = x0 * a + x1 * b (fp32 a, b): two products and one sum, u (|a x0| + |b x1| + |ref|); an fma
    drops one of the three roundings."""
    a, b = f32w(a), f32w(b)
    p0, p1 = a * x0.double(), b * x1.double()
    ref = p0 + p1
    return ref, storage_bound(ref, U32 * (p0.abs() + p1.abs() + ref.abs()) * SECOND + SUB32, dt)


def stage64(img, mode, cpad):
    """The two staging layouts of an NCHW image batch (B, C, H, W) -> (B, H', W', cpad), fp64, channel padding zero: mode 0 = NHWC,
    mode 1 = space-to-depth: channel sub * C + c with sub = 2 dy + dx taken from pixel (2 ho + dy, 2 wo + dx)."""
    x = img.double()
    B, C, H, W = x.shape
    if mode == 1:
        x = torch.cat([x[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)], 1)
    x = x.permute(0, 2, 3, 1)
    out = torch.zeros((*x.shape[:3], cpad), dtype=torch.float64)
    out[..., :x.shape[3]] = x
    return out


def u8_expected(dt):
    """Expected staged value of every uint8 level, in `dt`: RNE_dt of the fp32 quotient v / 255 (a true division, correctly rounded —
    the fp64 quotient rounded to fp32 is asserted to be the same number, so there is no double-rounding case among the 256)."""
    v = torch.arange(256, dtype=F32)
    q32 = v / 255.0
    assert torch.equal((v.double() / 255.0).float(), q32)
    return q32.to(dt)


def inexact_share(ref, dt):
    """Share of the fp64 results that `dt` cannot represent (0 for fp32 by convention: budgets there are about the arithmetic)."""
    if dt == F32:
        return 0.0
    r = ref.float().to(dt).double()
    return float((r != ref).double().mean())


def assert_rounding_exercised(ref, dt, what, least=0.05):
    """A 16-bit check is worth something only if rounding happens: at least `least` of the results are not representable."""
    share = inexact_share(ref, dt)
    print(f"{what} {dt}: not representable {share:.3f}")
    assert dt == F32 or share >= least, f"{what}: only {share:.4f} of the results need rounding in {dt}"
    return share


def check_pool(got, avg, mx, ref, w, pos, geom, dt, what):
    """The check of one modality's tokens: the expected bits where every device step is exact (pool_is_exact), the counted budget
    otherwise.  Returns the largest err / bound (0 stands for "bit-identical")."""
    if pool_is_exact(avg, mx, w, pos, geom[2] * geom[3]):
        assert_same_bits(got, rne(ref, dt) + 0.0, what)
        return 0.0
    return assert_budget(got, ref, storage_bound(ref, pool_budget32(avg, mx, w, ref), dt), what, signed=False)


def check_merge(got, ref, bound, exact, dt, what):
    if exact:
        assert_same_bits(got, rne(ref, dt) + 0.0, what)
        return 0.0
    return assert_budget(got, ref, bound, what, signed=False)


class PoisonedFlat:
    """A contiguous tensor of `shape` in the middle of a flat buffer whose every other element holds `fill_bits` (operands without a
    pixel stride: images, staged outputs, token arrays).  content None: the tensor itself holds the pattern too (an output)."""

    def __init__(self, shape, dt, device, fill_bits, content=None, guard=64):
        n = math.prod(shape)
        self.buf = torch.empty((n + 2 * guard,), dtype=dt, device=device)
        if dt == torch.uint8:
            self.buf.fill_(fill_bits)
        else:
            bits(self.buf).fill_(fill_bits)
        self.g, self.n = guard, n
        self.view = self.buf[guard:guard + n].view(shape)
        if content is not None:
            self.view.copy_(content)
        self.before = self.buf.clone()

    def assert_outside_intact(self, what=""):
        raw = (lambda t: t) if self.buf.dtype == torch.uint8 else bits
        now, was = raw(self.buf), raw(self.before)
        ne = now != was
        ne[self.g:self.g + self.n] = False
        assert not bool(ne.any()), f"{what}: {int(ne.sum())} elements around the tensor changed; first at flat index {_first(ne)}"


# ---- torch emulations (fp32 arithmetic in the device's order, then RNE to storage); defects are planted here --------------------------
def _store(x32, dt, defect):
    return truncate(x32, dt) if defect == "trunc" and dt != F32 else x32.to(dt)


def emulate_pool(x, geom, w, pos, dt, defect=None):
    """pool_tokens for one modality.  x (B, H, W, C) fp32 holding `dt` values -> (B, th * tw, C) in dt.  defect: None | "lastcol" (the last
    token column's window starts one pixel early) | "row12" (input row 12 of the window dropped) | "duprow" (the window's last row — the
    clamped duplicate load — added twice) | "max0" (maximum starts at 0) | "short" (last token row of an odd th unwritten: NaN) |
    "pos_nb" (pos of the next token) | "trunc"."""
    th, tw, kh, kw, sh, sw = geom
    win = windows(x, geom)
    if defect == "lastcol":
        win = win.clone()
        c0 = (tw - 1) * sw - 1
        win[:, :, tw - 1] = windows(x[:, :, c0:c0 + kw], (th, 1, kh, kw, sh, sw))[:, :, 0]
    rows = [r for r in range(kh) if not (defect == "row12" and r == 12)]
    B, C = x.shape[0], x.shape[3]
    s = win[..., rows, :].sum((-2, -1))
    m = win[..., rows, :].amax((-2, -1))
    if defect == "duprow":
        s = s + win[..., kh - 1, :].sum(-1)
    if defect == "max0":
        m = m.clamp(min=0.0)
    p = pos.roll(-1, 0) if defect == "pos_nb" else pos
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(kh * kw), dtype=F32)
    o = (s.reshape(B, th * tw, C) * inv) * torch.tensor(w[0], dtype=F32) + m.reshape(B, th * tw, C) * torch.tensor(w[1], dtype=F32) + p
    out = _store(o, dt, defect)
    if defect == "short":
        assert th % 2 == 1
        out.view(B, th, tw, C)[:, th - 1] = float("nan")
    return out


def emulate_merge(tok, fea, dt, defect=None):
    """upsample_merge: tok (2, B, th, tw, C), fea (2, B, H, W, C), fp32 holding `dt` values -> (B, H, W, 2C) in dt.  defect: None | "swap"
    (each modality interpolates the OTHER one's tokens) | "align" (half-pixel offset dropped: align_corners behaviour) | "noclamp" (the right
    neighbour of the last column is the next token in memory) | "trunc"."""
    _, B, th, tw, C = tok.shape
    H, W = fea.shape[2], fea.shape[3]
    f32 = lambda v: torch.tensor(float(v), dtype=F32)

    def axis(n_out, n_in):
        if defect == "align":
            f = torch.arange(n_out, dtype=F32) * (f32(n_in - 1) / f32(max(n_out - 1, 1)))
        else:
            f = (torch.arange(n_out, dtype=F32) + 0.5) * (f32(n_in) / f32(n_out)) - 0.5
        f = f.clamp(min=0.0)
        i0 = f.to(torch.int64).clamp(max=n_in - 1)
        return i0, (i0 + 1).clamp(max=n_in - 1), f - i0.float()

    y0, y1, ly = axis(H, th)
    x0, x1, lx = axis(W, tw)
    T = tok.flip(0) if defect == "swap" else tok
    flat = T.reshape(2, B * th * tw, C)
    last = B * th * tw - 1

    def at(ys, xs, right):
        n = ys.view(H, 1) * tw + (x0 + 1 if (right and defect == "noclamp") else xs).view(1, W)        # token index inside the image
        idx = (torch.arange(B).view(B, 1, 1) * (th * tw) + n.view(1, H, W)).clamp(max=last)
        return flat[:, idx]                                                                          # (2, B, H, W, C)

    lx_, ly_ = lx.view(1, 1, 1, W, 1), ly.view(1, 1, H, 1, 1)
    top = at(y0, x0, False) * (1.0 - lx_) + at(y0, x1, True) * lx_
    bot = at(y1, x0, False) * (1.0 - lx_) + at(y1, x1, True) * lx_
    o = (top * (1.0 - ly_) + bot * ly_) + fea
    return _store(torch.cat((o[0], o[1]), -1), dt, defect)


def emulate_nearest(x, scale, defect=None):
    """upsample_nearest; defect "ceil": source index ceil(ho / scale) instead of floor."""
    if defect != "ceil":
        return nearest64(x, scale)
    B, H, W, C = x.shape
    iy = (-(-torch.arange(H * scale) // scale)).clamp(max=H - 1)
    ix = (-(-torch.arange(W * scale) // scale)).clamp(max=W - 1)
    return x[:, iy][:, :, ix]


def emulate_axpby(x0, x1, a, b, dt, defect=None):
    return _store(x0 * torch.tensor(a, dtype=F32) + x1 * torch.tensor(b, dtype=F32), dt, defect)


def first_pass_only(out, prefill, dt):
    """The defect of a grid-stride loop that never takes its second step: vector items from STRIDE_ITEMS on keep the prefill."""
    flat = out.reshape(-1, VEC[dt]).clone()
    assert flat.shape[0] > STRIDE_ITEMS, "the case has no second pass"
    flat[STRIDE_ITEMS:] = prefill
    return flat.reshape(out.shape)


# ---- geometries of tests/test_gpu_exact_pool.py (here, so that the CPU self-test can check them) ---------------------------------------
# name: (B, H, W, C, (th, tw, kh, kw, sh, sw), expected {dtype: (kernel, R, TR)}, flags).  Grids: rows kernel 2 * B * ceil(th / TR) workgroups.
ELEM, ROWS = 0, 1
_ALL = lambda k, r, t: {F32: (k, r, t), BF16: (k, r, t), F16: (k, r, t)}
POOL_GEOMS = {
    "r4tr1":     (1, 9, 11, 32, (7, 9, 3, 3, 1, 1), _ALL(ROWS, 4, 1), {}),                  # kh 3, sh 1; 14 workgroups (not a multiple of 8)
    "r4tr2":     (16, 18, 12, 32, (16, 10, 3, 3, 1, 1), _ALL(ROWS, 4, 2), {}),              # the same window, 2 * 16 * 8 = 256 workgroups
    "r8tr1":     (1, 11, 13, 32, (4, 5, 5, 5, 2, 2), _ALL(ROWS, 8, 1), {}),                 # kh 5, sh 2; 8 workgroups
    "r8tr2":     (16, 35, 13, 32, (16, 5, 5, 5, 2, 2), _ALL(ROWS, 8, 2), {}),
    "r12tr2":    (16, 40, 40, 32, (16, 16, 10, 10, 2, 2), _ALL(ROWS, 12, 2), {}),           # the default workload's P4 window
    "r12tr1":    (1, 40, 40, 32, (16, 16, 10, 10, 2, 2), _ALL(ROWS, 12, 1), {}),
    "chunks2":   (1, 31, 20, 32, (16, 16, 16, 5, 1, 1), _ALL(ROWS, 12, 1), {}),             # window taller than R: two chunks, clamped duplicates
    "chunks3":   (1, 27, 10, 32, (3, 4, 25, 4, 1, 2), _ALL(ROWS, 12, 1), {}),               # kh 25: three chunks, the last holds one row; 6 workgroups
    "horiz":     (1, 12, 14, 32, (4, 5, 3, 6, 3, 2), _ALL(ROWS, 4, 1), {}),                 # kh == sh, kw > sw: only the columns overlap
    "oddth":     (32, 30, 33, 32, (7, 9, 6, 9, 4, 3), _ALL(ROWS, 12, 2), {}),               # TR 2 with th = 7: the last block of an image is short
    "wrap":      (1, 8, 40, 256, (3, 19, 4, 4, 2, 2), _ALL(ROWS, 4, 1), {}),                # W * nv = 1280 (16 bit) / 2560 items: the item loop wraps
    "hphase":    (16, 18, 70, 64, (16, 68, 3, 3, 1, 1), _ALL(ROWS, 4, 2), {}),              # 2 * 68 * nv = 1088 / 2176 outputs in the horizontal phase
    "f32edge":   (1, 6, 40, 512, (3, 20, 4, 2, 1, 2), _ALL(ROWS, 4, 1), {}),                # fp32: one token row needs 163,840 bytes, the <= boundary
    "f32over":   (1, 6, 41, 512, (3, 20, 4, 3, 1, 2), {F32: (ELEM, 0, 0), BF16: (ROWS, 4, 1), F16: (ROWS, 4, 1)}, {}),      # one more column: fp32 falls to the element kernel, windows overlapping
    "e4x4":      (2, 16, 20, 32, (4, 5, 4, 4, 4, 4), _ALL(ELEM, 0, 0), dict(idx64=True)),   # non-overlapping 4 x 4
    "ekw3":      (1, 9, 12, 32, (3, 4, 3, 3, 3, 3), _ALL(ELEM, 0, 0), dict(idx64=True)),    # kw 3: the four-wide load batch has a tail of three
    "ekw6":      (1, 8, 19, 64, (4, 3, 2, 6, 2, 6), _ALL(ELEM, 0, 0), {}),                  # kw 6: one full batch and a tail of two
    "e1x1":      (2, 5, 7, 32, (5, 7, 1, 1, 1, 1), _ALL(ELEM, 0, 0), dict(idx64=True)),     # identity
    "ebig":      (11, 80, 80, 128, (80, 40, 1, 2, 1, 2), _ALL(ELEM, 0, 0), dict(big=True)), # 2 * 11 * 3200 * nv = 1,126,400 (16 bit) items > 2^20: second pass
}
# readback only: 2 * B * ceil(th / 2) on both sides of the 256 workgroups that two token rows per workgroup must leave
TR_THRESHOLD = [((16, 18, 12, 32, (16, 10, 3, 3, 1, 1)), 2), ((128, 3, 12, 32, (1, 10, 3, 3, 1, 1)), 2), ((127, 4, 12, 32, (2, 10, 3, 3, 1, 1)), 1),
                ((127, 3, 12, 32, (1, 10, 3, 3, 1, 1)), 1)]

# merge geometries: name -> (B, H, W, C, th, tw, exact bits expected)
MERGE_GEOMS = {
    "identity":  (2, 10, 10, 32, 10, 10, True),
    "x2":        (2, 14, 10, 32, 7, 5, True),
    "x4":        (1, 12, 20, 32, 3, 5, True),
    "th1":       (1, 4, 10, 32, 1, 5, True),        # both vertical neighbours clamped
    "tw1":       (1, 12, 8, 32, 3, 1, True),
    "th1tw1":    (2, 4, 8, 32, 1, 1, True),
    "16to40":    (1, 40, 40, 32, 16, 16, False),
    "20to68x84": (1, 68, 84, 32, 20, 20, False),
    "7x9to30x33": (1, 30, 33, 32, 7, 9, False),
    "big":       (6, 80, 80, 128, 20, 20, True),    # 6 * 6400 * 2 * nv = 1,228,800 (16 bit) vectors > 2^20, 20 MB of output; x4: exact bits
}



# ====================================================================================================================================
# DMFF block kernels (dmff_wide.hip: ln_qkv, proj_mlp, proj_mlp_split + reduce; dmff_fused.hip: ln_qkv, attn_mlp) — the builders,
# references and the torch emulation behind tests/test_gpu_exact_dmff.py.  Tokens are (2, rows, C) with the modality in front.
#
# Exactness through the block comes from three constructions:
#   1. rows x[r, c] = m_r +- s with exactly C / 2 channels on either side and eps = 1 - s^2: mean m_r, q / C + eps = 1, rstd = 1 — every
#      step exact in fp32 in ANY summation order (all partial sums are multiples of a power of two far below 2^24 of them);
#   2. a zeroed GEMM isolates the others (W2 = 0: the launch returns x_att; W_o = 0: the MLP sees the rows of 1.);
#   3. a sparse W2 (32 non-zeros per output channel, one or more in every hidden chunk) keeps the fp32 accumulation error of the fc2 sum,
#      whose operands are NOT on a lattice after GELU, at (nnz - 1) u sum |w h|.
# ====================================================================================================================================
LN_EPS_EXACT = 0.75                                  # 1 - s^2 for deviations of s = 0.5
DMFF_ROWS = (64, 33, 154, 321)                       # one tile; one row in the second 32-row half; a last tile of 26 rows (second half empty);
DMFF_ROWS_MAX = 321                                  # six tiles: a second group of eight workgroups, one tile per eight under ksplit = 4
W2_NNZ = 32
# (C, dtype, ksplit, r32): every build WIDE_ROWS of dmff_wide.hip holds for the out-projection + MLP launch and its reduce
DMFF_CELLS = ([(128, dt, 1, False) for dt in (BF16, F16, F32)] + [(C, dt, 1, False) for C in (256, 512) for dt in (BF16, F16)] +
              [(C, dt, 1, True) for C in (128, 256) for dt in (BF16, F16)] +
              [(C, dt, ks, False) for C in (256, 512) for dt in (BF16, F16) for ks in (2, 4)] +
              [(C, dt, 2, True) for C in (256, 512) for dt in (BF16, F16)])
DT_NAME = {F32: "f32", BF16: "bf16", F16: "f16"}


def cell_id(cell):
    C, dt, ks, r32 = cell
    return f"C{C}-{DT_NAME[dt]}-ks{ks}-{'r32' if r32 else 'r16'}"


def wide_pass(C):
    """Output channels per pass of the dmff_wide build for width C (WG4 / WG8) — also the width of a hidden chunk."""
    return 128 if C == 128 else 256


def rne64(x64, dt):
    """fp64 -> `dt` -> fp64 in ONE rounding to nearest even, for values that are not fp32 numbers (rne() asserts they are)."""
    if dt == F32:
        return x64.float().double()
    u = ulp(x64, dt)
    return torch.round(x64 / u) * u


def fma32(a, b, c):
    """fp32 fma(a, b, c) for a Python float a and fp32 tensors b, c: the product is exact in fp64, the sum rounds once more only at the
    53rd bit."""
    return (f32w(a) * b.double() + c.double()).float()


def exact_ln_rows(rows, C, s, seed, kmax=16, big=None):
    """Construction 1: x[r, c] = m_r +- s, exactly C / 2 channels of every row on the + side under a fresh random permutation per row;
    m_r = k / 2 with |k| <= kmax.  big: every fourth row takes this mean instead (the fp32 stream: x * x is then inexact in fp32, so a
    one-pass variance shows)."""
    g = _gen(seed)
    m = torch.randint(-kmax, kmax + 1, (rows,), generator=g).float() / 2.0
    if big is not None:
        m[3::4] = float(big)
    sign = torch.ones((rows, C))
    sign[:, C // 2:] = -1.0
    order = torch.stack([torch.randperm(C, generator=g) for _ in range(rows)])
    return m[:, None] + s * torch.gather(sign, 1, order)


def assert_exact_ln(v, eps, dt=None, what=""):
    """The lattice condition of construction 1 on the rows `v` (fp32, (..., C)) a LayerNorm with this eps is about to see: every row holds
    two values m +- s, C / 2 channels each; fp32(eps) + s^2 is exactly 1; every element is a multiple of a power of two `unit` with
    C max|v| / unit < 2^24, so every partial sum of the row — and of the squared deviations, C s^2 / unit^2 — is an fp32 number in any
    order; and (dt given) the rows are representable in the storage type."""
    C = v.shape[-1]
    v64 = v.double().reshape(-1, C)
    hi, lo = v64.amax(1, keepdim=True), v64.amin(1, keepdim=True)
    s = (hi - lo) / 2.0
    assert bool(((v64 == hi) | (v64 == lo)).all()) and bool(((v64 == hi).sum(1) == C // 2).all()), f"{what}: rows are not m +- s, half each"
    assert bool((s > 0).all()) and bool((f32w(eps) + s * s == 1.0).all()), f"{what}: eps + s^2 != 1"
    k = next((k for k in range(0, 16) if bool((v64 * 2.0 ** k == torch.round(v64 * 2.0 ** k)).all())), None)
    assert k is not None and C * float(v64.abs().max()) * 2.0 ** k < 2.0 ** 24, f"{what}: the row sums are not exact in fp32"
    assert C * float((s * s).max()) * 4.0 ** k < 2.0 ** 24
    if dt is not None:
        assert torch.equal(v.to(dt).float(), v), f"{what}: rows not representable in {dt}"


def tile_layernorm32(x, gam, bet, eps, tpr, dt):
    """wide_tile_layernorm / tile_layernorm (dmff_wide.hip, dmff_fused.hip) in fp32 with the device's association: `tpr` threads per row,
    thread p summing the 16-byte vectors p, p + tpr, ... element by element, then the xor-shuffle tree over 1, 2 (, 4); two passes.
    x (rows, C) fp32 holding `dt` values -> (mean, rstd, output in dt)."""
    rows, C = x.shape
    vec = VEC[dt]
    xv = x.reshape(rows, C // vec // tpr, tpr, vec).permute(0, 2, 1, 3).reshape(rows, tpr, -1)      # [row][thread][its elements, in order]

    def tree(t):
        acc = torch.zeros((rows, tpr))
        for j in range(t.shape[2]):
            acc = acc + t[:, :, j]
        step = 1
        while step < tpr:
            acc = acc + acc[:, torch.arange(tpr) ^ step]
            step *= 2
        return acc[:, :1]
    mean = tree(xv) / torch.tensor(float(C), dtype=F32)
    d = xv - mean[:, :, None]
    rstd = 1.0 / torch.sqrt(tree(d * d) / torch.tensor(float(C), dtype=F32) + torch.tensor(eps, dtype=F32))
    return mean, rstd, ((x - mean) * rstd * gam + bet).to(dt)


def _ri(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _nonzero(g, hi, shape):
    """integers in [-hi, hi] without 0"""
    return _ri(g, 1, hi, shape) * (_ri(g, 0, 1, shape) * 2.0 - 1.0)


def sparse_w2(C, hid, dt, seed, nnz=W2_NNZ):
    """Construction 3: W2 (2, C, hid) with `nnz` non-zeros k / 2^s_w per output channel, one in each of the nnz column blocks of width
    hid / nnz — so at least one in every hidden chunk and every hidden-split slice — placed by an affine map of the channel index, so
    that every hidden column is used by C nnz / hid (= 8) output channels of its modality."""
    g = _gen(seed)
    sw = GRID[dt][0]
    blk = hid // nnz
    assert hid % nnz == 0 and C % blk == 0 and wide_pass(C) % blk == 0
    w = torch.zeros((2, C, hid))
    n = torch.arange(C)
    for m in range(2):
        for j in range(nnz):
            a = 2 * int(torch.randint(0, blk // 2, (1,), generator=g)) + 1
            b = int(torch.randint(0, blk, (1,), generator=g))
            w[m, n, j * blk + (n * a + b) % blk] = _nonzero(g, 2 ** sw, (C,)) / 2 ** sw
    nz = w != 0
    assert bool((nz.sum(2) == nnz).all()) and bool((nz.sum(1) >= 2).all())
    assert bool((nz.reshape(2, C, hid // wide_pass(C), -1).sum(3) >= 1).all()), "an output channel misses a hidden chunk"
    return w


def dmff_operands_a(C, dt, rows=DMFF_ROWS_MAX, seed=0):
    """Test (a), out-projection and coefficient mix: att, W_o, b_o, x on the lattice of `dt`; x32 fp32 values that NEITHER 16-bit type
    holds (odd multiples of 2^-10 in [2, 4)); the four attention coefficients distinct powers of two; W2 = b2 = 0 with c_res_mlp = 1, so
    the launch returns x_att; W1, b1 and the MLP LayerNorm random and non-zero (the MLP runs on real data and must leave no trace).
    Rows r % 16 == 5 of x_att are CONSTANT on purpose (att = 0, x = 1 / 4 - (c_acc / c_res) b_o): the LayerNorm then divides by sqrt(eps),
    which stays finite — a variance clamped to zero without eps would show as Inf * 0."""
    g = _gen(7000 + 10 * C + [F32, BF16, F16].index(dt) + seed)
    sw, sf = GRID[dt]
    hid = 4 * C
    co = [1.0, 0.5, 2.0, 0.25, 1.0, 0.5, 1.0, 2.0]          # (res, acc) of the attention mix per modality, then of the MLP mix
    d = dict(att=_ri(g, -8, 8, (2, rows, C)), wo=_ri(g, -2 ** sw, 2 ** sw, (2, C, C)) / 2 ** sw, bo=_ri(g, -64, 64, (2, C)) / 2 ** sf,
             x=_ri(g, -64, 64, (2, rows, C)) / 2 ** sf, x32=(2049.0 + 2.0 * _ri(g, 0, 1023, (2, rows, C))) * (_ri(g, 0, 1, (2, rows, C)) * 2.0 - 1.0) / 1024.0,
             w1=torch.randn((2, hid, C), generator=g) / math.sqrt(C), b1=torch.randn((2, hid), generator=g) * 0.3,
             w2=torch.zeros((2, C, hid)), b2=torch.zeros((2, C)), co=co, eps=(1e-5, 1e-5, 1e-5), hidden=hid,
             ln=dict(a1w=torch.ones(C), a1b=torch.zeros(C), a2w=torch.ones(C), a2b=torch.zeros(C),
                     mw=1.0 + 0.3 * torch.randn((C,), generator=g), mb=0.2 * torch.randn((C,), generator=g)))
    const = torch.arange(rows) % 16 == 5
    for m in range(2):
        d["att"][m, const] = 0.0
        flat = 0.25 - (co[2 * m + 1] / co[2 * m]) * d["bo"][m]
        d["x"][m, const] = flat
        d["x32"][m, const] = flat
    d["const"] = const
    for name in ("att", "wo", "x"):
        assert torch.equal(d[name].to(dt).float(), d[name]), f"lattice {name} is not representable in {dt}"
    if dt != F32:
        free = d["x32"][:, ~const]
        assert not bool((free.to(BF16).float() == free).any()) and not bool((free.to(F16).float() == free).any())
    return d


def dmff_xatt64(d, use_x32=False):
    """fp64 x_att = c_res x + c_acc (att W_o^T + b_o) of both modalities, asserted to be an fp32 number (on the lattice it is exact)."""
    out = []
    for m in range(2):
        x = (d["x32"] if use_x32 else d["x"])[m].double()
        acc = d["att"][m].double() @ d["wo"][m].double().T
        assert torch.equal((d["att"][m] @ d["wo"][m].T).double(), acc), "fp32 and fp64 out-projection differ: not on an exact lattice"
        z = f32w(d["co"][2 * m]) * x + f32w(d["co"][2 * m + 1]) * (acc + d["bo"][m].double())
        assert is_f32(z), "x_att is not an fp32 number"
        out.append(z)
    return torch.stack(out)


def dmff_operands_b(C, dt, rows=DMFF_ROWS_MAX, seed=0):
    """Test (b), LayerNorm + MLP + final mix: W_o = b_o = 0, x the rows of construction 1 — modality 0 with c_res = 1 and s = 0.5,
    modality 1 with c_res = 2 and s = 0.25, so both reach deviations of 0.5 under the one shared eps_mlp = 0.75; x32 (the fp32 stream of a
    later iteration) is a DIFFERENT set of such rows, every fourth one around a mean of 4096; gamma / beta = j / 8, W1 = j / 128, b1 = j / 32
    (pre-activations exact, most of them in |u| < 3), W2 sparse, b2 on the lattice.  The attention LayerNorm's parameters differ from the
    MLP's; att is random (against the zero W_o it must leave no trace)."""
    g = _gen(8000 + 10 * C + [F32, BF16, F16].index(dt) + seed)
    sf = GRID[dt][1]
    hid = 4 * C
    co = [1.0, 0.5, 2.0, 0.25, 0.5, 2.0, 0.25, 4.0]
    lat8 = lambda: _nonzero(g, 16, (C,)) / 8.0
    d = dict(att=_ri(g, -8, 8, (2, rows, C)), wo=torch.zeros((2, C, C)), bo=torch.zeros((2, C)),
             x=torch.stack((exact_ln_rows(rows, C, 0.5, 8100 + C), exact_ln_rows(rows, C, 0.25, 8200 + C, kmax=8))),
             x32=torch.stack((exact_ln_rows(rows, C, 0.5, 8300 + C, big=4096.0), exact_ln_rows(rows, C, 0.25, 8400 + C, kmax=8, big=2048.0))),
             w1=_ri(g, -8, 8, (2, hid, C)) / 128.0, b1=_ri(g, -32, 32, (2, hid)) / 32.0,
             w2=sparse_w2(C, hid, dt, 8500 + C), b2=_ri(g, -64, 64, (2, C)) / 2 ** sf, co=co, eps=(1e-5, 1e-5, LN_EPS_EXACT), hidden=hid,
             ln=dict(a1w=lat8(), a1b=lat8(), a2w=lat8(), a2b=lat8(), mw=lat8(), mb=_ri(g, -16, 16, (C,)) / 8.0))
    assert not torch.equal(d["ln"]["a1w"], d["ln"]["mw"]) and not torch.equal(d["ln"]["a2w"], d["ln"]["mw"])
    assert not torch.equal(d["b1"][:, :hid // 2], d["b1"][:, hid // 2:])
    for name in ("att", "x", "w1", "w2"):
        assert torch.equal(d[name].to(dt).float(), d[name]), f"lattice {name} is not representable in {dt}"
    return d


def dmff_ref_b(d, dt, use_x32=False):
    """fp64 reference and COUNTED per-element bounds of test (b).  Returns dict(out, by, b32, known, share, u_std): the reference (2, rows, C),
    the bound on the stored y, the bound on the fp32 stream y32, the outputs none of whose hidden operands is ambiguous (their bound is
    the accumulation and the mix alone), the share of hidden elements whose rounding is ambiguous, the spread of u.

    Everything up to the pre-activation u is exact (asserted).  From there, with u = 2^-24:
      1. h = RNE_dt(gelu(u)): the device evaluates GELU within act_budget32 of the true value; where true value +- budget round to the SAME
         number of the storage type, h is known exactly (h_ref); where they do not (`ambiguous`), h may be the neighbour: |W2[n, k]| ulp_dt(h_k).
         The fp32 build stores h unrounded: sum |W2| budget instead.
      2. the fc2 sum has nnz non-zero terms per output (products w h exact in fp32 for the 16-bit types: <= 7 + 11 bits): nnz - 1 roundings
         of partial sums bounded by S = sum |w h| — the chunk and slice order does not matter, adding an exact zero is exact.  The fp32 build
         rounds the nnz products as well: 2 nnz - 1.
      3. the final mix  fma(c_res, x_att, (sum + b2) * c_acc): the addition of b2 (u |mlp|), the product (u |c_acc mlp|), the fma (u |out|).
      4. the storage rounding of y (storage_bound); y32 and the fp32 build's y have none."""
    C, hid = d["x"].shape[2], d["hidden"]
    outs, bys, b32s, known, amb_n, ustd = [], [], [], [], 0, []
    for m in range(2):
        cr_a, cr_m, ca_m = f32w(d["co"][2 * m]), f32w(d["co"][4 + 2 * m]), f32w(d["co"][5 + 2 * m])
        assert not bool(d["wo"][m].any()) and not bool(d["bo"][m].any())
        xatt = cr_a * (d["x32"] if use_x32 else d["x"])[m].double()
        assert_exact_ln(xatt.float(), d["eps"][2], None if use_x32 else dt, "x_att")
        mean = (xatt.amax(1, keepdim=True) + xatt.amin(1, keepdim=True)) / 2.0
        n2 = (xatt - mean) * d["ln"]["mw"].double() + d["ln"]["mb"].double()                # rstd = 1
        assert torch.equal(n2.float().to(dt).double(), n2), "the normalised tile is not representable in the storage type"
        u = n2 @ d["w1"][m].double().T + d["b1"][m].double()
        assert torch.equal((n2.float() @ d["w1"][m].T + d["b1"][m]).double(), u), "the pre-activation is not exact in fp32"
        g64 = act64(u, ACT_GELU)
        bud = act_budget32(u, ACT_GELU, dt)
        w2 = d["w2"][m].double()
        if dt == F32:
            h, t1 = g64, bud @ w2.abs().T
            nround = 2 * W2_NNZ - 1
        else:
            h = rne64(g64, dt)
            amb = rne64(g64 - bud, dt) != rne64(g64 + bud, dt)
            amb_n += int(amb.sum())
            t1 = (amb.double() * ulp(g64.abs() + bud, dt)) @ w2.abs().T
            nround = W2_NNZ - 1
        mlp = h @ w2.T + d["b2"][m].double()
        t2 = nround * U32 * (h.abs() @ w2.abs().T)
        out = cr_m * xatt + ca_m * mlp
        b32 = (abs(ca_m) * (t1 + t2) + U32 * (mlp.abs() + (ca_m * mlp).abs() + out.abs())) * SECOND + SUB32
        outs.append(out)
        b32s.append(b32)
        known.append(t1 == 0 if dt != F32 else torch.ones_like(t1, dtype=torch.bool))
        bys.append(b32 if dt == F32 else storage_bound(out, b32, dt))
        ustd.append(float(u.std()))
    share = 0.0 if dt == F32 else amb_n / (2.0 * d["x"].shape[1] * hid)
    return dict(out=torch.stack(outs), by=torch.stack(bys), b32=torch.stack(b32s), known=torch.stack(known), share=share, u_std=ustd)


def proj_mlp64(d, dt, use_x32=False):
    """Plain fp64 statement of one proj_mlp launch on ANY data (weights and 16-bit operands as the storage type holds them; no
    intermediate rounding): what close() compared against in tests/test_gpu_dmff_fused.py's style of check."""
    q = lambda t: t.to(dt).double()
    outs = []
    for m in range(2):
        co = [f32w(c) for c in d["co"]]
        x = d["x32"][m].double() if use_x32 else q(d["x"][m])
        xatt = co[2 * m] * x + co[2 * m + 1] * (q(d["att"][m]) @ q(d["wo"][m]).T + d["bo"][m].double())
        dev = xatt - xatt.mean(1, keepdim=True)
        n2 = dev / torch.sqrt((dev * dev).mean(1, keepdim=True) + f32w(d["eps"][2])) * d["ln"]["mw"].double() + d["ln"]["mb"].double()
        h = act64(n2 @ q(d["w1"][m]).T + d["b1"][m].double(), ACT_GELU)
        outs.append(co[4 + 2 * m] * xatt + co[5 + 2 * m] * (h @ q(d["w2"][m]).T + d["b2"][m].double()))
    return torch.stack(outs)


PROJ_MLP_DEFECTS = ("trunc", "swap", "lastchunk", "b1off", "halfshift", "lnswap", "erf")


def emulate_proj_mlp(d, dt, ksplit=1, r32=False, use_x32=False, defect=None):
    """One icaf_dmff_wide_proj_mlp launch (ksplit > 1: proj_mlp_split + reduce) in torch fp32 with the rounding points of dmff_wide.hip:
    x_att = fma(c_res, x, (acc + b_o) c_acc), rounded to the storage type unless the fp32 stream keeps it (r32); two-pass LayerNorm on
    that value, its output rounded to the storage type; per hidden chunk of wide_pass(C) columns h = RNE(gelu(n2 W1^T + b1)) and
    acc2 += h W2^T in fp32, the slices of a split added in slice order; y = RNE(fma(c_res2, x_att, (acc2 + b2) c_acc2)), y32 the same
    unrounded.  Returns (y, y32 or None).
    defect: None | "trunc" (x_att truncated instead of rounded) | "swap" (the two modalities' coefficients exchanged) | "lastchunk" (the last
    hidden chunk skipped) | "b1off" (a hidden-split slice reads b1 from offset 0 instead of its own columns) | "halfshift" (the second
    32-row half of every tile takes the row below) | "lnswap" (the MLP LayerNorm with gamma / beta of the attention LayerNorm) | "erf" (a3
    of the erf polynomial changed, as emulate())."""
    rows, C = d["x"].shape[1], d["x"].shape[2]
    hid, wp = d["hidden"], wide_pass(C)
    assert use_x32 <= r32 and (ksplit == 1 or (C >= 256 and dt != F32)) and hid % (wp * ksplit) == 0
    q = lambda t: t.to(dt).float()
    eps_m = torch.tensor(d["eps"][2], dtype=F32)
    fC = torch.tensor(float(C), dtype=F32)
    coef = ERF_COEF if defect != "erf" else (ERF_COEF[0], ERF_COEF[1], 1.421513741, ERF_COEF[3], ERF_COEF[4])
    ys, y32s = [], []
    for m in range(2):
        mc = 1 - m if defect == "swap" else m
        cr_a, ca_a, cr_m, ca_m = (d["co"][2 * mc], d["co"][2 * mc + 1], d["co"][4 + 2 * mc], d["co"][5 + 2 * mc])
        xres = d["x32"][m] if use_x32 else q(d["x"][m])
        acc = q(d["att"][m]) @ q(d["wo"][m]).T
        v = fma32(cr_a, xres, (acc + d["bo"][m]) * torch.tensor(ca_a, dtype=F32))
        xatt = v if r32 else _store(v, dt, defect).float()
        mean = xatt.sum(1, keepdim=True) / fC
        dev = xatt - mean
        rstd = 1.0 / torch.sqrt((dev * dev).sum(1, keepdim=True) / fC + eps_m)
        lw, lb = (d["ln"]["a2w" if m else "a1w"], d["ln"]["a2b" if m else "a1b"]) if defect == "lnswap" else (d["ln"]["mw"], d["ln"]["mb"])
        n2 = q(dev * rstd * lw + lb)
        w1, w2 = q(d["w1"][m]), q(d["w2"][m])
        per = hid // wp // ksplit
        total = None
        for ks in range(ksplit):
            acc2 = torch.zeros((rows, C))
            for ch in range(per):
                if defect == "lastchunk" and ks == ksplit - 1 and ch == per - 1:
                    continue
                c0 = (ks * per + ch) * wp
                boff = ch * wp if defect == "b1off" else c0
                u = n2 @ w1[c0:c0 + wp].T + d["b1"][m][boff:boff + wp]
                h = torch.erf(u * 0.70710678118654752440).add(1.0).mul(0.5 * u) if dt == F32 else q(_gelu_fast32(u, coef))
                acc2 = acc2 + h @ w2[:, c0:c0 + wp].T
            total = acc2 if total is None else total + acc2
        out = fma32(cr_m, xatt, (total + d["b2"][m]) * torch.tensor(ca_m, dtype=F32))
        if defect == "halfshift":
            r = torch.arange(rows)
            out = out[torch.where(r % 64 >= 32, (r + 1).clamp(max=rows - 1), r)]
        ys.append(out.to(dt))
        y32s.append(out)
    return torch.stack(ys), (torch.stack(y32s) if r32 else None)


def check_proj_mlp_a(y, y32, z, dt, what):
    """Test (a): y == RNE(x_att) bit for bit, y32 == x_att bit for bit (z: dmff_xatt64 of the rows the launch saw)."""
    assert_same_bits(y, rne(z, dt) + 0.0, what + ": y")
    if y32 is not None:
        assert_same_bits(y32, z.float() + 0.0, what + ": y32")


def check_proj_mlp_b(y, y32, ref, dt, what):
    """Test (b): every element of y (and of y32) within its counted bound; returns the largest err / budget of each."""
    n = y.shape[1]
    r = assert_budget(y, ref["out"][:, :n], ref["by"][:, :n], what + ": y", signed=False)
    r32 = assert_budget(y32, ref["out"][:, :n], ref["b32"][:, :n], what + ": y32", signed=False) if y32 is not None else 0.0
    return r, r32


def dmff_operands_qkv(C, dt, rows=DMFF_ROWS_MAX, seed=0):
    """Test (d): the rows of construction 1 (s = 0.5, eps_attn = 0.75) in both modalities, gamma / beta = j / 8 DIFFERENT for the two
    attention LayerNorms, W_qkv = k / 2^s_w and bias = j / 2^s_f different per modality.  Returns the operands and the exact fp64 qkv
    (2, rows, 3C): normalised rows +-0.5 gamma + beta (representable), then an exact GEMM."""
    g = _gen(9000 + 10 * C + [F32, BF16, F16].index(dt) + seed)
    sw, sf = GRID[dt]
    lat8 = lambda: _nonzero(g, 16, (C,)) / 8.0
    d = dict(x=torch.stack((exact_ln_rows(rows, C, 0.5, 9100 + C), exact_ln_rows(rows, C, 0.5, 9200 + C))),
             wqkv=_ri(g, -2 ** sw, 2 ** sw, (2, 3 * C, C)) / 2 ** sw, bqkv=_ri(g, -64, 64, (2, 3 * C)) / 2 ** sf,
             ln=dict(a1w=lat8(), a1b=lat8(), a2w=lat8(), a2b=lat8(), mw=torch.ones(C), mb=torch.zeros(C)),
             co=[1.0] * 8, eps=(LN_EPS_EXACT, LN_EPS_EXACT, 1e-5), hidden=4 * C)
    assert not torch.equal(d["ln"]["a1w"], d["ln"]["a2w"]) and not torch.equal(d["ln"]["a1b"], d["ln"]["a2b"])
    assert_exact_ln(d["x"], LN_EPS_EXACT, dt, "qkv rows")
    zs = []
    for m in range(2):
        x = d["x"][m].double()
        mean = (x.amax(1, keepdim=True) + x.amin(1, keepdim=True)) / 2.0
        n = (x - mean) * d["ln"]["a2w" if m else "a1w"].double() + d["ln"]["a2b" if m else "a1b"].double()
        assert torch.equal(n.float().to(dt).double(), n)
        z = n @ d["wqkv"][m].double().T + d["bqkv"][m].double()
        assert torch.equal((n.float() @ d["wqkv"][m].T + d["bqkv"][m]).double(), z), "the QKV sums are not exact in fp32"
        zs.append(z)
    return d, torch.stack(zs)


def dmff_take_rows(d, rows):
    """The operands of a case cut to its first `rows` token rows (rows are independent: references are built once at DMFF_ROWS_MAX)."""
    out = dict(d)
    for k in ("att", "x", "x32"):
        if k in d:
            out[k] = d[k][:, :rows].contiguous()
    return out


def dmff_operands_rnd(C, rows, seed=31):
    """Gaussian operands of one proj_mlp launch in the style of tests/test_gpu_dmff_fused.py (tokens normal(0.2, 0.8), weights of a
    trained block's size): the data on which the self-test records what a max-norm tolerance makes of each planted defect."""
    hid = 4 * C
    r = lambda shape, k, scale=1.0: rnd(shape, seed + k, scale)
    return dict(att=r((2, rows, C), 0, 0.5), wo=r((2, C, C), 1, C ** -0.5), bo=r((2, C), 2, 0.1), x=0.2 + r((2, rows, C), 3, 0.8),
                x32=0.2 + r((2, rows, C), 4, 0.8), w1=r((2, hid, C), 5, C ** -0.5), b1=r((2, hid), 6, 0.1), w2=r((2, C, hid), 7, hid ** -0.5),
                b2=r((2, C), 8, 0.1), co=[0.9, 0.45, 0.8, 0.55, 0.85, 0.5, 0.95, 0.4], eps=(1e-5, 1e-5, 1e-5), hidden=hid,
                ln=dict(a1w=1.0 + r((C,), 9, 0.1), a1b=r((C,), 10, 0.1), a2w=1.0 + r((C,), 11, 0.1), a2b=r((C,), 12, 0.1),
                        mw=1.0 + r((C,), 13, 0.1), mb=r((C,), 14, 0.1)))


def attn_known_qkv(B, N, C, dt, seed):
    """Test (e): a qkv tensor (2, B * N, 3C) whose attention output is known exactly.  K = 0: every score is 0, every probability of an
    image's N keys equal, so a query's output is the MEAN of V over the keys of its image — of the modality whose K / V the direction
    reads, whatever Q holds (random integers).  V = a per-(modality, image, channel) integer in [-8, 8] plus per-key integer
    perturbations in [-4, 4] that sum to zero over the image: the key sum is N times the constant, exact in fp32 in any order, and the
    mean is representable in every type.  Returns (qkv, att (2, B * N, C): that mean on every row of the image)."""
    g = _gen(seed)
    base = _ri(g, -8, 8, (2, B, 1, C))
    assert not torch.equal(base[0], base[1])
    half = _ri(g, -4, 4, (2, B, N // 2, C))
    pert = torch.cat((half, -half, torch.zeros((2, B, N % 2, C))), 2)
    order = torch.stack([torch.randperm(N, generator=g) for _ in range(2 * B * C)]).reshape(2, B, C, N).permute(0, 1, 3, 2)
    v = base + torch.gather(pert, 2, order)
    assert torch.equal(v.sum(2, keepdim=True), N * base) and torch.equal(v.to(dt).float(), v)
    qkv = torch.cat((_ri(g, -8, 8, (2, B, N, C)), torch.zeros((2, B, N, C)), v), 3).reshape(2, B * N, 3 * C)
    return qkv, base.expand(2, B, N, C).reshape(2, B * N, C).contiguous()


# ====================================================================================================================================
# cross attention (dmff.hip: cross_attn_kernel, cross_attn_stream_kernel; attn_core.h: AttnCore, also inside dmff_attn_mlp_kernel).
# qkv is (2, B * N, 3C) = [Q | K | V], heads head-major inside each third; direction `dir` reads K / V of modality dir and Q of the OTHER
# modality:  out[dir] = softmax(Q[1 - dir] K[dir]^T / sqrt(d_k)) V[dir]  per (image, head).
# ====================================================================================================================================
LOG2E = 1.4426950408889634
EXP2_REL = 2.0 * U32             # v_exp_f32: 1 ulp — the figure silu_budget32 above takes from the ISA guide (the guide's text is not part of
                                 # this repository; tests/test_gpu_exact_attn.py records what the fp32 builds show against fp64 beside it)
ATTN_HEADS = 8
ATTN_RES_DK = (16, 32, 40, 64, 72, 128)              # resident form: DKP 16 / 32 / 48 / 64 / 96 / 128
ATTN_STREAM_DK = (64, 128, 192, 256)                 # streaming form: 64 and 128 through the knob attn_stream, 192 and 256 by the library's choice
ATTN_CELLS = [(0, dk) for dk in ATTN_RES_DK] + [(1, dk) for dk in ATTN_STREAM_DK]
ATTN_TOKENS = ((1, 77), (4, 77), (1, 130), (4, 130), (1, 32))       # (B, N)
ATTN_DEFER = 6.0                                     # AttnCore::DEFER (16-bit builds)
ATTN_UNDERFLOW = 149.0 + ATTN_DEFER + 8.0            # exponent distance below which a probability is 0 in fp32 whatever maximum is held
ATTN_DEFECTS = ("nomask", "vtperm", "scale_dkp", "l_norescale", "dirswap", "headoff", "lastq")


def attn_dkp(dk, form):
    """Padded head dimension of the instantiation (attn_select in dmff.hip)."""
    return next(p for p in ((64, 128, 256) if form else (16, 32, 48, 64, 96, 128)) if p >= dk)


def attn_resident_lds(dk, N, dt):
    """LDS bytes of the resident form (attn_resident_lds in dmff.hip): above 160 KiB the library streams the shape instead."""
    eb, NP, dkp = (4 if dt == F32 else 2), (N + 31) // 32 * 32, attn_dkp(dk, 0)
    return NP * (dkp * eb + 16) + (dkp + (1 if dt != F32 and dkp % 32 == 16 else 0)) * (NP * eb + 16)


def attn_form(dk, N, dt, form):
    """The form a cell's launch really takes: a resident cell whose K / V^T do not fit the LDS (fp32, d_k = 128, N = 130) streams."""
    return 1 if form or dk > 128 or attn_resident_lds(dk, N, dt) > 160 * 1024 else 0


def attn_den(dk, form, dt):
    """Where the instantiation forms the softmax denominator: "free" (a ones row of V^T in the unused rows of the last O^T tile), "xtra" (one
    more MFMA with an all-ones A operand) — both sum the ROUNDED probabilities — or "valu" (fp32 adds of the unrounded ones)."""
    if dt == F32 or form:
        return "valu"
    dkp = attn_dkp(dk, form)
    return "free" if dkp % 32 == 16 else "xtra" if dkp == 32 else "valu"


def attn_scale(dk):
    """scale_l2e as the launch computes it: fp32(log2(e) / sqrt(d_k)), as an fp64 number."""
    return f32w((1.0 / math.sqrt(dk)) * LOG2E)


def _attn_split(qkv, B, N, C, heads):
    """(2, B * N, 3C) -> q, k, v as (2, B, heads, N, dk) of the modality that STORES them."""
    f = qkv.reshape(2, B, N, 3, heads, C // heads)
    return tuple(f[:, :, :, i].permute(0, 1, 3, 2, 4) for i in range(3))


def _attn_join(o):
    """(2, B, heads, N, dk) -> (2, B * N, C)"""
    G, B, H, N, dk = o.shape
    return o.permute(0, 1, 3, 2, 4).reshape(G, B * N, H * dk).contiguous()


def attn_select_qkv(B, N, dk, seed, heads=ATTN_HEADS, vmax=127):
    """Family `select`: query i of (direction, image, head) has ONE winning key pi(i); every other probability is exactly 0 in fp32.
    Dimension 0 of a head holds q = -d_k a_q and k = a_k, dimensions 1 .. d_k - 1 hold a_q / a_k times a +-1 code word; a_q a_k = A is a power
    of two.  A key's code word is an 8-bit number (a random permutation of 0 .. 255 per group, cut to N) with bit (d mod 8) on code dimension d,
    the dimensions shuffled and sign-flipped per (direction, image, head); the query carries the word of its winner.  Hence
        score(i, j) = A ((d_k - 1) - 2 hamming(i, j)) - A d_k:   -A for the winner, <= -A (1 + 2 dmin) for every other key, dmin = (d_k - 1) // 8,
    every term a multiple of A below 2^24: an exact integer in fp32 in any order.  All scores are negative, so a zero-filled padding key
    that is not masked, or a zero K row, BEATS the winner by A c >= ATTN_UNDERFLOW / (2 dmin) in the exponent domain and the output
    collapses to 0.  A is the smallest power of two with 2 A dmin c >= ATTN_UNDERFLOW = 149 + 6 + 8: a loser's probability is at most
    2^-(149 + 8) relative to whatever maximum the deferred loop holds (at most 6 below the true one) — 0 in fp32 — and once the winner has
    been seen the rescale factor of everything before it is 0 as well.  V: non-zero integers in [-vmax, vmax], rows distinct.
    Returns (qkv (2, B * N, 3C), expected (2, B * N, C) = V[pi(i)] of the direction's own modality, pi (2, B, heads, N))."""
    g = _gen(seed)
    L, C = dk - 1, heads * dk
    dmin = L // 8
    c = LOG2E / math.sqrt(dk)
    A = 2.0 ** math.ceil(math.log2(ATTN_UNDERFLOW / (2.0 * dmin * c)))
    aq = 2.0 ** math.ceil(math.log2(A) / 2.0)
    ak = A / aq
    assert 2.0 * A * dk < 2.0 ** 24 and N <= 256 and dmin >= 1
    G = (2, B, heads)
    word = torch.stack([torch.randperm(256, generator=g)[:N] for _ in range(2 * B * heads)]).reshape(*G, N)
    dimp = torch.stack([torch.randperm(L, generator=g) for _ in range(2 * B * heads)]).reshape(*G, 1, L)
    sign = _ri(g, 0, 1, (*G, 1, L)) * 2.0 - 1.0
    code = (1.0 - 2.0 * ((word[..., None] >> (dimp % 8)) & 1).float()) * sign                  # (2, B, heads, N, L)
    pi = torch.randint(0, N, (*G, N), generator=g)
    qcode = torch.gather(code, 3, pi[..., None].expand(*G, N, L))                                # query i carries the word of key pi(i) ...
    k = torch.cat((torch.full((*G, N, 1), ak), ak * code), 4)
    q = torch.cat((torch.full((*G, N, 1), -dk * aq), aq * qcode), 4).flip(0)                     # ... and is stored in the OTHER modality
    v = _nonzero(g, vmax, (*G, N, dk))
    want = torch.gather(v, 3, pi[..., None].expand(*G, N, dk))
    qkv = torch.cat((_attn_join(q), _attn_join(k), _attn_join(v)), 2)
    # ---- the construction, asserted in fp64 ----
    s = q.flip(0).double() @ k.double().transpose(-1, -2)
    assert torch.equal(s, s.round()) and float(s.abs().max()) < 2.0 ** 24 and float(s.max()) < 0.0, "select: scores must be negative integers below 2^24"
    win = torch.gather(s, 4, pi[..., None])
    assert torch.equal(win, s.amax(4, keepdim=True)) and bool((win == -A).all())
    gap = (win - s) * c
    gap.scatter_(4, pi[..., None], float("inf"))
    assert float(gap.min()) >= ATTN_UNDERFLOW, f"select: a losing key lies only {float(gap.min()):.1f} below its winner"
    assert A * c < 2.0 ** 11                         # |m c| < 2^11: the fma's residual exponent is below 2^-13, P of the winner rounds to 1 in 16 bit
    chosen = torch.zeros(N, dtype=torch.bool)
    chosen[pi.reshape(-1)] = True
    assert bool(chosen.all()), "select: some key index is nobody's winner in any group"
    assert all(len(torch.unique(pi.reshape(-1, N)[i])) < N for i in range(2 * B * heads)), "select: pi must not be a bijection"
    rows = v.reshape(-1, dk)
    assert len(torch.unique(rows, dim=0)) == len(rows), "select: V rows must be distinct"
    for t in (qkv, want):
        assert torch.equal(t.to(BF16).float(), t) and torch.equal(t.to(F16).float(), t)
    return qkv, _attn_join(want), pi


def attn_select_bound(want, dt):
    """|out - V[pi(i)]| of family select, from attn_core.h.  m is the winner's score exactly once its tile has run (first tile: m = the tile
    maximum; later: the winner exceeds any held maximum by more than the slack, so the cold path runs and alpha = exp2(<= -155) = 0 wipes O
    and l).  The winner's exponent fma(s, c, -fl(m c)) is the rounding error of m c, below 2^-24 * 2^11; P = exp2 of it is 1 + O(2^-13):
      16 bit: P rounds to 1; O = v exactly.  free / xtra: l = 1, the result is v.  valu: l = 1 + O(2^-13) unrounded, o / l is within 2^-13 of v,
              less than a quarter unit of either type — RNE returns v.  None: BIT FOR BIT in all three forms.
      fp32:   O = fl(v P) (<= 2u, MFMA rounding not assumed to be RNE), l = P, 1 / l (<= 2u), the product (u): 5u |v|."""
    if dt != F32:
        return None
    return 5.0 * U32 * SECOND * want.double().abs() + SUB32


# (key, height in the exponent domain above the background's mean) of the dominant keys of family graded, per N
ATTN_STAIRS = {32: ((10, 12.0), (30, 20.0)),
               77: ((25, 12.0), (44, 16.0), (70, 46.0), (76, 50.0)),
               130: ((25, 12.0), (44, 16.0), (80, 22.0), (120, 50.0), (129, 54.0))}


def attn_graded_qkv(B, N, dk, seed, heads=ATTN_HEADS):
    """Family `graded`: real softmax weights with the cold path forced.  Q integers in {0, 1, 2}, background K integers in [-2, 2] (scores
    exact integers, about +-2.6 sigma wide in the exponent domain at every d_k), V = j / 4 with |j| <= 32.  ATTN_STAIRS[N] places dominant keys
    late in the key order: K = t on a random subset S of the head's dimensions and 0 elsewhere, t |S| ~ height / c, so a query's score is
    t sum_S q — the height holds on average and varies by a few units from query to query.  After the first tile the held maximum is about
    12; the step to 16 stays below the slack of 6 (no rescale, p up to 2^6, for most lanes), the step to 22 lies just above it, the steps
    to 46 / 50 far above (O and the denominator rescaled by 2^-30), the last one sits on the last key — in the ragged last tile, again less
    than the slack above the maximum held there.  |s - m| c stays below about 70."""
    g = _gen(seed)
    G = (2, B, heads)
    q = _ri(g, 0, 2, (*G, N, dk))
    k = _ri(g, -2, 2, (*G, N, dk))
    v = _ri(g, -32, 32, (*G, N, dk)) / 4.0
    c = LOG2E / math.sqrt(dk)
    for key, h in ATTN_STAIRS[N]:
        t = math.ceil(h / c / dk)
        ns = max(1, min(dk, round(h / c / t)))
        sel = torch.stack([torch.randperm(dk, generator=g) < ns for _ in range(2 * B * heads)]).reshape(*G, dk)
        k[:, :, :, key] = sel.float() * t
    qkv = torch.cat((_attn_join(q.flip(0)), _attn_join(k), _attn_join(v)), 2)
    assert torch.equal(qkv.to(BF16).float(), qkv) and torch.equal(qkv.to(F16).float(), qkv)
    return qkv


def attn_ref64(qkv, B, N, C, heads=ATTN_HEADS, dk_scale=None):
    """fp64 softmax(q k^T / sqrt(d_k)) v with the true d_k, and what the counted bound needs, each (2, B * N, C):
      out   the reference;
      dev   sqrt(sum_k w_k (v_k - out)^2) >= sum_k w_k |v_k - out| (Jensen): what a relative perturbation of the WEIGHTS multiplies;
      a1    sum_k w_k |v_k|: what a relative perturbation of the numerator alone, or of the accumulation, multiplies;
      sc    max_k |s_k| c of the query's row, repeated over the head's channels."""
    dk = C // heads
    q, k, v = (t.double() for t in _attn_split(qkv, B, N, C, heads))
    s = q.flip(0) @ k.transpose(-1, -2)
    w = torch.softmax(s / math.sqrt(dk_scale or dk), -1)
    out = w @ v
    dev = torch.sqrt(torch.clamp(w @ (v * v) - out * out, min=0.0)) + 2.0 ** -40
    sc = (s.abs().amax(-1, keepdim=True) * (LOG2E / math.sqrt(dk))).expand_as(out)
    return dict(out=_attn_join(out), dev=_attn_join(dev), a1=_attn_join(w @ v.abs()), sc=_attn_join(sc), vmax=float(v.abs().max()))


def attn_graded_bound(ref, N, dk, form, dt):
    """Per-element bound on |device - ref['out']| of one launch, counted from attn_core.h (u = 2^-24, nkt = key tiles, first order):
      exponent   fma(s, c, -fl(m c)): the rounding of c (u |s - m| c), of m c (u |m| c) and of the fma (u |s - m| c); alpha on the cold path:
                 fl((m - m') c) with the rounded c, 2u |m - m'| c, at most once per tile.  All at most (5 + 4 nkt) u max|s| c, times ln 2
                 as a relative error of the probability;
      exp2       EXP2_REL per probability and per alpha: (1 + nkt) EXP2_REL;
                 — both reach numerator and denominator alike (alpha scales O and the denominator together in every form), so they perturb
                 the WEIGHTS: times dev;
      P          RNE to the storage type, 2^-(MANT + 1) per probability: numerator and denominator alike in free / xtra (times dev, and
                 1 + 2 eta for the perturbed denominator), the numerator only in valu (times a1); fp16: a probability below 2^-14 is rounded
                 absolutely, 2^-25 each against a denominator >= 1: N 2^-25 max|v|;
      sums       fp32 accumulation over the keys in the MFMA (or the VALU adds of the denominator) and the rescales: (N + nkt + 2) roundings
                 of 3u each (product, add, no RNE assumed), in numerator and denominator: 2 (N + nkt + 2) 3u a1;
      1 / l      2u, the product u: 3u |out|;
      storage    half a unit of the type where the value lies (storage_bound)."""
    nkt = (N + 31) // 32
    out = ref["out"]
    eta_w = math.log(2.0) * U32 * ref["sc"] * (5.0 + 4.0 * nkt) + (1.0 + nkt) * EXP2_REL
    b32 = eta_w * ref["dev"] + 2.0 * (N + nkt + 2) * 3.0 * U32 * ref["a1"] + 3.0 * U32 * out.abs() + SUB32
    if dt != F32:
        eta_p = 2.0 ** -(MANT[dt] + 1)
        b32 = b32 + (eta_p * (1.0 + 2.0 * eta_p) * ref["dev"] if attn_den(dk, form, dt) != "valu" else eta_p * ref["a1"])
        if dt == F16:
            b32 = b32 + N * 2.0 ** -25 * ref["vmax"]
    return storage_bound(out, SECOND * b32, dt)


def attn_uniform_bound(att, N, dt):
    """Family uniform (attn_known_qkv: K = 0): p = exp2(0) = 1 for the N keys, O = N mean exactly, l = N; o * fl(1 / l) carries 2u + u.
    16 bit: the mean is representable and 3u is far inside a quarter unit: BIT FOR BIT (None).  fp32: 3u |mean| (exact at a power of two)."""
    if dt != F32:
        return None
    return 3.0 * U32 * SECOND * att.double().abs() + SUB32


def attn_gauss_qkv(B, N, C, seed=41):
    """The Gaussian data of test_cross_attention (tests/test_gpu_kernels.py), for the record of what close(factor=2) accepts."""
    qkv = rnd((2, B * N, 3 * C), seed, 1.0)
    qkv[:, :, :2 * C] *= 1.5
    return qkv


def emulate_attention(qkv, B, N, C, heads, dt, form, defect=None):
    """fp32 restatement of the tile loop of attn_core.h / cross_attn_stream_kernel for one launch: 32-key tiles, 32-query tiles (one wave
    each: the cold-path vote __any is taken over the tile's 32 queries, padding queries — zero Q rows — included), the deferred maximum
    with slack DEFER / c (none in fp32), P rounded to `dt` for the numerator, the denominator from the rounded P (free / xtra) or from the
    unrounded one (valu), the rescale of O and the denominator, o * (1 / l), RNE to `dt`.  qkv: CPU tensor holding `dt` values.
    defect: None or one of ATTN_DEFECTS —
      nomask       padding keys keep their score 0;                       vtperm    keys 21 and 26 (one 16-key group) trade places in V^T;
      scale_dkp    c = log2e / sqrt(DKP);                                 l_norescale  the denominator is not rescaled on the cold path;
      dirswap      queries taken from the direction's own modality;       headoff   K of head h against V of head h + 1;
      lastq        the last row of a ragged query tile is not written (stays NaN)."""
    assert defect is None or defect in ATTN_DEFECTS
    dk = C // heads
    dkp = attn_dkp(dk, form)
    den = attn_den(dk, form, dt)
    cf = torch.tensor(attn_scale(dkp if defect == "scale_dkp" else dk), dtype=F32)
    defer = torch.tensor(ATTN_DEFER, dtype=F32) / cf if dt != F32 else torch.tensor(0.0)
    q, k, v = (t.to(dt).float() for t in _attn_split(qkv, B, N, C, heads))
    if defect != "dirswap":
        q = q.flip(0)
    if defect == "headoff":
        v = v.roll(-1, 2)
    if defect == "vtperm":
        v = v.clone()
        v[:, :, :, [21, 26]] = v[:, :, :, [26, 21]]
    NP = (N + 31) // 32 * 32
    nkt = NP // 32
    pad = lambda t: torch.cat((t, torch.zeros((*t.shape[:3], NP - N, dk))), 3)
    q, k, v = pad(q), pad(k), pad(v)
    s = q @ k.transpose(-1, -2)                                    # (2, B, heads, NP, NP); exact on integer data in any order
    if defect != "nomask":
        s[..., N:] = float("-inf")
    m = torch.full((2, B, heads, NP, 1), float("-inf"))
    l = torch.zeros_like(m)
    acc = torch.zeros((2, B, heads, NP, dk))
    for kt in range(nkt):
        st, vt = s[..., kt * 32:(kt + 1) * 32], v[:, :, :, kt * 32:(kt + 1) * 32]
        tmax = st.amax(-1, keepdim=True)
        vote = (tmax > m + defer).reshape(2, B, heads, nkt, 32).any(-1, keepdim=True).expand(2, B, heads, nkt, 32).reshape(m.shape)
        m_new = torch.where(vote, torch.maximum(m, tmax), m)
        alpha = torch.where(vote, torch.exp2((m - m_new) * cf), torch.ones_like(m))
        if defect != "l_norescale":
            l = l * alpha
        acc = acc * alpha
        m = m_new
        mc = m * cf
        p = torch.exp2(fma32(float(cf), st, -mc.expand_as(st)))
        pr = p.to(dt).float()
        acc = acc + pr @ vt
        l = l + (p if den == "valu" else pr).sum(-1, keepdim=True)
    out = (acc * (1.0 / l))[:, :, :, :N].to(dt)
    if defect == "lastq" and N % 32:
        out[:, :, :, N - 1] = float("nan")
    return _attn_join(out)


def attn_bound(family, ref, N, dk, form, dt):
    """(fp64 reference, per-element bound or None for "bit for bit") of one launch of `family`."""
    if family == "graded":
        return ref["out"], attn_graded_bound(ref, N, dk, form, dt)
    return ref.double(), attn_select_bound(ref, dt) if family == "select" else attn_uniform_bound(ref, N, dt)


def attn_ratio(family, got, ref, N, dk, form, dt):
    """Largest err / budget of one launch, for the record; where the check is bit for bit the budget is half a unit of the type, so anything
    but 0 fails."""
    r64, bound = attn_bound(family, ref, N, dk, form, dt)
    return budget_ratio(got, r64, bound if bound is not None else 0.5 * ulp(r64, dt))


def check_attention(family, got, ref, N, dk, form, dt, what):
    """The check of one launch of `family` ("select": ref = expected tensor; "uniform": ref = the mean; "graded": ref = attn_ref64()).
    Returns the largest err / budget (0 stands for bit-identical)."""
    if family == "graded":
        return assert_budget(got, ref["out"], attn_graded_bound(ref, N, dk, form, dt), what, signed=False)
    bound = attn_select_bound(ref, dt) if family == "select" else attn_uniform_bound(ref, N, dt)
    if bound is None:
        assert_same_bits(got, rne(ref.double(), dt) + 0.0, what)
        return 0.0
    return assert_budget(got, ref.double(), bound, what, signed=False)
