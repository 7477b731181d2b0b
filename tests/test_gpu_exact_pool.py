"""Exact and poisoned-buffer tests of the kernels around the convolutions: icaf_dmff_pool_tokens and icaf_dmff_upsample_merge (dmff.hip),
icaf_upsample_nearest, icaf_copy_channels, icaf_axpby, icaf_preprocess_nchw and icaf_preprocess_u8 (pool.hip).

Every comparison is with an fp64 reference computed on the CPU (tests/numerics.py): bit for bit where every device step is exact (copies,
membership probes, lattice data at power-of-two areas and dyadic ratios), within a counted fp32 budget plus half a unit of the storage
type otherwise.  Every output is a NaN-prefilled view with NaN around it, every input a view with +Inf / NaN around it; after each launch
the surroundings of every buffer are compared bitwise, and the result must equal bit for bit that of a run whose surroundings hold ordinary
numbers.  The only device-with-device comparison is "index64 gives the same bits", on top of the fp64 check.

(a) every instantiation of the token pooling — read back through ops.dmff_pool_config and closed by a test that fails if one of the seven was
    never reached; (b) upsample_merge at exact ratios, clamped corners and non-dyadic ratios; (c) the pool.hip kernels at every scale, vector
    count and layout; (d) the argument checks.  One case per kernel has more than 2^20 vector items, so the second pass of the grid-stride
    loop runs.  Every test prints the largest err / budget before it asserts (`-s`); docs/HISTORY.md section 19 records them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm                                   # noqa: E402
from numerics import BF16, F16, F32                     # noqa: E402
from helpers import lib_option                          # noqa: E402
from icafusion_amd import ops                           # noqa: E402
from icafusion_amd._lib import IcafError                # noqa: E402

DEV = "cuda:0"
DTYPES = [F32, BF16, F16]
DT_ID = {F32: "f32", BF16: "bf16", F16: "f16"}
SEVEN = {(nm.ELEM, 0, 0)} | {(nm.ROWS, r, t) for r in (4, 8, 12) for t in (1, 2)}
REACHED = {}                                            # (kernel, R, TR) -> first "name dtype" that ran it
INDEX64_RAN = set()                                     # kernels whose 64-bit-index instantiation ran
RATIOS = {}                                             # (kernel, dtype) -> largest err / budget


def run(launch):
    launch(ops.current_stream_ptr())
    torch.cuda.synchronize()


def note(kernel, dt, ratio):
    RATIOS[(kernel, DT_ID[dt])] = max(RATIOS.get((kernel, DT_ID[dt]), 0.0), ratio)


def plain_bits(dt):
    return int(nm.bits(torch.tensor([7.0], dtype=dt))[0])


def act_in(x, dt, poison, extra=0, nan=False):
    """CPU fp32 NHWC -> device view in `dt` inside a wider buffer: +Inf (or NaN) around it under `poison`, 7.0 otherwise; `extra` more
    vectors behind it (a different ld)."""
    v = nm.VEC[dt]
    fill = (nm.NAN_BITS[dt] if nan else nm.INF_BITS[dt]) if poison else plain_bits(dt)
    return nm.Poisoned(x.shape[:-1], x.shape[-1], dt, DEV, fill, x.to(dt).to(DEV), hi=v * (1 + extra) + (-x.shape[-1]) % v)


def act_out(lead, C, dt, lo=None, hi=None):
    return nm.Poisoned(lead, C, dt, DEV, nm.NAN_BITS[dt], lo=lo, hi=hi)


# ------------------------------------------------------------------------------------------------------------------------------------
# (a) token pooling
# ------------------------------------------------------------------------------------------------------------------------------------
class PoolCase:
    """Operands and fp64 references of one (geometry, dtype): probes and lattice data for both modalities."""

    def __init__(self, name, dt):
        self.name, self.dt = name, dt
        self.B, self.H, self.W, self.C, self.geom, self.want, self.flags = nm.POOL_GEOMS[name]
        self.N = self.geom[0] * self.geom[1]
        self.data = {}
        if not self.flags.get("big"):
            self.data["probes"] = ([nm.pool_probes(self.B, self.H, self.W, self.C, self.geom, g) for g in range(2)],
                                   [torch.zeros((self.N, self.C))] * 2)
        lat = [nm.pool_lattice(self.B, self.H, self.W, self.C, self.N, nm.shape_seed(name, dt, g)) for g in range(2)]
        self.data["lattice"] = ([x for x, _ in lat], [p for _, p in lat])
        self._dev, self._stats = {}, {}

    def operands(self, kind, poison):
        """Device operands, built once per (kind, poison): rgb and ir with different pixel strides, pos inside guarded flat buffers."""
        if (kind, poison) not in self._dev:
            xs, ps = self.data[kind]
            fea = [act_in(xs[0], self.dt, poison), act_in(xs[1], self.dt, poison, extra=1, nan=True)]
            assert fea[0].view.stride(2) != fea[1].view.stride(2)
            pos = [nm.PoisonedFlat((self.N * self.C,), F32, DEV, nm.NAN_BITS[F32] if poison else 0x40E00000, p.reshape(-1).to(DEV)) for p in ps]
            self._dev[(kind, poison)] = (fea, pos)
        return self._dev[(kind, poison)]

    def launch(self, kind, ws, poison=True):
        fea, pos = self.operands(kind, poison)
        tok = nm.PoisonedFlat((2, self.B * self.N, self.C), self.dt, DEV, nm.NAN_BITS[self.dt])
        run(ops.dmff_pool_tokens(fea[0].view, fea[1].view, pos[0].view, pos[1].view, tok.view, *self.geom, ws[0], ws[1]))
        return tok

    def check(self, tok, kind, ws, what):
        """Tokens of both modalities against the fp64 reference; the surroundings of every buffer intact.  Returns the largest err / budget."""
        xs, ps = self.data[kind]
        got = tok.view.cpu().reshape(2, self.B, self.N, self.C)
        worst = 0.0
        for g in range(2):
            if (kind, g) not in self._stats:
                self._stats[(kind, g)] = nm.pool_stats64(xs[g], self.geom)
            avg, mx, ref = nm.pool64(xs[g], self.geom, ws[g], ps[g], self._stats[(kind, g)])
            if kind == "lattice":
                nm.assert_rounding_exercised(ref, self.dt, f"{what} g{g} w={ws[g]}")
            worst = max(worst, nm.check_pool(got[g], avg, mx, ref, ws[g], ps[g], self.geom, self.dt, f"{what} g{g} w={ws[g]}"))
        tok.assert_outside_intact(what + ": tokens")
        for p in self.operands(kind, True)[0] + self.operands(kind, True)[1]:
            p.assert_outside_intact(what + ": input")
        return worst

    def all_launches(self, what):
        """Probes through the max and the sum path of both modalities, lattice data with both weight pairs on both modalities, and the
        last launch again with unpoisoned surroundings: same bits."""
        worst = 0.0
        plans = [("lattice", (nm.W_DYADIC, nm.W_REAL))]
        if "probes" in self.data:                                                      # (not the case of tens of MB)
            plans.append(("lattice", (nm.W_REAL, nm.W_DYADIC)))
            plans = [("probes", ((0.0, 1.0), (1.0, 0.0))), ("probes", ((1.0, 0.0), (0.0, 1.0)))] + plans
        for kind, ws in plans:
            tok = self.launch(kind, ws)
            worst = max(worst, self.check(tok, kind, ws, f"{what} {kind}"))
        nm.assert_same_bits(self.launch(*plans[-1], poison=False).view, tok.view, what + ": poisoned vs ordinary surroundings")
        return worst


def pool_config(case):
    c = ops.dmff_pool_config(case.dt, case.B, case.H, case.W, case.C, *case.geom)
    return (c["kernel"], c["R"], c["TR"]), c["index64"]


POOL_PARAMS = [pytest.param(n, dt, id=f"{n}-{DT_ID[dt]}") for n in nm.POOL_GEOMS for dt in DTYPES]


@pytest.mark.parametrize("name,dt", POOL_PARAMS)
def test_pool_tokens_every_instantiation(name, dt):
    case = PoolCase(name, dt)
    inst, idx64 = pool_config(case)
    assert inst == case.want[dt] and idx64 == 0, f"{name} {DT_ID[dt]}: the library picks {inst}, the table names {case.want[dt]}"
    ratio = case.all_launches(f"pool {name} {DT_ID[dt]} {inst}")
    REACHED.setdefault(inst, f"{name} {DT_ID[dt]}")
    note("pool_tokens " + ("rows" if inst[0] else "element"), dt, ratio)
    print(f"\n[pool] {name} {DT_ID[dt]}: instantiation {inst}, largest err / budget {ratio:.3f}")


@pytest.mark.parametrize("dt", DTYPES, ids=list(DT_ID.values()))
def test_pool_tokens_launch_choice_at_the_thresholds(dt):
    """Readback only: two token rows per workgroup need 2 * B * ceil(th / 2) >= 256 workgroups (256 and 254, two geometries each); the fp32
    token row of 512 channels x 40 columns is exactly 160 KB and stays on the rows kernel, one more column leaves it."""
    for (B, H, W, C, geom), tr in nm.TR_THRESHOLD:
        c = ops.dmff_pool_config(dt, B, H, W, C, *geom)
        assert (c["kernel"], c["R"], c["TR"]) == (nm.ROWS, 4, tr), (B, geom, c)
    for name in ("f32edge", "f32over"):
        B, H, W, C, geom, want, _ = nm.POOL_GEOMS[name]
        c = ops.dmff_pool_config(dt, B, H, W, C, *geom)
        assert (c["kernel"], c["R"], c["TR"]) == want[dt], (name, c)


@pytest.mark.parametrize("name,dt", [pytest.param(n, dt, id=f"{n}-{DT_ID[dt]}") for n, g in nm.POOL_GEOMS.items() if g[6].get("idx64") for dt in DTYPES])
def test_pool_tokens_index64_instantiation(name, dt):
    """pool_tokens_kernel<DT, false> (64-bit divisions instead of FastDiv) through the probe knob: the same fp64 checks, and the same bits as
    the 32-bit instantiation."""
    case = PoolCase(name, dt)
    ws = (nm.W_DYADIC, nm.W_REAL)
    base = case.launch("lattice", ws)
    with lib_option("index64", 1):
        assert pool_config(case) == ((nm.ELEM, 0, 0), 1)
        ratio = case.all_launches(f"pool index64 {name} {DT_ID[dt]}")
        got = case.launch("lattice", ws)
    assert pool_config(case) == ((nm.ELEM, 0, 0), 0)
    nm.assert_same_bits(got.view, base.view, f"pool index64 {name} {DT_ID[dt]}: 64- vs 32-bit index")
    INDEX64_RAN.add("pool_tokens")
    note("pool_tokens element index64", dt, ratio)


def test_every_pooling_instantiation_was_reached():
    """Closing test of (a): the element kernel and rows<R, TR> for R in {4, 8, 12} x TR in {1, 2} each ran in at least one dtype."""
    if not REACHED:
        pytest.fail("run together with test_pool_tokens_every_instantiation (same process): nothing was recorded")
    print("\n[coverage] " + ", ".join(f"{k}: {v}" for k, v in sorted(REACHED.items())))
    assert set(REACHED) == SEVEN, f"never reached: {sorted(SEVEN - set(REACHED))}"


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) upsample_merge
# ------------------------------------------------------------------------------------------------------------------------------------
MERGE_LAYOUTS = {"x2": ((None, None), (0, "v")), "16to40": ((None, None), (0, "v"))}      # (lo, hi) of the output; (0, one vector): ldo = 2C + vector


@pytest.mark.parametrize("name,dt", [pytest.param(n, dt, id=f"{n}-{DT_ID[dt]}") for n in nm.MERGE_GEOMS for dt in DTYPES])
def test_upsample_merge(name, dt):
    B, H, W, C, th, tw, exact = nm.MERGE_GEOMS[name]
    tok, fea = nm.merge_lattice(dt, B, H, W, C, th, tw, nm.shape_seed("merge" + name, dt))
    ref, bound = nm.merge64(tok, fea, dt, need_bound=not exact)
    share = nm.assert_rounding_exercised(ref, dt, f"merge {name}")
    v = nm.VEC[dt]

    def operands(poison):
        t = nm.PoisonedFlat((2, B * th * tw, C), dt, DEV, nm.NAN_BITS[dt] if poison else plain_bits(dt), tok.reshape(2, -1, C).to(dt).to(DEV))
        return t, act_in(fea[0], dt, poison), act_in(fea[1], dt, poison, extra=1, nan=True)

    t, f0, f1 = operands(True)
    assert f0.view.stride(2) != f1.view.stride(2)
    worst, gots = 0.0, []
    for lo, hi in MERGE_LAYOUTS.get(name, ((None, None),)):
        out = act_out((B, H, W), 2 * C, dt, lo, v if hi == "v" else hi)
        what = f"merge {name} {DT_ID[dt]} ldo {out.view.stride(2)}"
        run(ops.dmff_upsample_merge(t.view, f0.view, f1.view, out.view, th, tw))
        gots.append(out.view.cpu())
        ratio = 0.0 if exact else nm.budget_ratio(gots[-1], ref, bound)
        print(f"\n[merge] {what}: {'bits' if exact else f'err / budget {ratio:.3f}'}, not representable {share:.3f}")
        worst = max(worst, ratio)
        nm.check_merge(gots[-1], ref, bound, exact, dt, what)
        for p in (out, t, f0, f1):
            p.assert_outside_intact(what)
    t2, g0, g1 = operands(False)
    out2 = act_out((B, H, W), 2 * C, dt)
    run(ops.dmff_upsample_merge(t2.view, g0.view, g1.view, out2.view, th, tw))
    nm.assert_same_bits(out2.view.cpu(), gots[0], what + ": poisoned vs ordinary surroundings")
    note("upsample_merge", dt, worst)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) pool.hip
# ------------------------------------------------------------------------------------------------------------------------------------
def patterns(dt, shape, seed):
    """Random finite bit patterns of the type (subnormals and -0 included): a copy must return them bit for bit."""
    vals = nm.all_finite_patterns(dt) if dt != F32 else nm.f32_sweep_grid()
    idx = torch.randint(0, vals.numel(), shape, generator=torch.Generator().manual_seed(seed))
    return vals[idx]


NEAREST_CASES = [(2, 5, 7, "v", 1), (2, 5, 7, 64, 1), (2, 5, 7, "v", 2), (1, 6, 5, 64, 2), (2, 5, 7, "v", 3), (1, 4, 9, 64, 3), (1, 3, 5, "v", 4),
                 (2, 5, 3, 64, 4), (8, 40, 40, 256, 2)]           # the last: 8 * 80 * 80 * nv = 1,638,400 (16 bit) vectors


def nearest_once(x, scale, dt, poison, what):
    B, H, W, C = x.shape
    v = nm.VEC[dt]
    xa = nm.Poisoned((B, H, W), C, dt, DEV, nm.INF_BITS[dt] if poison else plain_bits(dt), x.to(DEV))
    y = act_out((B, H * scale, W * scale), C, dt, lo=2 * v, hi=v)                  # the middle slice of a wider buffer
    run(ops.upsample_nearest(xa.view, y.view, scale))
    nm.assert_same_bits(y.view.cpu(), nm.nearest64(x, scale), what)
    y.assert_outside_intact(what + ": output")
    xa.assert_outside_intact(what + ": input")
    return y


@pytest.mark.parametrize("dt", DTYPES, ids=list(DT_ID.values()))
@pytest.mark.parametrize("case", NEAREST_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-s{c[4]}")
def test_upsample_nearest(case, dt):
    B, H, W, C, scale = case
    C = nm.VEC[dt] if C == "v" else C
    x = patterns(dt, (B, H, W, C), 100 * H + scale)
    what = f"nearest {case} {DT_ID[dt]}"
    y = nearest_once(x, scale, dt, True, what)
    nm.assert_same_bits(nearest_once(x, scale, dt, False, what).view, y.view, what + ": poisoned vs ordinary surroundings")
    if B * H * W * C < 100000:                                                    # the small cases again with 64-bit index arithmetic
        with lib_option("index64", 1):
            y64 = nearest_once(x, scale, dt, True, what + " index64")
        nm.assert_same_bits(y64.view, y.view, what + ": 64- vs 32-bit index")
        INDEX64_RAN.add("upsample_nearest")


def test_both_index64_kernels_ran():
    if not INDEX64_RAN:
        pytest.fail("run together with the index64 tests (same process): nothing was recorded")
    assert INDEX64_RAN == {"pool_tokens", "upsample_nearest"}, INDEX64_RAN


@pytest.mark.parametrize("dt", DTYPES, ids=list(DT_ID.values()))
@pytest.mark.parametrize("shape", [(2, 9, 11, 24), (1, 3, 5, "v"), (8, 80, 80, 256)], ids=["small", "one-vector", "second-pass"])
def test_copy_channels(shape, dt):
    v = nm.VEC[dt]
    shape = tuple(v if s == "v" else s for s in shape)
    x = patterns(dt, shape, 7 + shape[1])
    xa = nm.Poisoned(shape[:3], shape[3], dt, DEV, nm.INF_BITS[dt], x.to(DEV), lo=v, hi=2 * v)
    y = act_out(shape[:3], shape[3], dt, lo=3 * v, hi=v)
    assert xa.view.stride(2) != y.view.stride(2)
    run(ops.copy_channels(xa.view, y.view))
    nm.assert_same_bits(y.view.cpu(), x, f"copy {shape} {DT_ID[dt]}")
    y.assert_outside_intact("copy: output")
    xa.assert_outside_intact("copy: input")


AXPBY_SHAPES = {"small": (2, 9, 11, 24), "one-vector": (1, 5, 3, "v"), "second-pass": (8, 80, 80, 256)}


@pytest.mark.parametrize("dt", DTYPES, ids=list(DT_ID.values()))
@pytest.mark.parametrize("shape", AXPBY_SHAPES.values(), ids=AXPBY_SHAPES.keys())
def test_axpby(shape, dt):
    """(128, -127) — the reference's Add with weight = channel count — and (0.5, 0.25) on integer data: bits; (0.4, 0.7): counted budget."""
    v = nm.VEC[dt]
    shape = tuple(v if s == "v" else s for s in shape)
    x0, x1 = nm.axpby_lattice(dt, shape, 71 + shape[1])
    a0 = nm.Poisoned(shape[:3], shape[3], dt, DEV, nm.INF_BITS[dt], x0.to(DEV), lo=v, hi=v)
    a1 = nm.Poisoned(shape[:3], shape[3], dt, DEV, nm.NAN_BITS[dt], x1.to(DEV), lo=2 * v, hi=v)
    p0 = nm.Poisoned(shape[:3], shape[3], dt, DEV, plain_bits(dt), x0.to(DEV), lo=v, hi=v)
    p1 = nm.Poisoned(shape[:3], shape[3], dt, DEV, plain_bits(dt), x1.to(DEV), lo=2 * v, hi=v)
    for a, b, exact in ((128.0, -127.0, True), (0.5, 0.25, True), (0.4, 0.7, False)):
        what = f"axpby {shape} ({a}, {b}) {DT_ID[dt]}"
        ref, bound = nm.axpby64(x0, x1, a, b, dt)
        if a != 0.5:                                                              # (halves and quarters of small integers fit every type: that pair checks the scaling alone)
            nm.assert_rounding_exercised(ref, dt, what)
        y = act_out(shape[:3], shape[3], dt, lo=0, hi=4 * v)
        assert len({a0.view.stride(2), a1.view.stride(2), y.view.stride(2)}) == 3
        run(ops.axpby(a0.view, a1.view, y.view, a, b))
        got = y.view.cpu()
        ratio = nm.budget_ratio(got, ref, bound)
        print(f"\n[axpby] {what}: err / budget {ratio:.3f}")
        note("axpby", dt, ratio)
        if exact:
            nm.assert_same_bits(got, nm.rne(ref, dt) + 0.0, what)
        else:
            nm.assert_budget(got, ref, bound, what, signed=False)
        for p in (y, a0, a1):
            p.assert_outside_intact(what)
        y2 = act_out(shape[:3], shape[3], dt, lo=0, hi=4 * v)
        run(ops.axpby(p0.view, p1.view, y2.view, a, b))
        nm.assert_same_bits(y2.view, y.view, what + ": poisoned vs ordinary surroundings")


def cpads(dt, C, mode):
    v = nm.VEC[dt]
    least = -(-(4 * C if mode else C) // v) * v
    return least, least + v


@pytest.mark.parametrize("dt", DTYPES, ids=list(DT_ID.values()))
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("C", [1, 3])
def test_preprocess_nchw(C, mode, dt):
    """fp32 NCHW images -> NHWC / space-to-depth in `dt`: RNE of every value, channel padding +0 bit for bit (Cpad of one / two vectors at
    C = 1, more at C = 3)."""
    B, H, W = 2, 10, 14
    img = torch.rand((B, C, H, W), generator=torch.Generator().manual_seed(40 + C)) * 2.0 - 0.5
    ia = nm.PoisonedFlat(img.shape, F32, DEV, nm.NAN_BITS[F32], img.to(DEV))
    for cpad in cpads(dt, C, mode):
        want = nm.stage64(img, mode, cpad)
        nm.assert_rounding_exercised(want[..., :C], dt, f"preprocess C={C} mode {mode}")
        out = nm.PoisonedFlat(tuple(want.shape), dt, DEV, nm.NAN_BITS[dt])
        run(ops.preprocess(ia.view, out.view, mode))
        what = f"preprocess_nchw C={C} mode {mode} Cpad {cpad} {DT_ID[dt]}"
        nm.assert_same_bits(out.view.cpu(), nm.rne(want, dt), what)               # (+0 in the padding: stage64 holds 0.0 there)
        out.assert_outside_intact(what + ": output")
        ia.assert_outside_intact(what + ": input")


@pytest.mark.parametrize("dt", DTYPES, ids=list(DT_ID.values()))
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("c0", [0, 2])
def test_preprocess_u8(c0, mode, dt):
    """uint8 NCHW (8 channels) -> two streams of three channels from c0 on: every level 0 .. 255 appears in every channel; the expected
    value is RNE_dt of the fp32 quotient v / 255; padding +0."""
    B, H, W, ctot = 2, 16, 16, 8
    lv = torch.arange(H * W)
    img = torch.stack([torch.stack([(lv * (2 * c + 3) + 37 * c + 11 * b) % 256 for c in range(ctot)]) for b in range(B)]).to(torch.uint8).reshape(B, ctot, H, W)
    assert all(len(img[b, c].unique()) == 256 for b in range(B) for c in range(ctot))
    ia = nm.PoisonedFlat(img.shape, torch.uint8, DEV, 0xFF, img.to(DEV))
    table = nm.u8_expected(dt)
    for cpad in cpads(dt, 3, mode):
        streams = [img[:, c0 + 3 * s:c0 + 3 * s + 3] for s in range(2)]
        want = torch.stack([table[nm.stage64(s.float(), mode, cpad).long()] for s in streams])
        assert not bool(nm.bits(want[..., 12 if mode else 3:]).any())               # the padding: +0
        out = nm.PoisonedFlat(tuple(want.shape), dt, DEV, nm.NAN_BITS[dt])
        run(ops.preprocess_u8(ia.view, out.view, mode, c0=c0))
        what = f"preprocess_u8 c0={c0} mode {mode} Cpad {cpad} {DT_ID[dt]}"
        nm.assert_same_bits(out.view.cpu(), want, what)
        out.assert_outside_intact(what + ": output")
        ia.assert_outside_intact(what + ": input")


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) argument checks: IcafError with its message, nothing launched
# ------------------------------------------------------------------------------------------------------------------------------------
def refused(fn, args, message, outputs):
    st = fn(*args, ops.current_stream_ptr())
    torch.cuda.synchronize()
    assert st != 0, "the call was accepted"
    assert message in ops.lib().icaf_last_error().decode(), ops.lib().icaf_last_error().decode()
    for o in outputs:
        nm.assert_same_bits(o.buf, o.before, "a refused call must not write")


@pytest.mark.parametrize("dt", DTYPES, ids=list(DT_ID.values()))
def test_argument_checks(dt):
    v, C, code = nm.VEC[dt], 32, ops.dtype_code(dt)
    B, H, W = 1, 9, 11
    x, pos = nm.pool_lattice(B, H, W, C, 63, 1)
    f0, f1 = act_in(x, dt, True), act_in(x, dt, True, extra=1)
    p = pos.reshape(-1).to(DEV)
    tok = nm.PoisonedFlat((2, 63, C), dt, DEV, nm.NAN_BITS[dt])
    with pytest.raises(IcafError, match="window exceeds the feature map"):         # kh 4: (7 - 1) * 1 + 4 > 9
        run(ops.dmff_pool_tokens(f0.view, f1.view, p, p, tok.view, 7, 9, 4, 3, 1, 1, nm.W_REAL, nm.W_REAL))
    with pytest.raises(IcafError, match="window exceeds the feature map"):
        run(ops.dmff_pool_tokens(f0.view, f1.view, p, p, tok.view, 7, 9, 3, 4, 1, 1, nm.W_REAL, nm.W_REAL))
    lib = ops.lib()
    pool_args = lambda c: (f0.view.data_ptr(), f0.view.stride(2), f1.view.data_ptr(), f1.view.stride(2), p.data_ptr(), p.data_ptr(), tok.view.data_ptr(),
                           code, B, H, W, c, 7, 9, 3, 3, 1, 1, 0.4, 0.7, 0.4, 0.7)
    refused(lib.icaf_dmff_pool_tokens, pool_args(C - v // 2), f"multiples of {v}", [tok])
    nm.assert_same_bits(tok.buf, tok.before, "refused pooling launches wrote tokens")
    out = act_out((B, H, W), 2 * C, dt)
    merge_args = lambda c, ldo: (tok.view.data_ptr(), f0.view.data_ptr(), f0.view.stride(2), f1.view.data_ptr(), f1.view.stride(2), out.view.data_ptr(), ldo,
                                 code, B, H, W, c, 7, 9)
    refused(lib.icaf_dmff_upsample_merge, merge_args(C, 2 * C - v), "bad strides", [out])           # ldo < 2C
    refused(lib.icaf_dmff_upsample_merge, merge_args(C - v // 2, out.view.stride(2)), "bad strides", [out])
    y = act_out((B, H, W), C, dt)
    up_args = lambda c, scale: (f0.view.data_ptr(), f0.view.stride(2), y.view.data_ptr(), y.view.stride(2), code, B, H, W, c, scale)
    refused(lib.icaf_upsample_nearest, up_args(C, 0), "bad geometry", [y])                          # scale < 1
    refused(lib.icaf_upsample_nearest, up_args(C, -2), "bad geometry", [y])
    refused(lib.icaf_upsample_nearest, up_args(C - v // 2, 1), "bad geometry", [y])
    refused(lib.icaf_axpby, (f0.view.data_ptr(), f0.view.stride(2), f1.view.data_ptr(), f1.view.stride(2), y.view.data_ptr(), y.view.stride(2), code,
                             B * H * W, C - v // 2, 0.5, 0.5), f"multiples of {v}", [y])
    refused(lib.icaf_copy_channels, (f0.view.data_ptr(), f0.view.stride(2), y.view.data_ptr(), y.view.stride(2), code, B * H * W, C - v // 2),
            f"multiples of {v}", [y])
    for H_, W_ in ((9, 10), (10, 9)):                                                               # space-to-depth of an odd map
        img = torch.zeros((1, 3, H_, W_), device=DEV)
        o = nm.PoisonedFlat((1, H_ // 2, W_ // 2, 16), dt, DEV, nm.NAN_BITS[dt])
        with pytest.raises(IcafError, match="space-to-depth needs even H, W"):
            run(ops.preprocess(img, o.view, 1))
        u8 = torch.zeros((1, 6, H_, W_), dtype=torch.uint8, device=DEV)
        o2 = nm.PoisonedFlat((2, 1, H_ // 2, W_ // 2, 16), dt, DEV, nm.NAN_BITS[dt])
        with pytest.raises(IcafError, match="space-to-depth needs even H, W"):
            run(ops.preprocess_u8(u8, o2.view, 1))
        nm.assert_same_bits(o.buf, o.before, "refused staging wrote")
        nm.assert_same_bits(o2.buf, o2.before, "refused staging wrote")
    for b in (f0, f1):
        b.assert_outside_intact("argument checks: inputs")


def test_largest_ratios():
    """Prints the table of docs/HISTORY.md section 19."""
    print("\n[ratios] " + "; ".join(f"{k[0]} {k[1]}: {v:.3f}" for k, v in sorted(RATIOS.items())))
