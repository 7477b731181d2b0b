"""Exact-lattice, activation-sweep and poisoned-buffer tests of the convolution kernels (igemm / igemm_stream / igemm_wreg / cwide /
cstream / ctile / stem and the shared epilogue of conv_common.h), and LayerNorm on rows whose statistics are exact.

(a) every launch configuration `ops.conv_candidates` offers for a list of layer shapes — plus the ids it never offers (29, 31 - 34) —
    runs on LATTICE data (tests/numerics.py): without an activation the output must equal the expected bits, with SiLU / GELU every
    element must lie within half a unit of the output type plus the counted fp32 budget of the activation.  A closing test checks that
    the configurations reached contain every id of every kernel family.
(b) every finite 16-bit pattern (fp32: a grid holding them and the bf16 midpoints) goes through an identity convolution and each
    activation, once per epilogue code path.
(c) a subset re-runs with NaN-prefilled outputs and NaN / Inf-poisoned surroundings of every view.
icaf_bottleneck, icaf_stem2 and the chained / C3-tail launches apply SiLU between their stages, so their second stage never sees exact
operands; the existing "equals two launches" bit tests tie them to the single launches checked here.  The chained launch appears in (c)
for its store paths (y2, chain_keep) and is compared there with the two launches it replaces.  The DMFF block kernels — the shared LayerNorm
inside icaf_dmff_wide_proj_mlp included, on rows whose statistics are exact by choice of eps — have their gate in tests/test_gpu_exact_dmff.py.
The kernels around the convolutions — token pooling, bilinear merge, nearest resize, channel copy, axpby and the two staging kernels —
have the same kind of gate in tests/test_gpu_exact_pool.py (every pooling instantiation read back through ops.dmff_pool_config, the
second pass of the grid-stride loops, the 64-bit-index instantiations through the probe knob index64).

Every test prints the largest err / budget it saw before it asserts (`-s`); docs/HISTORY.md section 17 records them."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import numerics as nm                                   # noqa: E402
from numerics import ACT_GELU, ACT_NONE, ACT_SILU, BF16, F16, F32      # noqa: E402
from icafusion_amd import ops                           # noqa: E402
from icafusion_amd._lib import IcafError                # noqa: E402

DEV = "cuda:0"
DTYPES = [F32, BF16, F16]
DT_ID = {F32: "f32", BF16: "bf16", F16: "f16"}
ACT_NAME = {ACT_NONE: "none", ACT_SILU: "silu", ACT_GELU: "gelu"}
# every launch configuration that is built (icaf.h: icaf_conv_args.tile), by kernel-name prefix
REQUIRED = {"igemm_dma64x3": {1, 2, 3, 4}, "igemm_reg": {11, 12, 13, 14}, "igemm_dma128x2": {21, 22, 23, 24, 25, 26, 28, 29},
            "igemm_dma128x3": {31, 32, 33, 34}, "igemm_stream": {51, 52}, "igemm_wreg": {61, 62, 63, 64, 65, 66}, "cstream": {71},
            "cwide": {81, 82, 83, 84, 85}, "ctile": {41, 42, 43, 44, 45}}
RAN = {}                                                # tile id -> kernel name, filled by the tests of (a)
RATIOS = {}                                             # (family, act, dtype) -> largest err / budget


def family(name):
    return max((p for p in REQUIRED if name.startswith(p)), key=len)


def run(launch):
    launch(ops.current_stream_ptr())
    torch.cuda.synchronize()


def nhwc(t, dt):
    """CPU NCHW fp32 -> CPU NHWC `dt` (exact on the lattice)."""
    return t.permute(0, 2, 3, 1).contiguous().to(dt)


def stack(ts):
    return ts[0] if len(ts) == 1 else torch.stack(ts)


class Case:
    """Device operands and CPU references of one (shape, dtype): built once, reused for every activation, residual and configuration."""

    def __init__(self, name, dt, poison=False, pre=False):
        self.name, self.dt, self.poison = name, dt, poison
        if pre:
            B, H, W, cin, cout, self.pre_hw, self.nearest = nm.PRE_SHAPES[name]
            k, s, p, flags = 1, 1, 0, {}
        else:
            B, H, W, cin, cout, k, s, p, flags = nm.EXACT_SHAPES[name]
            self.pre_hw, self.nearest = None, False
        self.B, self.H, self.W, self.cin, self.cout, self.k, self.s, self.p, self.flags = B, H, W, cin, cout, k, s, p, flags
        self.pair, self.g2 = bool(flags.get("pair")), bool(flags.get("groups2"))
        self.G = 2 if (self.pair or self.g2) else 1
        self.Ho, self.Wo = nm.out_hw(H, W, k, s, p)
        self.d = [nm.lattice(dt, B, H, W, cin, cout, k, self.Ho, self.Wo, nm.shape_seed(name, dt, g), pre_hw=self.pre_hw) for g in range(self.G)]
        self.alphas = nm.ALPHAS_G2 if self.g2 else ((nm.ALPHA_ACC, nm.ALPHA_RES),) * self.G
        self.z = [nm.ref64(d["x"], d["w"], d["bias"], s, p, ACT_NONE, pre=d["pre"], pre_nearest=self.nearest)[0] for d in self.d]
        for g, z in enumerate(self.z):
            if dt != F32:
                nm.assert_lattice_condition(z, dt, self.alphas[g][0], f"{name} {dt} group {g}")
        # device operands.  x: a channel slice of a wider buffer (ldx > Cin); under `poison` its surroundings are +Inf, else 7.0
        lead = (self.G, B, H, W) if self.G == 2 else (B, H, W)
        lead_o = (self.G, B, self.Ho, self.Wo) if self.G == 2 else (B, self.Ho, self.Wo)
        self.lead_o = lead_o
        fill_in = nm.INF_BITS[dt] if poison else int(nm.bits(torch.tensor([7.0], dtype=dt))[0])
        self.x = nm.Poisoned(lead, cin, dt, DEV, fill_in, stack([nhwc(d["x"], dt) for d in self.d]).to(DEV))
        self.res = nm.Poisoned(lead_o, cout, dt, DEV, nm.NAN_BITS[dt] if poison else fill_in, stack([nhwc(d["res"], dt) for d in self.d]).to(DEV))
        self.wp, self.kp, self.bp = ops.pack_streams([(d["w"].to(DEV), d["bias"].to(DEV)) for d in self.d], dt)
        self.pre = None
        if pre:
            # ldpre must be a multiple of 4 floats and the row 16-byte aligned: lo = 4
            self.pre = nm.Poisoned((B, *self.pre_hw), cout, F32, DEV, nm.NAN_BITS[F32] if poison else 0x40E00000,
                                   self.d[0]["pre"].permute(0, 2, 3, 1).contiguous().to(DEV))
        self._want = {}

    def output(self, out_dt):
        """A fresh NaN-prefilled output buffer wider than Cout on both sides (ldy > Cout), its surroundings NaN as well."""
        return nm.Poisoned(self.lead_o, self.cout, out_dt, DEV, nm.NAN_BITS[out_dt])

    def launch(self, y, act, use_res, tile, chain=None):
        kw = {}
        if self.g2:
            gs = dict(x=self.x.view.stride(0), w=self.wp.stride(0), bias=self.bp.stride(0), y=y.view.stride(0), res=self.res.view.stride(0))
            xa, ya, ra = self.x.view[0], y.view[0], self.res.view[0]
            kw = dict(groups=2, group_strides=gs)
        else:
            xa, ya, ra = self.x.view, y.view, self.res.view
        aa = tuple(a for a, _ in self.alphas) if self.g2 else self.alphas[0][0]
        ar = tuple(r for _, r in self.alphas) if self.g2 else self.alphas[0][1]
        if chain is not None:
            aa = 1.0                          # (the chained launch needs alpha_acc = 1 with chain_keep)
        return ops.conv2d(xa, self.wp, self.kp, self.bp, ya, self.k, self.k, self.s, self.s, self.p, self.p, self.cin, self.cout, act,
                          res=ra if use_res else None, alpha_acc=aa, alpha_res=ar, tile=tile, chain=chain,
                          pre=None if self.pre is None else self.pre.view, pre_nearest=self.nearest, **kw)

    def want(self, act, use_res, out_dt):
        """(expected bits or None, fp64 reference, bound) on the device, NHWC with the group dim in front for G = 2."""
        key = (act, use_res, out_dt)
        if key not in self._want:
            ex, ref, bnd = [], [], []
            for g, d in enumerate(self.d):
                aa, ar = self.alphas[g]
                res = d["res"] if use_res else None
                a = aa * nm.act64(self.z[g], act)
                ref.append((a + ar * res.double() if use_res else a).permute(0, 2, 3, 1))
                bnd.append(nm.launch_bound(self.z[g], act, self.dt, out_dt, res, aa, ar).permute(0, 2, 3, 1))
                if act == ACT_NONE:
                    ex.append(nm.expected_exact(self.z[g], out_dt, res, aa, ar).permute(0, 2, 3, 1))
            self._want[key] = (stack(ex).contiguous() if ex else None, stack(ref).contiguous(), stack(bnd).contiguous())
        return self._want[key]

    def check(self, y, act, use_res, out_dt, what, signed=None):
        """Bit-exact without an activation, within the counted budget with one; every surrounding byte of every view untouched."""
        ex, ref, bnd = self.want(act, use_res, out_dt)
        got = y.view.cpu()
        y.assert_outside_intact(what + ": output")
        ratio = nm.budget_ratio(got, ref, bnd)
        if ex is not None:
            nm.assert_same_bits(got, ex, what)
        else:
            nm.assert_budget(got, ref, bnd, what, signed=not use_res)
        return ratio

    def inputs_intact(self, what):
        self.x.assert_outside_intact(what + ": x")
        self.res.assert_outside_intact(what + ": res")
        if self.pre is not None:
            self.pre.assert_outside_intact(what + ": pre")


def configurations(case, act, use_res, out_dt, extra=()):
    """[(tile id, kernel name)]: every candidate of the launch the library's own check accepts, plus `extra` ids passed directly."""
    probe = case.launch(case.output(out_dt), act, use_res, 0)
    out = []
    for t in list(dict.fromkeys(ops.conv_candidates(probe.keep[0]))) + [e for e in extra]:
        if t in extra or ops.tile_valid(probe, t):
            probe.keep[0].tile = t
            out.append((t, ops.conv_kernel_name(probe)))
    return out


def extras(case, out_dt):
    ex = list(case.flags.get("extra", ()))
    if case.dt == F32 or out_dt == F32:
        ex = [t for t in ex if t not in (29, 31)]          # the 8-wavefront tiles and 128 x 128 are not built for fp32 / fp32 output
    return tuple(ex)


def acts_of(case):
    return case.flags.get("acts", nm.A3)


EXACT_PARAMS = [pytest.param(n, dt, id=f"{n}-{DT_ID[dt]}") for n, sh in nm.EXACT_SHAPES.items() for dt in DTYPES
                if not (sh[8].get("only16") and dt == F32)]


@pytest.mark.parametrize("name,dt", EXACT_PARAMS)
def test_every_launch_configuration_on_lattice_data(name, dt):
    """(a): ACT_NONE with and without residual bit for bit, SiLU / GELU within the counted budget, on every configuration of the shape."""
    case = Case(name, dt)
    out_dts = [dt] + ([F32] if (case.flags.get("f32out") and dt != F32) else [])
    failures, seen = [], 0
    for out_dt in out_dts:
        for act in acts_of(case):
            for use_res in (False, True):
                for tile, kname in configurations(case, act, use_res, out_dt, extras(case, out_dt)):
                    what = f"{name} {DT_ID[dt]}->{DT_ID[out_dt]} {ACT_NAME[act]} res={int(use_res)} tile {tile} ({kname})"
                    y = case.output(out_dt)
                    try:
                        run(case.launch(y, act, use_res, tile))
                        ratio = case.check(y, act, use_res, out_dt, what)
                    except (AssertionError, IcafError) as e:
                        failures.append(f"{what}: {str(e)[:400]}")
                        continue
                    RAN[tile] = kname
                    seen += 1
                    key = (family(kname), ACT_NAME[act], DT_ID[dt])
                    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    case.inputs_intact(name)
    print(f"\n[exact] {name} {DT_ID[dt]}: {seen} launches, configurations {sorted(RAN)}")
    assert seen > 0 and not failures, f"{len(failures)} of {seen + len(failures)} launches failed:\n" + "\n".join(failures[:12])


PRE_PARAMS = [pytest.param(n, dt, id=f"{n}-{DT_ID[dt]}") for n in nm.PRE_SHAPES for dt in DTYPES]


@pytest.mark.parametrize("name,dt", PRE_PARAMS)
def test_pre_activation_term_on_lattice_data(name, dt):
    """The bilinear `pre` term at power-of-two factors (dyadic interpolation weights) and the nearest one at any factor keep the
    pre-activation exact: SiLU within the counted budget on every configuration offered for a pre-term launch (the term is built for
    SiLU layers only), with and without residual."""
    case = Case(name, dt, poison=True, pre=True)
    failures, seen = [], 0
    for use_res in (False, True):
        cfgs = configurations(case, ACT_SILU, use_res, dt)
        assert cfgs, "no configuration carries the pre term for this shape"
        for tile, kname in cfgs:
            what = f"{name} {DT_ID[dt]} res={int(use_res)} tile {tile} ({kname})"
            y = case.output(dt)
            try:
                run(case.launch(y, ACT_SILU, use_res, tile))
                ratio = case.check(y, ACT_SILU, use_res, dt, what)
            except (AssertionError, IcafError) as e:
                failures.append(f"{what}: {str(e)[:400]}")
                continue
            seen += 1
            key = ("pre:" + family(kname), "silu", DT_ID[dt])
            RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    case.inputs_intact(name)
    print(f"\n[pre] {name} {DT_ID[dt]}: {seen} launches")
    assert not failures, f"{len(failures)} launches failed:\n" + "\n".join(failures[:12])


def status_of_both_entry_points(launch, tile):
    """(icaf_conv2d_kernel_name's status, icaf_conv2d's status) for launch configuration `tile`; the launch, if accepted, is enqueued."""
    launch.keep[0].tile = tile
    named = 0 if ops.config_valid(launch, tile) else 1
    st = launch.fn(*launch.args, ops.current_stream_ptr())
    return named, st


SMALL_SHAPES = [n for n, sh in nm.EXACT_SHAPES.items() if not sh[8].get("only16")]
TABLE_PARAMS = [pytest.param(n, dt, False, id=f"{n}-{DT_ID[dt]}") for n in SMALL_SHAPES for dt in DTYPES] + \
               [pytest.param(n, dt, True, id=f"{n}-{DT_ID[dt]}") for n in nm.PRE_SHAPES for dt in DTYPES]


@pytest.mark.parametrize("name,dt,pre", TABLE_PARAMS)
def test_kernel_name_and_launch_agree_on_every_configuration(name, dt, pre):
    """Every id of the library's table (icaf_conv2d_config_ids), offered by conv_candidates or not, on every small shape, with and without SiLU
    and residual: icaf_conv2d_kernel_name accepts exactly what icaf_conv2d accepts; what is accepted returns the expected bits (ACT_NONE) or
    stays within the counted budget (SiLU); what is rejected comes back from the host check and leaves the NaN-prefilled output unwritten."""
    case = Case(name, dt, pre=pre)
    ids = (ctypes.c_int * 64)()
    ids = ids[:ops.lib().icaf_conv2d_config_ids(ids, 64)]
    assert sorted(ids) == sorted(set().union(*REQUIRED.values()))
    failures, ran, refused = [], 0, 0
    for act in (ACT_NONE, ACT_SILU):
        for use_res in (False, True):
            for tile in ids:
                what = f"{name} {DT_ID[dt]} {ACT_NAME[act]} res={int(use_res)} tile {tile}"
                y = case.output(dt)
                launch = case.launch(y, act, use_res, tile)
                named, st = status_of_both_entry_points(launch, tile)
                torch.cuda.synchronize()
                try:
                    assert (named == 0) == (st == 0), f"name call says {named}, launch says {st}"
                    if st == 0:
                        case.check(y, act, use_res, dt, what)
                        ran += 1
                    else:
                        nm.assert_same_bits(y.buf, y.before, what + ": a rejected configuration must not write")
                        refused += 1
                except AssertionError as e:
                    failures.append(f"{what}: {str(e)[:400]}")
    case.inputs_intact(name)
    print(f"\n[table] {name} {DT_ID[dt]}: {ran} launches checked, {refused} refused by both entry points")
    assert ran > 0 and not failures, f"{len(failures)} of {ran + refused + len(failures)} cases failed:\n" + "\n".join(failures[:12])


def test_every_built_configuration_was_reached():
    """Closing test of (a): the configurations the tests above ran (RAN: id -> kernel name from ops.conv_kernel_name) contain every id
    of every family, under the name of that family.  A configuration added to the library that no shape reaches fails here."""
    if not RAN:
        pytest.fail("run together with test_every_launch_configuration_on_lattice_data (same process): nothing was recorded")
    print("\n[coverage] " + ", ".join(f"{t}:{RAN[t]}" for t in sorted(RAN)))
    for prefix, ids in REQUIRED.items():
        missing = sorted(t for t in ids if t not in RAN)
        assert not missing, f"{prefix}: launch configurations {missing} were never run"
        for t in ids:
            assert family(RAN[t]) == prefix, f"configuration {t} ran {RAN[t]}, expected a {prefix} kernel"
    print("[ratios] " + "; ".join(f"{k[0]} {k[1]} {k[2]}: {v:.3f}" for k, v in sorted(RATIOS.items())))


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) activation and rounding sweep
# ------------------------------------------------------------------------------------------------------------------------------------
def sweep_values(dt):
    return nm.all_finite_patterns(dt) if dt != F32 else nm.f32_sweep_grid()


# (kernel family, cin = cout, filter, tile id, activations, fp32 output): one configuration per epilogue code path
SWEEP_PATHS = [
    ("igemm", 64, 1, 2, nm.A3, False),                  # shared epilogue (conv_common.h), LDS-DMA pipeline
    ("igemm_reg", 64, 1, 14, nm.A3, False),             # ... from the register-staged pipeline, 64 x 64 tile
    ("igemm_f32out", 64, 1, 4, nm.A3, True),            # ... fp32 store of a 16-bit layer (gelu_fast_f seen without the 16-bit rounding)
    ("igemm_stream", 64, 1, 52, nm.A3, False),          # ... reached from the persistent streaming GEMM
    ("igemm_wreg", 128, 1, 61, nm.A3, False),           # ... and from the register-fed weights kernel
    ("ctile", 64, 3, 42, (ACT_SILU,), False),           # ctile.hip's own epilogue, centre-tap identity 3x3
    ("cstream", 64, 3, 71, (ACT_SILU,), False),         # cstream.hip
    ("cwide", 128, 3, 81, (ACT_SILU,), False),          # cwide.hip
]
SWEEP_PARAMS = [pytest.param(p, dt, id=f"{p[0]}-{DT_ID[dt]}") for p in SWEEP_PATHS for dt in DTYPES
                if dt != F32 or p[0] in ("igemm", "igemm_reg")]


@pytest.mark.parametrize("path,dt", SWEEP_PARAMS)
def test_activation_sweep_over_every_finite_pattern(path, dt):
    """(b): an identity convolution passes every value through the MFMA unchanged (1 * v = v, 0 * finite = 0), so the epilogue sees
    every finite pattern of the type.  ACT_NONE returns the input bits — subnormals included; -0 comes back as +0, which is what adding
    -0 to an accumulator that starts at +0 gives (the fp64 convolution does the same).  SiLU / GELU: half a unit of the output type plus the
    counted fp32 budget, per element, and never on the wrong side of zero."""
    fam, c, k, tile, acts, f32out = path
    out_dt = F32 if f32out else dt
    vals = sweep_values(dt)
    n = vals.numel() // c
    H = 32
    x = vals.reshape(1, H, n // H, c).contiguous().to(DEV)
    w = torch.zeros((c, c, k, k))
    w[torch.arange(c), torch.arange(c), k // 2, k // 2] = 1.0
    wp, kp = ops.pack_conv_weight(w.to(DEV), dt)
    v64 = vals.double().reshape(x.shape)
    failures = []
    for act in acts:
        y = nm.Poisoned(x.shape[:3], c, out_dt, DEV, nm.NAN_BITS[out_dt])
        what = f"sweep {fam} {DT_ID[dt]}->{DT_ID[out_dt]} {ACT_NAME[act]} tile {tile}"
        try:
            launch = ops.conv2d(x, wp, kp, None, y.view, k, k, 1, 1, k // 2, k // 2, c, c, act, tile=tile)
            assert family(ops.conv_kernel_name(launch)).startswith(fam.split("_f32")[0]), ops.conv_kernel_name(launch)
            run(launch)
            got = y.view.cpu()
            y.assert_outside_intact(what)
            ref = nm.act64(v64, act)
            bound = nm.launch_bound(v64, act, dt, out_dt)
            ratio = nm.budget_ratio(got, ref, bound)
            sub = (ref.abs() < 2.0 ** nm.EMIN[out_dt]) & (ref != 0)
            flushed = int((sub & (got.double() == 0)).sum())
            print(f"\n[sweep] {what}: err / budget {ratio:.3f}; results in the subnormal range {int(sub.sum())}, returned as zero {flushed}")
            RATIOS[("sweep:" + fam, ACT_NAME[act], DT_ID[dt])] = ratio
            if act == ACT_NONE:
                nm.assert_same_bits(got, (vals.reshape(got.shape) + 0.0).to(out_dt), what)
            else:
                nm.assert_budget(got, ref, bound, what)
        except (AssertionError, IcafError) as e:
            failures.append(f"{what}: {str(e)[:500]}")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) poisoned buffers
# ------------------------------------------------------------------------------------------------------------------------------------
POISON_SHAPES = ["ragged3x3", "ragged3x3s2", "wide1x1", "pair3x3c64", "c128", "c64s2", "c128s2", "c16", "c32s2", "detect", "groups2"]
POISON_PARAMS = [pytest.param(n, dt, id=f"{n}-{DT_ID[dt]}") for n in POISON_SHAPES for dt in DTYPES]


@pytest.mark.parametrize("name,dt", POISON_PARAMS)
def test_poisoned_buffers(name, dt):
    """(c): outputs pre-filled with NaN; every byte around the output, residual and input views poisoned (NaN around what is written or
    added, +Inf around x: a read of a neighbour channel against a zero weight would give NaN).  Every logical element must be what (a)
    expects — bit for bit without an activation — and every poisoned byte unchanged.  One configuration per kernel family of the shape,
    16-bit and fp32 stores, ragged M / N.
    Input contract (icaf.h): no launch reads a channel outside [0, Cin) of a pixel into a product; the LDS-DMA slices issued past the end
    of K land in ring stages that are never consumed."""
    case = Case(name, dt, poison=True)
    out_dts = [dt] + ([F32] if (case.flags.get("f32out") and dt != F32) else [])
    failures, seen = [], 0
    for out_dt in out_dts:
        for act in acts_of(case):
            if act == ACT_GELU:
                continue
            fams = {}
            for tile, kname in configurations(case, act, True, out_dt, extras(case, out_dt)):
                fams.setdefault(family(kname), (tile, kname))           # the first configuration of every family
            for tile, kname in fams.values():
                for use_res in (True, False):
                    what = f"poison {name} {DT_ID[dt]}->{DT_ID[out_dt]} {ACT_NAME[act]} res={int(use_res)} tile {tile} ({kname})"
                    y = case.output(out_dt)
                    try:
                        run(case.launch(y, act, use_res, tile))
                        case.check(y, act, use_res, out_dt, what)
                        case.inputs_intact(what)
                    except (AssertionError, IcafError) as e:
                        failures.append(f"{what}: {str(e)[:400]}")
                        continue
                    seen += 1
    print(f"\n[poison] {name} {DT_ID[dt]}: {seen} launches")
    assert seen > 0 and not failures, f"{len(failures)} launches failed:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_inf_inside_the_view_propagates_and_outside_does_not(dt):
    """The input contract in both directions, on the linear-walk (1x1) and the tap-walk modes of igemm and on the register-fed kernel:
    +Inf in a channel INSIDE [0, Cin) reaches exactly the outputs whose receptive field holds that pixel (weights are non-zero there);
    +Inf in every channel OUTSIDE reaches none (test_poisoned_buffers checks that for every family)."""
    for name, tiles in (("wide1x1", (1, 22, 61)), ("ragged3x3", (2, 12, 21))):
        case = Case(name, dt, poison=True)
        b, h, w_, ch = 0, 3, 4, 5
        for d in case.d:
            d["w"][:, ch] = d["w"][:, ch].abs() + 2.0 ** -nm.GRID[dt][0]         # non-zero weights on the poisoned channel
        case.wp, case.kp, case.bp = ops.pack_streams([(d["w"].to(DEV), d["bias"].to(DEV)) for d in case.d], dt)
        case.x.view[b, h, w_, ch] = float("inf")
        hit = torch.zeros((case.B, case.Ho, case.Wo), dtype=torch.bool)
        for ho in range(case.Ho):
            for wo in range(case.Wo):
                hit[b, ho, wo] = (0 <= h - (ho * case.s - case.p) < case.k) and (0 <= w_ - (wo * case.s - case.p) < case.k)
        for tile in tiles:
            y = case.output(dt)
            run(case.launch(y, ACT_NONE, False, tile))
            got = y.view.float().cpu()
            assert bool((got[hit] == float("inf")).all()), f"{name} tile {tile}: +Inf inside the view did not reach its outputs"
            assert bool(torch.isfinite(got[~hit]).all()), f"{name} tile {tile}: +Inf reached outputs outside its receptive field"


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("keep", [False, True])
def test_poisoned_chained_launch_store_paths(dt, keep):
    """The chained 1x1 (y2; y as well with chain_keep) under poison, on igemm (22), cstream (71): y2 and y are bit-identical to the two
    launches they replace, unwritten buffers keep their NaN prefill, surroundings stay intact."""
    case = Case("pair3x3c64", dt, poison=True)
    c2 = 32
    d2 = [nm.lattice(dt, 1, 1, 1, case.cout, c2, 1, 1, 1, 77 + g) for g in range(2)]
    w2p, kp2, b2p = ops.pack_streams([(d["w"].to(DEV), d["bias"].to(DEV)) for d in d2], dt)
    # two launches: the 3x3 (+ residual when kept), then the 1x1 over what it stored
    mid = nm.Poisoned(case.lead_o, case.cout, dt, DEV, nm.NAN_BITS[dt])
    case.alphas = ((1.0, 1.0),) * 2
    run(case.launch(mid, ACT_SILU, keep, 2))
    ref2 = nm.Poisoned(case.lead_o, c2, dt, DEV, nm.NAN_BITS[dt])
    run(ops.conv2d(mid.view, w2p, kp2, b2p, ref2.view, 1, 1, 1, 1, 0, 0, case.cout, c2, ACT_SILU, tile=2))
    assert bool(torch.isfinite(ref2.view.float()).all())
    for tile in (22, 71):
        y, y2 = case.output(dt), nm.Poisoned(case.lead_o, c2, dt, DEV, nm.NAN_BITS[dt])
        run(case.launch(y, ACT_SILU, keep, tile, chain=dict(w=w2p, kp=kp2, bias=b2p, y=y2.view, cout=c2, keep=keep)))
        what = f"chain tile {tile} keep={keep} {DT_ID[dt]}"
        nm.assert_same_bits(y2.view, ref2.view, what + ": y2")
        y2.assert_outside_intact(what + ": y2")
        if keep:
            nm.assert_same_bits(y.view, mid.view, what + ": y")
            y.assert_outside_intact(what + ": y")
        else:
            nm.assert_same_bits(y.buf, y.before, what + ": y must not be written")
        case.inputs_intact(what)


# ------------------------------------------------------------------------------------------------------------------------------------
# icaf_stem on integer-valued images
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("cout,paired", [(32, False), (64, True)])
def test_stem_on_integer_images(cout, paired, dt):
    """icaf_stem (6x6 / stride 2 / pad 2 conv + SiLU straight from fp32 NCHW images) on images holding integers in [-8, 8]: the
    pre-activation is exact, every output within the SiLU budget; NaN-prefilled output, NaN-poisoned surroundings."""
    B, H, W, G = 2, 36, 44, 2 if paired else 1
    ds = [nm.lattice(dt, B, H, W, 3, cout, 6, H // 2, W // 2, 500 + 10 * cout + g) for g in range(G)]
    wp, kp, bp = ops.pack_streams([(ops.s2d_conv_weight(d["w"].to(DEV)), d["bias"].to(DEV)) for d in ds], dt, 16)
    img = stack([d["x"] for d in ds]).contiguous().to(DEV)
    lead = (G, B, H // 2, W // 2) if paired else (B, H // 2, W // 2)
    y = nm.Poisoned(lead, cout, dt, DEV, nm.NAN_BITS[dt])
    run(ops.stem(img, wp, kp, bp, y.view, cout))
    y.assert_outside_intact("stem")
    got = y.view.cpu()
    for g, d in enumerate(ds):
        z, ref = nm.ref64(d["x"], d["w"], d["bias"], 2, 2, ACT_SILU)
        bound = nm.launch_bound(z, ACT_SILU, dt, dt)
        gg = (got[g] if paired else got).permute(0, 3, 1, 2)
        print(f"\n[stem] cout {cout} {DT_ID[dt]} stream {g}: err / budget {nm.budget_ratio(gg, ref, bound):.3f}")
        RATIOS[("stem", "silu", DT_ID[dt])] = max(RATIOS.get(("stem", "silu", DT_ID[dt]), 0.0), nm.budget_ratio(gg, ref, bound))
        nm.assert_budget(gg, ref, bound, f"stem cout {cout} {DT_ID[dt]} stream {g}")


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm on rows whose statistics are exact
# ------------------------------------------------------------------------------------------------------------------------------------
LN_BASE = {F32: (4096.0, 1.0), BF16: (4096.0, 32.0), F16: (1024.0, 1.0)}     # (m, step): m + step * {-3..3} is representable in the type


def ln_rows(dt, rows, C, seed):
    """(x, kind) with three kinds of rows whose mean and sum of squared deviations are exact in fp32 in any order:
    0 constant; 1 m + d with d = step * small integers summing to zero (x*x is NOT exact: a one-pass variance is off by orders of
    magnitude); 2 zeros with one outlier of 4096 (C a power of two: mean 4096 / C, the sum of squares stays below 2^24)."""
    g = torch.Generator().manual_seed(seed)
    m, step = LN_BASE[dt]
    x = torch.empty((rows, C))
    kind = torch.arange(rows) % 3
    for r in range(rows):
        if kind[r] == 0:
            x[r] = float(torch.randint(-64, 65, (1,), generator=g)) / 4.0
        elif kind[r] == 1:
            half = torch.randint(-3, 4, (C // 2,), generator=g).float()
            x[r] = m + step * torch.cat((half, -half))[torch.randperm(C, generator=g)]
        else:
            x[r] = 0.0
            x[r, int(torch.randint(0, C, (1,), generator=g))] = 4096.0
    assert torch.equal(x.to(dt).float(), x)
    return x, kind


def ln_reference(x, gamma, beta, eps, dt):
    """fp64 LayerNorm and the per-element bound for layernorm_kernel's expression (x - mean) * rstd * gamma + beta (dmff.hip; two passes).
    With exact mean, deviations d and sum of squares q, the fp32 roundings are: q / C and + eps (u each, halved by the square root), sqrtf
    and the division 1 / sqrt (u each, both correctly rounded): rstd carries 3u; then d * rstd (u), * gamma (u) — 5u on the product t,
    6u with second-order terms — and the addition of beta (u of the result).  Plus half a unit of the storage type."""
    x64 = x.double()
    mean = x64.mean(1, keepdim=True)
    d = x64 - mean
    var = (d * d).mean(1, keepdim=True)
    t = d / torch.sqrt(var + eps) * gamma.double()
    ref = t + beta.double()
    return ref, nm.storage_bound(ref, 6.0 * nm.U32 * t.abs() + nm.U32 * ref.abs() + nm.SUB32, dt)


def ln_check(got, x, kind, gamma, beta, eps, dt, what):
    ref, bound = ln_reference(x, gamma, beta, eps, dt)
    ratio = nm.budget_ratio(got, ref, bound)
    print(f"\n[layernorm] {what}: err / budget {ratio:.3f}")
    RATIOS[("layernorm", what.split()[0], DT_ID[dt])] = ratio
    const = kind == 0
    nm.assert_same_bits(got[const], beta.to(dt).expand(int(const.sum()), -1).contiguous(), what + ": constant rows must give RNE(beta)")
    nm.assert_budget(got, ref, bound, what, signed=False)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("C", [64, 128, 512, 1024])
def test_layernorm_on_exact_rows(C, dt):
    rows, eps = 39, 1e-5
    gen = torch.Generator().manual_seed(C)
    gam = [torch.randint(-64, 65, (C,), generator=gen).float() / 32.0 for _ in range(2)]
    bet = [torch.randint(-2 ** 15, 2 ** 15, (C,), generator=gen).float() / 2 ** 14 for _ in range(2)]      # 16 bits: inexact in both 16-bit types
    xs = [ln_rows(dt, rows, C, 10 * C + g) for g in range(2)]
    xg = torch.stack([x for x, _ in xs]).to(dt).to(DEV)
    y = torch.full_like(xg, float("nan"))
    run(ops.layernorm(xg, y, gam[0].to(DEV), bet[0].to(DEV), gam[1].to(DEV), bet[1].to(DEV), eps))
    for g in range(2):
        ln_check(y[g].cpu(), xs[g][0], xs[g][1], gam[g], bet[g], eps, dt, f"icaf_layernorm C={C} {DT_ID[dt]} group {g}")


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("C,wide", [(128, False), (128, True), (256, True), (512, True)])
def test_fused_layernorm_qkv_with_identity_query_projection(C, wide, dt):
    """icaf_dmff_ln_qkv / icaf_dmff_wide_ln_qkv with Q = identity and zero bias: the normalised row, rounded to the storage type, passes
    through the GEMM exactly, so the Q third of qkv must equal icaf_layernorm's output bit for bit and meet the same per-element bound."""
    B, N, heads, eps = 1, 96, 4, 1e-5
    rows = B * N
    gen = torch.Generator().manual_seed(3 * C)
    gam = [torch.randint(-64, 65, (C,), generator=gen).float() / 32.0 for _ in range(2)]
    bet = [torch.randint(-2 ** 15, 2 ** 15, (C,), generator=gen).float() / 2 ** 14 for _ in range(2)]
    xs = [ln_rows(dt, rows, C, 20 * C + g) for g in range(2)]
    xg = torch.stack([x for x, _ in xs]).to(dt).to(DEV).contiguous()
    wq = torch.zeros((3 * C, C))
    wq[:C] = torch.eye(C)
    wq[C:] = torch.randint(-8, 9, (2 * C, C), generator=gen).float() / 8.0
    zero = lambda n, k: ops.pack_streams([(torch.zeros((n, k), device=DEV), torch.zeros((n,), device=DEV))] * 2, dt)
    packs = dict(qkv=ops.pack_streams([(wq.to(DEV), torch.zeros((3 * C,), device=DEV))] * 2, dt),
                 out=zero(C, C), fc1=zero(4 * C, C), fc2=zero(C, 4 * C))
    packs = {k: (v[0], v[1], v[2]) for k, v in packs.items()}
    dev = lambda t: t.to(DEV).contiguous()
    ln = dict(a1w=dev(gam[0]), a1b=dev(bet[0]), a2w=dev(gam[1]), a2b=dev(bet[1]), mw=dev(gam[0]), mb=dev(bet[0]))
    coef = dict(hidden=4 * C, co=[1.0] * 8)
    qkv = torch.full((2, rows, 3 * C), float("nan"), dtype=dt, device=DEV)
    fn = ops.dmff_wide_ln_qkv if wide else ops.dmff_ln_qkv
    run(fn(xg, qkv, packs, ln, coef, (eps, eps, eps), B, N, heads))
    y = torch.full_like(xg, float("nan"))
    run(ops.layernorm(xg, y, ln["a1w"], ln["a1b"], ln["a2w"], ln["a2b"], eps))
    assert bool(torch.isfinite(qkv.float()).all()), "qkv holds unwritten or non-finite elements"
    for g in range(2):
        what = f"{'icaf_dmff_wide_ln_qkv' if wide else 'icaf_dmff_ln_qkv'} C={C} {DT_ID[dt]} group {g}"
        ln_check(qkv[g, :, :C].cpu(), xs[g][0], xs[g][1], gam[g], bet[g], eps, dt, what)
        nm.assert_same_bits(qkv[g, :, :C].contiguous(), y[g], what + " vs icaf_layernorm")
