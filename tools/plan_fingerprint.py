"""Fingerprint of the execution plans a source tree builds: every launch with every argument, pointers replaced by what they point at.

    python tools/plan_fingerprint.py REPO_ROOT [--digest] [--only SUBSTRING]
    python tools/plan_fingerprint.py REPO_ROOT --candidates

imports icafusion_amd from REPO_ROOT (any checkout, e.g. a `git worktree` of another commit; ICAF_LIB may point it at a libicaf.so built
elsewhere), builds each configuration of MATRIX on the CPU with seeded parameters and prints one JSON line per configuration (--digest: its
name and the line's sha256 instead).  Plan-owned buffers are named buf<N> in allocation order, every other storage w<sha256 of its bytes>,
so two trees print the same bytes exactly when they record the same launches over the same packed weights, however the tensors are
shared or cached.  Host code only: no kernel runs and no GPU is needed.

--candidates prints instead one digest over the tuner's rules: for every layer signature of a grid (and of every committed tune cache), the
set of launch configurations ops.conv_candidates offers and whether ops.wants_wf builds the fragment-major weight copy: every signature
without the copy, and once more with it where the rule builds it (the states a plan can be in).  A second line lists every id offered.
ICAF_OPTIONS in the environment selects the switches, as everywhere.  A tree from before ops.wants_wf is read with the rule its conv2d carried.
"""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("root")
ap.add_argument("--digest", action="store_true", help="print '<configuration> <sha256 of its JSON line>' instead of the JSON")
ap.add_argument("--only", default="", help="configurations whose name contains this")
ap.add_argument("--candidates", action="store_true", help="digest of conv_candidates / wants_wf over a grid of layer signatures instead")
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
sys.path.insert(0, ROOT)

import yaml                                                     # noqa: E402
from icafusion_amd import engine                                # noqa: E402
from icafusion_amd.models import common                         # noqa: E402
from icafusion_amd.models.yolo import Model                     # noqa: E402

assert os.path.abspath(engine.__file__).startswith(ROOT + os.sep), f"icafusion_amd came from {engine.__file__}, not from {ROOT}"


def candidate_sweep():
    import glob
    import itertools
    from types import SimpleNamespace

    from icafusion_amd import ops
    wants_wf = getattr(ops, "wants_wf", None)
    if wants_wf is None:             # an older tree: conv2d decided inline (the packed Kp is always a multiple of 64 for the 16-bit types)
        def wants_wf(a):
            cw = ops.OPT.cwide and a.act == ops.ACT_SILU and ops.cwide_shapes(a.kh, a.kw, a.sh, a.sw, a.ph, a.pw, a.Cin, a.Cout)
            return (a.dtype != ops.F32 and a.out_dtype == a.dtype and (a.Cin * 2) % 128 == 0 and not a.pre
                    and ((ops.OPT.wreg_gemm and not a.w2 and a.Cout > 64) or bool(cw)))
    chans = (8, 16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1024)
    types = ((ops.F32, ops.F32), (ops.BF16, ops.BF16), (ops.F16, ops.F16), (ops.BF16, ops.F32))
    forms = (("plain", 0), ("pre", 0), ("chain", 32), ("chain", 64), ("chain", 128), ("tail", 256))

    def layer(cout, cin, k, s, dt, odt, act, res, pre, cout2, tail, groups, pix):
        return SimpleNamespace(Cout=cout, Cin=cin, kh=k, kw=k, sh=s, sw=s, ph=k // 2, pw=k // 2, dtype=dt, out_dtype=odt, act=act, pre=bool(pre),
                               w2=bool(cout2), Cout2=cout2, x2=tail, res=bool(res), groups=groups, B=1, Ho=1, Wo=pix)

    layers = [layer(cout, cin, k, s, dt, odt, act, False, form == "pre", c2, form == "tail", 1, pix)
              for cin, cout, (k, s), (dt, odt), act, pix, (form, c2) in itertools.product(
                  chans, chans, ((1, 1), (3, 1), (3, 2), (6, 2)), types, (0, 1, 2), (6400, 51200, 204800, 819200), forms)]
    ncache = 0
    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "tune_cache*.json"))):
        for (M, cout, cin, kh, kw, sh, sw, _, _, _, _, groups, dt, odt, act, res, pre, cout2, keep), _ in json.load(open(f)):
            layers.append(layer(cout, cin, kh, sh, dt, odt, act, res, pre, cout2, keep == 2, groups, M))      # (keep == 2: ops._conv_signature)
            ncache += 1
    h, reached, n = hashlib.sha256(), set(), 0
    for a in layers:
        want = bool(wants_wf(a))
        for a.wf in (False, True)[:1 + want]:
            cands = sorted(set(ops.conv_candidates(a)))
            reached.update(cands)
            h.update(repr((sorted(vars(a).items()), cands, want)).encode())
            n += 1
    print(f"{len(layers)} layers ({ncache} from the tune caches), {n} signatures, {len(reached)} configurations offered", file=sys.stderr)
    print(f"candidates {h.hexdigest()}")
    print(f"offered {json.dumps(sorted(reached))}")


if a.candidates:
    candidate_sweep()
    sys.exit(0)

SHAPE, SHAPE2 = (2, 320, 352), (1, 352, 416)
YAMLS = ["yolov5n_Transfusion_kaist.yaml", "yolov5s_Transfusion_kaist.yaml", "yolov5m_Transfusion_kaist.yaml", "yolov5l_Transfusion_VEDAI.yaml",
         "yolov5s_Add_kaist.yaml", "yolov5n_NiNfusion_FLIR.yaml", "yolov5m_NiNfusion_kaist.yaml", "yolov5m_Transfusion_SeaDrone.yaml",
         "yolov5_VGG16_Transfusion_kaist.yaml", "yolov5_VGG16_NiNfusion_kaist.yaml", "yolov5_ResNet50_Transfusion_kaist.yaml",
         "yolov5_ResNet50_NiNfusion_kaist.yaml", "yolov5s_Transfusion_kaist_loops3.yaml"]
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
S, V, R = "yolov5s_Transfusion_kaist.yaml", "yolov5_VGG16_Transfusion_kaist.yaml", "yolov5_ResNet50_Transfusion_kaist.yaml"
N5, M5, L5 = "yolov5n_Transfusion_kaist.yaml", "yolov5m_Transfusion_kaist.yaml", "yolov5l_Transfusion_VEDAI.yaml"
CTB = common.CrossTransformerBlock
U8, UNPAIRED = ("u8", {"u8": True}, {}, [], None), ("pair_streams=False", {}, {"pair_streams": False}, [], None)
# (name, yaml, dtype, (B, H, W), build_plan keywords, Model attributes, class-level switches, loops of the DMFF rows)
MATRIX = [(f"{y[:-5]}/{d}", y, d, SHAPE, {}, {}, [], None) for y in YAMLS for d in DTYPES] + [
    (f"{y[:-5]}/bf16/{tag}", y, "bf16", SHAPE, kw, attrs, sw, loops) for y, variants in [
        (S, [U8,
             ("fold_upsample", {}, {"fold_upsample": True}, [], None),
             UNPAIRED,
             ("fuse_stem2=False", {}, {}, [(common.Conv, "fuse_stem2", False)], None),
             ("fuse_cv3=False", {}, {}, [(common.C3, "fuse_cv3", False)], None),
             ("chain_bottlenecks=False", {}, {}, [(common.C3, "chain_bottlenecks", False)], None),
             ("chain_tail=False", {}, {}, [(common.Conv, "chain_tail", False)], None),
             ("fuse_max_c=128", {}, {}, [(CTB, "fuse_max_c", 128)], None),
             ("fuse_wide=False", {}, {}, [(CTB, "fuse_wide", False)], None),
             ("loops=3", {}, {}, [], 3)]),
        (V, [U8, UNPAIRED, ("fuse_stem=True", {}, {}, [(common.VGGblock, "fuse_stem", True)], None)]),
        (R, [U8, UNPAIRED])] for tag, kw, attrs, sw, loops in variants] + [
    (f"{y[:-5]}/bf16/{SHAPE2[1]}x{SHAPE2[2]}", y, "bf16", SHAPE2, {}, {}, [], None) for y in (S, V, R)] + [
    # the forms of the DMFF block (CrossTransformerBlock.block_form): C = 64 ... 1024 with and without iterations (yolov5l's P4 is the C = 512,
    # ksplit = 1 case), the fp32 parity builds, and every class switch; run once per ICAF_OPTIONS=dmff_ksplit=1 / 2 / 4 for the forced splits
    (f"{y[:-5]}/{d}/{tag}", y, d, SHAPE, {}, {}, sw, loops) for y, d, tag, sw, loops in [
        (S, "fp32", "fuse_fp32=True", [(CTB, "fuse_fp32", True)], None),
        (N5, "fp32", "fuse_fp32=True", [(CTB, "fuse_fp32", True)], None),
        (S, "bf16", "res32=False,loops=3", [(CTB, "res32", False)], 3),
        (N5, "bf16", "loops=3", [], 3), (M5, "bf16", "loops=3", [], 3), (L5, "bf16", "loops=3", [], 3),
        (S, "bf16", "wide_max_c=128", [(CTB, "wide_max_c", 128)], None),
        (S, "bf16", "fuse_block=False", [(CTB, "fuse_block", False)], None)]]


@contextlib.contextmanager
def switched(switches):
    old = [(c, n, getattr(c, n)) for c, n, _ in switches]
    for c, n, v in switches:
        setattr(c, n, v)
    try:
        yield
    finally:
        for c, n, v in old:
            setattr(c, n, v)


@contextlib.contextmanager
def numbered_buffers(owned):
    """Plan.act / tokens / empty record each buffer's storage -> allocation number, and keep the buffer alive (a freed scratch buffer's
    address would be handed to a later weight)."""
    orig = {n: getattr(engine.Plan, n) for n in ("act", "tokens", "empty")}

    def wrap(f):
        def g(*args, **kw):
            t = f(*args, **kw)
            owned[t.untyped_storage().data_ptr()] = (len(owned), t)
            return t
        return g
    for n, f in orig.items():
        setattr(engine.Plan, n, wrap(f))
    try:
        yield
    finally:
        for n, f in orig.items():
            setattr(engine.Plan, n, f)


def tensors(obj):
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from tensors(v)


class Resolver:
    def __init__(self, owned, plan):
        self.owned, self.hashes = owned, {}
        # second resort: the two launches of a split out-projection + MLP share one argument struct, and the reduce launch keeps
        # only the tensors it reads itself
        self.everything = [t for _, t in owned.values()] + [t for l in plan.launches for t in tensors(l.keep)]

    def tag(self, t):
        st = t.untyped_storage()
        base = st.data_ptr()
        if base in self.owned:
            return f"buf{self.owned[base][0]}"
        if base not in self.hashes:                # through numpy: bytes(storage) walks the storage element by element
            raw = torch.empty(0, dtype=torch.uint8).set_(st).numpy()
            self.hashes[base] = "w" + hashlib.sha256(raw.tobytes()).hexdigest()
        return self.hashes[base]

    def __call__(self, ptr, keep, what):
        if not ptr:
            return None
        for pool in (tensors(keep), self.everything):
            for t in pool:
                st = t.untyped_storage()
                if st.data_ptr() <= ptr < st.data_ptr() + max(st.nbytes(), 1):
                    return [self.tag(t), ptr - st.data_ptr()]
        raise RuntimeError(f"{what}: pointer {ptr:#x} lies in no tensor the plan keeps")


def plain(v):
    return [plain(e) for e in v] if isinstance(v, ctypes.Array) else v


def expand(s, resolve, keep, what):
    out = {}
    for name, ty in s._fields_:
        v = getattr(s, name)
        if ty is ctypes.c_void_p:
            out[name] = resolve(v, keep, f"{what}.{name}")
        elif issubclass(ty, ctypes.Array) and ty._type_ is ctypes.c_void_p:
            out[name] = [resolve(e, keep, f"{what}.{name}") for e in v]
        elif issubclass(ty, ctypes.Structure):
            out[name] = expand(v, resolve, keep, f"{what}.{name}")
        else:
            out[name] = plain(v)
    return out


def fingerprint(plan, resolve):
    launches = []
    for i, l in enumerate(plan.launches):
        what = f"launch {i} ({l.name})"
        args = []
        for j, (v, ty) in enumerate(zip(l.args, l.fn.argtypes)):
            if ty is ctypes.c_void_p:
                args.append(resolve(v, l.keep, f"{what} argument {j}"))
            elif hasattr(v, "_obj"):                                  # byref(struct)
                args.append(expand(v._obj, resolve, l.keep, f"{what} argument {j}"))
            else:
                args.append(plain(v))
        assert len(l.args) == len(l.fn.argtypes) - 1, what            # (the stream is appended at run time)
        launches.append(dict(name=l.name, fn=l.fn.__name__, branch=l.branch, flops=l.flops, bytes=l.bytes, args=args))
    inputs = [resolve(t.data_ptr(), (t,), "input") + [list(t.shape), str(t.dtype)] for t in plan.inputs]
    return dict(launches=launches, inputs=inputs, branches={str(k): v for k, v in sorted(plan.branches.items())})


def seed_parameters(m):
    """Every floating parameter and buffer except the anchors in [0.25, 0.75]: fresh BatchNorm statistics fold to all-zero biases otherwise."""
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, t in list(m.named_parameters()) + list(m.named_buffers()):
            if t.is_floating_point() and "anchor" not in n.rsplit(".", 1)[-1]:
                t.copy_(torch.rand(t.shape, generator=g) * 0.5 + 0.25)


for name, y, d, (B, H, W), kw, attrs, switches, loops in MATRIX:
    if a.only not in name:
        continue
    torch.manual_seed(0)
    with open(os.path.join(ROOT, "models", "transformer", y)) as f:
        m = Model(yaml.safe_load(f)).eval()
    seed_parameters(m)
    for k, v in attrs.items():
        setattr(m, k, v)
    if loops is not None:
        for row in m.model:
            if isinstance(row, common.TransformerFusionBlock):
                row.crosstransformer[0].loops = loops
    owned = {}
    with switched(switches), numbered_buffers(owned):
        plan = m.build_plan(B, H, W, "cpu", DTYPES[d], **kw)
    resolve = Resolver(owned, plan)
    line = json.dumps(dict(config=name, **fingerprint(plan, resolve)), sort_keys=True)
    print(f"{name}: {len(plan.launches)} launches, {len(owned)} buffers, {len(resolve.hashes)} other storages", file=sys.stderr)
    print(f"{name} {hashlib.sha256(line.encode()).hexdigest()}" if a.digest else line, flush=True)
