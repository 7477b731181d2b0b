"""The DMFF block forms on the device against the library's own statement of what is built (icaf.h: icaf_dmff_block_forms): at every point of
C x dtype x ksplit x token stream the entry points of a form the query reports run and fill y — in the 16-bit types to the bits
CrossTransformerBlock.emit_tokens produces for that form — and the entry points of a form it refuses return ICAF_ERR_UNSUPPORTED before any launch.
N = 77 leaves a ragged last 64-row tile.  Nothing is launched that the query has not approved."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from icafusion_amd import ops                                        # noqa: E402
from icafusion_amd._lib import ERR_UNSUPPORTED                       # noqa: E402
from icafusion_amd.engine import Plan                                # noqa: E402
from test_gpu_dmff_fused import DEV, make_block                      # noqa: E402

B, N, HEADS, LOOPS = 1, 77, 8, 2          # two iterations: the second one reads the fp32 token stream the first one wrote
F32 = torch.float32
_BLOCKS = {}


def block(C):
    if C not in _BLOCKS:
        _BLOCKS[C] = make_block(C, HEADS, LOOPS, seed=C)[0].to(DEV)
    return _BLOCKS[C]


def nan_filled(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


def call(launch):
    """the entry point's status, unchecked"""
    return launch.fn(*launch.args, ops.current_stream_ptr())


def direct(blk, plan, tok, form, ks, stream, approved):
    """The entry points of `form` over NaN-prefilled buffers, LOOPS iterations chained like emit_tokens chains them.  approved False: the
    out-projection + MLP entry points only, once.  Returns (statuses, the last y)."""
    C, dt = tok.shape[2], tok.dtype
    p = blk._packed(plan)
    common = (p, p["ln"], dict(co=p["co"], hidden=4 * C), p["eps"], B, N, HEADS)
    qkv, att = nan_filled((2, N, 3 * C), dt), nan_filled((2, N, C), dt)
    part = nan_filled((ks, 2, N, C), F32) if ks > 1 else None
    t32 = [nan_filled((2, N, C), F32) for _ in range(2)] if stream else None
    sts, x = [], tok
    for it in range(LOOPS if approved else 1):
        y = nan_filled((2, N, C), dt)
        if form == "two-launch":
            ls = ([ops.dmff_ln_qkv(x, qkv, *common)] if approved else []) + [ops.dmff_attn_mlp(x, qkv, y, *common)]
        else:
            ls = [ops.dmff_wide_ln_qkv(x, qkv, *common), ops.cross_attention(qkv, att, B, N, HEADS)] if approved else []
            ls += ops.dmff_launches(True, True, x, None, att, y, *common, "dmff_proj_mlp", part, ks,
                                    x32=(t32[(it - 1) & 1] if (stream and it > 0) else None), y32=(t32[it & 1] if stream else None))
        sts += [call(l) for l in ls]
        x = y
    torch.cuda.synchronize()
    return sts, y


def planned(blk, tok, dt, form, ks, stream, monkeypatch):
    """emit_tokens steered to (form, ks, stream) by the class switches and the split preference"""
    blk.fuse_block = blk.fuse_wide = blk.fuse_fp32 = True
    blk.fuse_max_c, blk.wide_max_c, blk.res32 = (512 if form == "two-launch" else 32), 512, stream
    monkeypatch.setattr(ops, "dmff_wide_ksplit", lambda n, c: ks)
    plan = Plan(DEV, dt)
    assert tuple(blk.block_form(plan, tok.shape[2], N)) == (form, ks, stream)
    t = plan.tokens(2, B * N, tok.shape[2])
    t.copy_(tok)
    out = blk.emit_tokens(plan, t, B, N)
    plan.run()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_entry_points_follow_the_forms_query(C, dt, monkeypatch):
    blk = block(C)
    plan = Plan(DEV, dt)
    tok = torch.randn((2, B * N, C), generator=torch.Generator().manual_seed(C)).to(dt).to(DEV)
    points = [("two-launch", 1, False)] + [("three-launch", ks, stream) for ks in (1, 2, 4) for stream in (False, True)]
    ran = 0
    for form, ks, stream in points:
        what = f"{form} C={C} {dt} ksplit={ks} fp32 stream={stream}"
        two, three = ops.dmff_block_forms(dt, C, N, HEADS, 4 * C, ks, stream)
        approved = two if form == "two-launch" else three
        sts, y = direct(blk, plan, tok, form, ks, stream, approved)
        if not approved:
            assert sts and all(st == ERR_UNSUPPORTED for st in sts), f"{what}: statuses {sts} of a form the query refuses"
            assert bool(torch.isnan(y).all()), f"{what}: y was written although the form is refused"
            continue
        ran += 1
        assert all(st == 0 for st in sts), f"{what}: statuses {sts} of a form the query reports"
        assert not bool(torch.isnan(y).any()), f"{what}: prefill NaN left in y"
        if dt != F32:
            ref = planned(blk, tok, dt, form, ks, stream, monkeypatch)
            assert torch.equal(y.view(torch.int16), ref.view(torch.int16)), f"{what}: y differs from emit_tokens' in that form"
    assert ran == {64: 1, 128: (2 if dt == F32 else 3), 256: (0 if dt == F32 else 6), 512: (0 if dt == F32 else 5)}[C]
