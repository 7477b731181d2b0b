// Test-time augmentation (reference models/yolo_test.py:116-131): input staging of the scaled / flipped passes and the merge of
// their decoded rows.  Both kernels are bandwidth-bound; both mirror torch's CPU arithmetic (built with fp contraction off, build.py).
#include "icaf_common.h"

namespace icaf {

struct TtaStageArgs {
    icaf_tta_pass p[ICAF_TTA_MAX_PASSES];
    int npass;
};

constexpr int TTA_QUADS = 16;     // column quads (64 output columns: 256-byte row segments) per workgroup
constexpr int TTA_ROWS = 16;      // thread rows per workgroup
constexpr int TTA_RPT = 2;        // output rows per thread: a workgroup covers a 32 x 64 tile of all three channels of one image

// scale_img (utils/torch_utils.py:257-267) of one modality's image per blockIdx.z = image * npass + pass — the passes of an image are
// neighbours in dispatch order, so the second pass finds most of its source lines in the cache.  A thread owns four consecutive output
// columns: their source columns and weights (the flip folded in) are computed ONCE and serve 2 rows x 3 channels, each written with one
// 16-byte store.  Indices are clamped into the source plane for padded columns too, so no load ever leaves it.
template <bool U8>
__global__ __launch_bounds__(TTA_QUADS * TTA_ROWS) void tta_stage_kernel(const void* __restrict__ src, int ctot, int B, int H, int W,
                                                                          TtaStageArgs a) {
    const int pass = blockIdx.z % a.npass, img = blockIdx.z / a.npass;       // img = modality * B + b
    const int Hr = a.p[pass].Hr, Wr = a.p[pass].Wr, Hp = a.p[pass].Hp, Wp = a.p[pass].Wp, flip = a.p[pass].flip;
    float* __restrict__ dst = a.p[pass].dst;
    const int x = (blockIdx.x * TTA_QUADS + threadIdx.x) * 4;
    const int row0 = blockIdx.y * (TTA_ROWS * TTA_RPT) + threadIdx.y;
    if (x >= Wp || row0 >= Hp) return;
    constexpr float PAD = 0.447f;
    const float sx = (float)W / (float)Wr, sy = (float)H / (float)Hr;
    int xa[4], xb[4];
    float lx0[4], lx1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = __builtin_fmaf(sx, (float)(x + j) + 0.5f, -0.5f);
        s = s < 0.0f ? 0.0f : s;
        const int i0 = min((int)s, W - 1), i1 = min(i0 + 1, W - 1);
        lx1[j] = s - (float)i0;
        lx0[j] = 1.0f - lx1[j];
        xa[j] = flip ? W - 1 - i0 : i0;
        xb[j] = flip ? W - 1 - i1 : i1;
    }
    long long plane;                                  // first of the image's three source planes
    if (U8) plane = (long long)(img % B) * ctot + 3 * (img / B);
    else plane = (long long)img * 3;
    const long long hw = (long long)H * W;
#pragma unroll
    for (int k = 0; k < TTA_RPT; ++k) {
        const int r = row0 + k * TTA_ROWS;
        if (r >= Hp) break;
        float* o = dst + ((long long)img * 3 * Hp + r) * Wp + x;
        if (r >= Hr) {
            const f32x4 v = {PAD, PAD, PAD, PAD};
#pragma unroll
            for (int c = 0; c < 3; ++c) *(f32x4*)(o + (long long)c * Hp * Wp) = v;
            continue;
        }
        float s = __builtin_fmaf(sy, (float)r + 0.5f, -0.5f);
        s = s < 0.0f ? 0.0f : s;
        const int y0 = min((int)s, H - 1), y1 = min(y0 + 1, H - 1);
        const float ly1 = s - (float)y0, ly0 = 1.0f - ly1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long p0 = (plane + c) * hw + (long long)y0 * W, p1 = (plane + c) * hw + (long long)y1 * W;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a00, a01, a10, a11;
                if (U8) {
                    const unsigned char* u = (const unsigned char*)src;
                    a00 = (float)u[p0 + xa[j]] / 255.0f; a01 = (float)u[p0 + xb[j]] / 255.0f;
                    a10 = (float)u[p1 + xa[j]] / 255.0f; a11 = (float)u[p1 + xb[j]] / 255.0f;
                } else {
                    const float* f = (const float*)src;
                    a00 = f[p0 + xa[j]]; a01 = f[p0 + xb[j]];
                    a10 = f[p1 + xa[j]]; a11 = f[p1 + xb[j]];
                }
                const float val = ly0 * (lx0[j] * a00 + lx1[j] * a01) + ly1 * (lx0[j] * a10 + lx1[j] * a11);
                v[j] = (x + j < Wr) ? val : PAD;
            }
            *(f32x4*)(o + (long long)c * Hp * Wp) = v;
        }
    }
}

constexpr int TTA_MERGE_MAX = ICAF_TTA_MAX_PASSES + 1;
struct TtaMergeArgs {
    const float* z[TTA_MERGE_MAX];
    long long start[TTA_MERGE_MAX], rows[TTA_MERGE_MAX];      // first merged row of the pass, its row count (0 for unused slots)
    float scale[TTA_MERGE_MAX];
    int flip[TTA_MERGE_MAX];
};
struct TtaMergeDiv { FastDiv no, rows; };

// out[b][start_i + r][o] = z_i[b][r][o], boxes de-scaled by an IEEE division and de-flipped (models/yolo_test.py:125-131); one thread per
// element, consecutive threads on consecutive output floats (reads are contiguous per pass and image as well).
template <bool I32>
__global__ __launch_bounds__(256) void tta_merge_kernel(TtaMergeArgs a, float* __restrict__ out, long long rows_total, int no, float width,
                                                        long long total, TtaMergeDiv dv) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        long long b, r;
        int o;
        if constexpr (I32) {
            unsigned int t, oo, bb, rr;
            fd_divmod((unsigned int)idx, dv.no, t, oo);
            fd_divmod(t, dv.rows, bb, rr);
            b = bb; r = rr; o = (int)oo;
        } else {
            o = (int)(idx % no);
            const long long t = idx / no;
            r = t % rows_total; b = t / rows_total;
        }
        float v = 0.0f;
#pragma unroll
        for (int i = 0; i < TTA_MERGE_MAX; ++i) {
            const long long ri = r - a.start[i];
            if (ri >= 0 && ri < a.rows[i]) {
                v = a.z[i][(b * a.rows[i] + ri) * no + o];
                if (o < 4) v = v / a.scale[i];
                if (a.flip[i] && o == 0) v = width - v;
            }
        }
        out[idx] = v;
    }
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_tta_stage(const void* src, int src_u8, int ctot, int B, int H, int W, const icaf_tta_pass* passes, int npass,
                              icaf_stream_t s) {
    if (!src || !passes) return fail(ICAF_ERR_ARG, "icaf_tta_stage: null pointer");
    if (npass < 1 || npass > ICAF_TTA_MAX_PASSES) return fail(ICAF_ERR_ARG, "icaf_tta_stage: %d passes (1 .. %d)", npass, ICAF_TTA_MAX_PASSES);
    if (B < 1 || H < 1 || W < 1) return fail(ICAF_ERR_ARG, "icaf_tta_stage: bad geometry");
    if (src_u8 ? ctot < 6 : ctot != 3) return fail(ICAF_ERR_ARG, "icaf_tta_stage: ctot %d (3 for fp32 images, >= 6 for the uint8 batch)", ctot);
    TtaStageArgs a{};
    a.npass = npass;
    int hp = 0, wp = 0;
    for (int i = 0; i < npass; ++i) {
        const icaf_tta_pass& p = passes[i];
        if (!p.dst || ((uintptr_t)p.dst & 15)) return fail(ICAF_ERR_ARG, "icaf_tta_stage: pass %d: dst must be 16-byte aligned", i);
        if (p.Hr < 1 || p.Wr < 1 || p.Hp < p.Hr || p.Wp < p.Wr || p.Wp % 4)
            return fail(ICAF_ERR_ARG, "icaf_tta_stage: pass %d: resized %dx%d, padded %dx%d (Wp %% 4 == 0)", i, p.Hr, p.Wr, p.Hp, p.Wp);
        a.p[i] = p;
        hp = p.Hp > hp ? p.Hp : hp;
        wp = p.Wp > wp ? p.Wp : wp;
    }
    const long long gz = 2ll * B * npass;
    constexpr int TH = TTA_ROWS * TTA_RPT, TW = TTA_QUADS * 4;
    const long long gy = (hp + TH - 1) / TH;
    if (gz > 65535 || gy > 65535) return fail(ICAF_ERR_UNSUPPORTED, "icaf_tta_stage: grid %lld x %lld too large", gy, gz);
    dim3 grid((unsigned)((wp + TW - 1) / TW), (unsigned)gy, (unsigned)gz), block(TTA_QUADS, TTA_ROWS);
    if (src_u8) hipLaunchKernelGGL(tta_stage_kernel<true>, grid, block, 0, S(s), src, ctot, B, H, W, a);
    else hipLaunchKernelGGL(tta_stage_kernel<false>, grid, block, 0, S(s), src, ctot, B, H, W, a);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

extern "C" int icaf_tta_merge(const float* const* z, const long long* rows, const float* scale, const int* flip, int npass, float* out,
                              int B, int no, float width, icaf_stream_t s) {
    if (!z || !rows || !scale || !flip || !out) return fail(ICAF_ERR_ARG, "icaf_tta_merge: null pointer");
    if (npass < 1 || npass > TTA_MERGE_MAX) return fail(ICAF_ERR_ARG, "icaf_tta_merge: %d passes (1 .. %d)", npass, TTA_MERGE_MAX);
    if (B < 1 || no < 5) return fail(ICAF_ERR_ARG, "icaf_tta_merge: bad geometry");
    TtaMergeArgs a{};
    long long total_rows = 0;
    for (int i = 0; i < npass; ++i) {
        if (!z[i] || rows[i] < 1 || !(scale[i] > 0.0f)) return fail(ICAF_ERR_ARG, "icaf_tta_merge: pass %d: null z, no rows or scale <= 0", i);
        a.z[i] = z[i]; a.start[i] = total_rows; a.rows[i] = rows[i]; a.scale[i] = scale[i]; a.flip[i] = flip[i];
        total_rows += rows[i];
    }
    const long long total = (long long)B * total_rows * no;
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (total < (1ll << 31)) {
        const TtaMergeDiv dv{make_fastdiv((unsigned)no), make_fastdiv((unsigned)total_rows)};
        hipLaunchKernelGGL(tta_merge_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, S(s), a, out, total_rows, no, width, total, dv);
    } else {
        hipLaunchKernelGGL(tta_merge_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, S(s), a, out, total_rows, no, width, total, TtaMergeDiv{});
    }
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
