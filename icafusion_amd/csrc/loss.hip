// Validation loss: the FORWARD VALUE of the reference's ComputeLoss (utils/loss.py:325-463; bbox_iou, utils/general.py:410-452) for gfx950.
// No gradients exist here: nothing is kept for a backward pass.
//
// One call is a memset and three kernels on the caller's stream, no host synchronisation:
//   memset              the dense tobj maps of all levels (the call zeroes its own: the workspace's contents are irrelevant on entry)
//   loss_assign_kernel  one thread per SLOT (level i, offset o, anchor a, target t), slot index (o * na + a) * nt + t inside its level:
//                         build_targets (:409-463) in separate fp32 operations, the reference's order (contraction off): targets * gain, the
//                         division by the anchor, `% 1.`, gain - gxy, the truncating .long(), the clamp — and tbox from the CLAMPED indices
//                         (:457 clamps views of gij in place before :458 reads it).  The slot record {valid, b, a, gj, gi, tbox[4], tcls} is
//                         written for every slot.  A valid slot gathers its `no` logits, widens them to fp64 and leaves 1 - CIoU and its
//                         class BCE sum in the slot-loss table, and raises tobj[b, a, gj, gi] to (1 - gr) + gr * max(iou, 0) with an
//                         integer atomic max on the float's bits: the values are non-negative, so the largest wins whatever the order, which
//                         is what the reference's ascending sort before the scatter (:379-382) produces.
//   loss_partial_kernel workgroup (x, level): a fixed chunk of 2048 slots and a fixed chunk of 2048 cells of the level (objectness BCE of the
//                         strided logit p[..., 4] against tobj), each thread its eight items in index order, then a fixed tree in LDS: four
//                         fp64 partial sums per workgroup, written by every workgroup (nothing to zero beforehand).
//   loss_final_kernel   one workgroup: the partials of a level in a fixed order, the means, balance, the hyp gains; four fp32 values and
//                         the per-level match counts.
// No float atomics and no order that depends on scheduling: two calls on the same inputs give the same bits.
// The loss arithmetic is fp64 (exp / log1p / atan of the device library); only the assignment is fp32, because its comparisons decide.
#pragma clang fp contract(off)
#include "icaf_common.h"
#include <algorithm>
#include <cmath>

namespace icaf {

constexpr int LS_THREADS = 256;
constexpr int LS_ITEMS = 8;                                  // items of a thread in the partial kernel
constexpr int LS_CHUNK = LS_THREADS * LS_ITEMS;
constexpr int LS_REC = ICAF_LOSS_SLOT_INTS;                  // int32 words of a slot record

struct LossArgs {
    const float* p[ICAF_LOSS_MAX_LEVELS];
    long long tobj_off[ICAF_LOSS_MAX_LEVELS];                // first float of the level's tobj map
    int ny[ICAF_LOSS_MAX_LEVELS], nx[ICAF_LOSS_MAX_LEVELS];
    float anchors[ICAF_LOSS_MAX_LEVELS][ICAF_LOSS_MAX_ANCHORS][2];
    int nl, B, na, nc, nt, nbx;
    float anchor_t;
    double gr, cp, cn, cls_pw, obj_pw;
};

struct LossFinal {
    double box, obj, cls, balance[ICAF_LOSS_MAX_LEVELS];
    long long cells[ICAF_LOSS_MAX_LEVELS];
    int nl, nc, nbx;
};

// torch.max of two floats: a NaN operand gives NaN
__device__ __forceinline__ float ls_max(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b); }
// x % 1. of torch for the operands the rule can accept (the `> 1.` beside it rejects every negative one)
__device__ __forceinline__ float ls_frac(float x) { return x - floorf(x); }
// .long() of an fp32 value: truncation; out-of-range and NaN values end up where the clamp or the range check that follows catches them
__device__ __forceinline__ int ls_trunc(float v) { return (int)fminf(fmaxf(v, -2.0e9f), 2.0e9f); }

// BCE-with-logits with pos_weight, one element (torch: (1 - t) x + (1 + (pw - 1) t) (log1p(exp(-|x|)) + max(-x, 0)))
__device__ __forceinline__ double ls_bce(double x, double t, double pw) {
    const double lw = (pw - 1.0) * t + 1.0;
    return (1.0 - t) * x + lw * (log1p(exp(-fabs(x))) + fmax(-x, 0.0));
}
__device__ __forceinline__ double ls_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// bbox_iou(pbox.T, tbox, x1y1x2y2=False, CIoU=True), eps = 1e-7 (utils/general.py:418-447)
__device__ __forceinline__ double ls_ciou(double px, double py, double pw, double ph, double tx, double ty, double tw, double th) {
    constexpr double eps = 1e-7;
    const double b1x1 = px - pw / 2, b1x2 = px + pw / 2, b1y1 = py - ph / 2, b1y2 = py + ph / 2;
    const double b2x1 = tx - tw / 2, b2x2 = tx + tw / 2, b2y1 = ty - th / 2, b2y2 = ty + th / 2;
    const double inter = fmax(fmin(b1x2, b2x2) - fmax(b1x1, b2x1), 0.0) * fmax(fmin(b1y2, b2y2) - fmax(b1y1, b2y1), 0.0);
    const double w1 = b1x2 - b1x1, h1 = b1y2 - b1y1 + eps, w2 = b2x2 - b2x1, h2 = b2y2 - b2y1 + eps;
    const double uni = w1 * h1 + w2 * h2 - inter + eps;
    const double iou = inter / uni;
    const double cw = fmax(b1x2, b2x2) - fmin(b1x1, b2x1), ch = fmax(b1y2, b2y2) - fmin(b1y1, b2y1);
    const double c2 = cw * cw + ch * ch + eps;
    const double dx = b2x1 + b2x2 - b1x1 - b1x2, dy = b2y1 + b2y2 - b1y1 - b1y2;
    const double rho2 = (dx * dx + dy * dy) / 4;
    const double da = atan(w2 / h2) - atan(w1 / h1);
    const double v = (4.0 / (M_PI * M_PI)) * (da * da);
    const double alpha = v / (v - iou + (1 + eps));
    return iou - (rho2 / c2 + v * alpha);
}

__global__ __launch_bounds__(LS_THREADS) void loss_assign_kernel(const LossArgs A, const float* __restrict__ targets, float* __restrict__ tobj,
                                                                 int* __restrict__ slots, double* __restrict__ slot_loss) {
    const int lvl = blockIdx.y, per = 5 * A.na * A.nt;
    const int s = blockIdx.x * LS_THREADS + threadIdx.x;
    if (s >= per) return;
    const int t = s % A.nt, a = (s / A.nt) % A.na, o = s / (A.nt * A.na);
    const int ny = A.ny[lvl], nx = A.nx[lvl], no = A.nc + 5;
    const float fx = (float)nx, fy = (float)ny;                       // gain[2:6] = shape[[3, 2, 3, 2]]
    const float* tg = targets + (long long)t * 6;
    const float gx = tg[2] * fx, gy = tg[3] * fy, gw = tg[4] * fx, gh = tg[5] * fy;
    const float aw = A.anchors[lvl][a][0], ah = A.anchors[lvl][a][1];
    const float rw = gw / aw, rh = gh / ah;
    const float worst = ls_max(ls_max(rw, 1.0f / rw), ls_max(rh, 1.0f / rh));
    bool ok = worst < A.anchor_t;
    float ox = 0.0f, oy = 0.0f;
    if (o == 1) { ok = ok && ls_frac(gx) < 0.5f && gx > 1.0f; ox = 0.5f; }
    else if (o == 2) { ok = ok && ls_frac(gy) < 0.5f && gy > 1.0f; oy = 0.5f; }
    else if (o == 3) { const float ix = fx - gx; ok = ok && ls_frac(ix) < 0.5f && ix > 1.0f; ox = -0.5f; }
    else if (o == 4) { const float iy = fy - gy; ok = ok && ls_frac(iy) < 0.5f && iy > 1.0f; oy = -0.5f; }
    const int b = ls_trunc(tg[0]), c = ls_trunc(tg[1]);
    ok = ok && b >= 0 && b < A.B;                                     // the reference raises an IndexError; here the row is skipped
    const int gi = min(max(ls_trunc(gx - ox), 0), nx - 1), gj = min(max(ls_trunc(gy - oy), 0), ny - 1);
    const float bx = gx - (float)gi, by = gy - (float)gj;             // gxy - gij AFTER the in-place clamp
    const long long g = (long long)lvl * per + s;
    int* rec = slots + g * LS_REC;
    rec[0] = ok ? 1 : 0;
    rec[1] = ok ? b : 0; rec[2] = ok ? a : 0; rec[3] = ok ? gj : 0; rec[4] = ok ? gi : 0;
    rec[5] = ok ? __float_as_int(bx) : 0; rec[6] = ok ? __float_as_int(by) : 0;
    rec[7] = ok ? __float_as_int(gw) : 0; rec[8] = ok ? __float_as_int(gh) : 0;
    rec[9] = ok ? c : 0;
    double liou = 0.0, lcls = 0.0;
    if (ok) {
        const long long cell = (((long long)b * A.na + a) * ny + gj) * nx + gi;
        const float* q = A.p[lvl] + cell * no;
        const double sx = ls_sigmoid((double)q[0]) * 2.0, sy = ls_sigmoid((double)q[1]) * 2.0;
        const double sw = ls_sigmoid((double)q[2]) * 2.0, sh = ls_sigmoid((double)q[3]) * 2.0;
        const double iou = ls_ciou(sx - 0.5, sy - 0.5, sw * sw * (double)aw, sh * sh * (double)ah, (double)bx, (double)by, (double)gw, (double)gh);
        liou = 1.0 - iou;
        const float tv = (float)((1.0 - A.gr) + A.gr * fmax(iou, 0.0));   // non-negative for gr in [0, 1]: its bits order like the values
        if (tv == tv) atomicMax(reinterpret_cast<unsigned int*>(tobj + A.tobj_off[lvl] + cell), __float_as_uint(tv));
        if (A.nc > 1)
            for (int k = 0; k < A.nc; ++k) lcls += ls_bce((double)q[5 + k], k == c ? A.cp : A.cn, A.cls_pw);
    }
    slot_loss[g * 2] = liou;
    slot_loss[g * 2 + 1] = lcls;
}

// fixed tree over the workgroup's 256 values; the result is valid in thread 0
__device__ __forceinline__ double ls_block_sum(double v, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int w = LS_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) sh[tid] = sh[tid] + sh[tid + w];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(LS_THREADS) void loss_partial_kernel(const LossArgs A, const float* __restrict__ tobj, const int* __restrict__ slots,
                                                                  const double* __restrict__ slot_loss, double* __restrict__ partial) {
    __shared__ double sh[LS_THREADS];
    const int lvl = blockIdx.y, tid = threadIdx.x;
    const long long per = 5LL * A.na * A.nt, cells = (long long)A.B * A.na * A.ny[lvl] * A.nx[lvl];
    const int no = A.nc + 5;
    double liou = 0.0, lcls = 0.0, cnt = 0.0, lobj = 0.0;
#pragma unroll
    for (int k = 0; k < LS_ITEMS; ++k) {
        const long long i = (long long)blockIdx.x * LS_CHUNK + k * LS_THREADS + tid;
        if (i < per) {
            const long long g = (long long)lvl * per + i;
            liou += slot_loss[g * 2];
            lcls += slot_loss[g * 2 + 1];
            cnt += (double)slots[g * LS_REC];
        }
        if (i < cells)                                          // one float of every `no`: the strided read of pi[..., 4]
            lobj += ls_bce((double)A.p[lvl][i * no + 4], (double)tobj[A.tobj_off[lvl] + i], A.obj_pw);
    }
    const double s0 = ls_block_sum(liou, sh), s1 = ls_block_sum(lcls, sh), s2 = ls_block_sum(cnt, sh), s3 = ls_block_sum(lobj, sh);
    if (tid == 0) {
        double* o = partial + ((long long)lvl * A.nbx + blockIdx.x) * 4;
        o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
    }
}

__global__ __launch_bounds__(LS_THREADS) void loss_final_kernel(const LossFinal F, const double* __restrict__ partial, float* __restrict__ out,
                                                                int* __restrict__ counts) {
    __shared__ double sh[LS_THREADS];
    const int tid = threadIdx.x;
    double lbox = 0.0, lobj = 0.0, lcls = 0.0;
    for (int lvl = 0; lvl < F.nl; ++lvl) {
        double sum[4];
        for (int k = 0; k < 4; ++k) {
            double v = 0.0;
            for (int x = tid; x < F.nbx; x += LS_THREADS) v += partial[((long long)lvl * F.nbx + x) * 4 + k];
            sum[k] = ls_block_sum(v, sh);
        }
        if (tid == 0) {
            const double n = sum[2];
            if (n > 0.0) {                                      // `if n:` (:367): a level without a match adds nothing
                lbox += sum[0] / n;
                if (F.nc > 1) lcls += sum[1] / (n * (double)F.nc);
            }
            lobj += (sum[3] / (double)F.cells[lvl]) * F.balance[lvl];
            counts[lvl] = (int)n;
        }
    }
    if (tid == 0) {
        out[0] = (float)(lbox * F.box);
        out[1] = (float)(lobj * F.obj);
        out[2] = (float)(lcls * F.cls);
        out[3] = 0.0f;                                          // lrk: never accumulated (:391)
    }
}

struct LossLayout {
    long long tobj_off[ICAF_LOSS_MAX_LEVELS];                   // floats from the workspace's start
    long long tobj_floats, cells[ICAF_LOSS_MAX_LEVELS];
    size_t partial_off, slot_loss_off, slots_off, bytes;
    int nbx;
};

static inline size_t ls_align(size_t v) { return (v + 255) / 256 * 256; }

// the argument checks shared by the two entry points; `what` names the caller
static int loss_layout(const char* what, int nl, const int* ny, const int* nx, int B, int na, int nt, LossLayout* L) {
    if (nl < 1 || nl > ICAF_LOSS_MAX_LEVELS) return fail(ICAF_ERR_UNSUPPORTED, "%s: nl must be in [1, %d] (%d)", what, ICAF_LOSS_MAX_LEVELS, nl);
    if (na < 1 || na > ICAF_LOSS_MAX_ANCHORS) return fail(ICAF_ERR_UNSUPPORTED, "%s: na must be in [1, %d] (%d)", what, ICAF_LOSS_MAX_ANCHORS, na);
    if (nt > ICAF_LOSS_MAX_TARGETS)
        return fail(ICAF_ERR_UNSUPPORTED, "%s: at most %d targets per call (%d); nothing is truncated", what, ICAF_LOSS_MAX_TARGETS, nt);
    if (!ny || !nx) return fail(ICAF_ERR_ARG, "%s: null ny / nx", what);
    if (nt < 0 || B < 1) return fail(ICAF_ERR_ARG, "%s: nt must not be negative and B positive", what);
    long long off = 0, most = 0;
    for (int i = 0; i < nl; ++i) {
        if (ny[i] < 1 || nx[i] < 1) return fail(ICAF_ERR_ARG, "%s: level %d has an empty map (%d x %d)", what, i, ny[i], nx[i]);
        L->cells[i] = (long long)B * na * ny[i] * nx[i];
        if (L->cells[i] > (1LL << 31)) return fail(ICAF_ERR_UNSUPPORTED, "%s: level %d has more than 2^31 cells", what, i);
        L->tobj_off[i] = off;
        off += (L->cells[i] + 63) / 64 * 64;                     // every level starts on a 256-byte boundary
        most = std::max(most, L->cells[i]);
    }
    const long long per = 5LL * na * nt;
    most = std::max(most, per);
    L->nbx = (int)std::max<long long>((most + LS_CHUNK - 1) / LS_CHUNK, 1);
    L->tobj_floats = off;
    L->partial_off = ls_align((size_t)off * sizeof(float));
    L->slot_loss_off = ls_align(L->partial_off + (size_t)nl * L->nbx * 4 * sizeof(double));
    L->slots_off = ls_align(L->slot_loss_off + (size_t)nl * per * 2 * sizeof(double));
    L->bytes = ls_align(L->slots_off + (size_t)nl * per * LS_REC * sizeof(int));
    return ICAF_OK;
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_loss_workspace_bytes(int nl, const int* ny, const int* nx, int B, int na, int nt, size_t* bytes, size_t* tobj_off,
                                         size_t* slots_off) {
    if (!bytes) return fail(ICAF_ERR_ARG, "icaf_loss_workspace_bytes: null bytes");
    LossLayout L;
    const int st = loss_layout("icaf_loss_workspace_bytes", nl, ny, nx, B, na, nt, &L);
    if (st != ICAF_OK) return st;
    *bytes = L.bytes;
    for (int i = 0; i < nl; ++i) {
        if (tobj_off) tobj_off[i] = (size_t)L.tobj_off[i] * sizeof(float);
        if (slots_off) slots_off[i] = L.slots_off + (size_t)i * 5 * na * nt * LS_REC * sizeof(int);
    }
    return ICAF_OK;
}

extern "C" int icaf_loss(const float* const* maps, const int* ny, const int* nx, int nl, int B, int na, int nc, const float* anchors,
                         const float* targets, int nt, const icaf_loss_params* prm, float* out, int* counts, void* workspace,
                         size_t workspace_bytes, icaf_stream_t s) {
    LossLayout L;
    const int st = loss_layout("icaf_loss", nl, ny, nx, B, na, nt, &L);
    if (st != ICAF_OK) return st;
    if (!maps || !anchors || !prm || !out || !counts || !workspace || (nt > 0 && !targets)) return fail(ICAF_ERR_ARG, "icaf_loss: null pointer");
    if (nc < 1) return fail(ICAF_ERR_ARG, "icaf_loss: nc must be positive (%d)", nc);
    if (!(prm->gr >= 0.0 && prm->gr <= 1.0))
        return fail(ICAF_ERR_ARG, "icaf_loss: gr must be in [0, 1] (%g): the duplicate rule orders non-negative tobj values by their bits", prm->gr);
    if (workspace_bytes < L.bytes || ((size_t)workspace & 255))
        return fail(ICAF_ERR_ARG, "icaf_loss: the workspace needs %zu bytes on a 256-byte boundary (%zu given)", L.bytes, workspace_bytes);
    LossArgs A;
    LossFinal F;
    for (int i = 0; i < ICAF_LOSS_MAX_LEVELS; ++i) {
        const bool on = i < nl;
        if (on && !maps[i]) return fail(ICAF_ERR_ARG, "icaf_loss: null map of level %d", i);
        A.p[i] = on ? maps[i] : nullptr;
        A.ny[i] = on ? ny[i] : 0;
        A.nx[i] = on ? nx[i] : 0;
        A.tobj_off[i] = on ? L.tobj_off[i] : 0;
        F.cells[i] = on ? L.cells[i] : 1;
        F.balance[i] = on ? prm->balance[i] : 0.0;
        for (int a = 0; a < ICAF_LOSS_MAX_ANCHORS; ++a)
            for (int k = 0; k < 2; ++k) A.anchors[i][a][k] = (on && a < na) ? anchors[((size_t)i * na + a) * 2 + k] : 1.0f;
    }
    A.nl = nl; A.B = B; A.na = na; A.nc = nc; A.nt = nt; A.nbx = L.nbx;
    A.anchor_t = (float)prm->anchor_t;
    A.gr = prm->gr; A.cp = prm->cp; A.cn = prm->cn; A.cls_pw = prm->cls_pw; A.obj_pw = prm->obj_pw;
    F.box = prm->box; F.obj = prm->obj; F.cls = prm->cls; F.nl = nl; F.nc = nc; F.nbx = L.nbx;
    char* ws = static_cast<char*>(workspace);
    float* tobj = reinterpret_cast<float*>(ws);
    double* partial = reinterpret_cast<double*>(ws + L.partial_off);
    double* slot_loss = reinterpret_cast<double*>(ws + L.slot_loss_off);
    int* slots = reinterpret_cast<int*>(ws + L.slots_off);
    ICAF_HIP(hipMemsetAsync(tobj, 0, (size_t)L.tobj_floats * sizeof(float), S(s)));
    if (nt > 0) {
        const unsigned gx = (unsigned)((5 * na * nt + LS_THREADS - 1) / LS_THREADS);
        loss_assign_kernel<<<dim3(gx, (unsigned)nl), dim3(LS_THREADS), 0, S(s)>>>(A, targets, tobj, slots, slot_loss);
        ICAF_LAUNCH_CHECK();
    }
    loss_partial_kernel<<<dim3((unsigned)L.nbx, (unsigned)nl), dim3(LS_THREADS), 0, S(s)>>>(A, tobj, slots, slot_loss, partial);
    ICAF_LAUNCH_CHECK();
    loss_final_kernel<<<dim3(1), dim3(LS_THREADS), 0, S(s)>>>(F, partial, out, counts);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
