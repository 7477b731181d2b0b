// Confluence suppression for gfx950 — replaces utils/confluence.py:50-193 of the reference (its alternative to NMS: boxes are picked by a
// normalised Manhattan proximity instead of IoU).
//
// The reference is a triple Python loop: every pick recomputes the proximity p(i, j) of every pair of the boxes still alive.  Here
//   confluence_cand_kernel     (icaf_confluence only) one 1024-thread workgroup per image: obj > conf, conf = cls * obj > conf, xywh -> xyxy
//                              in fp32, one row per (box, class) in row-major order — an ordered compaction (ballot + block scan) into the
//                              candidate list cand [B][max_cand][6]; the total is counted past the cap so that the image can be refused.
//   confluence_sweep_kernel    (icaf_confluence only) the initial n^2 sweep on the whole chip, one wavefront per candidate row: min_j p(i, j)
//                              over the candidates of the row's class with p < 2, and the lowest j attaining it.
//   confluence_pick_kernel     one 1024-thread workgroup per (image, class); its members (candidate order) live in LDS: box and conf in fp32,
//                              value(i) in fp64, the neighbour that attains it and an alive flag — 33 bytes each.  Without a sweep result the
//                              workgroup sweeps its own rows first (icaf_confluence_select).  Then, per pick:
//                                arg-min    the alive row of least value, the lowest index on a tie (values not below 10000 never win while
//                                           another does) — one shuffle reduction per wavefront, sixteen partial results through LDS;
//                                remove     every alive j with p(pick, j) < p_thres, one pair per thread;
//                                re-sweep   value(i) = min_j p(i, j) / conf_i changes only when the neighbour attaining it is removed: the rows
//                                           that lost theirs are listed and swept again, one wavefront per row, lanes over j.  A row whose
//                                           last neighbour went drops to value 0.
//                              The division by conf_i is monotone for conf_i > 0, so min_j fl(p / conf) = fl(min_j p / conf): the sweep keeps
//                              the least p and divides once.  Every member's kept flag goes to column 0 of its `det` row (scratch until the
//                              compaction below rewrites the block).
//   confluence_compact_kernel  one workgroup per image: flags -> LDS, then the kept candidates in ascending index into det / keep_idx, zeros
//                              behind them, count (or -n for a refused image).
// Pair arithmetic is fp64 on the fp32 inputs in the reference's operation order — one subtraction and one IEEE division per normalised
// coordinate, ((|dx1| + |dx2|) + |dy1|) + |dy2| — without contraction, reciprocals or reassociation: kept indices equal the reference's.
// A sweep does not pay those eight divisions for every pair: an fp32 estimate with a proven band (cf_estimate) finds the few pairs that can
// attain the minimum, or lie within the band around p_thres, and only those go through the fp64 arithmetic, which alone decides.
// The candidate scan (wg_incl_scan), the xywh decode and the ordered compaction of the kept rows (wg_rank) are box_core.h's.  The pick kernel keeps
// its member list and its own copy of the two-pass sweep written out.  A build with one sweep template for both kernels and the member list on
// wg_rank compiled the pick kernel to 94 instead of 108 registers and measured 3 - 7 % over its limits at 1,024 and 4,096 candidates; which of
// the two pieces cost that was not separated.  With this text the pick and the sweep kernel are the parent's assembly (profiles/postproc_share_ab.json).
#pragma clang fp contract(off)
#include "box_core.h"

namespace icaf {

constexpr int CF_THREADS = 1024;
constexpr int CF_WAVES = CF_THREADS / 64;
constexpr int CF_MAX = ICAF_CONFLUENCE_MAX_CAND;
constexpr int CF_SWEEP_THREADS = 256;
constexpr int CF_SWEEP_ROWS = 8;                     // candidate rows per wavefront of the sweep kernel
constexpr double CF_NEIGHBOUR = 2.0;                 // p < 2: j is a neighbour of i (utils/confluence.py:168)
constexpr double CF_START = 10000.0;                 // the running minimum of a pick starts here (:133)

// class id of a candidate row, -1 if no class loop of the reference visits it (`infos[:, 5] == c`, :123)
__device__ __forceinline__ int cf_class(float f, int nc) {
    if (!(f >= 0.0f && f < (float)nc)) return -1;
    const int c = (int)f;
    return (float)c == f ? c : -1;
}

// normalised Manhattan proximity of two boxes (:141-162): the four x values are normalised by their own range, each on its own, likewise y
__device__ __forceinline__ double cf_pair(float ax1f, float ay1f, float ax2f, float ay2f, float bx1f, float by1f, float bx2f, float by2f) {
    const double ax1 = ax1f, ay1 = ay1f, ax2 = ax2f, ay2 = ay2f, bx1 = bx1f, by1 = by1f, bx2 = bx2f, by2 = by2f;
    const double xlo = fmin(fmin(ax1, ax2), fmin(bx1, bx2)), xhi = fmax(fmax(ax1, ax2), fmax(bx1, bx2));
    const double ylo = fmin(fmin(ay1, ay2), fmin(by1, by2)), yhi = fmax(fmax(ay1, ay2), fmax(by1, by2));
    const double xr = xhi - xlo, yr = yhi - ylo;
    const double nax1 = (ax1 - xlo) / xr, nax2 = (ax2 - xlo) / xr, nbx1 = (bx1 - xlo) / xr, nbx2 = (bx2 - xlo) / xr;
    const double nay1 = (ay1 - ylo) / yr, nay2 = (ay2 - ylo) / yr, nby1 = (by1 - ylo) / yr, nby2 = (by2 - ylo) / yr;
    return ((fabs(nax1 - nbx1) + fabs(nax2 - nbx2)) + fabs(nay1 - nby1)) + fabs(nay2 - nby2);
}

// The same proximity in fp32 with one division per axis: mathematically p = (|a.x1 - b.x1| + |a.x2 - b.x2|) / (hi - lo) + the same in y, since
// every normalised value shares its axis' divisor.  On exact fp32 inputs (of magnitude below 1e18, so that nothing overflows) the estimate
// is within 3e-7 relative of the true p, and cf_pair within 2e-15 absolute; so with e the estimate, cf_pair lies in [cf_lower(e), cf_upper(e)].
// NaN exactly when cf_pair is (an axis whose four values coincide).  The estimate only decides which pairs need cf_pair at all — as iou_gt
// of nms.hip spares the division outside a band around the threshold; every value that is compared or stored comes from cf_pair.
__device__ __forceinline__ float cf_estimate(const f32x4& a, const f32x4& b) {
    const float xr = fmaxf(fmaxf(a[0], a[2]), fmaxf(b[0], b[2])) - fminf(fminf(a[0], a[2]), fminf(b[0], b[2]));
    const float yr = fmaxf(fmaxf(a[1], a[3]), fmaxf(b[1], b[3])) - fminf(fminf(a[1], a[3]), fminf(b[1], b[3]));
    return (fabsf(a[0] - b[0]) + fabsf(a[2] - b[2])) / xr + (fabsf(a[1] - b[1]) + fabsf(a[3] - b[3])) / yr;
}
__device__ __forceinline__ double cf_lower(float e) { return (double)e * (1.0 - 1e-5) - 1e-12; }
__device__ __forceinline__ double cf_upper(float e) { return (double)e * (1.0 + 1e-5) + 1e-12; }

// least estimate of a wavefront (+inf: no pair)
__device__ __forceinline__ float cf_wave_min_est(float e) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) e = fminf(e, __shfl_xor(e, o));
    return e;
}

// wavefront reduction of (p, j): the least p, the lowest j on a tie; j < 0 = nothing found
__device__ __forceinline__ void cf_wave_min(double& p, int& j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double op = __shfl_xor(p, o);
        const int oj = __shfl_xor(j, o);
        if (oj >= 0 && (j < 0 || op < p || (op == p && oj < j))) { p = op; j = oj; }
    }
}

// ---------------------------------------------------------------------------------------------------------------- candidate stage
__global__ __launch_bounds__(CF_THREADS) void confluence_cand_kernel(const float* __restrict__ pred, long long rows, int nc, float conf,
                                                                     int max_cand, float* __restrict__ cand, int* __restrict__ ncand) {
    __shared__ int wsum[CF_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int no = 5 + nc;
    const float* pb = pred + (long long)b * rows * no;
    float* cb = cand + (long long)b * max_cand * 6;
    long long base = 0;                                  // candidates before this chunk of rows (counted past the cap)
    for (long long r0 = 0; r0 < rows; r0 += CF_THREADS) {
        const long long r = r0 + tid;
        int mine = 0;
        float obj = 0.0f;
        if (r < rows) {
            obj = pb[r * no + 4];
            if (obj > conf)
                for (int j = 0; j < nc; ++j) mine += (pb[r * no + 5 + j] * obj > conf) ? 1 : 0;
        }
        int total;
        const int incl = wg_incl_scan<CF_WAVES>(mine, wsum, total);
        if (mine) {
            long long k = base + incl - mine;
            const float* p = pb + r * no;
            float x1, y1, x2, y2;
            xywh_to_xyxy(p, x1, y1, x2, y2);
            for (int j = 0; j < nc && k < max_cand; ++j) {
                const float c = p[5 + j] * obj;
                if (c > conf) {
                    float* o = cb + k * 6;
                    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; o[4] = c; o[5] = (float)j;
                    ++k;
                }
            }
        }
        base += total;
    }
    if (tid == 0) ncand[b] = base > 0x7fffffffLL ? 0x7fffffff : (int)base;
}

// ---------------------------------------------------------------------------------------------------------------- initial sweep, whole chip
__global__ __launch_bounds__(CF_SWEEP_THREADS) void confluence_sweep_kernel(const float* __restrict__ cand, const int* __restrict__ n_in,
                                                                            int max_cand, int nc, double* __restrict__ minp,
                                                                            int* __restrict__ nbr) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int n = n_in[b];
    if (n < 1 || n > max_cand) return;                   // refused or empty image
    const float* cb = cand + (long long)b * max_cand * 6;
    const int row0 = (blockIdx.x * (CF_SWEEP_THREADS / 64) + (threadIdx.x >> 6)) * CF_SWEEP_ROWS;
    for (int i = row0; i < row0 + CF_SWEEP_ROWS && i < n; ++i) {       // wave-uniform
        const float* a = cb + (long long)i * 6;
        f32x4 ab;
        ab[0] = a[0]; ab[1] = a[1]; ab[2] = a[2]; ab[3] = a[3];
        const int ci = cf_class(a[5], nc);
        // pass 1: the least estimate bounds the minimum from above; pass 2: cf_pair only where the estimate's band reaches that bound
        float emin = INFINITY;
        if (ci >= 0)
            for (int j = lane; j < n; j += 64) {
                const float* q = cb + (long long)j * 6;
                if (j == i || cf_class(q[5], nc) != ci) continue;
                f32x4 qb;
                qb[0] = q[0]; qb[1] = q[1]; qb[2] = q[2]; qb[3] = q[3];
                const float e = cf_estimate(ab, qb);
                if (e < emin) emin = e;
            }
        emin = cf_wave_min_est(emin);
        double best = 0.0;
        int bj = -1;
        if (cf_lower(emin) < CF_NEIGHBOUR) {             // wave-uniform
            const double bound = fmin(cf_upper(emin), CF_NEIGHBOUR);
            for (int j = lane; j < n; j += 64) {
                const float* q = cb + (long long)j * 6;
                if (j == i || cf_class(q[5], nc) != ci) continue;
                f32x4 qb;
                qb[0] = q[0]; qb[1] = q[1]; qb[2] = q[2]; qb[3] = q[3];
                if (!(cf_lower(cf_estimate(ab, qb)) <= bound)) continue;
                const double p = cf_pair(ab[0], ab[1], ab[2], ab[3], qb[0], qb[1], qb[2], qb[3]);
                if (p < CF_NEIGHBOUR && (bj < 0 || p < best)) { best = p; bj = j; }
            }
        }
        cf_wave_min(best, bj);
        if (lane == 0) {
            minp[(long long)b * max_cand + i] = best;
            nbr[(long long)b * max_cand + i] = bj;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the picks of one class
// dynamic LDS of the pick kernel for M member slots; every carve offset is a multiple of 16 (M is rounded up to 16)
struct PickLds {
    f32x4* box; double* val; float* conf; short* nbr; unsigned short* orig; unsigned short* list; unsigned char* alive;
    double* wval; int* widx; int* misc;
    __host__ __device__ static size_t bytes(int M) { return (size_t)M * (16 + 8 + 4 + 2 + 2 + 2 + 1) + CF_WAVES * 12 + 64; }
    __device__ PickLds(unsigned char* p, int M) {
        box = (f32x4*)p; p += (size_t)M * 16;
        val = (double*)p; p += (size_t)M * 8;
        wval = (double*)p; p += CF_WAVES * 8;
        conf = (float*)p; p += (size_t)M * 4;
        widx = (int*)p; p += CF_WAVES * 4;
        misc = (int*)p; p += 64;
        nbr = (short*)p; p += (size_t)M * 2;
        orig = (unsigned short*)p; p += (size_t)M * 2;
        list = (unsigned short*)p; p += (size_t)M * 2;
        alive = p;
    }
};

// value and attaining neighbour of member i over the alive members, by one wavefront (lanes over j)
__device__ __forceinline__ void cf_sweep_member(const PickLds& s, int i, int m, int lane) {
    const f32x4 a = s.box[i];
    // pass 1: the least estimate bounds the minimum from above; pass 2: cf_pair only where the estimate's band reaches that bound
    float emin = INFINITY;
    for (int j = lane; j < m; j += 64) {
        if (j == i || s.alive[j] != 1) continue;          // alive: 1 = alive, 0 = removed, 2 = picked
        const float e = cf_estimate(a, s.box[j]);
        if (e < emin) emin = e;
    }
    emin = cf_wave_min_est(emin);
    double best = 0.0;
    int bj = -1;
    if (cf_lower(emin) < CF_NEIGHBOUR) {                 // wave-uniform
        const double bound = fmin(cf_upper(emin), CF_NEIGHBOUR);
        for (int j = lane; j < m; j += 64) {
            if (j == i || s.alive[j] != 1) continue;
            const f32x4 q = s.box[j];
            if (!(cf_lower(cf_estimate(a, q)) <= bound)) continue;
            const double p = cf_pair(a[0], a[1], a[2], a[3], q[0], q[1], q[2], q[3]);
            if (p < CF_NEIGHBOUR && (bj < 0 || p < best)) { best = p; bj = j; }
        }
    }
    cf_wave_min(best, bj);
    if (lane == 0) {
        s.nbr[i] = (short)bj;
        s.val[i] = bj >= 0 ? best / (double)s.conf[i] : 0.0;          // (:167-173)
    }
}

__global__ __launch_bounds__(CF_THREADS) void confluence_pick_kernel(const float* __restrict__ cand, const int* __restrict__ n_in,
                                                                     int max_cand, int nc, double p_thres,
                                                                     const double* __restrict__ pre_minp, const int* __restrict__ pre_nbr,
                                                                     float* __restrict__ det) {
    extern __shared__ __attribute__((aligned(16))) unsigned char cf_smem[];
    const int M = (max_cand + 15) & ~15;
    const PickLds s(cf_smem, M);
    const int b = blockIdx.x / nc, c = blockIdx.x - b * nc;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = n_in[b];
    if (n < 1 || n > max_cand) return;                   // refused or empty image: the compaction reports it
    const float* cb = cand + (long long)b * max_cand * 6;

    // members of class c in candidate order
    if (tid == 0) s.misc[0] = 0;
    __syncthreads();
    int m = 0;
    for (int i0 = 0; i0 < n; i0 += CF_THREADS) {
        const int i = i0 + tid;
        const bool mine = i < n && cf_class(cb[(long long)i * 6 + 5], nc) == c;
        const unsigned long long bal = __ballot(mine);
        if (lane == 0) s.widx[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < CF_WAVES; ++w) {
            const int v = s.widx[w];
            if (w < wave) before += v;
            total += v;
        }
        if (mine) {
            const int l = m + before + __popcll(bal & ((1ull << lane) - 1ull));
            const float* a = cb + (long long)i * 6;
            f32x4 bx;
            bx[0] = a[0]; bx[1] = a[1]; bx[2] = a[2]; bx[3] = a[3];
            s.box[l] = bx;
            s.conf[l] = a[4];
            s.orig[l] = (unsigned short)i;
            s.alive[l] = 1;
        }
        m += total;
        __syncthreads();
    }
    if (m == 0) return;

    // value and attaining neighbour of every member
    if (pre_minp) {
        for (int l = tid; l < m; l += CF_THREADS) {
            const long long g = (long long)b * max_cand + s.orig[l];
            const int gj = pre_nbr[g];
            int lj = -1;
            if (gj >= 0) {                                // candidate index -> member index: orig[] ascends
                int lo = 0, hi = m - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((int)s.orig[mid] < gj) lo = mid + 1; else hi = mid;
                }
                lj = (int)s.orig[lo] == gj ? lo : -1;
            }
            s.nbr[l] = (short)lj;
            s.val[l] = lj >= 0 ? pre_minp[g] / (double)s.conf[l] : 0.0;
        }
    } else {
        for (int l = wave; l < m; l += CF_WAVES) cf_sweep_member(s, l, m, lane);
    }
    __syncthreads();

    for (int left = m; left > 0;) {                      // every pick removes at least itself
        // arg-min of the value over the alive members, the lowest index on a tie; a value that is not below 10000 counts as 10000
        double bv = CF_START;
        int bi = 0x7fffffff;
        for (int l = tid; l < m; l += CF_THREADS) {
            if (s.alive[l] != 1) continue;
            double v = s.val[l];
            if (!(v < CF_START)) v = CF_START;
            if (v < bv || (v == bv && l < bi)) { bv = v; bi = l; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s.wval[wave] = bv; s.widx[wave] = bi; }
        if (tid == 0) { s.misc[0] = 0; s.misc[1] = 0; }
        __syncthreads();
        bv = s.wval[0]; bi = s.widx[0];
#pragma unroll
        for (int w = 1; w < CF_WAVES; ++w) {
            const double ov = s.wval[w];
            const int oi = s.widx[w];
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (bi >= m) break;                              // nobody alive (cannot happen while left > 0)
        const int pick = bi;
        // remove the pick and every alive j with p(pick, j) < p_thres (:181-190)
        const f32x4 a = s.box[pick];
        int gone = 0;
        for (int l = tid; l < m; l += CF_THREADS) {
            if (s.alive[l] != 1) continue;
            if (l == pick) { s.alive[l] = 2; ++gone; continue; }
            const f32x4 q = s.box[l];
            const float e = cf_estimate(a, q);
            bool out = cf_upper(e) < p_thres;              // surely below; surely not below when cf_lower(e) >= p_thres
            if (!out && !(cf_lower(e) >= p_thres)) out = cf_pair(a[0], a[1], a[2], a[3], q[0], q[1], q[2], q[3]) < p_thres;      // the band, and NaN
            if (out) { s.alive[l] = 0; ++gone; }
        }
        if (gone) atomicAdd(&s.misc[1], gone);
        __syncthreads();
        // the rows whose attaining neighbour went
        for (int l = tid; l < m; l += CF_THREADS) {
            if (s.alive[l] != 1) continue;
            const int j = s.nbr[l];
            if (j >= 0 && s.alive[j] != 1) s.list[atomicAdd(&s.misc[0], 1)] = (unsigned short)l;
        }
        __syncthreads();
        const int nl = s.misc[0];
        left -= s.misc[1];
        for (int k = wave; k < nl; k += CF_WAVES) cf_sweep_member(s, s.list[k], m, lane);
        __syncthreads();
    }
    __syncthreads();
    for (int l = tid; l < m; l += CF_THREADS)
        det[((long long)b * max_cand + s.orig[l]) * 6] = s.alive[l] == 2 ? 1.0f : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------- ordered compaction
__global__ __launch_bounds__(CF_THREADS) void confluence_compact_kernel(const float* __restrict__ cand, const int* __restrict__ n_in,
                                                                        int max_cand, int nc, float* det, int* __restrict__ count,
                                                                        int* __restrict__ keep_idx) {
    __shared__ unsigned char flag[CF_MAX];
    __shared__ int wsum[CF_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n_raw = n_in[b];
    const int n = (n_raw < 0 || n_raw > max_cand) ? 0 : n_raw;
    const float* cb = cand + (long long)b * max_cand * 6;
    float* db = det + (long long)b * max_cand * 6;
    for (int i = tid; i < n; i += CF_THREADS)
        flag[i] = (cf_class(cb[(long long)i * 6 + 5], nc) >= 0 && db[(long long)i * 6] != 0.0f) ? 1 : 0;
    __syncthreads();
    int kept = 0;
    for (int i0 = 0; i0 < n; i0 += CF_THREADS) {
        const int i = i0 + tid;
        const bool mine = i < n && flag[i];
        int total;
        const int before = wg_rank<CF_WAVES>(mine, wsum, total);
        if (mine) {
            const int k = kept + before;                     // k <= i: rows are only read from cand
            const float* a = cb + (long long)i * 6;
            float* o = db + (long long)k * 6;
            o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = a[4]; o[5] = a[5];
            if (keep_idx) keep_idx[(long long)b * max_cand + k] = i;
        }
        kept += total;
    }
    for (int k = kept + tid; k < max_cand; k += CF_THREADS) {
        float* o = db + (long long)k * 6;
        o[0] = o[1] = o[2] = o[3] = o[4] = o[5] = 0.0f;
        if (keep_idx) keep_idx[(long long)b * max_cand + k] = -1;
    }
    if (tid == 0) count[b] = n_raw > max_cand ? -n_raw : kept;
}

struct CfWs { float* cand; int* ncand; double* minp; int* nbr; size_t total; };

static int cf_layout(int B, long long rows, int nc, int max_cand, void* base, CfWs& ws) {
    if (B < 1 || rows < 1 || nc < 1) return fail(ICAF_ERR_ARG, "icaf_confluence: bad B/rows/nc");
    if (max_cand < 1 || max_cand > CF_MAX) return fail(ICAF_ERR_ARG, "icaf_confluence: max_cand must be in [1, %d] (%d)", CF_MAX, max_cand);
    if ((long long)B * nc > 0x7fffffffLL || rows * nc > 0x7fffffffLL)
        return fail(ICAF_ERR_UNSUPPORTED, "icaf_confluence: B * nc and rows * nc must stay below 2^31");
    WsArena ar(base);
    ws.cand = ar.take_as<float>((size_t)B * max_cand * 6 * 4);
    ws.minp = ar.take_as<double>((size_t)B * max_cand * 8);
    ws.nbr = ar.take_as<int>((size_t)B * max_cand * 4);
    ws.ncand = ar.take_as<int>((size_t)B * 4);
    ws.total = ar.total;
    return ICAF_OK;
}

// pick + compaction on a candidate list; pre_minp / pre_nbr: the result of confluence_sweep_kernel or NULL
static int cf_select(const float* cand, const int* n, int B, int max_cand, int nc, double p_thres, const double* pre_minp, const int* pre_nbr,
                     float* det, int* count, int* keep_idx, hipStream_t hs) {
    const size_t lds = PickLds::bytes((max_cand + 15) & ~15);
    ICAF_LDS_OPTIN(confluence_pick_kernel, lds);
    confluence_pick_kernel<<<dim3((unsigned)(B * nc)), dim3(CF_THREADS), lds, hs>>>(cand, n, max_cand, nc, p_thres, pre_minp, pre_nbr, det);
    ICAF_LAUNCH_CHECK();
    confluence_compact_kernel<<<dim3((unsigned)B), dim3(CF_THREADS), 0, hs>>>(cand, n, max_cand, nc, det, count, keep_idx);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_confluence_select(const float* cand, const int* n, int B, int max_cand, int nc, double p_thres, float* det, int* count,
                                      int* keep_idx, icaf_stream_t s) {
    if (!cand || !n || !det || !count) return fail(ICAF_ERR_ARG, "icaf_confluence_select: null pointer");
    if (B < 1 || nc < 1 || (long long)B * nc > 0x7fffffffLL) return fail(ICAF_ERR_ARG, "icaf_confluence_select: bad B/nc (%d, %d)", B, nc);
    if (max_cand < 1 || max_cand > CF_MAX)
        return fail(ICAF_ERR_ARG, "icaf_confluence_select: max_cand must be in [1, %d] (%d)", CF_MAX, max_cand);
    if (!(p_thres == p_thres)) return fail(ICAF_ERR_ARG, "icaf_confluence_select: p_thres is NaN");
    return cf_select(cand, n, B, max_cand, nc, p_thres, nullptr, nullptr, det, count, keep_idx, S(s));
}

extern "C" int icaf_confluence_workspace_bytes(int B, long long rows, int nc, int max_cand, size_t* bytes) {
    if (!bytes) return fail(ICAF_ERR_ARG, "icaf_confluence_workspace_bytes: null pointer");
    CfWs ws;
    const int st = cf_layout(B, rows, nc, max_cand, nullptr, ws);
    if (st) return st;
    *bytes = ws.total;
    return ICAF_OK;
}

extern "C" int icaf_confluence(const float* pred, int B, long long rows, int nc, float conf_thres, double p_thres, int max_cand, float* det,
                               int* count, int* keep_idx, void* workspace, size_t workspace_bytes, icaf_stream_t s) {
    if (!pred || !det || !count || !workspace) return fail(ICAF_ERR_ARG, "icaf_confluence: null pointer");
    if (((uintptr_t)workspace & 255) != 0) return fail(ICAF_ERR_ARG, "icaf_confluence: workspace must be 256-byte aligned");
    if (!(conf_thres >= 2e-4f))
        return fail(ICAF_ERR_ARG, "icaf_confluence: conf_thres must be at least 2e-4 (%g): a value p / conf may not reach 10000", (double)conf_thres);
    if (!(p_thres == p_thres)) return fail(ICAF_ERR_ARG, "icaf_confluence: p_thres is NaN");
    CfWs ws;
    const int st = cf_layout(B, rows, nc, max_cand, workspace, ws);
    if (st) return st;
    if (ws.total > workspace_bytes) return fail(ICAF_ERR_ARG, "icaf_confluence: workspace too small (%zu < %zu)", workspace_bytes, ws.total);
    hipStream_t hs = S(s);
    confluence_cand_kernel<<<dim3((unsigned)B), dim3(CF_THREADS), 0, hs>>>(pred, rows, nc, conf_thres, max_cand, ws.cand, ws.ncand);
    ICAF_LAUNCH_CHECK();
    const int per_block = (CF_SWEEP_THREADS / 64) * CF_SWEEP_ROWS;
    confluence_sweep_kernel<<<dim3((unsigned)((max_cand + per_block - 1) / per_block), (unsigned)B), dim3(CF_SWEEP_THREADS), 0, hs>>>(
        ws.cand, ws.ncand, max_cand, nc, ws.minp, ws.nbr);
    ICAF_LAUNCH_CHECK();
    return cf_select(ws.cand, ws.ncand, B, max_cand, nc, p_thres, ws.minp, ws.nbr, det, count, keep_idx, hs);
}
