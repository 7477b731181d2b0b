// Validation statistics on the device (the reference's test.py:144-230 bookkeeping, utils/metrics.py:18-82, 85-110 and 113-159) for gfx950.
//
//   icaf_match_predictions  one workgroup per image: the detections mapped to the native image (predn, which the confusion matrix reads) and
//                           their TP flags at every IoU threshold; described at its kernel.
//   icaf_stats_stage        one 1024-thread workgroup per batch: exclusive prefix of the clamped counts, then every row below its image's count
//                           goes to the data-set-wide store at cursor + prefix + row — image order, then row order, the order in which the host
//                           loop concatenates its per-image statistics.  The cursor is read once and advanced once by the same workgroup: no
//                           atomic decides an order.  The TP flags of a row are packed into 16 bits.
//   icaf_ap_per_class       sort   stable LSD radix sort, 8 bits a pass, of (key, arrival index): four passes over ~bits(conf) (the pattern of a
//                                  non-negative fp32 orders as its value; inverted: descending), one over the class.  Equal keys keep their
//                                  arrival order in every pass, so the result is class ascending, confidence descending, arrival ascending.
//                                  A pass is three launches: per-tile digit histograms (VS_TILE rows a workgroup), one exclusive scan over the
//                                  digit-major [256][tiles] table, and the scatter.  The scatter is stable across tile boundaries because the
//                                  scanned table gives tile t its own first slot per digit, and stable inside a tile because every wave owns a
//                                  contiguous quarter of it (wave-private cursors, seeded in wave order) and ranks the 64 rows of a step with
//                                  ballots: a row's slot is cursor + the number of lower lanes holding the same digit.
//                           scans  one workgroup per (class, threshold) walks the class's rows 1024 at a time: integer inclusive scan of the TP
//                                  bit (tpc; fpc = row + 1 - tpc), then the 101 AP samples (binary search on recall, the precision envelope by a
//                                  reverse running maximum evaluated only where a sample needs it) and, for threshold 0, the 1000-point P / R curves.
//                           report one workgroup: F1 curves, first argmax of the class mean, TP / FP / FN at that index.
//   icaf_confusion_matrix   one workgroup per image; integer atomics into the (nc + 1)^2 matrix (integer adds commute: deterministic).
// fp64 with contraction off wherever the reference computes in numpy float64; np.interp is restated rule for rule (vs_interp).
// The exclusive scans (stage, sort) are a per-thread run around box_core.h's wg_incl_scan, the TP count is its wg_rank, and both IoU
// loops call its box_iou — the matching with the detection first, the confusion matrix with the label first, as the reference does.
#pragma clang fp contract(off)
#include "box_core.h"

namespace icaf {

constexpr int VS_TILE = ICAF_STATS_SORT_TILE;              // rows per workgroup of the sort kernels
constexpr int VS_SORT_THREADS = 256;
constexpr int VS_SUB = VS_TILE / 4;                        // rows per wave
constexpr int VS_MAX_T = ICAF_STATS_MAX_T;
constexpr int VS_MAX_ROWS = ICAF_STATS_MAX_ROWS;
constexpr int VS_MAX_BATCH = ICAF_STATS_MAX_BATCH;
constexpr int VS_PX = ICAF_AP_CURVE_POINTS;                // np.linspace(0, 1, 1000)
constexpr int VS_AP_POINTS = 101;
constexpr int VS_WG = 1024;
constexpr int CM_MAX_DET = 1024;

__device__ __forceinline__ int vs_clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- matching: TP flags of every detection at every IoU threshold (reference test.py:196-230) ------------------------------------------------------
// One workgroup per image.  Detections arrive as the NMS output block (letterboxed pixel space) and are first mapped to
// the native image (scale_coords + clip_coords, utils/general.py:386-407: subtract the pad, divide by the gain, clip).
// Phase 1, one thread per detection: best IoU over the labels of its class and the FIRST label reaching it (box_iou +
// torch max).  Phase 2, one thread: detections in index order claim their best label if nobody has and the IoU exceeds
// iouv[0]; a claim marks correct[i][t] = best > iouv[t].  (The reference walks class by class; claims of different
// classes never touch the same label, so index order gives the same flags.)  fp32, no contraction: the IoU values are
// bit-identical to the numpy statement of the same formula (icafusion_amd/utils/metrics.py, the test oracle).
constexpr int MATCH_MAX_DET = 1024, MATCH_MAX_LABELS = 2048;

__global__ __launch_bounds__(256) void match_predictions_kernel(const float* __restrict__ det, const int* __restrict__ count, int max_det,
                                                                const float* __restrict__ labels, const int* __restrict__ label_off,
                                                                const float* __restrict__ scale, const float* __restrict__ iouv, int T,
                                                                unsigned char* __restrict__ correct, float* __restrict__ predn) {
    __shared__ float best[MATCH_MAX_DET];
    __shared__ int arg[MATCH_MAX_DET];
    __shared__ unsigned char claimed[MATCH_MAX_LABELS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(count[b], max_det), l0 = label_off[b], nl = label_off[b + 1] - l0;
    const float* db = det + (long long)b * max_det * 6;
    for (int i = tid; i < nl; i += 256) claimed[i] = 0;
    for (int i = tid; i < n; i += 256) {
        float x1 = db[i * 6], y1 = db[i * 6 + 1], x2 = db[i * 6 + 2], y2 = db[i * 6 + 3];
        const float cls = db[i * 6 + 5];
        if (scale) native_box(scale + b * 5, x1, y1, x2, y2);
        if (predn) {
            float* o = predn + ((long long)b * max_det + i) * 4;
            o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
        }
        const float area_a = (x2 - x1) * (y2 - y1);
        float bst = -1.0f;
        int ba = -1;
        for (int j = 0; j < nl; ++j) {
            const float* lb = labels + (long long)(l0 + j) * 5;
            if (lb[0] != cls) continue;
            const float iou = box_iou(x1, y1, x2, y2, area_a, lb[1], lb[2], lb[3], lb[4], (lb[3] - lb[1]) * (lb[4] - lb[2]));
            if (iou > bst) { bst = iou; ba = j; }
        }
        best[i] = bst;
        arg[i] = ba;
        for (int t = 0; t < T; ++t) correct[((long long)b * max_det + i) * T + t] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        const float thr0 = iouv[0];
        int found = 0;
        for (int i = 0; i < n && found < nl; ++i) {
            if (arg[i] < 0 || !(best[i] > thr0) || claimed[arg[i]]) continue;
            claimed[arg[i]] = 1;
            ++found;
            for (int t = 0; t < T; ++t) correct[((long long)b * max_det + i) * T + t] = best[i] > iouv[t] ? 1 : 0;
        }
    }
}

// ---- stage ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VS_WG) void stats_stage_kernel(const unsigned char* __restrict__ correct, const float* __restrict__ det,
                                                            const int* __restrict__ count, int B, int max_det, int T,
                                                            unsigned short* __restrict__ store_mask, float* __restrict__ store_conf,
                                                            int* __restrict__ store_cls, int capacity, int* cursor, int* any_tp) {
    __shared__ int s_off[VS_MAX_BATCH + 1];
    __shared__ int s_ws[VS_WG / 64];
    const int tid = threadIdx.x;
    const int per = (B + VS_WG - 1) / VS_WG, b0 = min(tid * per, B), b1 = min(b0 + per, B);      // a thread owns `per` consecutive images
    int sum = 0, total;
    for (int b = b0; b < b1; ++b) sum += vs_clampi(count[b], 0, max_det);
    int run = wg_incl_scan<VS_WG / 64>(sum, s_ws, total) - sum;
    for (int b = b0; b < b1; ++b) {
        s_off[b] = run;
        run += vs_clampi(count[b], 0, max_det);
    }
    if (tid == 0) s_off[B] = total;
    __syncthreads();                                                            // s_off is complete before the rows below look images up in it
    const int base = *cursor;
    const long long cells = (long long)B * max_det;
    unsigned int any = 0;
    if (base >= 0 && base <= capacity) {
        for (long long idx = tid; idx < cells; idx += VS_WG) {
            const int b = (int)(idx / max_det), i = (int)(idx - (long long)b * max_det);
            if (i >= s_off[b + 1] - s_off[b]) continue;                        // rows at or beyond count[b] are never read
            const long long dst = (long long)base + s_off[b] + i;
            if (dst >= capacity) continue;                                      // never write at or beyond the capacity
            const unsigned char* c = correct + idx * T;
            unsigned int m = 0;
            for (int t = 0; t < T; ++t) m |= (c[t] ? 1u : 0u) << t;
            store_mask[dst] = (unsigned short)m;
            store_conf[dst] = det[idx * 6 + 4];
            store_cls[dst] = (int)det[idx * 6 + 5];
            any |= m;
        }
    }
    if (any) atomicOr(any_tp, 1);
    __syncthreads();                                                            // every thread has read the cursor
    if (tid == 0 && base >= 0 && base <= capacity) *cursor = base + total;      // above the capacity: the host sees the overflow
}

// ---- sort ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sort_init_kernel(const float* __restrict__ conf, unsigned int* __restrict__ key,
                                                        unsigned int* __restrict__ idx, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float c = conf[i];
    const unsigned int bits = c == 0.0f ? 0u : __float_as_uint(c);              // -0 sorts as 0
    key[i] = ~bits;
    idx[i] = (unsigned int)i;
}

// digit of a row in a pass: 8 bits of the key, or (cls != nullptr) the class, held to [0, 255] so that no table is indexed outside
__device__ __forceinline__ int vs_digit(unsigned int key, unsigned int idx, int shift, const int* __restrict__ cls) {
    return cls ? vs_clampi(cls[idx], 0, 255) : (int)((key >> shift) & 255u);
}

__global__ __launch_bounds__(VS_SORT_THREADS) void sort_hist_kernel(const unsigned int* __restrict__ key, const unsigned int* __restrict__ idx,
                                                                    int n, int shift, const int* __restrict__ cls, int ntiles,
                                                                    int* __restrict__ hist) {
    __shared__ int s_h[256];
    const int tid = threadIdx.x, tile = blockIdx.x;
    s_h[tid] = 0;
    __syncthreads();
    const int r0 = tile * VS_TILE, r1 = min(r0 + VS_TILE, n);
    for (int i = r0 + tid; i < r1; i += VS_SORT_THREADS) atomicAdd(&s_h[vs_digit(key[i], idx[i], shift, cls)], 1);
    __syncthreads();
    hist[(long long)tid * ntiles + tile] = s_h[tid];                            // digit-major: a flat exclusive scan gives the first slots
}

// exclusive scan of m ints in place, one workgroup
__global__ __launch_bounds__(VS_WG) void sort_scan_kernel(int* __restrict__ a, int m) {
    __shared__ int s_ws[VS_WG / 64];
    const int tid = threadIdx.x;
    const int per = (m + VS_WG - 1) / VS_WG;
    const long long lo = min((long long)tid * per, (long long)m), hi = min(lo + per, (long long)m);
    int sum = 0, total;
    for (long long i = lo; i < hi; ++i) sum += a[i];
    int run = wg_incl_scan<VS_WG / 64>(sum, s_ws, total) - sum;
    for (long long i = lo; i < hi; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(VS_SORT_THREADS) void sort_scatter_kernel(const unsigned int* __restrict__ key, const unsigned int* __restrict__ idx,
                                                                       int n, int shift, const int* __restrict__ cls, int ntiles,
                                                                       const int* __restrict__ offs, unsigned int* __restrict__ key_out,
                                                                       unsigned int* __restrict__ idx_out) {
    __shared__ int s_w[4][256];                              // per wave and digit: the count, then the wave's next slot
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
#pragma unroll
    for (int w = 0; w < 4; ++w) s_w[w][tid] = 0;
    __syncthreads();
    const int t0 = min(tile * VS_TILE + wave * VS_SUB, n), t1 = min(t0 + VS_SUB, n);
    for (int i = t0 + lane; i < t1; i += 64) atomicAdd(&s_w[wave][vs_digit(key[i], idx[i], shift, cls)], 1);
    __syncthreads();
    {
        int b = offs[(long long)tid * ntiles + tile];        // first slot of digit `tid` for this tile; the waves follow in order
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = s_w[w][tid];
            s_w[w][tid] = b;
            b += c;
        }
    }
    __syncthreads();
    for (int i0 = t0; i0 < t1; i0 += 64) {                   // wave-uniform
        const int i = i0 + lane;
        const bool valid = i < t1;
        const unsigned int k = valid ? key[i] : 0u, x = valid ? idx[i] : 0u;
        const int d = valid ? vs_digit(k, x, shift, cls) : 0;
        unsigned long long peers = __ballot(valid);          // the valid lanes holding this lane's digit
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1;
            const unsigned long long bl = __ballot(on);
            peers &= on ? bl : ~bl;
        }
        const int leader = valid ? __ffsll((long long)peers) - 1 : lane;
        int first = 0;
        if (valid && lane == leader) first = atomicAdd(&s_w[wave][d], __popcll(peers));
        first = __shfl(first, leader);
        if (valid) {
            const int dst = first + __popcll(peers & ((1ull << lane) - 1ull));
            if (dst >= 0 && dst < n) {
                key_out[dst] = k;
                idx_out[dst] = x;
            }
        }
    }
}

__global__ __launch_bounds__(256) void sort_gather_kernel(const unsigned int* __restrict__ idx, const unsigned short* __restrict__ mask,
                                                          const float* __restrict__ conf, int n, unsigned short* __restrict__ smask,
                                                          float* __restrict__ sconf, int* __restrict__ perm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned int a = min(idx[i], (unsigned int)(n - 1));
    smask[i] = mask[a];
    sconf[i] = conf[a];
    if (perm) perm[i] = (int)a;
}

// ---- curves --------------------------------------------------------------------------------------------------------------------------------
// np.interp's value once j = the largest index with xp[j] <= x is known (xp[0] <= x <= xp[last]); (xj1, fj1) are read only when used
__device__ __forceinline__ double vs_interp(double x, double xj, double fj, double xj1, double fj1, bool last) {
    if (last || xj == x) return fj;
    const double slope = (fj1 - fj) / (xj1 - xj);
    return slope * (x - xj) + fj;
}

__device__ __forceinline__ double vs_linspace(int k, int num) {                // np.linspace(0, 1, num)[k]
    return k == num - 1 ? 1.0 : (double)k * (1.0 / (double)(num - 1));
}

__global__ __launch_bounds__(VS_WG) void ap_class_kernel(const unsigned short* __restrict__ smask, const float* __restrict__ sconf, int n,
                                                         int ntiles, const int* __restrict__ offs, const int* __restrict__ uniq,
                                                         const int* __restrict__ n_l, int T, int* tpc, double* __restrict__ ap,
                                                         double* __restrict__ p, double* __restrict__ r) {
    __shared__ int s_ws[16];
    __shared__ double s_wm[16];
    __shared__ double s_env[VS_WG];
    __shared__ double s_y[VS_AP_POINTS];
    const int t = blockIdx.x, ci = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = uniq[ci], nl = n_l[ci];
    int s = 0, e = 0;                                         // the class's rows of the sorted store: the class pass's first slots
    if (ntiles > 0 && c >= 0 && c <= 255) {
        s = offs[(long long)c * ntiles];
        e = c < 255 ? offs[(long long)(c + 1) * ntiles] : n;
        s = vs_clampi(s, 0, n);
        e = vs_clampi(e, s, n);
    }
    const int np_ = e - s;
    if (np_ == 0 || nl <= 0) {                                // utils/metrics.py:48-49: the class keeps its zero rows
        if (tid == 0) ap[ci * T + t] = 0.0;
        if (t == 0 && tid < VS_PX) {
            p[(long long)ci * VS_PX + tid] = 0.0;
            r[(long long)ci * VS_PX + tid] = 0.0;
        }
        return;
    }
    int* tp = tpc + (long long)t * n + s;                     // tp[j]: inclusive TP count of the class's row j at threshold t
    int running = 0;
    for (int c0 = 0; c0 < np_; c0 += VS_WG) {
        const int j = c0 + tid;
        const bool bit = j < np_ && ((smask[s + j] >> t) & 1);
        int tot;
        const int before = wg_rank<16>(bit, s_ws, tot);
        if (j < np_) tp[j] = running + before + (bit ? 1 : 0);
        running += tot;
    }
    __threadfence_block();
    __syncthreads();                                          // the workgroup reads its own tpc row below
    const double nld = (double)nl + 1e-16;

    // AP (compute_ap, :85-110): mrec = [0, recall, recall[-1] + 0.01], mpre = envelope of [1, precision, 0]; m = np_ + 2 points
    const int m = np_ + 2;
    double x = 0.0, xj = 0.0, xj1 = 0.0;
    int j = -1;                                               // -1: beyond mrec[-1], the value is mpre[-1] = 0
    bool last = false;
    if (tid < VS_AP_POINTS) {
        x = vs_linspace(tid, VS_AP_POINTS);
        const double rec_last = (double)tp[np_ - 1] / nld, end = rec_last + 0.01;
        if (!(x > end)) {
            int lo = 0, hi = m - 1;
            while (lo < hi) {
                const int mid = lo + (hi - lo + 1) / 2;
                const double v = mid == m - 1 ? end : (double)tp[mid - 1] / nld;
                if (v <= x) lo = mid; else hi = mid - 1;
            }
            j = lo;
            last = j == m - 1;
            xj = j == 0 ? 0.0 : (j == m - 1 ? end : (double)tp[j - 1] / nld);
            if (!last) xj1 = j + 1 == m - 1 ? end : (double)tp[j] / nld;
        }
    }
    // envelope values wanted: mpre[j] and mpre[j + 1]; mpre[0] = 1 (precision <= 1), mpre[m - 1] = 0, mpre[q + 1] = max(precision[q:], 0)
    const int qa = (j >= 1 && j <= np_) ? j - 1 : -1, qb = (j >= 0 && !last && j + 1 <= np_) ? j : -1;
    double ea = j == 0 ? 1.0 : 0.0, eb = 0.0;
    double rm = 0.0;
    for (int c0 = ((np_ - 1) / VS_WG) * VS_WG; c0 >= 0; c0 -= VS_WG) {
        const int q = c0 + tid;
        double sv = q < np_ ? (double)tp[q] / (double)(q + 1) : 0.0;             // tpc / (tpc + fpc)
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_down(sv, off);
            if (lane + off < 64) sv = fmax(sv, o);
        }
        if (lane == 0) s_wm[wave] = sv;
        __syncthreads();
        double later = rm;
        for (int w = wave + 1; w < 16; ++w) later = fmax(later, s_wm[w]);
        s_env[tid] = fmax(sv, later);
        __syncthreads();
        if (qa >= c0 && qa < c0 + VS_WG) ea = s_env[qa - c0];
        if (qb >= c0 && qb < c0 + VS_WG) eb = s_env[qb - c0];
        rm = s_env[0];
        __syncthreads();
    }
    if (tid < VS_AP_POINTS) s_y[tid] = j < 0 ? 0.0 : vs_interp(x, xj, ea, xj1, eb, last);
    __syncthreads();
    if (tid == 0) {                                           // np.trapz: sum of d * (y1 + y0) / 2, here in index order
        double acc = 0.0;
        for (int k = 0; k + 1 < VS_AP_POINTS; ++k) {
            const double d = vs_linspace(k + 1, VS_AP_POINTS) - vs_linspace(k, VS_AP_POINTS);
            acc += d * (s_y[k + 1] + s_y[k]) / 2.0;
        }
        ap[ci * T + t] = acc;
    }

    // P / R curves (:56-61) at threshold 0: np.interp(-px, -conf, f, left)
    if (t == 0 && tid < VS_PX) {
        const double xq = -vs_linspace(tid, VS_PX);
        const float* cf = sconf + s;
        double rv, pv;
        if (xq < -(double)cf[0]) {
            rv = 0.0;
            pv = 1.0;
        } else if (xq > -(double)cf[np_ - 1]) {
            rv = (double)tp[np_ - 1] / nld;
            pv = (double)tp[np_ - 1] / (double)np_;
        } else {
            int lo = 0, hi = np_ - 1;
            while (lo < hi) {
                const int mid = lo + (hi - lo + 1) / 2;
                if (-(double)cf[mid] <= xq) lo = mid; else hi = mid - 1;
            }
            const bool lst = lo == np_ - 1;
            const double x0 = -(double)cf[lo], x1 = lst ? 0.0 : -(double)cf[lo + 1];
            const double r0 = (double)tp[lo] / nld, p0 = (double)tp[lo] / (double)(lo + 1);
            const double r1 = lst ? 0.0 : (double)tp[lo + 1] / nld, p1 = lst ? 0.0 : (double)tp[lo + 1] / (double)(lo + 2);
            rv = vs_interp(xq, x0, r0, x1, r1, lst);
            pv = vs_interp(xq, x0, p0, x1, p1, lst);
        }
        r[(long long)ci * VS_PX + tid] = rv;
        p[(long long)ci * VS_PX + tid] = pv;
    }
}

// F1 curves, the first argmax of their class mean (:70, 77) and TP / FP / FN there (:78-80; n_l is the loop's last value: the last class's)
__global__ __launch_bounds__(VS_WG) void ap_report_kernel(const double* __restrict__ p, const double* __restrict__ r, const int* __restrict__ n_l,
                                                          int nu, double* __restrict__ f1, int* __restrict__ best, double* __restrict__ report) {
    __shared__ double s_mean[VS_PX];
    __shared__ int s_best;
    const int tid = threadIdx.x;
    if (tid < VS_PX) {
        double sum = 0.0;
        for (int ci = 0; ci < nu; ++ci) {
            const double pp = p[(long long)ci * VS_PX + tid], rr = r[(long long)ci * VS_PX + tid];
            const double f = 2.0 * pp * rr / (pp + rr + 1e-16);
            f1[(long long)ci * VS_PX + tid] = f;
            sum += f;
        }
        s_mean[tid] = sum / (double)nu;
    }
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int k = 1; k < VS_PX; ++k)
            if (s_mean[k] > s_mean[b]) b = k;
        s_best = b;
        *best = b;
    }
    __syncthreads();
    const int b = s_best;
    const double nl = (double)n_l[nu - 1];
    for (int ci = tid; ci < nu; ci += VS_WG) {
        const double pp = p[(long long)ci * VS_PX + b], rr = r[(long long)ci * VS_PX + b];
        const double tpn = rint(rr * nl);                    // np.round: half to even
        report[ci * 3 + 0] = tpn;
        report[ci * 3 + 1] = rint(tpn / (pp + 1e-16) - tpn);
        report[ci * 3 + 2] = nl - tpn;
    }
}

// ---- confusion matrix (ConfusionMatrix.process_batch, utils/metrics.py:121-159) ------------------------------------------------------------------
__global__ __launch_bounds__(256) void confusion_matrix_kernel(const float* __restrict__ predn, const float* __restrict__ det,
                                                               const int* __restrict__ count, int max_det, const float* __restrict__ labels,
                                                               const int* __restrict__ label_off, int nc, float conf, float iou_thres,
                                                               int* matrix) {
    __shared__ int s_lab[CM_MAX_DET];                         // the detection's label (local index), -1 none, -2 not kept
    __shared__ float s_iou[CM_MAX_DET];
    __shared__ unsigned char s_used[CM_MAX_DET];
    __shared__ int s_any;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = vs_clampi(count[b], 0, min(max_det, CM_MAX_DET)), l0 = label_off[b], nl = label_off[b + 1] - l0;
    if (n == 0 || nl <= 0) return;                            // test.py:151-153, 198-206: process_batch is never called for such an image
    if (tid == 0) s_any = 0;
    const float* db = det + (long long)b * max_det * 6;
    const float* pb = predn + (long long)b * max_det * 4;
    for (int d = tid; d < n; d += 256) {
        int bl = -2;
        float bi = 0.0f;
        if (db[d * 6 + 4] > conf) {
            bl = -1;
            const float x1 = pb[d * 4], y1 = pb[d * 4 + 1], x2 = pb[d * 4 + 2], y2 = pb[d * 4 + 3];
            const float area_d = (x2 - x1) * (y2 - y1);
            for (int j = 0; j < nl; ++j) {                   // box_iou(labels, detections), utils/general.py:455-477
                const float* lb = labels + (long long)(l0 + j) * 5;
                const float area_l = (lb[3] - lb[1]) * (lb[4] - lb[2]);
                const float iou = box_iou(lb[1], lb[2], lb[3], lb[4], area_l, x1, y1, x2, y2, area_d);
                if (iou > iou_thres && (bl < 0 || iou > bi)) { bl = j; bi = iou; }        // the lowest label index wins a tie
            }
        }
        s_lab[d] = bl;
        s_iou[d] = bi;
        s_used[d] = 0;
    }
    __syncthreads();
    const int stride = nc + 1;
    for (int j = tid; j < nl; j += 256) {
        int bd = -1;
        float bi = 0.0f;
        for (int d = 0; d < n; ++d)
            if (s_lab[d] == j && (bd < 0 || s_iou[d] > bi)) { bd = d; bi = s_iou[d]; }    // the lowest detection index wins a tie
        const int gc = (int)labels[(long long)(l0 + j) * 5];
        if (gc < 0 || gc >= nc) continue;                    // never index outside the matrix
        if (bd >= 0) {
            s_used[bd] = 1;                                   // a detection chose one label: no other thread writes this flag
            atomicOr(&s_any, 1);
            const int dc = (int)db[bd * 6 + 5];
            if (dc >= 0 && dc < nc) atomicAdd(&matrix[dc * stride + gc], 1);
        } else {
            atomicAdd(&matrix[nc * stride + gc], 1);
        }
    }
    __syncthreads();
    if (!s_any) return;                                       // the reference's `if n:`: without a match no unmatched detection is counted
    for (int d = tid; d < n; d += 256) {
        if (s_lab[d] == -2 || s_used[d]) continue;
        const int dc = (int)db[d * 6 + 5];
        if (dc >= 0 && dc < nc) atomicAdd(&matrix[dc * stride + nc], 1);
    }
}

struct ApWs {
    size_t key[2], idx[2], hist, smask, sconf, tpc, bytes;
    int ntiles;
};

static ApWs ap_layout(int n, int T) {
    ApWs w;
    WsArena ar;
    const size_t rows = (size_t)(n > 0 ? n : 1);
    w.ntiles = (n + VS_TILE - 1) / VS_TILE;
    for (int k = 0; k < 2; ++k) w.key[k] = ar.take(rows * 4);
    for (int k = 0; k < 2; ++k) w.idx[k] = ar.take(rows * 4);
    w.hist = ar.take((size_t)256 * (size_t)(w.ntiles > 0 ? w.ntiles : 1) * 4);
    w.smask = ar.take(rows * 2);
    w.sconf = ar.take(rows * 4);
    w.tpc = ar.take(rows * 4 * (size_t)T);
    w.bytes = ar.total;
    return w;
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_match_predictions(const float* det, const int* count, int B, int max_det, const float* labels, const int* label_off,
                                      int max_labels_per_image, const float* scale, const float* iouv, int T, unsigned char* correct,
                                      float* predn, icaf_stream_t s) {
    if (!det || !count || !label_off || !iouv || !correct) return fail(ICAF_ERR_ARG, "icaf_match_predictions: null pointer");
    if (B < 1 || T < 1 || max_det < 1 || max_det > MATCH_MAX_DET) return fail(ICAF_ERR_ARG, "icaf_match_predictions: max_det must be in [1, %d]", MATCH_MAX_DET);
    if (max_labels_per_image > MATCH_MAX_LABELS) return fail(ICAF_ERR_UNSUPPORTED, "icaf_match_predictions: at most %d labels per image", MATCH_MAX_LABELS);
    if (max_labels_per_image > 0 && !labels) return fail(ICAF_ERR_ARG, "icaf_match_predictions: labels missing");
    match_predictions_kernel<<<dim3((unsigned)B), dim3(256), 0, S(s)>>>(det, count, max_det, labels, label_off, scale, iouv, T, correct, predn);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

extern "C" int icaf_stats_stage(const unsigned char* correct, const float* det, const int* count, int B, int max_det, int T,
                                void* store_mask, float* store_conf, int* store_cls, int capacity, int* cursor, int* any_tp,
                                icaf_stream_t s) {
    if (!correct || !det || !count || !store_mask || !store_conf || !store_cls || !cursor || !any_tp)
        return fail(ICAF_ERR_ARG, "icaf_stats_stage: null pointer");
    if (T < 1 || T > VS_MAX_T) return fail(ICAF_ERR_UNSUPPORTED, "icaf_stats_stage: T must be in [1, %d] (%d)", VS_MAX_T, T);
    if (capacity < 1 || capacity > VS_MAX_ROWS)
        return fail(ICAF_ERR_UNSUPPORTED, "icaf_stats_stage: the store's capacity must be in [1, %d] rows (%d)", VS_MAX_ROWS, capacity);
    if (B < 1 || B > VS_MAX_BATCH) return fail(ICAF_ERR_UNSUPPORTED, "icaf_stats_stage: B must be in [1, %d] (%d)", VS_MAX_BATCH, B);
    if (max_det < 1 || max_det > 65536) return fail(ICAF_ERR_ARG, "icaf_stats_stage: max_det must be in [1, 65536] (%d)", max_det);
    stats_stage_kernel<<<dim3(1), dim3(VS_WG), 0, S(s)>>>(correct, det, count, B, max_det, T, (unsigned short*)store_mask, store_conf, store_cls, capacity,
                                                         cursor, any_tp);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

static int ap_check(const char* who, int n, int T) {
    if (T < 1 || T > VS_MAX_T) return fail(ICAF_ERR_UNSUPPORTED, "%s: T must be in [1, %d] (%d)", who, VS_MAX_T, T);
    if (n < 0 || n > VS_MAX_ROWS) return fail(ICAF_ERR_UNSUPPORTED, "%s: the row count must be in [0, %d] (%d)", who, VS_MAX_ROWS, n);
    return ICAF_OK;
}

extern "C" int icaf_ap_workspace_bytes(int n, int T, size_t* bytes, size_t* tpc_off) {
    if (!bytes) return fail(ICAF_ERR_ARG, "icaf_ap_workspace_bytes: null pointer");
    const int st = ap_check("icaf_ap_workspace_bytes", n, T);
    if (st) return st;
    const ApWs w = ap_layout(n, T);
    *bytes = w.bytes;
    if (tpc_off) *tpc_off = w.tpc;
    return ICAF_OK;
}

extern "C" int icaf_ap_per_class(const void* mask, const float* conf, const int* cls, int n, int T, const int* unique_classes,
                                 const int* n_l, int nc, double* ap, double* p, double* r, double* f1, int* best, double* report, int* perm,
                                 void* workspace, size_t workspace_bytes, icaf_stream_t s) {
    if (nc > ICAF_STATS_MAX_CLASSES)
        return fail(ICAF_ERR_UNSUPPORTED, "icaf_ap_per_class: at most %d classes, one 8-bit pass sorts them (%d)", ICAF_STATS_MAX_CLASSES, nc);
    if (nc < 1) return fail(ICAF_ERR_ARG, "icaf_ap_per_class: nc must be positive (%d)", nc);
    const int st = ap_check("icaf_ap_per_class", n, T);
    if (st) return st;
    if (!unique_classes || !n_l || !ap || !p || !r || !f1 || !best || !report || !workspace || (n > 0 && (!mask || !conf || !cls)))
        return fail(ICAF_ERR_ARG, "icaf_ap_per_class: null pointer");
    const ApWs w = ap_layout(n, T);
    if (workspace_bytes < w.bytes || ((uintptr_t)workspace & 255))
        return fail(ICAF_ERR_ARG, "icaf_ap_per_class: the workspace must hold %zu bytes at a 256-byte boundary", w.bytes);
    char* base = (char*)workspace;
    unsigned int* key[2] = {(unsigned int*)(base + w.key[0]), (unsigned int*)(base + w.key[1])};
    unsigned int* idx[2] = {(unsigned int*)(base + w.idx[0]), (unsigned int*)(base + w.idx[1])};
    int* hist = (int*)(base + w.hist);
    unsigned short* smask = (unsigned short*)(base + w.smask);
    float* sconf = (float*)(base + w.sconf);
    int* tpc = (int*)(base + w.tpc);
    if (n > 0) {
        const unsigned g256 = (unsigned)((n + 255) / 256), tiles = (unsigned)w.ntiles;
        sort_init_kernel<<<dim3(g256), dim3(256), 0, S(s)>>>(conf, key[0], idx[0], n);
        ICAF_LAUNCH_CHECK();
        int cur = 0;
        for (int pass = 0; pass < 5; ++pass) {
            const int shift = pass * 8;
            const int* pc = pass == 4 ? cls : nullptr;
            sort_hist_kernel<<<dim3(tiles), dim3(VS_SORT_THREADS), 0, S(s)>>>(key[cur], idx[cur], n, shift, pc, w.ntiles, hist);
            ICAF_LAUNCH_CHECK();
            sort_scan_kernel<<<dim3(1), dim3(VS_WG), 0, S(s)>>>(hist, 256 * w.ntiles);
            ICAF_LAUNCH_CHECK();
            sort_scatter_kernel<<<dim3(tiles), dim3(VS_SORT_THREADS), 0, S(s)>>>(key[cur], idx[cur], n, shift, pc, w.ntiles, hist, key[cur ^ 1],
                                                                               idx[cur ^ 1]);
            ICAF_LAUNCH_CHECK();
            cur ^= 1;
        }
        sort_gather_kernel<<<dim3(g256), dim3(256), 0, S(s)>>>(idx[cur], (const unsigned short*)mask, conf, n, smask, sconf, perm);
        ICAF_LAUNCH_CHECK();
    }
    ap_class_kernel<<<dim3((unsigned)T, (unsigned)nc), dim3(VS_WG), 0, S(s)>>>(smask, sconf, n, n > 0 ? w.ntiles : 0, hist, unique_classes, n_l, T,
                                                                             tpc, ap, p, r);
    ICAF_LAUNCH_CHECK();
    ap_report_kernel<<<dim3(1), dim3(VS_WG), 0, S(s)>>>(p, r, n_l, nc, f1, best, report);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

extern "C" int icaf_confusion_matrix(const float* predn, const float* det, const int* count, int B, int max_det, const float* labels,
                                     const int* label_off, int nc, float conf, float iou_thres, int* matrix, icaf_stream_t s) {
    if (!predn || !det || !count || !label_off || !matrix) return fail(ICAF_ERR_ARG, "icaf_confusion_matrix: null pointer");
    if (B < 1 || B > 65535 || nc < 1 || nc > 32767) return fail(ICAF_ERR_ARG, "icaf_confusion_matrix: B must be in [1, 65535], nc in [1, 32767]");
    if (max_det < 1 || max_det > CM_MAX_DET)
        return fail(ICAF_ERR_UNSUPPORTED, "icaf_confusion_matrix: max_det must be in [1, %d] (%d)", CM_MAX_DET, max_det);
    if (conf != conf || iou_thres != iou_thres) return fail(ICAF_ERR_ARG, "icaf_confusion_matrix: NaN threshold");
    confusion_matrix_kernel<<<dim3((unsigned)B), dim3(256), 0, S(s)>>>(predn, det, count, max_det, labels, label_off, nc, conf, iou_thres, matrix);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
