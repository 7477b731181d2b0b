// Non-maximum suppression for gfx950 — replaces utils/general.py:518-607 + torchvision.ops.nms (greedy, IoU > thr).
//
// The reference filters candidates, sorts ALL of them by score and walks the sorted list greedily; only the first max_det
// (300) survivors are returned.  The walk therefore reaches at most a few hundred to a few thousand of the (up to 25 200 x nc)
// candidates, so nothing here sorts more than it walks:
//   0. hipMemsetAsync          clears the per-image score histograms and candidate counters.
//   1. nms_keys_kernel         every prediction row in parallel (B x rows / 4096 workgroups — the whole chip, not one
//                              workgroup per image): obj > conf, conf = obj * cls > conf, class filter; writes ONE 32-bit word
//                              per candidate slot (order-preserving score bits, 0 = not a candidate), the class of
//                              single-label rows, a 2178-bin histogram of the score's upper 16 bits per image (LDS
//                              atomics, flushed once per workgroup) and the candidate count of every 4096-row chunk.
//   2. nms_walk_kernel         one 1024-thread workgroup per image, rounds of
//                                select   the highest-score histogram bins that are still unvisited and hold <= 1024 (first
//                                         round) / 4096 keys — one LDS prefix scan over the histogram;
//                                gather   those candidates into LDS as unique 64-bit keys (score bits << 32 | ~slot);
//                                sort     bitonic network in LDS, descending (unique keys: the order is total; a rank sort — every
//                                         thread counting the keys above its own — was 5x slower: n^2 64-bit compares);
//                                walk     greedy suppression, 64 candidates per step: all 16 wavefronts test the step against
//                                         the kept boxes (<= max_det, in LDS) AND build the step's own 64 x 64 suppression
//                                         relation (one ballot per candidate); wave 0 then resolves the step with scalar mask
//                                         arithmetic only — no IoU in the serial part — and the kept lanes write at once;
//                              until max_det boxes are kept or the candidates (capped at max_nms, by score) are exhausted.
//                              Rounds visit disjoint, descending score ranges, each sorted by the full key, so the visiting
//                              order equals a stable descending sort of all candidates — ties fall back to the slot index,
//                              which increases with the reference's candidate index.  A histogram bin holding more than 4096
//                              keys (thousands of near-identical scores) is split by an 8-digit radix refinement of the
//                              64-bit key range — slow, exact, and never taken by real score distributions.
//                              Boxes are decoded from the prediction rows on demand; no candidate list is materialised.
//   3. nms_rank_kernel         (only when keep_idx is requested) converts the kept slots into torchvision's indices: the
//                              rank of the slot among the image's candidates = chunk counts before it + candidates before
//                              it inside its chunk.
//   icaf_nms_ex adds the two modes of the reference that icaf_nms cannot express (both described at their kernels below):
//   1b. nms_label_keys_kernel  (apriori labels, :545-552) one workgroup per image behind the keys kernel: the label rows as candidates
//                              behind the prediction rows.  The walk, rank and merge kernels then read such a slot's box from the label
//                              table (decode_slot<true>); the plain path runs the <false> instantiations — the code it always ran.
//   4.  nms_merge_kernel       (merge-NMS, :594-600) one workgroup per image behind the walk and the rank kernel.
// All box arithmetic is fp32 with contraction disabled, in the reference's operation order, so kept indices are
// bit-identical to the CPU algorithm on the same prediction tensor.  The workgroup scan, the xywh decode, box_iou and the mapping to
// the native image (scale_detections_kernel) are box_core.h's; the validation matching that consumes these detections is valstats.hip's.
#pragma clang fp contract(off)
#include <cstring>
#include "box_core.h"

namespace icaf {

struct ClassMask { unsigned int w[8]; };     // classes 0..255

__device__ __forceinline__ bool class_ok(const ClassMask& cm, int use, int c) {
    return !use || (c < 256 && ((cm.w[c >> 5] >> (c & 31)) & 1u));
}

constexpr int NMS_NB = 2178;                 // histogram bins over the upper 16 bits of the ordered score word
constexpr unsigned NMS_BIN_LO = 0xB700u;     // bin 0 = everything below 2^-17 (and negative scores), bin NB-1 = [1.0, inf)
constexpr int NMS_CAP = 4096;                // keys gathered / sorted per round
constexpr int NMS_FIRST = 1024;              // target of the first round (the walk usually ends inside it)
constexpr int NMS_CHUNK_ROWS = 4096;         // prediction rows per nms_keys workgroup (one histogram flush per 4096 rows)
constexpr int MAX_KEEP = 1024;
constexpr int WALK_THREADS = 1024;

// float -> unsigned with the same ordering (negative floats below positive ones); never 0 for a candidate (c > conf, not NaN)
__device__ __forceinline__ unsigned int ordered_bits(float c) {
    const unsigned int b = __float_as_uint(c);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ int bin_of(unsigned int u) {
    const int v = (int)(u >> 16) - (int)NMS_BIN_LO;
    return v < 0 ? 0 : (v > NMS_NB - 1 ? NMS_NB - 1 : v);
}
// smallest 64-bit key of histogram bin t
__device__ __forceinline__ unsigned long long bin_floor_key(int t) {
    return t <= 0 ? 0ull : ((unsigned long long)((unsigned)(t + (int)NMS_BIN_LO) << 16)) << 32;
}

__global__ __launch_bounds__(256) void nms_keys_kernel(const float* __restrict__ pred, long long rows, int nc, float conf, int multi,
                                                       ClassMask cm, int use_cm, long long cap, int nchunks,
                                                       unsigned int* __restrict__ key32, unsigned short* __restrict__ cls16,
                                                       unsigned int* __restrict__ ghist, unsigned int* __restrict__ ncand,
                                                       unsigned int* __restrict__ chunk_cnt) {
    __shared__ unsigned int hist[NMS_NB];
    __shared__ int wsum[4];
    const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
    const int no = 5 + nc;
    for (int i = tid; i < NMS_NB; i += 256) hist[i] = 0;
    __syncthreads();
    const float* pb = pred + (long long)b * rows * no;
    unsigned int* kb = key32 + (long long)b * cap;
    int cnt = 0;
    for (int it0 = 0; it0 < NMS_CHUNK_ROWS / 256; it0 += 4) {
        // four rows per thread at a time: their objectness loads are issued together (the kernel is latency-bound otherwise)
        long long rr[4];
        float objs[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            rr[u] = (long long)chunk * NMS_CHUNK_ROWS + (it0 + u) * 256 + tid;
            objs[u] = rr[u] < rows ? pb[rr[u] * no + 4] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long r = rr[u];
            if (r >= rows) continue;
            const float* p = pb + r * no;
            const float obj = objs[u];
            if (multi) {
                for (int j = 0; j < nc; ++j) {
                    unsigned int k = 0;
                    if (obj > conf) {
                        const float c = p[5 + j] * obj;
                        if (c > conf && class_ok(cm, use_cm, j)) k = ordered_bits(c);
                    }
                    kb[r * nc + j] = k;
                    if (k) { atomicAdd(&hist[bin_of(k)], 1u); ++cnt; }
                }
            } else {
                unsigned int k = 0;
                int best_j = 0;
                if (obj > conf) {
                    float best = -INFINITY;
                    for (int j = 0; j < nc; ++j) {
                        const float c = p[5 + j] * obj;
                        if (c > best) { best = c; best_j = j; }
                    }
                    if (best > conf && class_ok(cm, use_cm, best_j)) k = ordered_bits(best);
                }
                kb[r] = k;
                cls16[(long long)b * rows + r] = (unsigned short)best_j;
                if (k) { atomicAdd(&hist[bin_of(k)], 1u); ++cnt; }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        chunk_cnt[(long long)b * nchunks + chunk] = (unsigned)total;
        if (total) atomicAdd(&ncand[b], (unsigned)total);
    }
    for (int i = tid; i < NMS_NB; i += 256) {
        const unsigned int v = hist[i];
        if (v) atomicAdd(&ghist[(long long)b * NMS_NB + i], v);
    }
}

__device__ __forceinline__ bool iou_gt_exact(float inter, float uni, float thr) {
    // torchvision nms_kernel: ovr = inter / (area_a + area_b - inter); suppress if ovr > thr
    const float ovr = inter / uni;
    return ovr > thr;
}
// IoU(a, b) > thr with the reference's arithmetic (w = max(0, min(x2) - max(x1)), inter = w * h, union = area_a + area_b - inter,
// all fp32, no contraction) and the reference's DECISION, without its division in the common case: the correctly rounded quotient
// q = fl(inter / union) differs from the exact ratio by at most 2^-24 relative, so inter > thr * union * (1 + 2^-20) implies q > thr
// and inter < thr * union * (1 - 2^-20) implies q <= thr (the two products add < 2^-22 of rounding); only inside that band — and for
// degenerate unions (<= 0, NaN) or thr <= 0 — the division itself decides.  ~12 VALU instructions instead of ~25.
__device__ __forceinline__ bool iou_gt(float ax1, float ay1, float ax2, float ay2, float aarea, float bx1, float by1, float bx2,
                                       float by2, float barea, float thr) {
    const float xx1 = fmaxf(ax1, bx1), yy1 = fmaxf(ay1, by1), xx2 = fminf(ax2, bx2), yy2 = fminf(ay2, by2);
    const float w = fmaxf(0.0f, xx2 - xx1), h = fmaxf(0.0f, yy2 - yy1);
    const float inter = w * h;
    const float uni = aarea + barea - inter;
    const float t = thr * uni;
    const bool sure_yes = inter > t * 1.00000095367431640625f;      // 1 + 2^-20
    const bool sure_no = inter < t * 0.99999904632568359375f;       // 1 - 2^-20
    const bool regular = uni > 0.0f && thr > 0.0f;                    // (false for NaN as well)
    if (__builtin_expect(!__all((sure_yes || sure_no) && regular), 0)) {
        const bool exact = iou_gt_exact(inter, uni, thr);
        return (regular && (sure_yes || sure_no)) ? sure_yes : exact;
    }
    return sure_yes;
}

struct WalkSmem {
    unsigned long long keys[NMS_CAP];                                     // gathered / sorted keys of the round
    float kx1[MAX_KEEP], ky1[MAX_KEEP], kx2[MAX_KEEP], ky2[MAX_KEEP], kar[MAX_KEEP];      // kept boxes (class-offset), areas
    float cx1[WALK_THREADS], cy1[WALK_THREADS], cx2[WALK_THREADS], cy2[WALK_THREADS], car[WALK_THREADS];   // decoded candidates
    unsigned int kslot[MAX_KEEP];                                         // candidate slot of every kept box
    unsigned int kpos[MAX_KEEP];                                          // its position in the sorted order
    unsigned int hist[NMS_NB];
    unsigned int dh[256];
    unsigned int wsum[16];
    unsigned long long deadmask;
    unsigned long long supp[64];                                          // supp[j]: lanes of the step that candidate j suppresses
    unsigned long long lo;
    unsigned int batch_n, sel_cnt, sel_val, nkept;
};

// what the walk and the merge kernel read of their image: prediction rows, key words, single-label classes, first label row (LAB only)
struct NmsImage {
    const float* __restrict__ pb;
    const unsigned int* __restrict__ kb;
    const unsigned short* __restrict__ cb;
    const float* __restrict__ lb;
    long long rows, cap;
    int nc, multi;
};

// decode the box of candidate slot `slot`: xywh -> xyxy exactly as the reference (utils/general.py:332-339).  LAB: rows at or beyond `rows` are
// the image's apriori labels (lb = its first label row, [cls, cx, cy, w, h]): obj = 1, one-hot class confidence (:548-551), read where they lie
template <bool LAB>
__device__ __forceinline__ void decode_slot(const NmsImage& im, unsigned int slot, float& x1, float& y1, float& x2, float& y2, float& sc,
                                            int& cl) {
    const unsigned int row = im.multi ? slot / (unsigned)im.nc : slot;
    if (LAB && (long long)row >= im.rows) {
        const float* l = im.lb + ((long long)row - im.rows) * 5;
        const int lc = (int)l[0];
        cl = im.multi ? (int)(slot - row * (unsigned)im.nc) : lc;
        xywh_to_xyxy(l + 1, x1, y1, x2, y2);
        sc = (cl == lc ? 1.0f : 0.0f) * 1.0f;
        return;
    }
    cl = im.multi ? (int)(slot - row * (unsigned)im.nc) : (int)im.cb[row];
    const float* p = im.pb + (long long)row * (5 + im.nc);
    xywh_to_xyxy(p, x1, y1, x2, y2);
    sc = p[5 + cl] * p[4];
}

// ---- the walk kernel: its cursor and its phases ---------------------------------------------------------------------------------------------------
// where the walk stands.  Rounds visit disjoint, descending ranges [lo, hi) of the 64-bit key space; every field is workgroup-uniform
struct WalkCursor {
    int hib = NMS_NB;                              // histogram bins [0, hib) are entirely unvisited
    unsigned long long hi = ~0ull;                 // keys >= hi have been visited
    unsigned long long lo = 0ull;                  // the round in flight gathers the keys of [lo, hi)
    unsigned int in_bin_left = 0;                  // refinement mode: unvisited keys left in bin hib (which is then partially visited)
    unsigned int processed = 0, nkept = 0;
    int round = 0;
};

// select: lo = the floor of the lowest of the highest unvisited bins that together hold <= target keys — NMS_FIRST in the first round, widened
// to NMS_CAP when the next non-empty bin alone exceeds it.  When that bin alone exceeds NMS_CAP as well, refinement mode is entered instead
// (in_bin_left != 0, walk_refine finds lo).  false: nothing is left anywhere.
__device__ __forceinline__ bool walk_select(WalkSmem& sm, WalkCursor& cur) {
    const int tid = threadIdx.x;
    // P(d) = keys in bins (hib-1-d .. hib-1]; largest d with P(d) <= target
    unsigned int target = cur.round == 0 ? NMS_FIRST : NMS_CAP;
    for (;;) {
        unsigned int loc[3], s = 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int d = tid * 3 + e;
            loc[e] = d < cur.hib ? sm.hist[cur.hib - 1 - d] : 0u;
            s += loc[e];
        }
        unsigned int total;
        const unsigned int incl = wg_incl_scan<16>(s, sm.wsum, total);
        if (tid == 0) { sm.sel_cnt = 0; sm.sel_val = 0; }
        __syncthreads();
        unsigned int run = incl - s, nle = 0, last = 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            run += loc[e];
            if (tid * 3 + e < cur.hib && run <= target) { ++nle; last = run; }
        }
        if (nle) { atomicAdd(&sm.sel_cnt, nle); atomicMax(&sm.sel_val, last); }
        __syncthreads();
        const unsigned int dcnt = sm.sel_cnt, val = sm.sel_val;     // dcnt bins from the top hold `val` keys in total
        __syncthreads();
        if (total == 0) { cur.hib = 0; return false; }              // nothing left anywhere
        cur.hib -= (int)dcnt;                                        // (val == 0: these are the empty bins above the next non-empty one)
        if (val > 0) { cur.lo = bin_floor_key(cur.hib); return true; }
        // the next non-empty bin alone exceeds the target
        if (target < NMS_CAP) { target = NMS_CAP; continue; }
        cur.hib -= 1;                                                // > NMS_CAP keys in one bin: refine inside it
        cur.in_bin_left = sm.hist[cur.hib];                          // (bins between it and `hi` are empty: hi stays a valid bound)
        return true;
    }
}

// radix refinement inside bin `hib` over the keys in [bin_floor_key(hib), hi): find lo with 1 <= #[lo, hi) <= NMS_CAP
__device__ __forceinline__ void walk_refine(WalkSmem& sm, const unsigned int* __restrict__ kb, long long cap, WalkCursor& cur) {
    const int tid = threadIdx.x;
    const unsigned long long blo = bin_floor_key(cur.hib), hi = cur.hi;
    if (cur.in_bin_left <= NMS_CAP) { cur.lo = blo; return; }
    unsigned long long lo = 0ull;
    unsigned long long prefix = 0ull;      // the digits chosen so far (upper bits of lo)
    for (int level = 0; level < 8; ++level) {
        const int shift = 56 - 8 * level;
        for (int i = tid; i < 256; i += WALK_THREADS) sm.dh[i] = 0;
        __syncthreads();
        for (long long i = tid; i < cap; i += WALK_THREADS) {
            const unsigned int k32 = kb[i];
            if (!k32) continue;
            const unsigned long long k = ((unsigned long long)k32 << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
            if (k < blo || k >= hi) continue;
            if (level > 0 && (k >> (shift + 8)) != (prefix >> (shift + 8))) continue;
            atomicAdd(&sm.dh[(unsigned)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int dmax = 255;
            while (dmax > 0 && sm.dh[dmax] == 0) --dmax;
            if (sm.dh[dmax] > NMS_CAP) {                         // descend into the top digit (no key of the range lies above it)
                sm.lo = prefix | ((unsigned long long)dmax << shift);
                sm.sel_val = 0;
            } else {
                unsigned int suf = 0;
                int d = dmax;
                while (d >= 0 && suf + sm.dh[d] <= NMS_CAP) { suf += sm.dh[d]; --d; }
                sm.lo = prefix | ((unsigned long long)(d + 1) << shift);
                sm.sel_val = suf;                                // >= 1
            }
        }
        __syncthreads();
        prefix = sm.lo;
        const unsigned int got = sm.sel_val;
        __syncthreads();
        if (got) { lo = prefix; break; }
    }
    cur.lo = lo < blo ? blo : lo;
}

// gather the keys of [lo, hi) into LDS (any order); returns their number (<= NMS_CAP by construction of lo)
__device__ __forceinline__ unsigned int walk_gather(WalkSmem& sm, const unsigned int* __restrict__ kb, long long cap, const WalkCursor& cur) {
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned long long lo = cur.lo, hi = cur.hi;
    if (tid == 0) sm.batch_n = 0;
    __syncthreads();
    for (long long i0 = 0; i0 < cap; i0 += 8 * WALK_THREADS) {
        unsigned int k32[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {                      // eight independent loads in flight per thread (the scan is latency-bound)
            const long long i = i0 + u * WALK_THREADS + tid;
            k32[u] = i < cap ? kb[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long i = i0 + u * WALK_THREADS + tid;
            const unsigned long long k = ((unsigned long long)k32[u] << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
            const bool take = k32[u] != 0u && k >= lo && k < hi;
            const unsigned long long m = __ballot(take);
            if (m) {
                unsigned int base = 0;
                if (lane == 0) base = atomicAdd(&sm.batch_n, (unsigned)__popcll(m));
                base = __shfl(base, 0);
                if (take) {
                    const unsigned int slot = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                    if (slot < NMS_CAP) sm.keys[slot] = k;
                }
            }
        }
    }
    __syncthreads();
    return sm.batch_n < NMS_CAP ? sm.batch_n : NMS_CAP;
}

// bitonic sort of keys[0, bn) in LDS, descending (padding = key 0, the smallest)
// (a rank sort — every thread counting the keys greater than its own through broadcast reads — measured 150 k cycles for 1020
//  keys: 64-bit compares x n^2 are VALU-bound; the network below is 55 barrier stages for 1024 keys, 78 for 4096)
__device__ __forceinline__ void walk_sort(WalkSmem& sm, unsigned int bn) {
    const int tid = threadIdx.x;
    unsigned int P = 64;
    while (P < bn) P <<= 1;
    for (unsigned int i = bn + tid; i < P; i += WALK_THREADS) sm.keys[i] = 0ull;
    __syncthreads();
    for (unsigned int k = 2; k <= P; k <<= 1)
        for (unsigned int j = k >> 1; j > 0; j >>= 1) {
            for (unsigned int t = tid; t < P / 2; t += WALK_THREADS) {
                const unsigned int i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));
                const unsigned int l = i | j;
                const bool up = (i & k) != 0u;                // ascending sub-blocks of the network; the last merge is all-descending
                const unsigned long long a = sm.keys[i], c = sm.keys[l];
                if ((a < c) != up) { sm.keys[i] = c; sm.keys[l] = a; }
            }
            __syncthreads();
        }
}

// greedy walk over the sorted round: the first `limit` keys (max_nms cap, by score rank), 1024 decoded at a time, 64 resolved per step
template <bool LAB>
__device__ __forceinline__ void walk_steps(WalkSmem& sm, const NmsImage& im, WalkCursor& cur, unsigned int limit, float iou_thr, float cls_off,
                                           int max_det) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned int nkept = cur.nkept;
    for (unsigned int base = 0; base < limit && nkept < (unsigned)max_det; base += WALK_THREADS) {
        {
            const unsigned int pos = base + tid;
            if (pos < limit) {
                const unsigned int slot = 0xffffffffu - (unsigned)(sm.keys[pos] & 0xffffffffull);
                float x1, y1, x2, y2, sc;
                int cl;
                decode_slot<LAB>(im, slot, x1, y1, x2, y2, sc, cl);
                const float off = (float)cl * cls_off;                 // boxes + cls * max_wh (reference :589-590)
                x1 = x1 + off; y1 = y1 + off; x2 = x2 + off; y2 = y2 + off;
                sm.cx1[tid] = x1; sm.cy1[tid] = y1; sm.cx2[tid] = x2; sm.cy2[tid] = y2;
                sm.car[tid] = (x2 - x1) * (y2 - y1);
            }
        }
        __syncthreads();
        const unsigned int span = (limit - base) < WALK_THREADS ? (limit - base) : WALK_THREADS;
        for (unsigned int c0 = 0; c0 < span && nkept < (unsigned)max_det; c0 += 64) {
            const unsigned int ci = c0 + lane;
            const bool valid = ci < span;
            float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, area = 0.f;
            if (valid) { x1 = sm.cx1[ci]; y1 = sm.cy1[ci]; x2 = sm.cx2[ci]; y2 = sm.cy2[ci]; area = sm.car[ci]; }
            // phase A: the 16 wavefronts test the step against interleaved sixteenths of the kept list
            bool dead = !valid;
            for (unsigned int k = wave; k < nkept && !__all(dead); k += 16) {
                const bool hit = iou_gt(sm.kx1[k], sm.ky1[k], sm.kx2[k], sm.ky2[k], sm.kar[k], x1, y1, x2, y2, area, iou_thr);    // (all lanes: wave-uniform control flow)
                dead = dead || hit;
            }
            const unsigned long long dm = __ballot(dead);
            if (lane == 0 && dm) atomicOr(&sm.deadmask, dm);
            // ... and the step's own 64 x 64 suppression relation, four candidates j per wavefront: supp[j] = the lanes that
            // overlap candidate j (box broadcast from lane j's registers); the serial pass below then needs no IoU at all
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = wave * 4 + u;
                const float jx1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x1), j));
                const float jy1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y1), j));
                const float jx2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x2), j));
                const float jy2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y2), j));
                const float jar = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, area), j));
                const bool over = iou_gt(jx1, jy1, jx2, jy2, jar, x1, y1, x2, y2, area, iou_thr);
                const unsigned long long m = __ballot(over && valid);
                if (lane == 0) sm.supp[j] = m;
            }
            __syncthreads();
            if (wave == 0) {
                // phase B: resolve the step in order — a kept candidate j removes the LATER lanes of supp[j].  Lane l holds supp[l]
                // in registers; per kept box the serial pass is a find-first-set, two v_readlane and scalar mask arithmetic.
                const unsigned long long mysupp = sm.supp[lane];
                const int slo = (int)(unsigned)(mysupp & 0xffffffffull), shi = (int)(unsigned)(mysupp >> 32);
                unsigned long long alive = ~sm.deadmask, keptmask = 0ull;
                const unsigned int nkept0 = nkept;
                while (alive && nkept < (unsigned)max_det) {
                    const int j = __ffsll((long long)alive) - 1;          // wave-uniform
                    keptmask |= 1ull << j;
                    ++nkept;
                    const unsigned long long sj = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(shi, j) << 32) |
                                                  (unsigned long long)(unsigned)__builtin_amdgcn_readlane(slo, j);
                    alive &= ~((sj & ~((2ull << j) - 1ull)) | (1ull << j));
                }
                if ((keptmask >> lane) & 1ull) {
                    const unsigned int kk = nkept0 + (unsigned)__popcll(keptmask & ((1ull << lane) - 1ull));
                    sm.kx1[kk] = x1; sm.ky1[kk] = y1; sm.kx2[kk] = x2; sm.ky2[kk] = y2; sm.kar[kk] = area;
                    sm.kslot[kk] = 0xffffffffu - (unsigned)(sm.keys[base + ci] & 0xffffffffull);
                    sm.kpos[kk] = cur.processed + base + ci;
                }
                if (lane == 0) { sm.nkept = nkept; sm.deadmask = 0ull; }
            }
            __syncthreads();
            nkept = sm.nkept;
        }
    }
    cur.nkept = nkept;
}

// outputs, all kept boxes in parallel
template <bool LAB>
__device__ __forceinline__ void walk_write(const WalkSmem& sm, const NmsImage& im, int b, unsigned int nkept, bool reordered, int max_det,
                                           float* __restrict__ det, int* __restrict__ count, int* __restrict__ keep_idx) {
    const int tid = threadIdx.x;
    if (tid == 0) count[b] = (int)nkept;
    for (unsigned int k = tid; k < nkept; k += WALK_THREADS) {
        float x1, y1, x2, y2, sc;
        int cl;
        decode_slot<LAB>(im, sm.kslot[k], x1, y1, x2, y2, sc, cl);
        float* o = det + ((long long)b * max_det + k) * 6;
        o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; o[4] = sc; o[5] = (float)cl;
        if (keep_idx) keep_idx[(long long)b * max_det + k] = (int)(reordered ? sm.kpos[k] : sm.kslot[k]);
    }
}

#ifdef ICAF_NMS_DEBUG
#define NMS_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) stamps[i] = (long long)__builtin_amdgcn_s_memtime(); } while (0)
#else
#define NMS_STAMP(i) do { } while (0)
#endif
template <bool LAB>
__global__ __launch_bounds__(WALK_THREADS) void nms_walk_kernel(const float* __restrict__ pred, long long rows, int nc, int multi,
                                                                const float* __restrict__ labels, const int* __restrict__ label_off,
                                                                long long cap, const unsigned int* __restrict__ key32,
                                                                const unsigned short* __restrict__ cls16,
                                                                const unsigned int* __restrict__ ghist,
                                                                const unsigned int* __restrict__ ncand, float iou_thr, float cls_off,
                                                                int max_det, int max_nms, float* __restrict__ det,
                                                                int* __restrict__ count, int* __restrict__ keep_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char walk_smem_raw[];
    WalkSmem& sm = *reinterpret_cast<WalkSmem*>(walk_smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x;
    const NmsImage im = {pred + (long long)b * rows * (5 + nc), key32 + (long long)b * cap, cls16 + (long long)b * rows,
                          LAB ? labels + (long long)label_off[b] * 5 : nullptr, rows, cap, nc, multi};
#ifdef ICAF_NMS_DEBUG
    __shared__ long long stamps[16];
    for (int i = tid; i < 16; i += WALK_THREADS) stamps[i] = 0;
    __syncthreads();
#endif
    NMS_STAMP(0);
    const unsigned int n_all = ncand[b];
    const bool reordered = n_all > (unsigned)max_nms;             // reference re-indexes x by score rank in that case (:586)
    const unsigned int n = reordered ? (unsigned)max_nms : n_all;
    for (int i = tid; i < NMS_NB; i += WALK_THREADS) sm.hist[i] = ghist[(long long)b * NMS_NB + i];
    if (tid == 0) { sm.nkept = 0; sm.deadmask = 0ull; }
    __syncthreads();
    WalkCursor cur;
    while (cur.nkept < (unsigned)max_det && cur.processed < n) {
        cur.lo = 0ull;
        if (cur.in_bin_left == 0 && !walk_select(sm, cur)) break;
        if (cur.in_bin_left != 0) walk_refine(sm, im.kb, cap, cur);
        if (cur.round == 0) NMS_STAMP(1);
        const unsigned int bn = walk_gather(sm, im.kb, cap, cur);
        if (cur.round == 0) NMS_STAMP(2);
        walk_sort(sm, bn);
        if (cur.round == 0) NMS_STAMP(3);
        walk_steps<LAB>(sm, im, cur, (n - cur.processed) < bn ? (n - cur.processed) : bn, iou_thr, cls_off, max_det);
        if (cur.round == 0) NMS_STAMP(4);
        cur.processed += bn;
        cur.hi = cur.lo;
        if (cur.in_bin_left != 0) cur.in_bin_left = cur.in_bin_left > bn ? cur.in_bin_left - bn : 0u;       // bin `hib` done once nothing is left in it
        ++cur.round;
        if (bn == 0) break;                                        // defensive: no progress is impossible by construction
    }
    NMS_STAMP(5);
#ifdef ICAF_NMS_DEBUG
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0)
        printf("nms_walk b0: n_all=%u rounds=%d processed=%u kept=%u | clocks: select %lld gather %lld sort %lld walk(round0) %lld later rounds %lld\n", n_all,
               cur.round, cur.processed, cur.nkept, stamps[1] - stamps[0], stamps[2] - stamps[1], stamps[3] - stamps[2], stamps[4] - stamps[3],
               stamps[5] - stamps[4]);
#endif
    walk_write<LAB>(sm, im, b, cur.nkept, reordered, max_det, det, count, keep_idx);
}

// keep_idx holds candidate SLOTS (row * nc + class) after the walk; torchvision returns indices into the candidate list,
// i.e. the rank of the slot among the image's candidates (slots are visited in candidate order).  One wavefront per kept box.
__global__ __launch_bounds__(256) void nms_rank_kernel(const unsigned int* __restrict__ key32, long long cap, int ncm, int nchunks,
                                                       const unsigned int* __restrict__ chunk_cnt,
                                                       const unsigned int* __restrict__ ncand, const int* __restrict__ count,
                                                       int max_det, int max_nms, int* __restrict__ keep_idx) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= count[b] || ncand[b] > (unsigned)max_nms) return;           // re-ordered images already hold sorted positions
    const unsigned int slot = (unsigned)keep_idx[(long long)b * max_det + k];
    const unsigned int per_chunk = (unsigned)NMS_CHUNK_ROWS * (unsigned)ncm;
    const unsigned int chunk = slot / per_chunk;
    unsigned int r = 0;
    for (unsigned int c = lane; c < chunk; c += 64) r += chunk_cnt[(long long)b * nchunks + c];
    const unsigned int* kb = key32 + (long long)b * cap;
    for (unsigned int i = chunk * per_chunk + lane; i < slot; i += 64) r += kb[i] != 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o);
    if (lane == 0) keep_idx[(long long)b * max_det + k] = (int)r;
}

// Apriori labels (utils/general.py:545-552) as a second candidate source: label row r of image b is candidate row rows + r, behind the
// prediction rows, with obj = 1 and a one-hot class confidence, so conf = 1 for its class and 0 for the others.  Runs after nms_keys_kernel
// on the same stream and fills the key words of ALL max_labels label rows (0 behind the image's labels), adding its candidates to the
// histogram, the candidate counter and the chunk counts that kernel wrote.  Integer atomics only: the sums do not depend on their order.
__global__ __launch_bounds__(256) void nms_label_keys_kernel(const float* __restrict__ labels, const int* __restrict__ label_off,
                                                             int max_labels, long long rows, int nc, float conf, int multi, ClassMask cm,
                                                             int use_cm, long long cap, int nchunks, unsigned int* __restrict__ key32,
                                                             unsigned int* __restrict__ ghist, unsigned int* __restrict__ ncand,
                                                             unsigned int* __restrict__ chunk_cnt) {
    const int b = blockIdx.x;
    const int l0 = label_off[b];
    int nl = label_off[b + 1] - l0;
    nl = nl < 0 ? 0 : (nl > max_labels ? max_labels : nl);
    unsigned int* kb = key32 + (long long)b * cap;
    for (int r = threadIdx.x; r < max_labels; r += 256) {
        const long long row = rows + r;
        int lc = -1;
        if (r < nl) {
            const float c = labels[(long long)(l0 + r) * 5];
            if (c >= 0.0f && c < (float)nc) lc = (int)c;                 // (the host wrapper refuses other classes; never index with one)
        }
        const unsigned int chunk = (unsigned)(row / NMS_CHUNK_ROWS);
        for (int j = 0; j < (multi ? nc : 1); ++j) {
            unsigned int k = 0;
            if (lc >= 0) {
                const int cj = multi ? j : lc;                           // best class of a one-hot row: the label's
                const float c = (cj == lc ? 1.0f : 0.0f) * 1.0f;
                if (c > conf && class_ok(cm, use_cm, cj)) k = ordered_bits(c);
            }
            kb[multi ? row * nc + j : row] = k;
            if (k) {
                atomicAdd(&ghist[(long long)b * NMS_NB + bin_of(k)], 1u);
                atomicAdd(&ncand[b], 1u);
                atomicAdd(&chunk_cnt[(long long)b * nchunks + chunk], 1u);
            }
        }
    }
}

// Merge-NMS (utils/general.py:594-600), one workgroup per image, after the walk (and the rank kernel).  An image whose candidate count n
// (after the class filter, before max_nms) is not inside 1 < n < 3000 returns at once: its plain result stands.  Otherwise
//   1. the image's candidates are compacted into LDS in slot (= candidate) order: un-offset xyxy, score, class offset;
//   2. one wavefront per kept box i: hit(i, j) = box_iou(boxes[i], boxes[j]) > iou_thres on the class-offset boxes, fp32, contraction off,
//      the operation order of :455-477 (areas, clamp(0), inter / (a1 + a2 - inter), an IEEE division).  THE SUMMATION ORDER: lane l adds
//      the products score_j * xyxy_j (exact in fp64) and the scores of its hits j = l, l + 64, l + 128, ... in ascending j into fp64
//      accumulators that start at 0; the 64 lanes are then combined by the butterfly v += shfl_xor(v, o), o = 32, 16, 8, 4, 2, 1 (fp64 adds
//      commute, so every lane holds the same bits).  Each of the five sums is rounded to fp32 once, the quotient is an fp32 division;
//   3. with `redundant` the kept boxes with fewer than two hits are dropped: one prefix scan, det / keep_idx / count compacted in order.
//      Only rows below the new count are written; the rows at or behind it keep what the walk left there.
// A zero-area box has IoU NaN with everything, itself included: no hit, 0 / 0 coordinates — as the reference.
constexpr int MERGE_N = ICAF_NMS_MERGE_LIMIT;
struct MergeSmem {
    float x1[MERGE_N], y1[MERGE_N], x2[MERGE_N], y2[MERGE_N], sc[MERGE_N], off[MERGE_N];
    float res[MAX_KEEP][4];
    unsigned int hits[MAX_KEEP];
    unsigned int cnt[4][16];
    unsigned int wsum[16];
};

template <bool LAB>
__global__ __launch_bounds__(WALK_THREADS) void nms_merge_kernel(const float* __restrict__ pred, long long rows, int nc, int multi,
                                                                 const float* __restrict__ labels, const int* __restrict__ label_off,
                                                                 long long cap, const unsigned int* __restrict__ key32,
                                                                 const unsigned short* __restrict__ cls16,
                                                                 const unsigned int* __restrict__ ncand, float iou_thr, float cls_off,
                                                                 int max_det, int redundant, float* __restrict__ det, int* __restrict__ count,
                                                                 int* __restrict__ keep_idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char merge_smem_raw[];
    MergeSmem& sm = *reinterpret_cast<MergeSmem*>(merge_smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned int n = ncand[b];
    if (!(n > 1u && n < (unsigned)MERGE_N)) return;                       // workgroup-uniform
    const int nk = min(count[b], max_det);
    const NmsImage im = {pred + (long long)b * rows * (5 + nc), key32 + (long long)b * cap, cls16 + (long long)b * rows,
                         LAB ? labels + (long long)label_off[b] * 5 : nullptr, rows, cap, nc, multi};
    // ------------------------------------------------------------------ 1. candidates into LDS, slot order
    unsigned int base = 0;
    for (long long i0 = 0; i0 < cap; i0 += 4 * WALK_THREADS) {
        unsigned int k32[4];
        unsigned long long m[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = i0 + u * WALK_THREADS + tid;
            k32[u] = i < cap ? im.kb[i] : 0u;
        }
        // the ordered rank of four predicates a thread behind ONE barrier pair, written out (box_core.h's wg_rank ranks one predicate).  A build
        // that had this loop on a four-slot wg_rank measured the kernel 2 - 6 % over its limit at nc = 3; what inside the kernel cost that was not
        // separated, and with this text the kernel is within its limits (profiles/postproc_share_ab.json)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            m[u] = __ballot(k32[u] != 0u);
            if (lane == 0) sm.cnt[u][wave] = (unsigned)__popcll(m[u]);
        }
        __syncthreads();
        unsigned int before[4] = {0, 0, 0, 0}, total = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                const unsigned int c = sm.cnt[u][w];
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (u < v || (u == v && w < wave)) before[v] += c;
                total += c;
            }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (k32[u] == 0u) continue;
            const unsigned int pos = base + before[u] + (unsigned)__popcll(m[u] & ((1ull << lane) - 1ull));
            if (pos >= (unsigned)MERGE_N) continue;                        // (cannot happen: n < MERGE_N keys exist)
            float x1, y1, x2, y2, sc;
            int cl;
            decode_slot<LAB>(im, (unsigned)(i0 + u * WALK_THREADS + tid), x1, y1, x2, y2, sc, cl);
            sm.x1[pos] = x1; sm.y1[pos] = y1; sm.x2[pos] = x2; sm.y2[pos] = y2; sm.sc[pos] = sc; sm.off[pos] = (float)cl * cls_off;
        }
        __syncthreads();
        base += total;
    }
    const unsigned int nc_lds = base < (unsigned)MERGE_N ? base : (unsigned)MERGE_N;       // == n
    // ------------------------------------------------------------------ 2. one wavefront per kept box
    for (int k = wave; k < nk; k += 16) {
        const float* d = det + ((long long)b * max_det + k) * 6;
        const float ko = d[5] * cls_off;                                   // boxes + cls * max_wh (:589-590), as the walk offset them
        const float kx1 = d[0] + ko, ky1 = d[1] + ko, kx2 = d[2] + ko, ky2 = d[3] + ko;
        const float karea = (kx2 - kx1) * (ky2 - ky1);
        double sw = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        unsigned int hits = 0;
        for (unsigned int j = lane; j < nc_lds; j += 64) {
            const float ux1 = sm.x1[j], uy1 = sm.y1[j], ux2 = sm.x2[j], uy2 = sm.y2[j], o = sm.off[j];
            const float cx1 = ux1 + o, cy1 = uy1 + o, cx2 = ux2 + o, cy2 = uy2 + o;
            const float carea = (cx2 - cx1) * (cy2 - cy1);
            if (box_iou(kx1, ky1, kx2, ky2, karea, cx1, cy1, cx2, cy2, carea) > iou_thr) {
                const double s = (double)sm.sc[j];
                sw += s;
                a0 += s * (double)ux1; a1 += s * (double)uy1; a2 += s * (double)ux2; a3 += s * (double)uy2;
                ++hits;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sw += __shfl_xor(sw, o); a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o); a2 += __shfl_xor(a2, o); a3 += __shfl_xor(a3, o);
            hits += __shfl_xor(hits, o);
        }
        if (lane == 0) {
            const float fw = (float)sw;
            sm.res[k][0] = (float)a0 / fw; sm.res[k][1] = (float)a1 / fw; sm.res[k][2] = (float)a2 / fw; sm.res[k][3] = (float)a3 / fw;
            sm.hits[k] = hits;
        }
    }
    __syncthreads();
    // ------------------------------------------------------------------ 3. write back, compacted when `redundant`
    float sc = 0.0f, cl = 0.0f;
    int ki = 0;
    unsigned int flag = 0;
    if (tid < nk) {
        const float* d = det + ((long long)b * max_det + tid) * 6;
        sc = d[4]; cl = d[5];
        if (keep_idx) ki = keep_idx[(long long)b * max_det + tid];
        flag = (!redundant || sm.hits[tid] > 1u) ? 1u : 0u;
    }
    unsigned int total;
    const unsigned int incl = wg_incl_scan<16>(flag, sm.wsum, total);      // (its barriers order the reads above before the writes below)
    if (flag) {
        const unsigned int pos = incl - 1u;
        float* o = det + ((long long)b * max_det + pos) * 6;
        o[0] = sm.res[tid][0]; o[1] = sm.res[tid][1]; o[2] = sm.res[tid][2]; o[3] = sm.res[tid][3]; o[4] = sc; o[5] = cl;
        if (keep_idx) keep_idx[(long long)b * max_det + pos] = ki;
    }
    if (tid == 0) count[b] = (int)total;
}

struct NmsWs {
    unsigned int* key32; unsigned short* cls16; unsigned int* ghist; unsigned int* ncand; unsigned int* chunk_cnt;
    size_t zero_bytes; int nchunks; size_t total;
};

// max_labels: label rows per image behind the prediction rows (0: the layout of icaf_nms)
static int nms_layout(int B, long long rows, int nc, int multi, int max_labels, void* base, NmsWs& ws) {
    if (B < 1 || rows < 1 || nc < 1) return fail(ICAF_ERR_ARG, "icaf_nms: bad B/rows/nc");
    if (nc > 65535) return fail(ICAF_ERR_UNSUPPORTED, "icaf_nms: at most 65535 classes");
    if (max_labels < 0 || max_labels > ICAF_NMS_MAX_LABELS) return fail(ICAF_ERR_ARG, "icaf_nms: max_labels must be in [0, %d]", (int)ICAF_NMS_MAX_LABELS);
    const long long cap = (rows + max_labels) * ((multi && nc > 1) ? nc : 1);
    if (cap > 0xfffffff0LL || (long long)B > 65535) return fail(ICAF_ERR_UNSUPPORTED, "icaf_nms: rows*nc exceeds 2^32 candidate slots per image");
    WsArena ar(base);
    ws.nchunks = (int)((rows + max_labels + NMS_CHUNK_ROWS - 1) / NMS_CHUNK_ROWS);
    ws.zero_bytes = (size_t)B * NMS_NB * 4 + (size_t)B * 4;
    ws.ghist = ar.take_as<unsigned int>(ws.zero_bytes);                            // histograms + candidate counters: cleared per call
    ws.ncand = ws.ghist ? ws.ghist + (size_t)B * NMS_NB : nullptr;
    ws.key32 = ar.take_as<unsigned int>((size_t)B * cap * 4);
    ws.cls16 = ar.take_as<unsigned short>((size_t)B * rows * 2);
    ws.chunk_cnt = ar.take_as<unsigned int>((size_t)B * ws.nchunks * 4);
    ws.total = ar.total;
    return ICAF_OK;
}


// det [B][max_det][6] -> out (may alias det: a thread reads its row before it writes it): rows < count[b] mapped to the native image,
// optionally rounded half-to-even (torch.round, detect_twostream.py:80), conf / cls copied; rows >= count[b] zeroed
__global__ __launch_bounds__(256) void scale_detections_kernel(const float* det, const int* __restrict__ count, int max_det,
                                                               const float* __restrict__ scale, int round, float* out) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= max_det) return;
    const long long row = ((long long)b * max_det + i) * 6;
    float x1 = 0.0f, y1 = 0.0f, x2 = 0.0f, y2 = 0.0f, conf = 0.0f, cls = 0.0f;
    if (i < count[b]) {
        x1 = det[row]; y1 = det[row + 1]; x2 = det[row + 2]; y2 = det[row + 3]; conf = det[row + 4]; cls = det[row + 5];
        native_box(scale + b * 5, x1, y1, x2, y2);
        if (round) { x1 = rintf(x1); y1 = rintf(y1); x2 = rintf(x2); y2 = rintf(y2); }
    }
    out[row] = x1; out[row + 1] = y1; out[row + 2] = x2; out[row + 3] = y2; out[row + 4] = conf; out[row + 5] = cls;
}

}  // namespace icaf

using namespace icaf;

// labels without a table or without room count as none: the layout, the launches and the results are icaf_nms'
static inline int nms_label_rows(const icaf_nms_args* a) { return (a->labels && a->max_labels > 0) ? a->max_labels : 0; }

extern "C" int icaf_nms_ex_workspace_bytes(const icaf_nms_args* a, size_t* bytes) {
    if (!a || !bytes) return fail(ICAF_ERR_ARG, "icaf_nms_workspace_bytes: null pointer");
    NmsWs ws;
    int st = nms_layout(a->B, a->rows, a->nc, a->multi_label, a->max_labels, nullptr, ws);      // (sized for max_labels whether or not a table is set yet)
    if (st) return st;
    *bytes = ws.total;
    return ICAF_OK;
}

extern "C" int icaf_nms_workspace_bytes(int B, long long rows, int nc, int multi_label, size_t* bytes) {
    icaf_nms_args a;
    memset(&a, 0, sizeof(a));
    a.B = B; a.rows = rows; a.nc = nc; a.multi_label = multi_label;
    return icaf_nms_ex_workspace_bytes(&a, bytes);
}

template <bool LAB>
static int nms_launch(const icaf_nms_args* a, const NmsWs& ws, const ClassMask& cm, int multi, int ml, hipStream_t hs) {
    const long long rows = a->rows, cap = (rows + ml) * (multi ? a->nc : 1);
    const int B = a->B, nc = a->nc, use_cm = a->n_classes > 0 ? 1 : 0;
    const float cls_off = a->agnostic ? 0.0f : a->max_wh;
    ICAF_LDS_OPTIN(nms_walk_kernel<LAB>, sizeof(WalkSmem));
    ICAF_LDS_OPTIN(nms_merge_kernel<LAB>, sizeof(MergeSmem));
    ICAF_HIP(hipMemsetAsync(ws.ghist, 0, ws.zero_bytes, hs));
    nms_keys_kernel<<<dim3((unsigned)ws.nchunks, (unsigned)B), dim3(256), 0, hs>>>(a->pred, rows, nc, a->conf_thres, multi, cm, use_cm, cap,
                                                                                   ws.nchunks, ws.key32, ws.cls16, ws.ghist, ws.ncand,
                                                                                   ws.chunk_cnt);
    ICAF_LAUNCH_CHECK();
    if (LAB) {
        nms_label_keys_kernel<<<dim3((unsigned)B), dim3(256), 0, hs>>>(a->labels, a->label_off, ml, rows, nc, a->conf_thres, multi, cm, use_cm, cap,
                                                                       ws.nchunks, ws.key32, ws.ghist, ws.ncand, ws.chunk_cnt);
        ICAF_LAUNCH_CHECK();
    }
    nms_walk_kernel<LAB><<<dim3((unsigned)B), dim3(WALK_THREADS), sizeof(WalkSmem), hs>>>(a->pred, rows, nc, multi, a->labels, a->label_off, cap,
                                                                                          ws.key32, ws.cls16, ws.ghist, ws.ncand, a->iou_thres,
                                                                                          cls_off, a->max_det, a->max_nms, a->det, a->count,
                                                                                          a->keep_idx);
    ICAF_LAUNCH_CHECK();
    if (a->keep_idx) {
        nms_rank_kernel<<<dim3((unsigned)((a->max_det + 3) / 4), (unsigned)B), dim3(256), 0, hs>>>(ws.key32, cap, multi ? nc : 1, ws.nchunks,
                                                                                                 ws.chunk_cnt, ws.ncand, a->count, a->max_det,
                                                                                                 a->max_nms, a->keep_idx);
        ICAF_LAUNCH_CHECK();
    }
    if (a->merge) {
        nms_merge_kernel<LAB><<<dim3((unsigned)B), dim3(WALK_THREADS), sizeof(MergeSmem), hs>>>(a->pred, rows, nc, multi, a->labels, a->label_off,
                                                                                                cap, ws.key32, ws.cls16, ws.ncand, a->iou_thres,
                                                                                                cls_off, a->max_det, a->redundant ? 1 : 0, a->det,
                                                                                                a->count, a->keep_idx);
        ICAF_LAUNCH_CHECK();
    }
    return ICAF_OK;
}

extern "C" int icaf_nms_ex(const icaf_nms_args* a, icaf_stream_t s) {
    if (!a) return fail(ICAF_ERR_ARG, "icaf_nms: null pointer");
    if (!a->pred || !a->det || !a->count || !a->workspace) return fail(ICAF_ERR_ARG, "icaf_nms: null pointer");
    if (a->max_det < 1 || a->max_det > MAX_KEEP) return fail(ICAF_ERR_ARG, "icaf_nms: max_det must be in [1, %d]", MAX_KEEP);
    if (a->max_nms < 1) return fail(ICAF_ERR_ARG, "icaf_nms: max_nms must be positive");
    if (a->n_classes < 0 || (a->n_classes > 0 && !a->classes)) return fail(ICAF_ERR_ARG, "icaf_nms: class filter of %d ids without a list", a->n_classes);
    if (((uintptr_t)a->workspace & 255) != 0) return fail(ICAF_ERR_ARG, "icaf_nms: workspace must be 256-byte aligned");
    if (a->merge && a->max_nms < MERGE_N)
        return fail(ICAF_ERR_ARG, "icaf_nms: merge needs max_nms >= %d (the reference would merge over a truncated candidate list)", MERGE_N);
    if (a->labels && a->max_labels > 0 && !a->label_off) return fail(ICAF_ERR_ARG, "icaf_nms: labels without label_off");
    const int multi = a->multi_label && a->nc > 1;
    const int ml = nms_label_rows(a);
    NmsWs ws;
    int st = nms_layout(a->B, a->rows, a->nc, multi, ml, a->workspace, ws);
    if (st) return st;
    if (ws.total > a->workspace_bytes) return fail(ICAF_ERR_ARG, "icaf_nms: workspace too small (%zu < %zu)", a->workspace_bytes, ws.total);
    ClassMask cm;
    memset(&cm, 0, sizeof(cm));
    for (int i = 0; i < a->n_classes; ++i) {
        const int c = a->classes[i];
        if (c < 0 || c > 255) return fail(ICAF_ERR_UNSUPPORTED, "icaf_nms: class filter supports ids 0..255");
        cm.w[c >> 5] |= 1u << (c & 31);
    }
    return ml ? nms_launch<true>(a, ws, cm, multi, ml, S(s)) : nms_launch<false>(a, ws, cm, multi, 0, S(s));
}

extern "C" int icaf_nms(const float* pred, int B, long long rows, int nc, float conf_thres, float iou_thres, int multi_label, int agnostic,
                        const int* classes_host, int n_classes, int max_det, int max_nms, float max_wh, float* det, int* count,
                        int* keep_idx, void* workspace, size_t workspace_bytes, icaf_stream_t s) {
    icaf_nms_args a;
    memset(&a, 0, sizeof(a));
    a.pred = pred; a.B = B; a.rows = rows; a.nc = nc; a.conf_thres = conf_thres; a.iou_thres = iou_thres;
    a.multi_label = multi_label; a.agnostic = agnostic; a.classes = classes_host; a.n_classes = n_classes;
    a.max_det = max_det; a.max_nms = max_nms; a.max_wh = max_wh; a.det = det; a.count = count; a.keep_idx = keep_idx;
    a.workspace = workspace; a.workspace_bytes = workspace_bytes;
    return icaf_nms_ex(&a, s);
}

extern "C" int icaf_scale_detections(const float* det, const int* count, int B, int max_det, const float* scale, int round, float* out,
                                     icaf_stream_t s) {
    if (!det || !count || !scale || !out) return fail(ICAF_ERR_ARG, "icaf_scale_detections: null pointer");
    if (B < 1 || B > 65535 || max_det < 1) return fail(ICAF_ERR_ARG, "icaf_scale_detections: B must be in [1, 65535], max_det positive");
    scale_detections_kernel<<<dim3((unsigned)((max_det + 255) / 256), (unsigned)B), dim3(256), 0, S(s)>>>(det, count, max_det, scale, round, out);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
