// KAIST log-average miss rate, per-image half (evaluation_script/evaluation_script.py:46-79, 119-179, 181-294 of the reference) for gfx950.
//
// The reference evaluator runs nine passes (All / Day / Night on set-up 0, six scale and occlusion subsets on set-ups 1-6) of pure-Python IoU and
// greedy-matching loops over every image.  The per-image result of a pass depends on the set-up only, so ONE launch produces all seven:
//   icaf_missrate_stage   one thread per detection of a validation batch: the native-space box [x1, y1, x2 - x1, y2 - y1] (the subtraction in fp32,
//                         as the result-file writer does it) and the score, widened to fp64, into the detection store dt[I][cap][5] at the
//                         image's position in the annotation file.  No host sync; it can sit on the validation stream between batches.
//   icaf_missrate_match   one 512-thread workgroup per image:
//                           flags    one thread per label: the 7-bit mask "ignored in set-up s" (height / occlusion / border rules);
//                           sort     rank sort of the scores by all eight waves (descending, equal scores in arrival order: the rank of a
//                                    detection is the number of detections that a stable sort puts before it — no key is moved), the first
//                                    1000 boxes land in LDS in sorted order;
//                           order    wave s builds the label order of set-up s (non-ignored first, then ignored, each in annotation order)
//                                    with two ballot prefix passes;
//                           match    wave s walks the sorted detections serially; its lanes hold the labels (up to 4 per lane, in registers)
//                                    and recompute the fp64 IoU of (detection, label) — no D x G matrix exists.  The reference's sequential
//                                    walk over the labels reduces to: the non-ignored, untaken label of maximal IoU >= 0.5, the LATER one on
//                                    a tie (one 6-step butterfly, skipped when no lane has a candidate); failing that the FIRST ignored
//                                    label with IoU >= 0.5 (a ballot).  Only a non-ignored match takes its label (one bit per lane and chunk).
// fp64 throughout, contraction off, the reference's operation order: the matches equal the CPU evaluator's exactly.
// The FPPI sweep over the whole data set (a global sort + two cumulative sums) stays on the host: icafusion_amd/utils/missrate.py.
#pragma clang fp contract(off)
#include "icaf_common.h"

namespace icaf {

constexpr int MR_THREADS = 512;
constexpr int MR_MAX_DET = ICAF_MISSRATE_MAX_DET;          // rows of the detection store per image (LDS: 32 KiB of sorted boxes)
constexpr int MR_KEEP = ICAF_MISSRATE_KEEP;                // KAISTParams.maxDets
constexpr int MR_MAX_LABELS = ICAF_MISSRATE_MAX_LABELS;    // 4 labels per lane of the set-up's wave
constexpr int MR_SETUPS = ICAF_MISSRATE_SETUPS;
constexpr int MR_CHUNKS = MR_MAX_LABELS / 64;

// bit s = the label is ignored in set-up s (KAISTParams.HtRng / OccRng / bndRng, :478-497; rule of _prepare, :59-71)
__device__ __forceinline__ unsigned int mr_label_mask(double x, double y, double w, double h, double height, int occ, int base) {
    constexpr double lo[MR_SETUPS] = {55.0, 115.0, 45.0, 1.0, 1.0, 1.0, 1.0};
    constexpr double hi[MR_SETUPS] = {1e10, 1e10, 115.0, 45.0, 1e10, 1e10, 1e10};
    constexpr unsigned int occ_in[MR_SETUPS] = {3u, 1u, 1u, 1u, 1u, 2u, 4u};          // bit o = occlusion o belongs to the set-up
    const bool outside = x < 5.0 || y < 5.0 || x + w > 635.0 || y + h > 507.0;
    const unsigned int obit = (occ >= 0 && occ <= 2) ? (1u << occ) : 0u;
    unsigned int m = 0;
#pragma unroll
    for (int s = 0; s < MR_SETUPS; ++s) {
        const bool ig = base != 0 || outside || height < lo[s] || height > hi[s] || !(occ_in[s] & obit);
        m |= (ig ? 1u : 0u) << s;
    }
    return m;
}

__global__ __launch_bounds__(MR_THREADS) void missrate_match_kernel(const double* __restrict__ gt_box, const double* __restrict__ gt_height,
                                                                    const int* __restrict__ gt_occ, const int* __restrict__ gt_base,
                                                                    const int* __restrict__ gt_off, const double* __restrict__ dt,
                                                                    const int* __restrict__ dt_count, int cap, int* __restrict__ order,
                                                                    int* __restrict__ dt_gt, unsigned char* __restrict__ dt_ignore,
                                                                    unsigned char* __restrict__ gt_ignore) {
    __shared__ double s_box[MR_KEEP][4];                    // x, y, w, h of the kept detections, sorted order
    __shared__ double s_score[MR_MAX_DET];                  // arrival order
    __shared__ unsigned char s_dig[MR_KEEP][8];             // s_dig[k][s]: detection k matched an ignored label in set-up s
    __shared__ unsigned char s_lab[MR_SETUPS][MR_MAX_LABELS];   // label order of each set-up (indices local to the image)
    __shared__ unsigned char s_gmask[MR_MAX_LABELS];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = gt_off[img];
    const int nl = min(max(gt_off[img + 1] - g0, 0), MR_MAX_LABELS);       // the launcher refuses more; never index past the tables
    const int n = min(max(dt_count[img], 0), min(cap, MR_MAX_DET));
    const int m = min(n, MR_KEEP);
    const long long row0 = (long long)img * cap;
    const double* db = dt + row0 * 5;

    for (int i = tid; i < n; i += MR_THREADS) s_score[i] = db[(long long)i * 5 + 4];
    for (int j = tid; j < nl; j += MR_THREADS) {
        const double* g = gt_box + (long long)(g0 + j) * 4;
        const unsigned int mk = mr_label_mask(g[0], g[1], g[2], g[3], gt_height[g0 + j], gt_occ[g0 + j], gt_base[g0 + j]);
        s_gmask[j] = (unsigned char)mk;
        gt_ignore[g0 + j] = (unsigned char)mk;
    }
    __syncthreads();

    // rank sort: np.argsort(-score, kind='mergesort') — descending, equal scores in arrival order
    for (int a = tid; a < n; a += MR_THREADS) {
        const double sa = s_score[a];
        int r = 0;
        for (int b = 0; b < n; ++b) {
            const double sb = s_score[b];
            r += (sb > sa || (sb == sa && b < a)) ? 1 : 0;
        }
        order[row0 + r] = a;
        if (r < MR_KEEP) {
            const double* d = db + (long long)a * 5;
            s_box[r][0] = d[0]; s_box[r][1] = d[1]; s_box[r][2] = d[2]; s_box[r][3] = d[3];
        }
    }
    // label order of set-up `wave`: a stable sort on the ignore flag (:205)
    const int s = wave;
    int nn = 0;                                             // non-ignored labels of the set-up
    if (s < MR_SETUPS) {
        for (int pass = 0; pass < 2; ++pass) {
            int pos = pass ? nn : 0;
            for (int c = 0; c * 64 < nl; ++c) {
                const int j = c * 64 + lane;
                const bool mine = j < nl && (int)((s_gmask[j] >> s) & 1u) == pass;
                const unsigned long long bal = __ballot(mine);
                if (mine) s_lab[s][pos + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned char)j;
                pos += __popcll(bal);
            }
            if (!pass) nn = pos;
        }
    }
    __syncthreads();

    if (s < MR_SETUPS) {
        double gx1[MR_CHUNKS], gy1[MR_CHUNKS], gx2[MR_CHUNKS], gy2[MR_CHUNKS], garea[MR_CHUNKS];
#pragma unroll
        for (int c = 0; c < MR_CHUNKS; ++c) {
            const int p = c * 64 + lane;
            gx1[c] = gy1[c] = gx2[c] = gy2[c] = garea[c] = 0.0;
            if (p < nl) {
                const double* g = gt_box + (long long)(g0 + s_lab[s][p]) * 4;
                gx1[c] = g[0]; gy1[c] = g[1]; gx2[c] = g[0] + g[2]; gy2[c] = g[1] + g[3]; garea[c] = g[2] * g[3];
            }
        }
        unsigned int taken = 0;                             // bit c: this lane's label of chunk c is matched (non-ignored labels only)
        for (int k = 0; k < m; ++k) {
            const double dx1 = s_box[k][0], dy1 = s_box[k][1], dw = s_box[k][2], dh = s_box[k][3];
            const double dx2 = dx1 + dw, dy2 = dy1 + dh, darea = dw * dh;
            double best = -1.0;                             // this lane's best non-ignored candidate
            int bp = -1, first_ign = -1;
#pragma unroll
            for (int c = 0; c < MR_CHUNKS; ++c) {
                if (c * 64 < nl) {                          // wave-uniform
                    const int p = c * 64 + lane;
                    const bool ign = p >= nn;
                    double iou = 0.0;
                    const double iw = fmin(dx2, gx2[c]) - fmax(dx1, gx1[c]);
                    const double ih = fmin(dy2, gy2[c]) - fmax(dy1, gy1[c]);
                    if (iw > 0.0 && ih > 0.0) {
                        const double t = iw * ih;
                        const double uni = ign ? darea : (darea + garea[c]) - t;
                        iou = t / uni;
                    }
                    const bool hit = p < nl && !(iou < 0.5);
                    if (hit && !ign && !((taken >> c) & 1u) && !(iou < best)) { best = iou; bp = p; }      // later chunk wins a tie
                    const unsigned long long bal = __ballot(hit && ign);
                    if (first_ign < 0 && bal) first_ign = c * 64 + (__ffsll((long long)bal) - 1);
                }
            }
            int gt = -1, ig = 0;
            if (__ballot(bp >= 0)) {                        // maximal IoU among the untaken non-ignored labels, the later label on a tie
#pragma unroll
                for (int off = 32; off >= 1; off >>= 1) {
                    const double ob = __shfl_xor(best, off);
                    const int op = __shfl_xor(bp, off);
                    if (ob > best || (ob == best && op > bp)) { best = ob; bp = op; }
                }
                if ((bp & 63) == lane) taken |= 1u << (bp >> 6);
                gt = g0 + s_lab[s][bp];
            } else if (first_ign >= 0) {                    // no regular match: the FIRST ignored label at IoU >= 0.5, never consumed
                gt = g0 + s_lab[s][first_ign];
                ig = 1;
            }
            if (lane == 0) {
                dt_gt[(row0 + k) * MR_SETUPS + s] = gt;
                s_dig[k][s] = (unsigned char)ig;
            }
        }
    }
    __syncthreads();
    for (int k = tid; k < m; k += MR_THREADS) {
        unsigned int mk = 0;
#pragma unroll
        for (int q = 0; q < MR_SETUPS; ++q) mk |= (unsigned int)s_dig[k][q] << q;
        dt_ignore[row0 + k] = (unsigned char)mk;
    }
}

__global__ __launch_bounds__(256) void missrate_stage_kernel(const float* __restrict__ predn, const float* __restrict__ det,
                                                             const int* __restrict__ count, const int* __restrict__ image_index, int max_det,
                                                             int I, int cap, double* __restrict__ dt, int* __restrict__ dt_count) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int img = image_index[b];
    if (img < 0 || img >= I) return;                        // the host validates; never write outside the store
    const int n = min(min(max(count[b], 0), max_det), cap);
    if (i == 0) dt_count[img] = n;
    if (i >= n) return;
    const float* p = predn + ((long long)b * max_det + i) * 4;
    const float x1 = p[0], y1 = p[1], w = p[2] - x1, h = p[3] - y1;       // fp32, as xyxy -> xywh of the result files
    double* o = dt + ((long long)img * cap + i) * 5;
    o[0] = (double)x1; o[1] = (double)y1; o[2] = (double)w; o[3] = (double)h;
    o[4] = (double)det[((long long)b * max_det + i) * 6 + 4];
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_missrate_stage(const float* predn, const float* det, const int* count, const int* image_index, int B, int max_det, double* dt,
                                   int* dt_count, int I, int cap, icaf_stream_t s) {
    if (!predn || !det || !count || !image_index || !dt || !dt_count) return fail(ICAF_ERR_ARG, "icaf_missrate_stage: null pointer");
    if (B < 1 || B > 65535 || max_det < 1 || I < 1) return fail(ICAF_ERR_ARG, "icaf_missrate_stage: B must be in [1, 65535], max_det and I positive");
    if (cap < 1 || cap > MR_MAX_DET) return fail(ICAF_ERR_UNSUPPORTED, "icaf_missrate_stage: cap must be in [1, %d]", MR_MAX_DET);
    missrate_stage_kernel<<<dim3((unsigned)((max_det + 255) / 256), (unsigned)B), dim3(256), 0, S(s)>>>(predn, det, count, image_index, max_det, I,
                                                                                                      cap, dt, dt_count);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

extern "C" int icaf_missrate_match(const double* gt_box, const double* gt_height, const int* gt_occlusion, const int* gt_ignore_base,
                                   const int* gt_off, int I, int max_labels_per_image, const double* dt, const int* dt_count, int cap,
                                   int* order, int* dt_gt, unsigned char* dt_ignore, unsigned char* gt_ignore, icaf_stream_t s) {
    if (!gt_off || !dt || !dt_count || !order || !dt_gt || !dt_ignore) return fail(ICAF_ERR_ARG, "icaf_missrate_match: null pointer");
    if (I < 1 || max_labels_per_image < 0) return fail(ICAF_ERR_ARG, "icaf_missrate_match: I must be positive, max_labels_per_image not negative");
    if (max_labels_per_image > MR_MAX_LABELS)
        return fail(ICAF_ERR_UNSUPPORTED, "icaf_missrate_match: at most %d labels per image (%d)", MR_MAX_LABELS, max_labels_per_image);
    if (cap < 1 || cap > MR_MAX_DET) return fail(ICAF_ERR_UNSUPPORTED, "icaf_missrate_match: cap must be in [1, %d] (%d)", MR_MAX_DET, cap);
    if (max_labels_per_image > 0 && (!gt_box || !gt_height || !gt_occlusion || !gt_ignore_base || !gt_ignore))
        return fail(ICAF_ERR_ARG, "icaf_missrate_match: label table missing");
    missrate_match_kernel<<<dim3((unsigned)I), dim3(MR_THREADS), 0, S(s)>>>(gt_box, gt_height, gt_occlusion, gt_ignore_base, gt_off, dt, dt_count,
                                                                           cap, order, dt_gt, dt_ignore, gt_ignore);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
