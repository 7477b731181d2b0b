// Shared device pieces of the post-processing kernels (nms.hip, confluence.hip, valstats.hip): the workgroup-wide ordered rank of a predicate,
// the workgroup-wide inclusive scan, and the fp32 box expressions of the reference.  Device code only.  Every file that includes this header is
// compiled with fp contraction off (`#pragma clang fp contract(off)` ahead of the include, -ffp-contract=off in build.py) and the pragma is
// repeated here: the box expressions must round like the reference's separate fp32 torch ops, one rounding per operation.
#pragma once
#pragma clang fp contract(off)
#include "icaf_common.h"

namespace icaf {

// ---- ordered rank ------------------------------------------------------------------------------------------------------------------------------
// The number of threads before this one (thread order) whose predicate is set; total = all set predicates; the inclusive count is rank + own bit.
// One ballot, the per-wave popcounts through LDS, one barrier pair.  `lds`: WAVES ints of the caller.  The call is workgroup-uniform
// (WAVES * 64 threads, all of them).
// THE BARRIERS: the leading one publishes the popcounts, the trailing one frees `lds` for the next call — and that is all it does.  It does NOT
// order what the caller then writes with the rank against later readers: a call site keeps its own barrier between those writes and the first
// read of them by another thread.
template <int WAVES>
__device__ __forceinline__ int wg_rank(bool pred, int* lds, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(pred);
    if (lane == 0) lds[wave] = __popcll(m);
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int c = lds[w];
        if (w < wave) before += c;
        tot += c;
    }
    __syncthreads();
    total = tot;
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// ---- inclusive scan ----------------------------------------------------------------------------------------------------------------------------
// inclusive prefix sum of v over the WAVES * 64 threads of the workgroup, the total through `total`: shuffles inside a wave, the wave sums through
// `wsum` (WAVES entries of the caller) — two barriers, the trailing one frees `wsum` (and, as above, orders nothing else of the caller's).
// An exclusive scan of more values than threads is a per-thread run sum, this scan, and the run again from incl - sum.
template <int WAVES, typename T>
__device__ __forceinline__ T wg_incl_scan(T v, T* wsum, T& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return base + inc;
}

// ---- boxes -------------------------------------------------------------------------------------------------------------------------------------
// xywh -> xyxy exactly as the reference (utils/general.py:332-339): centre -/+ half the size, the half by a division
__device__ __forceinline__ void xywh_to_xyxy(const float* __restrict__ p, float& x1, float& y1, float& x2, float& y2) {
    const float hw = p[2] / 2.0f, hh = p[3] / 2.0f;
    x1 = p[0] - hw; y1 = p[1] - hh; x2 = p[0] + hw; y2 = p[1] + hh;
}

// box_iou (utils/general.py:455-477) of box a against box b with their areas (x2 - x1) * (y2 - y1): clamp(0) on the overlap's width and height,
// inter / (area_a + area_b - inter), an IEEE division.  The operand order is the reference's (box1 = a): pass the boxes as the call site's
// reference statement does.
__device__ __forceinline__ float box_iou(float ax1, float ay1, float ax2, float ay2, float area_a, float bx1, float by1, float bx2, float by2,
                                         float area_b) {
    const float w = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.0f), h = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.0f);
    const float inter = w * h;
    return inter / (area_a + area_b - inter);
}

// scale_coords + clip_coords (utils/general.py:386-407) of one xyxy box, sc = {gain, pad_x, pad_y, w0, h0}: THE expression of the mapping,
// shared by match_predictions_kernel and scale_detections_kernel (tests/golden/match_predictions.npz, made by the reference, guards both)
__device__ __forceinline__ void native_box(const float* __restrict__ sc, float& x1, float& y1, float& x2, float& y2) {
    const float gain = sc[0], padx = sc[1], pady = sc[2], w0 = sc[3], h0 = sc[4];
    x1 = (x1 - padx) / gain; x2 = (x2 - padx) / gain; y1 = (y1 - pady) / gain; y2 = (y2 - pady) / gain;
    x1 = fminf(fmaxf(x1, 0.0f), w0); x2 = fminf(fmaxf(x2, 0.0f), w0);
    y1 = fminf(fmaxf(y1, 0.0f), h0); y2 = fminf(fmaxf(y2, 0.0f), h0);
}

}  // namespace icaf
