// The arithmetic and the tile machinery of the device letterbox (utils/datasets.py: resize_bilinear + grey padding), shared by
// icaf_letterbox_frames (frames.hip) and the mode-0 rows of icaf_resize_frames (resize.hip).  Both files are built with fp contraction off.
#pragma once
#include "icaf_common.h"

namespace icaf {

constexpr int LB_TW = 64, LB_TH = 32;      // output tile of one workgroup: 32 rows x 64 columns of all three planes of one (image, modality)
constexpr int LB_PX = 16;                  // output columns per thread: one 16-byte store per plane
constexpr int LB_TX = LB_TW / LB_PX;       // 4 thread columns x 32 thread rows = 128 threads, one output row each
constexpr int LB_LDS = ICAF_LETTERBOX_LDS_BYTES;
constexpr unsigned char LB_PAD = 114;

// source tap of resize_bilinear for output index j: s = (j + 0.5) * scale - 0.5 as two rounded operations, i0 = floor(s) (may be -1),
// frac = s - i0 BEFORE clamping, both indices clamped into [0, n - 1]
__device__ __forceinline__ void lb_tap(int j, float scale, int n, int& i0, int& i1, float& frac) {
    float s = ((float)j + 0.5f) * scale;
    s = s - 0.5f;
    const float fl = floorf(s);
    frac = s - fl;
    const int i = (int)fl;
    i0 = min(max(i, 0), n - 1);
    i1 = min(max(i + 1, 0), n - 1);
}

struct LbTile {
    int x_lo, y_lo, ncols, nrows;      // source rectangle the tile's resized pixels tap (zero-sized: the tile is padding only)
};

// One thread: 16 output columns of one output row, three planes.  STAGED: taps come from the LDS copy of the tile's source rectangle
// (row r of it starts at lds + r * lstride + phase of that row); otherwise from the frame itself with clamped indices.
template <bool STAGED>
__device__ __forceinline__ void lb_rows(const unsigned char* __restrict__ frame, const icaf_frame_geom& g, const unsigned char* lds, int lstride,
                                        const LbTile& t, unsigned char* __restrict__ dst, long long plane_stride, int H, int W, int swap_rb) {
    const int x = blockIdx.x * LB_TW + threadIdx.x * LB_PX, r = blockIdx.y * LB_TH + threadIdx.y;
    if (x >= W || r >= H) return;
    unsigned char* o = dst + (long long)r * W + x;
    const u32x4 padv = {0x72727272u, 0x72727272u, 0x72727272u, 0x72727272u};
    const int jr = r - g.top;
    if (jr < 0 || jr >= g.nh || x + LB_PX <= g.left || x >= g.left + g.nw) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *(u32x4*)(o + c * plane_stride) = padv;
        return;
    }
    int y0, y1;
    float fy;
    lb_tap(jr, g.sy, g.h0, y0, y1, fy);
    const float gy = 1.0f - fy;
    long long row0, row1;                      // byte offset of the two source rows, the rectangle's first column folded in
    if (STAGED) {
        const long long c0 = (long long)t.x_lo * g.ch;
        row0 = (long long)(y0 - t.y_lo) * lstride + (int)(((long long)y0 * g.pitch + c0) & 15) - c0;
        row1 = (long long)(y1 - t.y_lo) * lstride + (int)(((long long)y1 * g.pitch + c0) & 15) - c0;
    } else {
        row0 = (long long)y0 * g.pitch;
        row1 = (long long)y1 * g.pitch;
    }
    const unsigned char* src = STAGED ? lds : frame;
    const bool rgb = g.ch == 3;
    u32x4 out[3] = {padv, padv, padv};
#pragma unroll
    for (int j = 0; j < LB_PX; ++j) {
        const int jx = x + j - g.left;
        if (jx < 0 || jx >= g.nw) continue;
        int x0, x1;
        float fx;
        lb_tap(jx, g.sx, g.w0, x0, x1, fx);
        const float gx = 1.0f - fx;
        const int b0 = x0 * g.ch, b1 = x1 * g.ch;
        unsigned int val = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c == 0 || rgb) {
                const int sc = rgb ? (swap_rb ? 2 - c : c) : 0;
                const float a00 = (float)src[row0 + b0 + sc], a01 = (float)src[row0 + b1 + sc];
                const float a10 = (float)src[row1 + b0 + sc], a11 = (float)src[row1 + b1 + sc];
                const float top = a00 * gx + a01 * fx;
                const float bot = a10 * gx + a11 * fx;
                float v = top * gy + bot * fy;
                v = floorf(v + 0.5f);
                v = fminf(fmaxf(v, 0.0f), 255.0f);
                val = (unsigned int)v;
            }
            const int sh = 8 * (j & 3);
            out[c][j >> 2] = (out[c][j >> 2] & ~(0xffu << sh)) | (val << sh);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *(u32x4*)(o + c * plane_stride) = out[c];
}

// descriptor-level budget rule (ops.letterbox_staged states the same on the host): the rectangle a 32 x 64 tile can tap is at most
// (int)(32 sy) + 4 rows of (int)(64 sx) + 4 pixels; a staged row is that many bytes plus up to 15 of alignment phase, in whole 16-byte vectors
__device__ __forceinline__ bool lb_budget(const icaf_frame_geom& g, int& rows_cap, int& cols_cap, int& nvec) {
    rows_cap = min(g.h0, (int)(32.0f * g.sy) + 4);
    cols_cap = min(g.w0, (int)(64.0f * g.sx) + 4);
    nvec = (cols_cap * g.ch + 30) >> 4;
    return g.sy < 1024.0f && g.sx < 1024.0f && (long long)rows_cap * nvec * 16 <= LB_LDS;
}

}  // namespace icaf
