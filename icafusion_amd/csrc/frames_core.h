// The device letterbox (utils/datasets.py: resize_bilinear + grey padding) stated once: its arithmetic (lb_tap, lb_rows), its tile (lb_tile:
// the whole body of letterbox_frames_kernel in frames.hip and of the mode-0 branch of resize_frames_kernel in resize.hip) and the host checks
// and grid of the two entry points (frames_launch_prepare).  Both files are built with fp contraction off.
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

// One workgroup: the 32 x 64 output tile of a bilinear (mode 0) descriptor, three planes from `d` on.  Tiles that hold resized pixels and
// pass the budget rule stage the source rectangle those pixels tap in `lds` (LB_LDS bytes, 16-byte aligned); the others, and every tile
// under force_direct, tap the frame itself.  The choice is workgroup-uniform: every thread reaches the barrier.
__device__ __forceinline__ void lb_tile(const unsigned char* __restrict__ frame, const icaf_frame_geom& g, unsigned char* lds,
                                        unsigned char* __restrict__ d, long long plane_stride, int H, int W, int swap_rb, int force_direct) {
    // resized pixels of this tile: output rows [ra, rb], columns [ca, cb] in resized coordinates (empty: padding only)
    const int ra = max((int)blockIdx.y * LB_TH, g.top) - g.top, rb = min(min((int)blockIdx.y * LB_TH + LB_TH, H), g.top + g.nh) - 1 - g.top;
    const int ca = max((int)blockIdx.x * LB_TW, g.left) - g.left, cb = min(min((int)blockIdx.x * LB_TW + LB_TW, W), g.left + g.nw) - 1 - g.left;
    LbTile t{0, 0, 0, 0};
    bool staged = false;
    int rows_cap, cols_cap, nvec;
    if (ra <= rb && ca <= cb && !force_direct && lb_budget(g, rows_cap, cols_cap, nvec)) {
        int i0, i1, hi0, hi1;
        float f;
        lb_tap(ra, g.sy, g.h0, i0, i1, f);
        lb_tap(rb, g.sy, g.h0, hi0, hi1, f);
        t.y_lo = i0; t.nrows = hi1 - i0 + 1;
        lb_tap(ca, g.sx, g.w0, i0, i1, f);
        lb_tap(cb, g.sx, g.w0, hi0, hi1, f);
        t.x_lo = i0; t.ncols = hi1 - i0 + 1;
        staged = t.nrows <= rows_cap && t.ncols <= cols_cap;      // holds by construction of the caps; a tile that did not fit would go direct
    }
    if (staged) {
        const int tid = threadIdx.y * LB_TX + threadIdx.x, lstride = nvec * 16;
        const long long frame_bytes = (long long)g.h0 * g.pitch;
        for (int idx = tid; idx < t.nrows * nvec; idx += LB_TX * LB_TH) {
            const int row = idx / nvec, v = idx - row * nvec;
            // g.offset is 16-byte aligned, so rounding a row's first byte down to a vector boundary never leaves the frame
            const long long a = ((((long long)(t.y_lo + row) * g.pitch + (long long)t.x_lo * g.ch) >> 4) + v) << 4;
            u32x4 q = {0u, 0u, 0u, 0u};
            if (a + 16 <= frame_bytes) {
                q = *(const u32x4*)(frame + a);
            } else {                                               // the frame's last, partial vector: byte by byte, nothing past h0 * pitch
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (a + k < frame_bytes) q[k >> 2] |= (unsigned int)frame[a + k] << (8 * (k & 3));
            }
            *(u32x4*)(lds + (long long)row * lstride + v * 16) = q;
        }
        __syncthreads();
        lb_rows<true>(frame, g, lds, lstride, t, d, plane_stride, H, W, swap_rb);
    } else {
        lb_rows<false>(frame, g, lds, 0, t, d, plane_stride, H, W, swap_rb);
    }
}

// Host side of icaf_letterbox_frames / icaf_resize_frames (`who`, for the messages): every refusal in front of the launch, then the grid —
// one workgroup per 32 x 64 tile of each (modality, image).  `mode` may be null (every row mode 0); returns ICAF_OK or the failure's code.
inline int frames_launch_prepare(const char* who, const void* arena, const icaf_frame_geom* geom, const int* mode, const void* dst, int nstreams,
                                 int B, int ctot, int H, int W, dim3& grid) {
    if (!arena || !geom || !dst) return fail(ICAF_ERR_ARG, "%s: null pointer", who);
    if (((uintptr_t)arena & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)geom & 7) || ((uintptr_t)mode & 3))
        return fail(ICAF_ERR_ARG, "%s: arena and dst must be 16-byte aligned, the geometry table 8-byte, a mode table 4-byte aligned", who);
    if (nstreams < 1 || B < 1 || H < 1 || W < 1 || W % LB_PX) return fail(ICAF_ERR_ARG, "%s: bad geometry (W %% 16 == 0)", who);
    if (ctot < 3 * nstreams) return fail(ICAF_ERR_ARG, "%s: %d modalities need ctot >= %d, got %d", who, nstreams, 3 * nstreams, ctot);
    const long long gz = (long long)nstreams * B, gy = (H + LB_TH - 1) / LB_TH;
    if (gz > 65535 || gy > 65535) return fail(ICAF_ERR_UNSUPPORTED, "%s: grid %lld x %lld too large", who, gy, gz);
    grid = dim3((unsigned)((W + LB_TW - 1) / LB_TW), (unsigned)gy, (unsigned)gz);
    return ICAF_OK;
}

}  // namespace icaf
