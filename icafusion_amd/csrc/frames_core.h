// The device letterbox (utils/datasets.py: resize_bilinear + grey padding) stated once: its arithmetic (lb_tap, lb_rows), its tile (lb_tile:
// the whole body of letterbox_frames_kernel in frames.hip and of the mode-0 branch of resize_frames_kernel in resize.hip) and the host checks
// and grid of the entry points (frames_launch_prepare).  The kernels of the other table kinds (frames_yuv.hip, frames_warp.hip,
// frames_y16.hip) are built from the same pieces: the tile's tap rectangle (lb_extent), the aligned staging copy (lb_stage), the row
// skeleton around a tap functor (lb_rows_taps), the kernel prologue with its kind-0 branch (lb_table_row) and the launcher
// (frames_launch).  Every file that includes this one is built with fp contraction off.
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

// lb_rows for the kinds whose taps are CONVERTED pixels (YUV 4:2:0 samples, pixels seen through a homography): one thread, 16 output
// columns of one output row, three planes.  tap.rows(yy) takes the two source rows of this output row once, tap(i, x, out) gives pixel
// (yy[i], x) as three bytes held as floats, one per output plane; the tap arithmetic on them is lb_rows', operation for operation.
// (lb_rows and y16_rows_direct stay as they are: their taps are plain loads, they read all four of them and compute a grey pixel once
// for the three planes, while this skeleton skips zero-weight taps and blends every plane.  Folding them in would add the skip's
// compares and two blends a pixel to the two kernels that serve every plain stream.)
template <class Tap>
__device__ __forceinline__ void lb_rows_taps(const icaf_frame_geom& g, Tap& tap, unsigned char* __restrict__ dst, long long plane_stride, int H, int W) {
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
    int yy[2];
    float fy;
    lb_tap(jr, g.sy, g.h0, yy[0], yy[1], fy);
    const float gy = 1.0f - fy;
    tap.rows(yy);
    u32x4 out[3] = {padv, padv, padv};
#pragma unroll
    for (int j = 0; j < LB_PX; ++j) {
        const int jx = x + j - g.left;
        if (jx < 0 || jx >= g.nw) continue;
        int xx[2];
        float fx;
        lb_tap(jx, g.sx, g.w0, xx[0], xx[1], fx);
        const float gx = 1.0f - fx;
        // [row][column][plane] of the four taps.  A tap whose weight is +0 is neither read nor converted: it takes its neighbour's finite
        // bytes and adds +0 to the lerp, the same bits (a frame copied between pads evaluates one tap, not four)
        float a[2][2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if ((i == 0 || fy != 0.0f) && (h == 0 || fx != 0.0f)) {
                    tap(i, xx[h], a[i][h]);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) a[i][h][c] = h ? a[i][0][c] : a[0][0][c];
                }
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float top = a[0][0][c] * gx + a[0][1][c] * fx;
            const float bot = a[1][0][c] * gx + a[1][1][c] * fx;
            float v = top * gy + bot * fy;
            v = floorf(v + 0.5f);
            v = fminf(fmaxf(v, 0.0f), 255.0f);
            const int sh = 8 * (j & 3);
            out[c][j >> 2] = (out[c][j >> 2] & ~(0xffu << sh)) | ((unsigned int)v << sh);
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

// The resized pixels of this workgroup's tile — output rows [ra, rb], columns [ca, cb] in resized coordinates — and the source rectangle
// their taps touch, clamped into the frame: t.y_lo / t.x_lo the first row / column, t.nrows / t.ncols its size.  False (t untouched): the
// tile is padding only.  Workgroup-uniform.
__device__ __forceinline__ bool lb_extent(const icaf_frame_geom& g, int H, int W, LbTile& t) {
    const int ra = max((int)blockIdx.y * LB_TH, g.top) - g.top, rb = min(min((int)blockIdx.y * LB_TH + LB_TH, H), g.top + g.nh) - 1 - g.top;
    const int ca = max((int)blockIdx.x * LB_TW, g.left) - g.left, cb = min(min((int)blockIdx.x * LB_TW + LB_TW, W), g.left + g.nw) - 1 - g.left;
    if (ra > rb || ca > cb) return false;
    int i0, i1, hi0, hi1;
    float f;
    lb_tap(ra, g.sy, g.h0, i0, i1, f);
    lb_tap(rb, g.sy, g.h0, hi0, hi1, f);
    t.y_lo = i0; t.nrows = hi1 - i0 + 1;
    lb_tap(ca, g.sx, g.w0, i0, i1, f);
    lb_tap(cb, g.sx, g.w0, hi0, hi1, f);
    t.x_lo = i0; t.ncols = hi1 - i0 + 1;
    return true;
}

// Copy `nrows` rows of `nvec` aligned 16-byte vectors into LDS, one after the other (row r at out + r * nvec * 16): row r starts at the
// vector that holds byte first + r * pitch of `base`, which is 16-byte aligned.  Only bytes of [lo, hi) — the frame, or one plane of it —
// are read: a vector that crosses either end goes byte by byte (a frame starts on a vector boundary, a chroma plane need not).  Every
// thread of the workgroup calls it.  (yuv_tile: luma and chroma rectangles; warp_tile: the source box.  lb_tile keeps its own loop.)
__device__ __forceinline__ void lb_stage(const unsigned char* __restrict__ base, long long lo, long long hi, long long first, int pitch, int nrows,
                                         int nvec, unsigned char* out) {
    const int tid = threadIdx.y * LB_TX + threadIdx.x;
    for (int idx = tid; idx < nrows * nvec; idx += LB_TX * LB_TH) {
        const int row = idx / nvec, v = idx - row * nvec;
        const long long a = (((first + (long long)row * pitch) >> 4) + v) << 4;
        u32x4 w = {0u, 0u, 0u, 0u};
        if (a >= lo && a + 16 <= hi) {
            w = *(const u32x4*)(base + a);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (a + k >= lo && a + k < hi) w[k >> 2] |= (unsigned int)base[a + k] << (8 * (k & 3));
        }
        *(u32x4*)(out + ((long long)row * nvec + v) * 16) = w;
    }
}

// One workgroup: the 32 x 64 output tile of a bilinear (mode 0) descriptor, three planes from `d` on.  Tiles that hold resized pixels and
// pass the budget rule stage the source rectangle those pixels tap in `lds` (LB_LDS bytes, 16-byte aligned); the others, and every tile
// under force_direct, tap the frame itself.  The choice is workgroup-uniform: every thread reaches the barrier.
__device__ __forceinline__ void lb_tile(const unsigned char* __restrict__ frame, const icaf_frame_geom& g, unsigned char* lds,
                                        unsigned char* __restrict__ d, long long plane_stride, int H, int W, int swap_rb, int force_direct) {
    // This tile serves every plain stream and every kind-0 row, and it keeps its own statement of lb_extent and lb_stage: through the shared
    // forms its staged items measured 1.2 - 1.7 % slower (lb_stage) and still about 1 % slower (lb_extent alone) than the parent's
    // (profiles/frames_share_ab.json), so the two stay written out here, as they were.
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

// The prologue of a table kernel (rows that embed icaf_frame_geom as `g` behind a `kind`): this workgroup's row q = geom[img], img =
// modality * B + b, and `d`, the first of its three output planes.  A kind-0 row is icaf_letterbox_frames' descriptor: its tile, its
// bytes, run here and false comes back.  The branch is workgroup-uniform.
template <class Row>
__device__ __forceinline__ bool lb_table_row(const unsigned char* __restrict__ arena, const Row* __restrict__ geom, int B, int ctot, int H, int W,
                                             unsigned char* __restrict__ dst, unsigned char* lds, int swap_rb, int force_direct, Row& q,
                                             unsigned char*& d) {
    const int img = blockIdx.z, m = img / B, b = img - m * B;
    q = geom[img];
    const long long plane_stride = (long long)H * W;
    d = dst + ((long long)b * ctot + 3 * m) * plane_stride;
    if (q.kind != 0) return true;
    lb_tile(arena + q.g.offset, q.g, lds, d, plane_stride, H, W, swap_rb, force_direct);
    return false;
}

// An entry point of a letterbox kernel (arena, table, B, ctot, H, W, dst, swap_rb, force_direct, extra...): prepare, launch, launch check.
// `aux` is the kernel's second table where it has one (checked for alignment only), else null.
template <class Kernel, class Row, class... Extra>
inline int frames_launch(const char* who, Kernel kernel, const void* arena, const Row* geom, const int* aux, void* dst, int nstreams, int B, int ctot,
                         int H, int W, int swap_rb, icaf_stream_t s, Extra... extra) {
    dim3 grid;
    if (const int rc = frames_launch_prepare(who, arena, (const icaf_frame_geom*)geom, aux, dst, nstreams, B, ctot, H, W, grid)) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(LB_TX, LB_TH), 0, S(s), (const unsigned char*)arena, geom, B, ctot, H, W, (unsigned char*)dst,
                       swap_rb ? 1 : 0, g_opt.letterbox_direct ? 1 : 0, extra...);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

}  // namespace icaf
