// Device letterbox of native YUV 4:2:0 camera frames (NV12 / NV21 / I420 / YV12 surfaces), byte for byte equal to
// letterbox(yuv420_to_bgr(...)) of utils/datasets.py followed by BGR -> RGB planes: every one of the four bilinear taps of an output pixel
// is converted to three bytes with the integer rule of include/icaf.h (nearest chroma: pixel (y, x) reads chroma sample (y >> 1, x >> 1)),
// then the fp32 tap arithmetic of frames_core.h (lb_tap, top / bot / out, floor(v + 0.5), clip) runs on those bytes.  Built with fp
// contraction off like frames.hip.  A kind-0 row of the table is icaf_letterbox_frames' descriptor and runs lb_tile itself, so that a YUV
// stream beside an interleaved or grey one is still one launch.
#include "frames_core.h"

namespace icaf {

constexpr int YUV_LDS = ICAF_YUV_LDS_BYTES;
constexpr int YUV_LDS_ALLOC = YUV_LDS > LB_LDS ? YUV_LDS : LB_LDS;      // one array serves both kinds of row

// R = clip8((ky * (Y - yoff) + rv * e + rnd) >> sh) and so on.  The full-range rule Y + ((k e + 32768) >> 16) is the same number as
// ((Y << 16) + k e + 32768) >> 16 (Y << 16 is a multiple of 2^16, the flooring shift passes it through), so one form serves all three
// matrices; the largest magnitude, 255 * 65536 + 116130 * 127 + 32768, is far inside 32 bits.
struct YuvCoef {
    int yoff, ky, rv, gu, gv, bu, rnd, sh;
};

__device__ __forceinline__ YuvCoef yuv_coef(int matrix) {
    if (matrix == 0) return {16, 298, 409, -100, -208, 516, 128, 8};             // BT.601, limited range
    if (matrix == 1) return {16, 298, 459, -55, -136, 541, 128, 8};              // BT.709, limited range
    return {0, 65536, 91881, -22554, -46802, 116130, 32768, 16};                 // BT.601, full range (JFIF)
}

__device__ __forceinline__ void yuv_to_rgb(const YuvCoef& k, int Y, int Cb, int Cr, float* rgb) {
    const int d = Cb - 128, e = Cr - 128;
    const int t = k.ky * (Y - k.yoff) + k.rnd;
    rgb[0] = (float)min(max((t + k.rv * e) >> k.sh, 0), 255);
    rgb[1] = (float)min(max((t + k.gu * d + k.gv * e) >> k.sh, 0), 255);
    rgb[2] = (float)min(max((t + k.bu * d) >> k.sh, 0), 255);
}

// What a tile staged: the luma rectangle [y_lo, y_lo + nrows) x [x_lo, x_lo + ncols) at lds + 0 in rows of `ystride` bytes, and the chroma
// samples [cy_lo, cy_lo + ncr) x [cx_lo, cx_lo + ncc) under it in rows of `cstride` bytes: interleaved chroma (c_step 2) as ONE rectangle
// of byte pairs from the lower of the two offsets on, planar chroma (c_step 1) as one rectangle per plane.  Component k (0 = Cb, 1 = Cr)
// finds its rectangle at lds + cbase[k]; its first byte is arena byte cfirst[k] (its low four bits are the alignment phase of row 0, every
// further row adds c_pitch) and the component sits cdelta[k] bytes into a sample.
struct YuvTile {
    int x_lo, y_lo, ncols, nrows, cx_lo, cy_lo, ncc, ncr;
    int ystride, cstride, cbase[2], cdelta[2];
    long long cfirst[2];
};

// the budget rule (include/icaf.h; ops.yuv_letterbox_staged states the same on the host)
__device__ __forceinline__ bool yuv_budget(const icaf_yuv_geom& q, int& rows_cap, int& cols_cap, int& nvec_y, int& crows_cap, int& ccols_cap,
                                           int& nvec_c, int& nrect) {
    const icaf_frame_geom& g = q.g;
    rows_cap = min(g.h0, (int)(32.0f * g.sy) + 4);
    cols_cap = min(g.w0, (int)(64.0f * g.sx) + 4);
    nvec_y = (cols_cap + 30) >> 4;
    crows_cap = min((g.h0 + 1) >> 1, (rows_cap >> 1) + 1);       // n luma rows from any row on touch at most n / 2 + 1 chroma rows
    ccols_cap = min((g.w0 + 1) >> 1, (cols_cap >> 1) + 1);
    nrect = q.c_step == 2 ? 1 : 2;
    nvec_c = (ccols_cap * q.c_step + 30) >> 4;
    return g.sy < 1024.0f && g.sx < 1024.0f && ((long long)rows_cap * nvec_y + (long long)nrect * crows_cap * nvec_c) * 16 <= YUV_LDS;
}

// Copy `nrows` rows of `nvec` aligned 16-byte vectors into LDS: row r starts at the vector that holds arena byte first + r * pitch.  Only
// bytes of [lo, hi) — the plane — are read: a vector that crosses either end goes byte by byte (the arena is 16-byte aligned, a chroma plane
// need not be).
__device__ __forceinline__ void yuv_stage(const unsigned char* __restrict__ arena, long long lo, long long hi, long long first, int pitch, int nrows,
                                          int nvec, unsigned char* out, int tid) {
    for (int idx = tid; idx < nrows * nvec; idx += LB_TX * LB_TH) {
        const int row = idx / nvec, v = idx - row * nvec;
        const long long a = (((first + (long long)row * pitch) >> 4) + v) << 4;
        u32x4 w = {0u, 0u, 0u, 0u};
        if (a >= lo && a + 16 <= hi) {
            w = *(const u32x4*)(arena + a);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (a + k >= lo && a + k < hi) w[k >> 2] |= (unsigned int)arena[a + k] << (8 * (k & 3));
        }
        *(u32x4*)(out + ((long long)row * nvec + v) * 16) = w;
    }
}

// One thread: 16 output columns of one output row, planes R, G, B.  STAGED: taps come from the LDS rectangles of `t`, otherwise from the
// arena with clamped indices.
template <bool STAGED>
__device__ __forceinline__ void yuv_rows(const unsigned char* __restrict__ arena, const icaf_yuv_geom& q, const unsigned char* lds, const YuvTile& t,
                                         const YuvCoef& k, unsigned char* __restrict__ dst, long long plane_stride, int H, int W) {
    const icaf_frame_geom& g = q.g;
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
    long long yrow[2], crow[2][2];             // byte offsets of the two luma rows and of their chroma rows per component, first column folded in
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int cy = yy[i] >> 1;
        if (STAGED) {
            yrow[i] = (long long)(yy[i] - t.y_lo) * t.ystride + (int)(((long long)yy[i] * g.pitch + t.x_lo) & 15) - t.x_lo;
#pragma unroll
            for (int c = 0; c < 2; ++c)
                crow[i][c] = t.cbase[c] + (long long)(cy - t.cy_lo) * t.cstride + (int)((t.cfirst[c] + (long long)(cy - t.cy_lo) * q.c_pitch) & 15) +
                             t.cdelta[c] - (long long)t.cx_lo * q.c_step;
        } else {
            yrow[i] = g.offset + (long long)yy[i] * g.pitch;
            crow[i][0] = q.cb_offset + (long long)cy * q.c_pitch;
            crow[i][1] = q.cr_offset + (long long)cy * q.c_pitch;
        }
    }
    const unsigned char* src = STAGED ? lds : arena;
    u32x4 out[3] = {padv, padv, padv};
#pragma unroll
    for (int j = 0; j < LB_PX; ++j) {
        const int jx = x + j - g.left;
        if (jx < 0 || jx >= g.nw) continue;
        int xx[2];
        float fx;
        lb_tap(jx, g.sx, g.w0, xx[0], xx[1], fx);
        const float gx = 1.0f - fx;
        // [row][column][R, G, B] of the four taps, converted at native resolution.  A tap whose weight is +0 is neither read nor converted: it
        // takes its neighbour's finite bytes and adds +0 to the lerp, the same bits (a frame copied between pads converts one tap, not four)
        float a[2][2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if ((i == 0 || fy != 0.0f) && (h == 0 || fx != 0.0f)) {
                    const int cx = (xx[h] >> 1) * q.c_step;
                    yuv_to_rgb(k, src[yrow[i] + xx[h]], src[crow[i][0] + cx], src[crow[i][1] + cx], a[i][h]);
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

// One workgroup: the 32 x 64 output tile of a kind-1 row.  As lb_tile: tiles that hold resized pixels and pass the budget rule stage what
// those pixels tap, the others, and every tile under force_direct, tap the arena.  The choice is workgroup-uniform.
__device__ __forceinline__ void yuv_tile(const unsigned char* __restrict__ arena, const icaf_yuv_geom& q, unsigned char* lds, unsigned char* __restrict__ d,
                                         long long plane_stride, int H, int W, int force_direct) {
    const icaf_frame_geom& g = q.g;
    const int ra = max((int)blockIdx.y * LB_TH, g.top) - g.top, rb = min(min((int)blockIdx.y * LB_TH + LB_TH, H), g.top + g.nh) - 1 - g.top;
    const int ca = max((int)blockIdx.x * LB_TW, g.left) - g.left, cb = min(min((int)blockIdx.x * LB_TW + LB_TW, W), g.left + g.nw) - 1 - g.left;
    const YuvCoef k = yuv_coef(q.matrix);
    YuvTile t{};
    bool staged = false;
    int rows_cap, cols_cap, nvec_y, crows_cap, ccols_cap, nvec_c, nrect;
    if (ra <= rb && ca <= cb && !force_direct && yuv_budget(q, rows_cap, cols_cap, nvec_y, crows_cap, ccols_cap, nvec_c, nrect)) {
        int i0, i1, hi0, hi1;
        float f;
        lb_tap(ra, g.sy, g.h0, i0, i1, f);
        lb_tap(rb, g.sy, g.h0, hi0, hi1, f);
        t.y_lo = i0; t.nrows = hi1 - i0 + 1;
        t.cy_lo = i0 >> 1; t.ncr = (hi1 >> 1) - t.cy_lo + 1;
        lb_tap(ca, g.sx, g.w0, i0, i1, f);
        lb_tap(cb, g.sx, g.w0, hi0, hi1, f);
        t.x_lo = i0; t.ncols = hi1 - i0 + 1;
        t.cx_lo = i0 >> 1; t.ncc = (hi1 >> 1) - t.cx_lo + 1;
        staged = t.nrows <= rows_cap && t.ncols <= cols_cap && t.ncr <= crows_cap && t.ncc <= ccols_cap;      // holds by construction of the caps
    }
    if (staged) {
        const int tid = threadIdx.y * LB_TX + threadIdx.x;
        const int chh = (g.h0 + 1) >> 1, cw = (g.w0 + 1) >> 1;
        t.ystride = nvec_y * 16;
        t.cstride = nvec_c * 16;
        const int c0 = t.nrows * t.ystride;                            // the chroma rectangles follow the luma rows that are there
        yuv_stage(arena, g.offset, g.offset + (long long)g.h0 * g.pitch, g.offset + (long long)t.y_lo * g.pitch + t.x_lo, g.pitch, t.nrows, nvec_y, lds, tid);
        const long long crect = (long long)t.cy_lo * q.c_pitch + (long long)t.cx_lo * q.c_step;
        if (nrect == 1) {                                              // byte pairs: Cb and Cr one byte apart, whichever comes first
            const long long lo = min(q.cb_offset, q.cr_offset);
            t.cbase[0] = t.cbase[1] = c0;
            t.cfirst[0] = t.cfirst[1] = lo + crect;
            t.cdelta[0] = (int)(q.cb_offset - lo); t.cdelta[1] = (int)(q.cr_offset - lo);
            yuv_stage(arena, lo, lo + (long long)(chh - 1) * q.c_pitch + 2 * cw, t.cfirst[0], q.c_pitch, t.ncr, nvec_c, lds + c0, tid);
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const long long lo = c ? q.cr_offset : q.cb_offset;
                t.cbase[c] = c0 + c * t.ncr * t.cstride;
                t.cfirst[c] = lo + crect;
                t.cdelta[c] = 0;
                yuv_stage(arena, lo, lo + (long long)(chh - 1) * q.c_pitch + cw, t.cfirst[c], q.c_pitch, t.ncr, nvec_c, lds + t.cbase[c], tid);
            }
        }
        __syncthreads();
        yuv_rows<true>(arena, q, lds, t, k, d, plane_stride, H, W);
    } else {
        yuv_rows<false>(arena, q, lds, t, k, d, plane_stride, H, W);
    }
}

__global__ __launch_bounds__(LB_TX * LB_TH) void letterbox_yuv_frames_kernel(const unsigned char* __restrict__ arena,
                                                                            const icaf_yuv_geom* __restrict__ geom, int B, int ctot, int H, int W,
                                                                            unsigned char* __restrict__ dst, int swap_rb, int force_direct) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[YUV_LDS_ALLOC];
    const int img = blockIdx.z, m = img / B, b = img - m * B;      // img = modality * B + b
    const icaf_yuv_geom q = geom[img];
    const long long plane_stride = (long long)H * W;
    unsigned char* d = dst + ((long long)b * ctot + 3 * m) * plane_stride;
    if (q.kind == 0)                                               // workgroup-uniform: icaf_letterbox_frames' row, its tile, its bytes
        lb_tile(arena + q.g.offset, q.g, lds, d, plane_stride, H, W, swap_rb, force_direct);
    else
        yuv_tile(arena, q, lds, d, plane_stride, H, W, force_direct);
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_letterbox_yuv_frames(const void* arena, const icaf_yuv_geom* geom, int nstreams, int B, void* dst, int ctot, int H, int W,
                                         int swap_rb, icaf_stream_t s) {
    dim3 grid;
    if (const int rc = frames_launch_prepare("icaf_letterbox_yuv_frames", arena, (const icaf_frame_geom*)geom, nullptr, dst, nstreams, B, ctot, H, W, grid))
        return rc;
    hipLaunchKernelGGL(letterbox_yuv_frames_kernel, grid, dim3(LB_TX, LB_TH), 0, S(s), (const unsigned char*)arena, geom, B, ctot, H, W,
                       (unsigned char*)dst, swap_rb ? 1 : 0, g_opt.letterbox_direct ? 1 : 0);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
