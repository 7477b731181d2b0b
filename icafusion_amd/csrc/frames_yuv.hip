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

// The tap of lb_rows_taps: pixel (yy[i], x) as R, G, B.  STAGED: its samples come from the LDS rectangles of `t`, otherwise from the
// arena with clamped indices.
template <bool STAGED>
struct YuvTap {
    const unsigned char* __restrict__ src;     // lds or the arena
    const icaf_yuv_geom& q;
    const YuvTile& t;
    const YuvCoef& k;
    long long yrow[2], crow[2][2];             // byte offsets of the two luma rows and of their chroma rows per component, first column folded in

    __device__ __forceinline__ void rows(const int* yy) {
        const icaf_frame_geom& g = q.g;
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
    }

    // converted at native resolution
    __device__ __forceinline__ void operator()(int i, int x, float* rgb) const {
        const int cx = (x >> 1) * q.c_step;
        yuv_to_rgb(k, src[yrow[i] + x], src[crow[i][0] + cx], src[crow[i][1] + cx], rgb);
    }
};

// One workgroup: the 32 x 64 output tile of a kind-1 row.  As lb_tile: tiles that hold resized pixels and pass the budget rule stage what
// those pixels tap, the others, and every tile under force_direct, tap the arena.  The choice is workgroup-uniform.
__device__ __forceinline__ void yuv_tile(const unsigned char* __restrict__ arena, const icaf_yuv_geom& q, unsigned char* lds, unsigned char* __restrict__ d,
                                         long long plane_stride, int H, int W, int force_direct) {
    const icaf_frame_geom& g = q.g;
    const YuvCoef k = yuv_coef(q.matrix);
    YuvTile t{};
    LbTile y{0, 0, 0, 0};
    bool staged = false;
    int rows_cap, cols_cap, nvec_y, crows_cap, ccols_cap, nvec_c, nrect;
    if (!force_direct && yuv_budget(q, rows_cap, cols_cap, nvec_y, crows_cap, ccols_cap, nvec_c, nrect) && lb_extent(g, H, W, y)) {
        t.y_lo = y.y_lo; t.nrows = y.nrows;
        t.cy_lo = y.y_lo >> 1; t.ncr = ((y.y_lo + y.nrows - 1) >> 1) - t.cy_lo + 1;
        t.x_lo = y.x_lo; t.ncols = y.ncols;
        t.cx_lo = y.x_lo >> 1; t.ncc = ((y.x_lo + y.ncols - 1) >> 1) - t.cx_lo + 1;
        staged = t.nrows <= rows_cap && t.ncols <= cols_cap && t.ncr <= crows_cap && t.ncc <= ccols_cap;      // holds by construction of the caps
    }
    if (staged) {
        const int chh = (g.h0 + 1) >> 1, cw = (g.w0 + 1) >> 1;
        t.ystride = nvec_y * 16;
        t.cstride = nvec_c * 16;
        const int c0 = t.nrows * t.ystride;                            // the chroma rectangles follow the luma rows that are there
        lb_stage(arena, g.offset, g.offset + (long long)g.h0 * g.pitch, g.offset + (long long)t.y_lo * g.pitch + t.x_lo, g.pitch, t.nrows, nvec_y, lds);
        const long long crect = (long long)t.cy_lo * q.c_pitch + (long long)t.cx_lo * q.c_step;
        if (nrect == 1) {                                              // byte pairs: Cb and Cr one byte apart, whichever comes first
            const long long lo = min(q.cb_offset, q.cr_offset);
            t.cbase[0] = t.cbase[1] = c0;
            t.cfirst[0] = t.cfirst[1] = lo + crect;
            t.cdelta[0] = (int)(q.cb_offset - lo); t.cdelta[1] = (int)(q.cr_offset - lo);
            lb_stage(arena, lo, lo + (long long)(chh - 1) * q.c_pitch + 2 * cw, t.cfirst[0], q.c_pitch, t.ncr, nvec_c, lds + c0);
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const long long lo = c ? q.cr_offset : q.cb_offset;
                t.cbase[c] = c0 + c * t.ncr * t.cstride;
                t.cfirst[c] = lo + crect;
                t.cdelta[c] = 0;
                lb_stage(arena, lo, lo + (long long)(chh - 1) * q.c_pitch + cw, t.cfirst[c], q.c_pitch, t.ncr, nvec_c, lds + t.cbase[c]);
            }
        }
        __syncthreads();
        YuvTap<true> tap{lds, q, t, k};
        lb_rows_taps(g, tap, d, plane_stride, H, W);
    } else {
        YuvTap<false> tap{arena, q, t, k};
        lb_rows_taps(g, tap, d, plane_stride, H, W);
    }
}

__global__ __launch_bounds__(LB_TX * LB_TH) void letterbox_yuv_frames_kernel(const unsigned char* __restrict__ arena,
                                                                            const icaf_yuv_geom* __restrict__ geom, int B, int ctot, int H, int W,
                                                                            unsigned char* __restrict__ dst, int swap_rb, int force_direct) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[YUV_LDS_ALLOC];
    icaf_yuv_geom q;
    unsigned char* d;
    if (lb_table_row(arena, geom, B, ctot, H, W, dst, lds, swap_rb, force_direct, q, d)) yuv_tile(arena, q, lds, d, (long long)H * W, H, W, force_direct);
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_letterbox_yuv_frames(const void* arena, const icaf_yuv_geom* geom, int nstreams, int B, void* dst, int ctot, int H, int W,
                                         int swap_rb, icaf_stream_t s) {
    return frames_launch("icaf_letterbox_yuv_frames", letterbox_yuv_frames_kernel, arena, geom, nullptr, dst, nstreams, B, ctot, H, W, swap_rb, s);
}
