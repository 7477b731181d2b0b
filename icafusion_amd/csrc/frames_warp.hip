// Device letterbox of a calibrated RGB / IR pair: one modality is seen through a homography (aligned -> source pixel coordinates), byte
// for byte equal to letterbox(warp_perspective(...)) of utils/datasets.py.  The letterbox's four bilinear taps of an output pixel are
// pixels of the ALIGNED frame; each is evaluated from the source frame by the fp32 rule of include/icaf.h (three dot products, two IEEE
// divisions, a constant-border bilinear blend rounded to a byte), then the fp32 tap arithmetic of frames_core.h (lb_tap, top / bot / out,
// floor(v + 0.5), clip) runs on those bytes: the aligned frame never exists in memory.  Built with fp contraction off like frames.hip.  A
// kind-0 row of the table is icaf_letterbox_frames' descriptor and runs lb_tile itself, so that a plain stream beside a warped one is
// still one launch.
#include "frames_core.h"

namespace icaf {

constexpr int WARP_LDS = ICAF_WARP_LDS_BYTES;
constexpr int WARP_LDS_ALLOC = WARP_LDS > LB_LDS ? WARP_LDS : LB_LDS;      // one array serves both kinds of row

// What a tile staged: source pixels [j_lo, j_lo + nrows) x [i_lo, i_lo + ncols) in rows of `lstride` bytes; row j starts at its alignment
// phase, the low four bits of byte j * pitch + i_lo * ch of the frame (rows are copied as aligned 16-byte vectors).
struct WarpTile {
    int i_lo, j_lo, ncols, nrows, lstride;
};

// the projective coordinates of aligned pixel (x, y): the rule of include/icaf.h, every operation rounded on its own
__device__ __forceinline__ void warp_uv(const icaf_warp_geom& q, int y, int x, float& u, float& v, float& Z) {
    const float xf = (float)x, yf = (float)y;
    const float X = (q.m[0] * xf + q.m[1] * yf) + q.m[2];
    const float Y = (q.m[3] * xf + q.m[4] * yf) + q.m[5];
    Z = (q.m[6] * xf + q.m[7] * yf) + q.m[8];
    u = X / Z;
    v = Y / Z;
}

// One in-frame source byte: from the staged box where it holds (jc, ic), otherwise — and always when nothing is staged — from the frame.
// The guard makes the bytes independent of how the box was chosen.
template <bool STAGED>
__device__ __forceinline__ float warp_byte(const unsigned char* __restrict__ src, const icaf_warp_geom& q, const unsigned char* lds, const WarpTile& t,
                                           int jc, int ic, int sc) {
    if (STAGED) {
        const int dj = jc - t.j_lo, di = ic - t.i_lo;
        if ((unsigned)dj < (unsigned)t.nrows && (unsigned)di < (unsigned)t.ncols)
            return (float)lds[dj * t.lstride + (int)(((long long)jc * q.g.pitch + (long long)t.i_lo * q.g.ch) & 15) + di * q.g.ch + sc];
    }
    return (float)src[(long long)jc * q.g.pitch + ic * q.g.ch + sc];
}

// Aligned pixel (y, x) of a kind-1 row as bytes (held as floats) for the planes of `out`: plane c reads source channel sc[c].  The
// coordinates are computed once for all channels.  Taps are read at indices clamped into the frame and replaced by the border where the
// unclamped index lies outside: ok bounds i0, j0 to [-1, ws - 1] x [-1, hs - 1], so no load leaves hs * pitch.
template <bool STAGED>
__device__ __forceinline__ void warp_px(const unsigned char* __restrict__ src, const icaf_warp_geom& q, const unsigned char* lds, const WarpTile& t,
                                        int y, int x, int nplanes, const int* sc, float* out) {
    const float bord = (float)q.border;
    float u, v, Z;
    warp_uv(q, y, x, u, v, Z);
    const bool ok = Z > 0.0f && u > -1.0f && u < (float)q.ws && v > -1.0f && v < (float)q.hs;
    if (!ok) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = bord;
        return;
    }
    const float fi = floorf(u), fj = floorf(v);
    const float fu = u - fi, fv = v - fj, gu = 1.0f - fu, gv = 1.0f - fv;
    const int i0 = (int)fi, j0 = (int)fj;
    const bool il = i0 >= 0, ih = i0 + 1 < q.ws, jl = j0 >= 0, jh = j0 + 1 < q.hs;
    const int ja = max(j0, 0), jb = min(j0 + 1, q.hs - 1), ia = max(i0, 0), ib = min(i0 + 1, q.ws - 1);
    float val = bord;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c < nplanes) {
            float a00 = bord, a01 = bord, a10 = bord, a11 = bord;
            if (jl && il) a00 = warp_byte<STAGED>(src, q, lds, t, ja, ia, sc[c]);
            if (jl && ih) a01 = warp_byte<STAGED>(src, q, lds, t, ja, ib, sc[c]);
            if (jh && il) a10 = warp_byte<STAGED>(src, q, lds, t, jb, ia, sc[c]);
            if (jh && ih) a11 = warp_byte<STAGED>(src, q, lds, t, jb, ib, sc[c]);
            const float top = a00 * gu + a01 * fu;
            const float bot = a10 * gu + a11 * fu;
            val = top * gv + bot * fv;
            val = floorf(val + 0.5f);
            val = fminf(fmaxf(val, 0.0f), 255.0f);
        }
        out[c] = val;                              // a grey source: the one channel feeds all three planes
    }
}

// The tap of lb_rows_taps: aligned pixel (yy[i], x) — lb_rows with its four byte fetches replaced by warp_px.  STAGED: source bytes come
// from the LDS box of `t` where it holds them.
template <bool STAGED>
struct WarpTap {
    const unsigned char* __restrict__ src;
    const icaf_warp_geom& q;
    const unsigned char* lds;
    const WarpTile& t;
    int swap_rb, yy[2];

    __device__ __forceinline__ WarpTap(const unsigned char* src, const icaf_warp_geom& q, const unsigned char* lds, const WarpTile& t, int swap_rb)
        : src(src), q(q), lds(lds), t(t), swap_rb(swap_rb) {}
    __device__ __forceinline__ void rows(const int* y) { yy[0] = y[0]; yy[1] = y[1]; }
    __device__ __forceinline__ void operator()(int i, int x, float* out) const {
        const bool rgb = q.g.ch == 3;
        const int nplanes = rgb ? 3 : 1;
        const int sc[3] = {rgb && swap_rb ? 2 : 0, rgb ? 1 : 0, rgb && !swap_rb ? 2 : 0};
        warp_px<STAGED>(src, q, lds, t, yy[i], x, nplanes, sc, out);
    }
};

// One workgroup: the 32 x 64 output tile of a kind-1 row.  The stage rule (include/icaf.h; ops.warp_letterbox_staged states the same on the
// host): the four corners of the aligned rectangle the tile taps are warped; if all have Z > 0 and finite coordinates, their bounding box,
// widened by one pixel on the low and two on the high side and cut to the frame, is not empty and fits WARP_LDS, it is copied into LDS
// with aligned 16-byte row copies (lb_stage).  Z is affine in (x, y), so it is positive on the whole rectangle and the rectangle's image is
// the convex hull of the corners' images; the widening covers the floor / + 1 of the taps and the rounding of the fp32 coordinates, and a
// tap that still falls outside the box reads the frame (warp_byte).  The choice is workgroup-uniform: every thread reaches the barrier.
__device__ __forceinline__ void warp_tile(const unsigned char* __restrict__ src, const icaf_warp_geom& q, unsigned char* lds, unsigned char* __restrict__ d,
                                          long long plane_stride, int H, int W, int swap_rb, int force_direct) {
    const icaf_frame_geom& g = q.g;
    WarpTile t{0, 0, 0, 0, 0};
    LbTile al{0, 0, 0, 0};                                         // the aligned rectangle the tile taps
    bool staged = false;
    int nvec = 0;
    if (!force_direct && lb_extent(g, H, W, al)) {
        const int ylo = al.y_lo, yhi = al.y_lo + al.nrows - 1, xlo = al.x_lo, xhi = al.x_lo + al.ncols - 1;
        float umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY;
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float u, v, Z;
            warp_uv(q, (k & 2) ? yhi : ylo, (k & 1) ? xhi : xlo, u, v, Z);
            ok = ok && Z > 0.0f && fabsf(u) < INFINITY && fabsf(v) < INFINITY;      // false on NaN
            umin = fminf(umin, u); umax = fmaxf(umax, u);
            vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
        }
        if (ok) {
            const float ilo = fmaxf(floorf(umin) - 1.0f, 0.0f), ihi = fminf(floorf(umax) + 2.0f, (float)(q.ws - 1));
            const float jlo = fmaxf(floorf(vmin) - 1.0f, 0.0f), jhi = fminf(floorf(vmax) + 2.0f, (float)(q.hs - 1));
            if (ilo <= ihi && jlo <= jhi) {                                        // inside [0, ws - 1] x [0, hs - 1]: exact as ints
                t.i_lo = (int)ilo; t.ncols = (int)ihi - t.i_lo + 1;
                t.j_lo = (int)jlo; t.nrows = (int)jhi - t.j_lo + 1;
                nvec = (t.ncols * g.ch + 30) >> 4;
                staged = (long long)t.nrows * nvec * 16 <= WARP_LDS;
            }
        }
    }
    if (staged) {
        t.lstride = nvec * 16;
        // g.offset is 16-byte aligned, so rounding a row's first byte down to a vector boundary never leaves the frame; the frame's last,
        // partial vector goes byte by byte, nothing past hs * pitch
        lb_stage(src, 0, (long long)q.hs * g.pitch, (long long)t.j_lo * g.pitch + (long long)t.i_lo * g.ch, g.pitch, t.nrows, nvec, lds);
        __syncthreads();
        WarpTap<true> tap(src, q, lds, t, swap_rb);
        lb_rows_taps(g, tap, d, plane_stride, H, W);
    } else {
        WarpTap<false> tap(src, q, lds, t, swap_rb);
        lb_rows_taps(g, tap, d, plane_stride, H, W);
    }
}

__global__ __launch_bounds__(LB_TX * LB_TH) void letterbox_warp_frames_kernel(const unsigned char* __restrict__ arena,
                                                                             const icaf_warp_geom* __restrict__ geom, int B, int ctot, int H, int W,
                                                                             unsigned char* __restrict__ dst, int swap_rb, int force_direct) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[WARP_LDS_ALLOC];
    icaf_warp_geom q;
    unsigned char* d;
    if (lb_table_row(arena, geom, B, ctot, H, W, dst, lds, swap_rb, force_direct, q, d))
        warp_tile(arena + q.g.offset, q, lds, d, (long long)H * W, H, W, swap_rb, force_direct);
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_letterbox_warp_frames(const void* arena, const icaf_warp_geom* geom, int nstreams, int B, void* dst, int ctot, int H, int W,
                                          int swap_rb, icaf_stream_t s) {
    static_assert(sizeof(icaf_warp_geom) == 104, "icaf_warp_geom is 104 bytes (include/icaf.h)");
    return frames_launch("icaf_letterbox_warp_frames", letterbox_warp_frames_kernel, arena, geom, nullptr, dst, nstreams, B, ctot, H, W, swap_rb, s);
}
