// Device resize of native VALIDATION frames (utils/datasets.py:1116-1122, load_image_rgb_ir: longest side to img_size — INTER_AREA when
// shrinking, INTER_LINEAR when growing — then letterbox's padding), byte for byte: one launch serves a batch that mixes frames that
// shrink (mode 1: the pixel-area average of utils.datasets.resize_area_scalar), frames that grow and frames that are copied (mode 0:
// lb_tile of frames_core.h, the tile icaf_letterbox_frames runs).  Built with fp contraction off (build.py): every product and
// sum rounds on its own, in the order resize_area_scalar fixes (vertical taps first, ascending, fp32 accumulator from 0).
#include "frames_core.h"

namespace icaf {

constexpr int RS_LDS = ICAF_RESIZE_LDS_BYTES;      // the fp32 v rows of a mode-1 sub-tile, or the source rectangle of a mode-0 tile
constexpr int RS_NT = ICAF_RESIZE_MAX_TAPS;        // taps per output row / column whose weights are tabulated in LDS
constexpr int RS_THREADS = LB_TX * LB_TH;          // 128: the letterbox's block (lb_tile and lb_rows index by it), two waves
static_assert(RS_LDS >= LB_LDS && RS_LDS % 16 == 0, "mode-0 tiles stage their source rectangle in the same bytes");

// resize_area.weights in fp64, one element: output index j covers [j s, j s + s); the weight of source pixel px is its overlap with
// [px, px + 1) over s, rounded to fp32.  s = n_in / (double)n_out; the first pixel the interval can touch is floor(j s).
__device__ __forceinline__ float area_weight(int j, double s, int px) {
    const double lo = (double)j * s, hi = lo + s;
    const double ov = fmax(fmin(hi, (double)px + 1.0) - fmax(lo, (double)px), 0.0);
    return (float)(ov / s);
}
__device__ __forceinline__ int area_first(int j, double s) { return (int)((double)j * s); }

// value of lane (lane & ~3) + k of every quad, in all four lanes of the quad (DPP quad_perm; the whole wave is active where this is used)
template <int K>
__device__ __forceinline__ unsigned int quad_lane(unsigned int v) {
    return (unsigned int)__builtin_amdgcn_update_dpp(0, (int)v, K * 0x55, 0xf, 0xf, false);
}

struct AreaTile {
    int ra, nty, ntx;              // first resized row of the tile (the tables' row 0); taps per output along y / x: (int)s + 2
    double sy, sx;
    const float *wy, *wx;          // [tap][row] / [tap][column] weights (TAB), 0 where the tap leaves the frame or the output
    const int *py0, *px0;          // first source row / column of each output row / column of the tile (TAB)
};

// Horizontal pass, rounding and store of resized rows [o0, o0 + nr): one wave per row, one lane per output column of the 64-column tile,
// four neighbouring lanes packed into one 32-bit store per plane; columns outside the block get 114.  STAGED: the vertical sums come
// from the fp32 rows in LDS (row ol at v + ol * stride, source byte column xs * ch + c at offset voff + that); otherwise each horizontal
// tap recomputes its vertical sum from the frame — the same operations in the same order.  TAB: weights from the LDS tables, otherwise
// computed on the spot (more than RS_NT taps).
template <bool STAGED, bool TAB>
__device__ __forceinline__ void area_rows(const unsigned char* __restrict__ frame, const icaf_frame_geom& g, const AreaTile& a, const float* v,
                                          int stride, int voff, int x_hi, int o0, int nr, unsigned char* __restrict__ d, long long plane_stride,
                                          int W, int swap_rb) {
    const int tid = threadIdx.y * LB_TX + threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x = blockIdx.x * LB_TW + lane, jx = x - g.left;
    const bool in = jx >= 0 && jx < g.nw && x < W;
    const bool rgb = g.ch == 3;
    int xp0 = 0;
    if (in) xp0 = TAB ? a.px0[lane] : area_first(jx, a.sx);
    for (int ol = wave; ol < nr; ol += RS_THREADS / 64) {               // wave-uniform
        const int jr = o0 + ol, o = jr - a.ra;
        unsigned int val[3] = {LB_PAD, LB_PAD, LB_PAD};
        if (in) {
            const int yp0 = TAB ? a.py0[o] : area_first(jr, a.sy);
            float acc[3] = {0.0f, 0.0f, 0.0f};
            // staged: taps two at a time so that their LDS reads are in flight together; the first tap of a column always weighs, the
            // weighing taps are contiguous, and a tap past them (the table's weight 0, column clamped into the span) adds + 0
            for (int t = 0; STAGED && t < a.ntx; t += 2) {
                const float w0 = a.wx[t * LB_TW + lane];
                if (w0 == 0.0f) break;
                const float w1 = t + 1 < RS_NT ? a.wx[(t + 1) * LB_TW + lane] : 0.0f;
                const float* p0 = v + ol * stride + voff + (xp0 + t) * g.ch;
                const float* p1 = v + ol * stride + voff + min(xp0 + t + 1, x_hi) * g.ch;
                float v0[3] = {0.0f, 0.0f, 0.0f}, v1[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    if (c == 0 || rgb) { v0[c] = p0[c]; v1[c] = p1[c]; }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    acc[c] = acc[c] + w0 * v0[c];
                    acc[c] = acc[c] + w1 * v1[c];
                }
            }
            for (int t = 0; !STAGED && t < a.ntx; ++t) {                // per channel: its taps in ascending x, whatever the loop nesting
                const int xs = xp0 + t;
                float w;
                if (TAB) w = a.wx[t * LB_TW + lane];
                else w = xs < g.w0 ? area_weight(jx, a.sx, xs) : 0.0f;
                if (w == 0.0f) continue;                                // + 0 changes nothing: every term is non-negative
                float vs[3] = {0.0f, 0.0f, 0.0f};
                {
                    for (int u = 0; u < a.nty; ++u) {
                        const int h = yp0 + u;
                        float wv;
                        if (TAB) wv = a.wy[u * LB_TH + o];
                        else wv = h < g.h0 ? area_weight(jr, a.sy, h) : 0.0f;
                        if (wv == 0.0f) continue;
                        const unsigned char* p = frame + (long long)h * g.pitch + xs * g.ch;
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            if (c == 0 || rgb) vs[c] = vs[c] + wv * (float)p[c];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] = acc[c] + w * vs[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {                               // plane c takes source channel 2 - c of a BGR frame; a grey frame feeds all three
                float r = floorf(acc[rgb ? (swap_rb ? 2 - c : c) : 0] + 0.5f);
                r = fminf(fmaxf(r, 0.0f), 255.0f);
                val[c] = (unsigned int)r;
            }
        }
        unsigned char* orow = d + (long long)(g.top + jr) * W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned int q = val[c] | (quad_lane<1>(val[c]) << 8) | (quad_lane<2>(val[c]) << 16) | (quad_lane<3>(val[c]) << 24);
            if ((lane & 3) == 0 && x < W) *(unsigned int*)(orow + c * plane_stride) = q;      // W % 16 == 0: a quad is inside or outside
        }
    }
}

// One workgroup: the 32 x 64 output tile of a mode-1 descriptor.  Every byte of the tile's three planes is written exactly once: first
// the rows (or the whole tile) that hold no resized pixel, then the resized rows in sub-tiles of `rows` rows.
__device__ __forceinline__ void area_tile(const unsigned char* __restrict__ frame, const icaf_frame_geom& g, unsigned char* lds, float* wy, float* wx,
                                          int* py0, int* px0, unsigned char* __restrict__ d, long long plane_stride, int H, int W, int swap_rb,
                                          int force_direct) {
    const int tid = threadIdx.y * LB_TX + threadIdx.x;
    const int r0 = blockIdx.y * LB_TH, x0 = blockIdx.x * LB_TW;
    // resized pixels of this tile: output rows [ra, rb], columns [ca, cb] in resized coordinates (empty: padding only)
    const int ra = max(r0, g.top) - g.top, rb = min(min(r0 + LB_TH, H), g.top + g.nh) - 1 - g.top;
    const int ca = max(x0, g.left) - g.left, cb = min(min(x0 + LB_TW, W), g.left + g.nw) - 1 - g.left;
    const bool has = ra <= rb && ca <= cb;
    for (int idx = tid; idx < LB_TH * (LB_TW / 4); idx += RS_THREADS) {
        const int r = r0 + idx / (LB_TW / 4), x = x0 + (idx % (LB_TW / 4)) * 4;
        if (r >= H || x >= W) continue;
        const int jr = r - g.top;
        if (has && jr >= 0 && jr < g.nh) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) *(unsigned int*)(d + c * plane_stride + (long long)r * W + x) = 0x72727272u;
    }
    if (!has) return;                                                   // workgroup-uniform, like everything up to the barriers below
    AreaTile a;
    a.ra = ra;
    a.sy = (double)g.h0 / (double)g.nh;
    a.sx = (double)g.w0 / (double)g.nw;
    a.nty = (int)a.sy + 2;
    a.ntx = (int)a.sx + 2;
    a.wy = wy; a.wx = wx; a.py0 = py0; a.px0 = px0;
    const bool tab = a.nty <= RS_NT && a.ntx <= RS_NT;
    if (!tab) {                                                         // a shrink of 7 x and more: no tables, no staging
        area_rows<false, false>(frame, g, a, nullptr, 0, 0, 0, ra, rb - ra + 1, d, plane_stride, W, swap_rb);
        return;
    }
    for (int idx = tid; idx < RS_NT * LB_TH; idx += RS_THREADS) {
        const int t = idx / LB_TH, o = idx - t * LB_TH, j = ra + o;
        float w = 0.0f;
        if (j <= rb && t < a.nty) {
            const int p = area_first(j, a.sy) + t;
            if (p < g.h0) w = area_weight(j, a.sy, p);
            if (t == 0) py0[o] = p;
        }
        wy[idx] = w;
    }
    for (int idx = tid; idx < RS_NT * LB_TW; idx += RS_THREADS) {
        const int t = idx / LB_TW, xc = idx - t * LB_TW, j = x0 + xc - g.left;
        float w = 0.0f;
        if (j >= ca && j <= cb && t < a.ntx) {
            const int p = area_first(j, a.sx) + t;
            if (p < g.w0) w = area_weight(j, a.sx, p);
            if (t == 0) px0[xc] = p;
        }
        wx[idx] = w;
    }
    __syncthreads();
    // budget rule (ops.area_staged states the same on the host): a tile's 64 columns touch at most (int)(64 sx) + 2 source pixels; a v row
    // holds that many pixels of ch floats, rounded up to whole 16-byte vectors, plus one vector for the alignment phase of the first byte
    const int cols_cap = min(g.w0, (int)(64.0 * a.sx) + 2);
    const int stride = ((cols_cap * g.ch + 3) & ~3) + 4;               // floats
    const int rows = min(LB_TH, RS_LDS / (stride * 4));
    const int x_lo = px0[ca + g.left - x0], x_hi = min(g.w0 - 1, (int)((double)cb * a.sx + a.sx));
    const bool staged = !force_direct && rows >= 2 && x_hi - x_lo + 1 <= cols_cap;     // the last holds by construction of the cap
    if (!staged) {
        area_rows<false, true>(frame, g, a, nullptr, 0, 0, 0, ra, rb - ra + 1, d, plane_stride, W, swap_rb);
        return;
    }
    // Phase A: a thread owns four consecutive source byte columns of one output row and runs that row's vertical taps down the frame.
    // Rows whose pitch is a multiple of 4 keep one phase, so the span starts on a 4-byte boundary and every tap is one aligned 32-bit
    // load that stays inside the row's pitch; any other pitch is read byte by byte inside the row's w0 * ch bytes.
    const bool aligned = (g.pitch & 3) == 0;
    const int c_start = aligned ? (x_lo * g.ch) & ~3 : x_lo * g.ch, c_end = (x_hi + 1) * g.ch, row_bytes = g.w0 * g.ch;
    const int ng = (c_end - c_start + 3) >> 2;                          // 4 ng <= stride
    const int step_o = RS_THREADS / ng, step_k = RS_THREADS - step_o * ng;      // the next item of a thread, without a division per item
    float* v = (float*)lds;
    for (int o0 = ra; o0 <= rb; o0 += rows) {
        const int nr = min(rows, rb - o0 + 1);
        int ol = tid / ng, k = tid - ol * ng;
        for (int idx = tid; idx < nr * ng; idx += 2 * RS_THREADS) {
            // two items of the thread at a time, taps two at a time: four loads in flight.  The first tap of a row always weighs, the
            // weighing taps are contiguous, and a tap past them (the table's weight 0, row clamped into the frame) adds + 0.  A missing
            // second item repeats the first and is not written.
            int iol[2], ik[2], io[2];
            const bool second = idx + RS_THREADS < nr * ng;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                iol[m] = ol; ik[m] = k;
                if (m == 0 && !second) continue;
                k += step_k;
                ol += step_o;
                if (k >= ng) { k -= ng; ++ol; }
            }
            f32x4 acc[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                io[m] = o0 + iol[m] - ra;
                acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
            const int p0[2] = {py0[io[0]], py0[io[1]]};
            for (int t = 0; t < a.nty; t += 2) {
                float w[2][2];
                unsigned int q[2][2] = {{0u, 0u}, {0u, 0u}};
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    w[m][0] = wy[t * LB_TH + io[m]];
                    w[m][1] = t + 1 < RS_NT ? wy[(t + 1) * LB_TH + io[m]] : 0.0f;
                }
                if (w[0][0] == 0.0f && w[1][0] == 0.0f) break;
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int cb4 = c_start + 4 * ik[m];
                        const unsigned char* p = frame + (long long)min(p0[m] + t + e, g.h0 - 1) * g.pitch + cb4;
                        if (aligned) {
                            q[m][e] = *(const unsigned int*)p;
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (cb4 + i < row_bytes) q[m][e] |= (unsigned int)p[i] << (8 * i);
                        }
                    }
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int e = 0; e < 2; ++e)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[m][i] = acc[m][i] + w[m][e] * (float)((q[m][e] >> (8 * i)) & 255u);
            }
            *(f32x4*)(v + iol[0] * stride + 4 * ik[0]) = acc[0];
            if (second) *(f32x4*)(v + iol[1] * stride + 4 * ik[1]) = acc[1];
        }
        __syncthreads();
        // Phase B: horizontal taps from LDS
        area_rows<true, true>(frame, g, a, v, stride, -c_start, x_hi, o0, nr, d, plane_stride, W, swap_rb);
        __syncthreads();
    }
}

__global__ __launch_bounds__(RS_THREADS) void resize_frames_kernel(const unsigned char* __restrict__ arena, const icaf_frame_geom* __restrict__ geom,
                                                                   const int* __restrict__ mode, int B, int ctot, int H, int W,
                                                                   unsigned char* __restrict__ dst, int swap_rb, int lb_direct, int area_direct) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[RS_LDS];
    __shared__ float wy[RS_NT * LB_TH], wx[RS_NT * LB_TW];
    __shared__ int py0[LB_TH], px0[LB_TW];
    const int img = blockIdx.z, m = img / B, b = img - m * B;      // img = modality * B + b
    const icaf_frame_geom g = geom[img];
    const unsigned char* frame = arena + g.offset;
    const long long plane_stride = (long long)H * W;
    unsigned char* d = dst + ((long long)b * ctot + 3 * m) * plane_stride;
    if (mode && mode[img] == 1) {                                  // workgroup-uniform
        area_tile(frame, g, lds, wy, wx, py0, px0, d, plane_stride, H, W, swap_rb, area_direct);
        return;
    }
    lb_tile(frame, g, lds, d, plane_stride, H, W, swap_rb, lb_direct);     // mode 0
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_resize_frames(const void* arena, const icaf_frame_geom* geom, const int* mode, int nstreams, int B, void* dst, int ctot, int H,
                                  int W, int swap_rb, icaf_stream_t s) {
    dim3 grid;
    if (const int rc = frames_launch_prepare("icaf_resize_frames", arena, geom, mode, dst, nstreams, B, ctot, H, W, grid)) return rc;
    hipLaunchKernelGGL(resize_frames_kernel, grid, dim3(LB_TX, LB_TH), 0, S(s), (const unsigned char*)arena, geom, mode, B, ctot, H, W, (unsigned char*)dst,
                       swap_rb ? 1 : 0, g_opt.letterbox_direct ? 1 : 0, g_opt.area_direct ? 1 : 0);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
