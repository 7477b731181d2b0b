// 16-bit thermal frames (Y16: little-endian uint16 counts): automatic gain control inside the device letterbox, byte for byte equal to
// letterbox(agc_u16_to_u8(frame, *agc_window(frame, clip))) of utils/datasets.py.  Two entry points: icaf_y16_window selects the window
// [lo, hi] of every frame from its histogram (or copies the caller's), icaf_letterbox_y16_frames maps each of the four bilinear taps of an
// output pixel to a byte with the integer rule of include/icaf.h and then runs the fp32 tap arithmetic of frames_core.h on those bytes.
// Built with fp contraction off like frames.hip.  A kind-0 row of the table is icaf_letterbox_frames' descriptor and runs lb_tile itself,
// so that a BGR visible stream beside a Y16 thermal one is still one launch.
#include "frames_core.h"

namespace icaf {

constexpr int Y16_LDS = ICAF_Y16_LDS_BYTES;
constexpr int Y16_LDS_ALLOC = Y16_LDS > LB_LDS ? Y16_LDS : LB_LDS;      // one array serves both kinds of row

// out(v) = min(255, ((max(v, lo) - lo) * 255 + (d >> 1)) / d), d = max(hi - lo, 1).  The division is a multiplication by m = 2^40 / d + 1
// and a shift: exact for every numerator below 2^24 and every d below 2^16 (the proof stands in include/icaf.h); x * m fits 64 bits.
struct Y16Map {
    unsigned int lo, half;
    unsigned long long m;
};

__device__ __forceinline__ Y16Map y16_map_of(int lo, int hi) {
    const unsigned int d = (unsigned int)max(hi - lo, 1);
    return {(unsigned int)lo, d >> 1, (1ull << 40) / d + 1ull};
}

__device__ __forceinline__ unsigned int y16_map(const Y16Map& k, unsigned int v) {
    const unsigned int x = (max(v, k.lo) - k.lo) * 255u + k.half;
    return min((unsigned int)(((unsigned long long)x * k.m) >> 40), 255u);
}

// ---- the window -------------------------------------------------------------------------------------------------------------------------
constexpr int WIN_T = 1024, WIN_WAVES = WIN_T / 64;      // one workgroup per frame: 16 waves, each with its own histograms in LDS

// Count `bin` once for every lane of the wave whose `valid` is set, into the wave's own histogram `h`.  Thermal scenes put almost every
// pixel of a wave into a few bins, and 64 additions to one LDS address run one after the other: up to PEEL times, the lanes that hold the
// first valid lane's bin are counted with ONE addition by that lane and leave; what is left adds lane by lane.  Every lane of the wave
// calls this together.
template <int PEEL>
__device__ __forceinline__ void hist_add(unsigned int* h, int bin, bool valid) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < PEEL; ++r) {
        const unsigned long long act = __ballot(valid);
        if (act == 0ull) return;                                  // wave-uniform
        const int leader = __ffsll((long long)act) - 1;
        const int lb = __shfl(bin, leader);
        const bool same = valid && bin == lb;
        const unsigned long long grp = __ballot(same);
        if (lane == leader) atomicAdd(&h[lb], (unsigned int)__popcll(grp));
        valid = valid && !same;
    }
    if (valid) atomicAdd(&h[bin], 1u);
}

// Eight pixels of one aligned 16-byte vector of frame row `row`: vector `v` counted from the vector that holds the row's first byte.  ok
// bit k: pixel k lies in the row's 2 * w0 bytes (padding and the neighbouring rows' pixels do not).  Only bytes below frame_bytes are read.
__device__ __forceinline__ unsigned int y16_vec(const unsigned char* __restrict__ frame, const icaf_frame_geom& g, long long frame_bytes, int row, int v,
                                                unsigned int* px) {
    const long long r0 = (long long)row * g.pitch, a = ((r0 >> 4) + v) << 4;
    u32x4 q = {0u, 0u, 0u, 0u};
    if (a + 16 <= frame_bytes) {
        q = *(const u32x4*)(frame + a);
    } else {                                                      // the frame's last, partial vector: pixel by pixel
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (a + 2 * k + 2 <= frame_bytes) q[k >> 1] |= (unsigned int)*(const unsigned short*)(frame + a + 2 * k) << (16 * (k & 1));
    }
    unsigned int ok = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        px[k] = (q[k >> 1] >> (16 * (k & 1))) & 0xffffu;
        const long long p = a + 2 * k;
        if (p >= r0 && p < r0 + 2ll * g.w0) ok |= 1u << k;
    }
    return ok;
}

// inclusive scan of s[0][0..255] in place (Hillis-Steele, eight steps: the result is back in s[0]); every thread of the workgroup calls it
__device__ __forceinline__ void scan256(unsigned int (*s)[256], int tid) {
    int cur = 0;
#pragma unroll
    for (int off = 1; off < 256; off <<= 1) {
        if (tid < 256) s[cur ^ 1][tid] = s[cur][tid] + (tid >= off ? s[cur][tid - off] : 0u);
        __syncthreads();
        cur ^= 1;
    }
}

// One level of the radix select on the scanned 256 bins of s[0] (their total is s[0][255]): the ONE bin t whose inclusive count first
// makes `10000 * (below + count) > clip * n` true is the lo digit (below_out: pixels under it), the ONE bin t that is the last whose
// count from above `above + total - exclusive count` makes it true for clip_hi is the hi digit.  which: bit 0 select lo, bit 1 select hi.
__device__ __forceinline__ void select256(const unsigned int (*s)[256], int tid, long long n, int which, long long clip_lo, long long below,
                                          long long clip_hi, long long above, int* sel) {
    if (tid >= 256) return;
    const long long cum = s[0][tid], prev = tid ? s[0][tid - 1] : 0, tot = s[0][255];
    if ((which & 1) && 10000ll * (below + cum) > clip_lo * n && !(10000ll * (below + prev) > clip_lo * n)) {
        sel[0] = tid;
        sel[1] = (int)(below + prev);
    }
    if ((which & 2) && 10000ll * (above + tot - prev) > clip_hi * n && !(10000ll * (above + tot - cum) > clip_hi * n)) {
        sel[2] = tid;
        sel[3] = (int)(above + tot - cum);
    }
}

__global__ __launch_bounds__(WIN_T) void y16_window_kernel(const unsigned char* __restrict__ arena, const icaf_y16_geom* __restrict__ geom,
                                                           int* __restrict__ window) {
    __shared__ unsigned int hist[WIN_WAVES * 512];              // pass 1: 256 bins a wave; pass 2: 256 for the lo digit, 256 for the hi digit
    __shared__ unsigned int s[2][256];
    __shared__ int sel[4];                                      // lo digit, pixels below it, hi digit, pixels above it
    const int img = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const icaf_y16_geom q = geom[img];
    if (q.kind != 1) return;                                    // workgroup-uniform, as every branch around a barrier below
    if (q.mode == 0) {
        if (tid == 0) {
            window[2 * img] = q.lo;
            window[2 * img + 1] = q.hi;
        }
        return;
    }
    const icaf_frame_geom& g = q.g;
    const unsigned char* frame = arena + g.offset;
    const long long frame_bytes = (long long)g.h0 * g.pitch, n = (long long)g.h0 * g.w0;
    const int nvec = (2 * g.w0 + 29) >> 4;                      // a row of 2 * w0 bytes from an even phase of up to 14 touches at most this many vectors
    const int total = g.h0 * nvec;
    unsigned int px[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};

    // pass 1: the high bytes
    for (int i = tid; i < WIN_WAVES * 256; i += WIN_T) hist[i] = 0u;
    __syncthreads();
    for (int base = 0; base < total; base += WIN_T) {
        const int idx = base + tid;
        unsigned int ok = 0;
        if (idx < total) ok = y16_vec(frame, g, frame_bytes, idx / nvec, idx % nvec, px);
#pragma unroll
        for (int k = 0; k < 8; ++k) hist_add<2>(hist + wave * 256, (int)(px[k] >> 8), (ok >> k) & 1u);
    }
    __syncthreads();
    if (tid < 256) {
        unsigned int c = 0;
#pragma unroll
        for (int w = 0; w < WIN_WAVES; ++w) c += hist[w * 256 + tid];
        s[0][tid] = c;
    }
    __syncthreads();
    scan256(s, tid);
    select256(s, tid, n, 3, q.clip_lo, 0, q.clip_hi, 0, sel);
    __syncthreads();
    const int blo = sel[0], bhi = sel[2];
    const long long below = sel[1], above = sel[3];
    const bool one = blo == bhi;                                // a narrow scene: both ranks in one high byte, one histogram serves both
    __syncthreads();

    // pass 2: the low bytes inside the two high bytes
    for (int i = tid; i < WIN_WAVES * 512; i += WIN_T) hist[i] = 0u;
    __syncthreads();
    for (int base = 0; base < total; base += WIN_T) {
        const int idx = base + tid;
        unsigned int ok = 0;
        if (idx < total) ok = y16_vec(frame, g, frame_bytes, idx / nvec, idx % nvec, px);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool in = (ok >> k) & 1u;
            const int hb = (int)(px[k] >> 8), lb = (int)(px[k] & 255u);
            hist_add<1>(hist + wave * 512, lb, in && hb == blo);
            if (!one) hist_add<1>(hist + wave * 512 + 256, lb, in && hb == bhi);
        }
    }
    __syncthreads();
    for (int level = 0; level < 2; ++level) {                   // 0: the lo digit from the first histogram, 1: the hi digit from the second
        if (tid < 256) {
            unsigned int c = 0;
            const int at = level && !one ? 256 : 0;
#pragma unroll
            for (int w = 0; w < WIN_WAVES; ++w) c += hist[w * 512 + at + tid];
            s[0][tid] = c;
        }
        __syncthreads();
        scan256(s, tid);
        select256(s, tid, n, level ? 2 : 1, q.clip_lo, below, q.clip_hi, above, sel);
        __syncthreads();
        if (tid == 0) window[2 * img + level] = (level ? bhi : blo) * 256 + sel[level ? 2 : 0];
        __syncthreads();
    }
}

// ---- the letterbox ----------------------------------------------------------------------------------------------------------------------
// lb_rows<false> for a Y16 frame: one thread, 16 output columns of one output row; every tap is one clamped 2-byte load plus the mapping.
__device__ __forceinline__ void y16_rows_direct(const unsigned char* __restrict__ frame, const icaf_frame_geom& g, const Y16Map& k,
                                                unsigned char* __restrict__ dst, long long plane_stride, int H, int W) {
    const int x = blockIdx.x * LB_TW + threadIdx.x * LB_PX, r = blockIdx.y * LB_TH + threadIdx.y;
    if (x >= W || r >= H) return;
    unsigned char* o = dst + (long long)r * W + x;
    const u32x4 padv = {0x72727272u, 0x72727272u, 0x72727272u, 0x72727272u};
    const int jr = r - g.top;
    u32x4 out = padv;
    if (!(jr < 0 || jr >= g.nh || x + LB_PX <= g.left || x >= g.left + g.nw)) {
        int y0, y1;
        float fy;
        lb_tap(jr, g.sy, g.h0, y0, y1, fy);
        const float gy = 1.0f - fy;
        const unsigned short* row0 = (const unsigned short*)(frame + (long long)y0 * g.pitch);
        const unsigned short* row1 = (const unsigned short*)(frame + (long long)y1 * g.pitch);
#pragma unroll
        for (int j = 0; j < LB_PX; ++j) {
            const int jx = x + j - g.left;
            if (jx < 0 || jx >= g.nw) continue;
            int x0, x1;
            float fx;
            lb_tap(jx, g.sx, g.w0, x0, x1, fx);
            const float gx = 1.0f - fx;
            const float a00 = (float)y16_map(k, row0[x0]), a01 = (float)y16_map(k, row0[x1]);
            const float a10 = (float)y16_map(k, row1[x0]), a11 = (float)y16_map(k, row1[x1]);
            const float top = a00 * gx + a01 * fx;
            const float bot = a10 * gx + a11 * fx;
            float v = top * gy + bot * fy;
            v = floorf(v + 0.5f);
            v = fminf(fmaxf(v, 0.0f), 255.0f);
            const int sh = 8 * (j & 3);
            out[j >> 2] = (out[j >> 2] & ~(0xffu << sh)) | ((unsigned int)v << sh);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) *(u32x4*)(o + c * plane_stride) = out;
}

// One workgroup: the 32 x 64 output tile of a kind-1 row.  The MAPPED frame is a grey frame of h0 rows of pitch / 2 bytes (`m8`): a staged
// tile holds exactly the bytes lb_tile would stage of it, vector for vector, so lb_rows<true> and lb_budget run on it unchanged.  A staged
// vector is 16 mapped pixels from a pixel index that is a multiple of 16, that is 32 source bytes from a 32-byte multiple of the (16-byte
// aligned) frame: two aligned 16-byte loads.  The choice between the paths is workgroup-uniform.
__device__ __forceinline__ void y16_tile(const unsigned char* __restrict__ frame, const icaf_frame_geom& g, const Y16Map& k, unsigned char* lds,
                                         unsigned char* __restrict__ d, long long plane_stride, int H, int W, int force_direct) {
    icaf_frame_geom m8 = g;
    m8.pitch = g.pitch >> 1;
    LbTile t{0, 0, 0, 0};
    bool staged = false;
    int rows_cap, cols_cap, nvec;
    if (!force_direct && lb_budget(m8, rows_cap, cols_cap, nvec) && lb_extent(g, H, W, t))      // LB_LDS == Y16_LDS (asserted below)
        staged = t.nrows <= rows_cap && t.ncols <= cols_cap;
    if (staged) {
        const int tid = threadIdx.y * LB_TX + threadIdx.x, lstride = nvec * 16;
        const long long frame_bytes = (long long)g.h0 * g.pitch;
        for (int idx = tid; idx < t.nrows * nvec; idx += LB_TX * LB_TH) {
            const int row = idx / nvec, v = idx - row * nvec;
            const long long a = (((((long long)(t.y_lo + row) * m8.pitch + t.x_lo) >> 4) + v) << 4) * 2;      // first source byte of 16 pixels
            u32x4 out = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const long long b = a + 16 * h;
                u32x4 w = {0u, 0u, 0u, 0u};
                if (b + 16 <= frame_bytes) {
                    w = *(const u32x4*)(frame + b);
                } else {
#pragma unroll
                    for (int p = 0; p < 8; ++p)
                        if (b + 2 * p + 2 <= frame_bytes) w[p >> 1] |= (unsigned int)*(const unsigned short*)(frame + b + 2 * p) << (16 * (p & 1));
                }
#pragma unroll
                for (int p = 0; p < 8; ++p) {
                    const unsigned int byte = y16_map(k, (w[p >> 1] >> (16 * (p & 1))) & 0xffffu);
                    out[2 * h + (p >> 2)] |= byte << (8 * (p & 3));
                }
            }
            *(u32x4*)(lds + (long long)row * lstride + v * 16) = out;
        }
        __syncthreads();
        lb_rows<true>(frame, m8, lds, lstride, t, d, plane_stride, H, W, 0);
    } else {
        y16_rows_direct(frame, g, k, d, plane_stride, H, W);
    }
}

static_assert(Y16_LDS == LB_LDS, "y16_tile states its budget through lb_budget: the two limits are one number");

__global__ __launch_bounds__(LB_TX * LB_TH) void letterbox_y16_frames_kernel(const unsigned char* __restrict__ arena,
                                                                            const icaf_y16_geom* __restrict__ geom, int B, int ctot, int H, int W,
                                                                            unsigned char* __restrict__ dst, int swap_rb, int force_direct,
                                                                            const int* __restrict__ window) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[Y16_LDS_ALLOC];
    icaf_y16_geom q;
    unsigned char* d;
    if (lb_table_row(arena, geom, B, ctot, H, W, dst, lds, swap_rb, force_direct, q, d)) {
        const int img = blockIdx.z;
        const Y16Map k = y16_map_of(window[2 * img], window[2 * img + 1]);
        y16_tile(arena + q.g.offset, q.g, k, lds, d, (long long)H * W, H, W, force_direct);
    }
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_y16_window(const void* arena, const icaf_y16_geom* geom, int nstreams, int B, int* window, icaf_stream_t s) {
    if (!arena || !geom || !window) return fail(ICAF_ERR_ARG, "icaf_y16_window: null pointer");
    if (((uintptr_t)arena & 15) || ((uintptr_t)geom & 7) || ((uintptr_t)window & 3))
        return fail(ICAF_ERR_ARG, "icaf_y16_window: the arena must be 16-byte aligned, the geometry table 8-byte, the window table 4-byte aligned");
    if (nstreams < 1 || B < 1) return fail(ICAF_ERR_ARG, "icaf_y16_window: bad geometry");
    if ((long long)nstreams * B > 65535) return fail(ICAF_ERR_UNSUPPORTED, "icaf_y16_window: %lld frames are too many for one launch", (long long)nstreams * B);
    hipLaunchKernelGGL(y16_window_kernel, dim3((unsigned)(nstreams * B)), dim3(WIN_T), 0, S(s), (const unsigned char*)arena, geom, window);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

extern "C" int icaf_letterbox_y16_frames(const void* arena, const icaf_y16_geom* geom, const int* window, int nstreams, int B, void* dst, int ctot,
                                         int H, int W, int swap_rb, icaf_stream_t s) {
    if (!window) return fail(ICAF_ERR_ARG, "icaf_letterbox_y16_frames: null window table");
    return frames_launch("icaf_letterbox_y16_frames", letterbox_y16_frames_kernel, arena, geom, window, dst, nstreams, B, ctot, H, W, swap_rb, s, window);
}
