// Device letterbox of native camera frames (utils/datasets.py: letterbox = resize_bilinear to new_unpad + grey padding), byte for byte:
// decoder-layout frames (H0 x W0 x ch interleaved uint8, own row pitch) -> the plan's uint8 [B][ctot][H][W] input planes.  Built with fp
// contraction off (build.py): every product and sum below rounds like resize_bilinear's separate fp32 numpy operations.
#include "frames_core.h"

namespace icaf {

__global__ __launch_bounds__(LB_TX * LB_TH) void letterbox_frames_kernel(const unsigned char* __restrict__ arena,
                                                                        const icaf_frame_geom* __restrict__ geom, int B, int ctot, int H,
                                                                        int W, unsigned char* __restrict__ dst, int swap_rb, int force_direct) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LB_LDS];
    const int img = blockIdx.z, m = img / B, b = img - m * B;      // img = modality * B + b
    const icaf_frame_geom g = geom[img];
    const unsigned char* frame = arena + g.offset;
    const long long plane_stride = (long long)H * W;
    unsigned char* d = dst + ((long long)b * ctot + 3 * m) * plane_stride;
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
    if (staged) {                                                  // workgroup-uniform: every thread reaches the barrier
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

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_letterbox_frames(const void* arena, const icaf_frame_geom* geom, int nstreams, int B, void* dst, int ctot, int H, int W,
                                     int swap_rb, icaf_stream_t s) {
    if (!arena || !geom || !dst) return fail(ICAF_ERR_ARG, "icaf_letterbox_frames: null pointer");
    if (((uintptr_t)arena & 15) || ((uintptr_t)dst & 15) || ((uintptr_t)geom & 7))
        return fail(ICAF_ERR_ARG, "icaf_letterbox_frames: arena and dst must be 16-byte aligned, the geometry table 8-byte aligned");
    if (nstreams < 1 || B < 1 || H < 1 || W < 1 || W % LB_PX) return fail(ICAF_ERR_ARG, "icaf_letterbox_frames: bad geometry (W %% 16 == 0)");
    if (ctot < 3 * nstreams) return fail(ICAF_ERR_ARG, "icaf_letterbox_frames: %d modalities need ctot >= %d, got %d", nstreams, 3 * nstreams, ctot);
    const long long gz = (long long)nstreams * B, gy = (H + LB_TH - 1) / LB_TH;
    if (gz > 65535 || gy > 65535) return fail(ICAF_ERR_UNSUPPORTED, "icaf_letterbox_frames: grid %lld x %lld too large", gy, gz);
    dim3 grid((unsigned)((W + LB_TW - 1) / LB_TW), (unsigned)gy, (unsigned)gz), block(LB_TX, LB_TH);
    hipLaunchKernelGGL(letterbox_frames_kernel, grid, block, 0, S(s), (const unsigned char*)arena, geom, B, ctot, H, W, (unsigned char*)dst,
                       swap_rb ? 1 : 0, g_opt.letterbox_direct ? 1 : 0);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
