// Image-fed first layer of a VGG block (reference models/common.py:109-128, yaml rows 0 and 5 of the yolov5_VGG16_* files):
//   y = ReLU(conv3x3 / s1 / p1 (img) + bias),  3 -> 64 channels, straight from the NCHW images into the NHWC map.
// The generic route stages the image as an 8-channel NHWC tensor (a write and a read of 16 bytes per pixel) and runs an implicit GEMM with
// K = 72, of which 27 columns are not padding.  Here K = 27 is padded to 32 = two MFMA steps, the 64 x 32 weights of a stream sit in eight
// registers per lane for the whole kernel, and a wavefront turns 32 consecutive pixels of an image row into their 64 channels per round:
// 16 taps per lane gathered from the image planes (coalesced along the row; neighbours' re-reads hit the vector cache), four MFMAs, bias +
// ReLU in fp32, one rounding, four 16-byte stores per lane.  No LDS, no barrier, no counted wait.
//
// Register layout.  mma_step (icaf_common.h) returns, in the lane of pixel j = lane & 31 and half hi = lane >> 5, the weight rows
// i = e + 8 q + 4 hi (e < 4, q < 4) of its 32-row block.  Row i of block a is therefore loaded from output channel
//   ch(a, i) = 32 * ((i >> 2) & 1) + 8 * (i >> 3) + 4 a + (i & 3),
// which makes the eight values {a, e} a lane holds for one q the CONTIGUOUS channels 32 hi + 8 q .. + 8 of its pixel: one 16-byte store.
#include "icaf_common.h"

namespace icaf {

constexpr int VGG_C = 64, VGG_K = 27, VGG_KP = 32;

template <int DT, bool U8>
__global__ __launch_bounds__(256) void vgg_stem_kernel(const void* __restrict__ img, int ctot, const unsigned short* __restrict__ w,
                                                       const float* __restrict__ bias, unsigned short* __restrict__ y, int ldy, int nstreams,
                                                       int B, int H, int W, long long w_gs, long long bias_gs, long long y_gs) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
    const int segs_row = (W + 31) >> 5;                                   // 32-pixel segments per image row
    const long long segs_stream = (long long)B * H * segs_row, nseg = segs_stream * nstreams;
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwave = (long long)gridDim.x * 4;
    const long long plane = (long long)H * W;

    // this lane's 16 taps: K index kk = 16 s + 8 hi + e = (ky * 3 + kx) * 3 + c; off = offset from the pixel in plane c, dyx = (dy, dx) packed
    int off[2][8], dyx[2][8];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = 16 * s + 8 * hi + e, tap = kk / 3, c = kk - 3 * tap, ky = tap / 3, kx = tap - 3 * ky;
            const bool real = kk < VGG_K;
            off[s][e] = real ? (int)(c * plane) + (ky - 1) * W + (kx - 1) : 0;
            dyx[s][e] = real ? (ky - 1) * 256 + ((kx - 1) & 0xff) : -(1 << 30);            // padding columns: row y - 2^22, never inside (H <= 2^20)
        }

    int cur_stream = -1;
    u32x4 fw[2][2];
    float bq[4][8];
    for (long long seg = wave0; seg < nseg; seg += nwave) {
        const int st = (int)(seg / segs_stream);
        const long long r = seg - st * segs_stream;
        const int sx = (int)(r % segs_row);
        const long long row = r / segs_row;
        const int yy = (int)(row % H), b = (int)(row / H);
        if (st != cur_stream) {                                           // (wave-uniform: at most once per stream and wave)
            cur_stream = st;
            const unsigned short* wg = w + st * w_gs;
            const float* bg = bias + st * bias_gs;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int ch = 32 * ((l31 >> 2) & 1) + 8 * (l31 >> 3) + 4 * a + (l31 & 3);
#pragma unroll
                for (int s = 0; s < 2; ++s) fw[a][s] = *(const u32x4*)(wg + ch * VGG_KP + 16 * s + 8 * hi);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 8; ++j) bq[q][j] = bg[32 * hi + 8 * q + j];
        }
        const int xx = sx * 32 + l31;
        const bool okx = xx < W;
        // fp32: [nstreams][B][3][H][W]; uint8: [B][ctot][H][W], stream st = channels [3 st, 3 st + 3)
        const long long base = (U8 ? ((long long)b * ctot + 3 * st) : ((long long)st * B + b) * 3) * plane + (long long)yy * W + xx;
        u32x4 fp[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int dy = dyx[s][e] >> 8, dx = (int)(signed char)(dyx[s][e] & 0xff);
                const bool ok = okx && (unsigned)(yy + dy) < (unsigned)H && (unsigned)(xx + dx) < (unsigned)W;
                float v = 0.0f;
                if (ok) {
                    if constexpr (U8) v = (float)((const unsigned char*)img)[base + off[s][e]] / 255.0f;      // true division, as icaf_preprocess_u8
                    else v = ((const float*)img)[base + off[s][e]];
                }
                f[e] = v;
            }
            fp[s] = pack16<DT>(f);                                        // the image rounded to the storage type, as the staged copy would be
        }
        f32x16 acc[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][i] = 0.0f;
#pragma unroll
            for (int s = 0; s < 2; ++s) mma_step<DT>(acc[a], fw[a][s], fp[s]);
        }
        if (okx) {
            unsigned short* yp = y + st * y_gs + (row * W + xx) * ldy + 32 * hi;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v[8];
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[4 * a + e] = fmaxf(acc[a][4 * q + e] + bq[q][4 * a + e], 0.0f);
                *(u32x4*)(yp + 8 * q) = pack16<DT>(v);
            }
        }
    }
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_vgg_stem(const void* img, int img_u8, int ctot, const void* w, const float* bias, void* y, int ldy, int dtype, int nstreams,
                             int B, int H, int W, int Cout, int Kp, long long w_gs, long long bias_gs, long long y_gs, icaf_stream_t s) {
    if (!img || !w || !bias || !y) return fail(ICAF_ERR_ARG, "icaf_vgg_stem: null pointer");
    if (dtype != ICAF_BF16 && dtype != ICAF_F16) return fail(ICAF_ERR_UNSUPPORTED, "icaf_vgg_stem: 16-bit types only (fp32 runs the generic route)");
    if (Cout != VGG_C || Kp != VGG_KP) return fail(ICAF_ERR_UNSUPPORTED, "icaf_vgg_stem: built for Cout = %d with K = 27 padded to %d (got %d, %d)", VGG_C, VGG_KP, Cout, Kp);
    if (nstreams < 1 || nstreams > 2 || B < 1 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) return fail(ICAF_ERR_ARG, "icaf_vgg_stem: bad geometry");
    if (img_u8 ? ctot < 3 * nstreams : ctot != 3) return fail(ICAF_ERR_ARG, "icaf_vgg_stem: ctot = %d does not hold %d streams of 3 channels", ctot, nstreams);
    if (ldy < VGG_C || ldy % 8 || ((uintptr_t)y & 15) || (y_gs * 2) % 16) return fail(ICAF_ERR_ARG, "icaf_vgg_stem: y must take 16-byte vectors (ldy %% 8, alignment) with ldy >= 64");
    if (((uintptr_t)w & 15) || (w_gs * 2) % 16 || ((uintptr_t)bias & 3)) return fail(ICAF_ERR_ARG, "icaf_vgg_stem: w must be 16-byte aligned");
    if (!img_u8 && ((uintptr_t)img & 3)) return fail(ICAF_ERR_ARG, "icaf_vgg_stem: fp32 images must be 4-byte aligned");
    // 32-bit tap offsets inside one image (3 planes), 31-bit pixel count per stream
    if ((long long)(img_u8 ? ctot : 3) * H * W > 0x7fffffffLL || (long long)B * H * W > 0x7fffffffLL) return fail(ICAF_ERR_ARG, "icaf_vgg_stem: image too large");
    const long long nseg = (long long)nstreams * B * H * ((W + 31) / 32);
    long long blocks = (nseg + 3) / 4;
    if (blocks > 256 * 8) blocks = 256 * 8;                               // grid-stride: 8 workgroups of 4 waves per CU
    const dim3 grid((unsigned)blocks), block(256);
    const unsigned short* wp = (const unsigned short*)w;
    unsigned short* yp = (unsigned short*)y;
    if (dtype == ICAF_BF16) {
        if (img_u8) vgg_stem_kernel<ICAF_BF16, true><<<grid, block, 0, S(s)>>>(img, ctot, wp, bias, yp, ldy, nstreams, B, H, W, w_gs, bias_gs, y_gs);
        else vgg_stem_kernel<ICAF_BF16, false><<<grid, block, 0, S(s)>>>(img, ctot, wp, bias, yp, ldy, nstreams, B, H, W, w_gs, bias_gs, y_gs);
    } else {
        if (img_u8) vgg_stem_kernel<ICAF_F16, true><<<grid, block, 0, S(s)>>>(img, ctot, wp, bias, yp, ldy, nstreams, B, H, W, w_gs, bias_gs, y_gs);
        else vgg_stem_kernel<ICAF_F16, false><<<grid, block, 0, S(s)>>>(img, ctot, wp, bias, yp, ldy, nstreams, B, H, W, w_gs, bias_gs, y_gs);
    }
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}
