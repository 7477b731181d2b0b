/*
 * icaf.h — C ABI of libicaf.so, the MI355X (gfx950) implementation of ICAFusion's inference hot path.
 *
 * The reference (chanchanchan97/ICAFusion) is pure Python on PyTorch: it has no FFI / plugin layer to mirror
 * (SURVEY.md §8b).  Its "operator interface" for this path is the set of nn.Module forwards in
 * models/common.py and models/yolo_test.py plus utils/general.non_max_suppression; each entry point below
 * replaces the arithmetic of one of those (file:line cited per function, paths relative to the reference root).
 * The host side (the icafusion_amd/models package) keeps the reference's Python class names and constructor signatures
 * and calls these functions through ctypes — see INTEGRATION.md for the binding stub.
 *
 * Conventions
 *   - every pointer parameter is a DEVICE pointer unless it is marked ICAF_HOST (char* is always host memory);
 *   - activations are NHWC ("channels-last"): element (b,h,w,c) lives at ((b*H + h)*W + w)*ld + c, where the
 *     pixel stride `ld` >= C lets a tensor be a channel slice of a wider buffer (this is how Concat, C3's
 *     torch.cat and SPPF's torch.cat are eliminated);
 *   - dtype codes select the storage/compute type of activations and packed weights; accumulation, bias,
 *     normalisation statistics, softmax and the Detect/NMS arithmetic are always fp32;
 *   - kernels are enqueued on the caller's HIP stream (hipStream_t passed as void*), never synchronise, never
 *     allocate;
 *   - return value 0 = ok, negative = error; icaf_last_error() returns a thread-local message.
 */
#ifndef ICAF_H
#define ICAF_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* icaf_stream_t; /* hipStream_t */
/* marks a pointer parameter that is HOST memory (char* always is); every other pointer is a device pointer.  The Python binding reads it. */
#define ICAF_HOST

enum { ICAF_F32 = 0, ICAF_BF16 = 1, ICAF_F16 = 2 };
enum { ICAF_ACT_NONE = 0, ICAF_ACT_SILU = 1, ICAF_ACT_GELU = 2, ICAF_ACT_RELU = 3 };
enum { ICAF_OK = 0, ICAF_ERR_ARG = -1, ICAF_ERR_HIP = -2, ICAF_ERR_UNSUPPORTED = -3 };

const char* icaf_last_error(void);
/* Probe knobs of the library, set by the host's one options object (icafusion_amd/options.py) when the library is loaded — the library reads no
 * environment variable: "detect_elementwise" (!= 0: icaf_detect_decode by the one-thread-per-element kernel), "attn_qsplit" (n > 0: query splits per
 * head of icaf_cross_attention), "sppf_vpb" (n > 0: cap on the channel vectors per workgroup of icaf_sppf_pool), "letterbox_direct" (!= 0:
 * icaf_letterbox_frames, icaf_letterbox_yuv_frames, icaf_letterbox_warp_frames and icaf_letterbox_y16_frames tap global memory in every tile instead of staging in LDS; set by a caller for an A/B, not by the options object),
 * "index64" (!= 0: the element kernel of icaf_dmff_pool_tokens and icaf_upsample_nearest launch the 64-bit-index instantiations they otherwise
 * keep for 2^31 vectors and more), "attn_stream" (!= 0: icaf_cross_attention launches the key-streaming form for every shape, for A/B timings
 * and tests; set by a caller, not by the options object), "area_direct" (!= 0: the area rows of icaf_resize_frames recompute their vertical
 * sums per horizontal tap instead of staging them in LDS; set by a caller for an A/B, not by the options object); 0 = the library's own choice.
 * ICAF_ERR_ARG for an unknown name.  None of them changes a result. */
int icaf_set_option(const char* name, int value);
int icaf_version(void);
/* device facts used by the host for grid sizing / reporting: CU count, LDS bytes per workgroup, gcnArchName */
int icaf_device_info(ICAF_HOST int* cu_count, ICAF_HOST int* lds_bytes, char* arch, int arch_len);

/* ---- input staging -------------------------------------------------------------------------------------
 * Reference: detect_twostream.py:70-80 / test.py:116-123 hand the model NCHW float tensors in [0,1].
 * mode 0: NCHW fp32 -> NHWC `dtype`, channels zero-padded from C to Cpad.
 * mode 1: NCHW fp32 -> space-to-depth NHWC: out[b][h/2][w/2][(dy*2+dx)*C + c] = in[b][c][h][w], padded to
 *         Cpad.  A 6x6 / stride-2 / pad-2 convolution over the image (first layer of each stream,
 *         rows 0 and 10 of the Transfusion yaml files) equals a 3x3 / stride-1 / pad-1 convolution over this tensor.
 */
int icaf_preprocess_nchw(const float* img, void* out, int dtype, int B, int C, int H, int W, int Cpad, int mode,
                         icaf_stream_t s);
/* Same staging straight from the dataloader's uint8 batch (reference test.py:116-123: `img.to(device)`, `.float()`,
 * `/= 255.0`, `img[:, :3]` / `img[:, 3:]`).  img: [B][Ctot][H][W] uint8; stream s (0 <= s < nstreams) takes channels
 * [c0 + s*C, c0 + (s+1)*C) and is written to out[s][b] (nstreams*B images), value = (float)u8 / 255.0f. */
int icaf_preprocess_u8(const unsigned char* img, void* out, int dtype, int B, int Ctot, int c0, int C, int nstreams,
                       int H, int W, int Cpad, int mode, icaf_stream_t s);

/* Staging + stem convolution in one persistent kernel: the 6x6 / stride 2 / pad 2 Conv(+BN+SiLU) of yaml rows 0 and 10
 * (models/common.py:48-60) computed straight from the NCHW images (fp32 [nstreams*B][3][H][W], or img_u8 != 0: the
 * dataloader's uint8 [B][ctot][H][W] batch, stream s = channels [3s, 3s+3), value / 255) — no staged copy of the images
 * is written.  w: packed space-to-depth weights [Np][192] per stream (icafusion_amd.ops.s2d_conv_weight), y: NHWC
 * [nstreams][B][H/2][W/2][ldy]; *_gs = per-stream strides in elements / floats.  16-bit types, Cout in {32, 64}. */
int icaf_stem(const void* img, int img_u8, int ctot, const void* w, const float* bias, void* y, int ldy, int dtype,
              int nstreams, int B, int H, int W, int Cout, int Kp, long long w_gs, long long bias_gs, long long y_gs,
              icaf_stream_t s);

/* Yaml rows 0-2 (10-12) up to the C3's first GEMM in ONE persistent kernel — the three layers every image pixel goes
 * through at the highest resolutions (models/common.py:48-60, 216-227; models/transformer/yolov5s_*.yaml rows 0-2):
 *   t0 = SiLU(conv6x6/s2/p2(img) + bias0)          C0 channels at H/2 x W/2   (the stem, as icaf_stem)
 *   t1 = SiLU(conv3x3/s2/p1(t0) + bias1)           C1 channels at H/4 x W/4
 *   y  = SiLU(W2 . t1 + bias2)                     C2 channels (the C3's cv1 | cv2), NHWC [nstreams][B][H/4][W/4][ldy]
 * t0 and t1 live in LDS only (rounded to the storage type exactly where the three-launch form writes them, so the
 * result is bit-identical to icaf_stem -> icaf_conv2d with a chained 1x1).  Weights are the packed matrices of those
 * launches: w0 [Np][192] (space-to-depth), w1 [Np][Kp1] (k = ky, kx, c0), w2 [Np][Kp2]; *_gs = per-stream strides.
 * Built for C0 = 32, C1 = 64, C2 <= 64 (yolov5s), 16-bit types. */
typedef struct icaf_stem2_args {
    const void* img; int img_u8, ctot;             /* as icaf_stem */
    int dtype, nstreams, B, H, W;
    const void* w0; const float* bias0; long long w0_gs, bias0_gs; int Kp0, C0;
    const void* w1; const float* bias1; long long w1_gs, bias1_gs; int Kp1, C1;
    const void* w2; const float* bias2; long long w2_gs, bias2_gs; int Kp2, C2;
    void* y; long long y_gs; int ldy, reserved;
} icaf_stem2_args;
int icaf_stem2(ICAF_HOST const icaf_stem2_args* a, icaf_stream_t s);

/* Image-fed first layer of a VGG block (models/common.py:109-128: Conv2d(3, 64, 3, padding=1) + ReLU, yaml rows 0 and 5 of the
 * yolov5_VGG16_* files) in one launch, both streams: y = ReLU(conv3x3 / s1 / p1 (img) + bias) computed straight from the NCHW images
 * (img / img_u8 / ctot as icaf_stem; the uint8 value / 255 is a true division, as icaf_preprocess_u8) — no staged copy of the images is
 * written.  w: [nstreams][64][32] in the storage type, K = 27 in the order (ky, kx, c) zero-padded to 32 (icafusion_amd.ops.vgg_stem_weight);
 * bias: fp32 [nstreams][64]; y: NHWC [nstreams][B][H][W][ldy], written as 128-byte pixels with 16-byte stores (ldy % 8 == 0, 16-byte aligned);
 * *_gs = per-stream strides in elements / floats.  The images are rounded to the storage type first (what the staged copy of the generic
 * route holds), products and the 27-term sum are fp32, bias and ReLU fp32, ONE rounding at the store.  16-bit types, Cout = 64, Kp = 32,
 * H, W <= 2^20; everything else is refused before any launch (fp32 runs icaf_preprocess_* + icaf_conv2d). */
int icaf_vgg_stem(const void* img, int img_u8, int ctot, const void* w, const float* bias, void* y, int ldy, int dtype,
                  int nstreams, int B, int H, int W, int Cout, int Kp, long long w_gs, long long bias_gs, long long y_gs,
                  icaf_stream_t s);

/* ---- implicit-GEMM convolution / linear ------------------------------------------------------------------
 * Replaces Conv.forward / fuseforward (models/common.py:48-60: SiLU(BN(Conv2d))) with BN folded into the
 * weights (utils/torch_utils.py:182-202), nn.Linear (+GELU) inside CrossAttention / CrossTransformerBlock
 * (models/common.py:607-618,704-709), the residual add of Bottleneck (models/common.py:194) and the
 * LearnableCoefficient mixes (models/common.py:746-750), and Detect's 1x1 output convs (models/yolo_test.py:50).
 *
 *   y[m][n] = alpha_res * res[m][n] + alpha_acc * act( sum_k A[m][k] * Wp[n][k] + bias[n] [+ bilinear(pre)[m][n]] )
 *
 * m = (b, ho, wo) output pixel, k = (kh, kw, cin) gathered on the fly from x (zero outside the image),
 * Wp = packed weights [Np][Kp] (K-major, Np = Cout rounded up to 128, Kp = K rounded up to 64 elements, zero
 * padded).  `groups` > 1 batches independent problems (the two modalities of DMFF) in gridDim.z; the *_gs
 * fields are the per-group strides in ELEMENTS (bytes/sizeof for x,w,y,res; floats for bias).
 *
 * Rounding.  The sum, bias, pre term, activation and alpha_acc are evaluated in fp32.  The result is rounded to out_dtype (nearest even,
 * subnormals kept); with a residual, alpha_res * res is then added to that ROUNDED value by one fp32 fma and the sum rounded to out_dtype
 * again — the rounding points of the unfused layers (a convolution's output is a tensor of the storage type, the shortcut adds to it).
 * With fp32 output nothing is rounded in between.  With res_mode = 1 (below) the residual is widened to fp32 and added IN FRONT of the
 * activation: sum, bias, residual and ReLU in fp32, one rounding at the store.  ACT_RELU is max(v, 0), torch.relu for every finite v; ACT_SILU uses the hardware exp2 / reciprocal (-0 for pre-activations below -87.3, where
 * the true value is below 1.05e-36); ACT_GELU is erff in the fp32 build and Abramowitz & Stegun 7.1.26 in the 16-bit builds, accurate to
 * 0.5 |v| (1.5e-7 + 2^-23) in ABSOLUTE terms: several fp16 units of the result for v <= -3.5.
 * Reads and writes.  x, res and pre may be channel slices of wider buffers holding anything, Inf and NaN included: no launch configuration
 * lets a channel outside [0, Cin) of a pixel, or outside [0, Cout) of res / pre, reach a result, and none writes outside [0, Cout) of
 * y / y2.  (The LDS-DMA pipelines prefetch K slices past the end of a pixel row — inside the buffer range of the view — into ring stages
 * that are never consumed.)  Inside the views the usual IEEE rules hold: an Inf in x reaches every output whose receptive field holds it.
 * tests/test_gpu_exact.py checks all of this bit for bit on every launch configuration.
 */
typedef struct icaf_conv_args {
    const void* x;
    const void* w;
    const float* bias; /* may be NULL */
    void* y;
    const void* res; /* may be NULL */
    long long x_gs, w_gs, bias_gs, y_gs, res_gs;
    int groups;
    int B, H, W, Cin, ldx;
    int Ho, Wo, Cout, ldy;
    int kh, kw, sh, sw, ph, pw;
    int ldr;
    int Kp;
    int act;
    int dtype;     /* x, w, res */
    int out_dtype; /* y: same as dtype, or ICAF_F32 */
    float alpha_acc[2];
    float alpha_res[2];
    int tile; /* 0 = auto; otherwise force a launch configuration (tuning / tests).  An id that is not built is ICAF_ERR_ARG, a built one the
               * layer does not satisfy ICAF_ERR_UNSUPPORTED: neither is ever replaced silently (one exception: tiles 1 - 4 of an LDS-DMA
               * pipeline run on the register-staged one, id % 10 + 10, when an operand exceeds the 2 GiB buffer-descriptor range).
               * The built ids (icaf_conv2d_config_ids), one family of kernels per row of igemm.hip's table:
               *   igemm.hip         tile + 10 * pipeline: 1 - 4, 11 - 14, 21 - 26, 28, 29, 31 - 34
               *   ctile.hip         41 - 45          igemm_stream.hip  51, 52          igemm_wreg.hip  61 - 66
               *   cstream.hip       71               cwide.hip         81 - 85
               * ACT_RELU runs on igemm.hip, igemm_stream.hip and igemm_wreg.hip; ctile / cstream / cwide and the chained / pre-term launches
               * are SiLU-only and answer ICAF_ERR_UNSUPPORTED before any device call.
               * Every configuration of a layer produces the same bits (same K order, MFMA step, epilogue expressions). */
    /* Optional pre-activation term, bilinearly resized (align_corners=False) from a coarse fp32 map:
     *   y = alpha_res*res + alpha_acc * act( A.W + bias + bilinear(pre)[b][ho][wo][n] )
     * pre: [B][pre_h][pre_w][ldpre] fp32 (NULL = none).  This is how DMFF's tail (models/common.py:827-841:
     * F.interpolate(tokens) + feature, cat, conv1x1_out) runs as ONE GEMM over the untouched features: the 1x1
     * convolution commutes with the (linear) resize, so conv(cat(f + up(t))) = conv(cat(f)) + up(conv(cat(t))). */
    const float* pre;
    int pre_h, pre_w, ldpre;
    int pre_mode; /* 0: bilinear (align_corners=False); 1: nearest, src = floor(dst * pre_h / Ho) — nn.Upsample('nearest') in
                   * front of a Concat feeding a 1x1 conv (head rows 24-26 / 28-30): W.cat(up(a), b) = up(Wa.a) + Wb.b, so
                   * the low-resolution product Wa.a is the `pre` map of the GEMM over b and neither up(a) nor the concat exist */
    /* Optional chained 1x1 convolution + SiLU consuming this layer's output tile in place (w2 != NULL):
     *   y2 = SiLU( W2 . SiLU(A.W + bias) + bias2 )        [this layer must be SiLU, 16-bit, one N tile: Cout <= 256]
     * The intermediate tensor is never written (y is ignored) unless chain_keep is set.  It is how a backbone down-sampling Conv and the fused
     * cv1|cv2 GEMM of the C3 block behind it (models/common.py:56-60 then :226) run as one launch.
     * w2: packed [Np][Kp2] with K = Cout, bias2 may be NULL, y2: NHWC with pixel stride ldy2, Cout2 <= 256 channels. */
    const void* w2;
    const float* bias2;
    void* y2;
    long long w2_gs, bias2_gs, y2_gs;
    int Kp2, Cout2, ldy2;
    int chain_keep; /* != 0: y IS written as well; only then may `res` be set: the chained 1x1 consumes y as stored, residual
                     * included (a Bottleneck's 3x3 + shortcut followed by the next Bottleneck's 1x1, models/common.py:193-194) */
    /* Optional second copy of the packed weights in FRAGMENT-MAJOR order (NULL = none), read by the launch configurations that feed
     * the weight operand from registers (igemm_wreg.hip, cwide.hip: tile ids 61 - 66, 81 - 85): [Np / 32][Kp / 16][64 lanes][8 elements], lane
     * (hi * 32 + r) of block (nb, ks) holding w[nb * 32 + r][ks * 16 + hi * 8 .. + 8] of the K-major matrix above; wf_gs = group
     * stride in elements.  16-bit types (icafusion_amd.ops.frag_weights builds it once per layer). */
    const void* wf;
    long long wf_gs;
    /* Optional second half of the chained 1x1's input (NULL = none; needs w2): the chained layer then reads K = [this layer's output
     * tile (Cout channels) | x2 (Cout more channels of the same pixels)]:
     *   y2 = SiLU( W2 . cat( [alpha_res*res +] SiLU(A.W + bias), x2 ) + bias2 )
     * This is the TAIL of a C3 block (models/common.py:216-227: cv3(cat(m(cv1(x)), cv2(x)))): the last Bottleneck's 3x3 (+ shortcut,
     * `res` allowed without chain_keep) carries cv3, x2 = cv2's output; the Bottleneck chain's result and the concatenation never reach HBM.
     * x2: NHWC, pixel stride ldx2 elements, x2_gs = group stride in elements; W2 packed [Np][Kp2] with K in cv3's own order [m | cv2].
     * Built for 128 -> 128 3x3 / stride 1 layers with Cout2 = 256, Kp2 = 256, 16-bit types, launch configurations 81 / 82 (cwide.hip);
     * bit-identical to the two launches. */
    const void* x2;
    long long x2_gs;
    int ldx2;
    /* Where the residual enters.  0: behind the activation, y = alpha_res*res + alpha_acc*act(...) as above (the YOLO Bottleneck).
     * 1: in front of it,
     *   y = relu( A.W + bias + res )
     * — a ResNet bottleneck's conv3 + bn3 (folded) + shortcut add + ReLU (models/common.py:149-156) as one launch.  res is read in the storage
     * type and widened to fp32; the sum and the ReLU are fp32 and there is ONE rounding, at the store.  (The reference in a 16-bit type rounds
     * three times: after bn3, after the add, after the ReLU.)  Accepted in exactly this form: res != NULL, act == ICAF_ACT_RELU, all four
     * alphas 1, no pre, no w2 / x2, out_dtype == dtype — anything else is ICAF_ERR_UNSUPPORTED before any device call; a value other than
     * 0 / 1 is ICAF_ERR_ARG.  It runs on the families that run ACT_RELU (igemm.hip, igemm_stream.hip, igemm_wreg.hip), every
     * configuration giving the same bits; ctile / cstream / cwide refuse it as they refuse ReLU.  It is no activation code. */
    int res_mode;
} icaf_conv_args;

int icaf_conv2d(ICAF_HOST const icaf_conv_args* a, icaf_stream_t s);

/* Whole Bottleneck in one launch (models/common.py:184-194): y = [x +] SiLU(conv3x3(SiLU(conv1x1(x)))) for c_ -> c_ -> c_
 * channels with c_ in {32, 64}, 16-bit types.  `conv` describes the 3x3 / stride 1 / pad 1 layer (x = block input,
 * w / bias = its packed weights, y = block output — a DIFFERENT buffer than x —, res = x for the shortcut or NULL);
 * w1 / bias1 are the packed 1x1 weights ([Np][Kp1], Kp1 = 128 bytes) applied first.  The 1x1 output never reaches HBM.
 * shape: LDS patch 1 = 8x32 pixels (c_ = 32), 2 = 8x32 (c_ = 64), 3 = 8x16 (c_ = 64).
 * With conv.w2 != NULL (shape 1 only) the C3's cv3 rides on the block (models/common.py:226):
 *   y2 = SiLU( W2 . cat(x2, [x +] SiLU(conv3x3(...))) + bias2 )
 * x2 = the cv2 half of cv3's input (NHWC, c_ channels, pixel stride ldx2), W2 packed [Np][64] with its K columns in the
 * order [cv2 | m]; only y2 (conv.y2 / ldy2, Cout2 = 64, 16-byte aligned rows) is written — conv.y is ignored.  Bit-identical to icaf_bottleneck
 * followed by the 1x1 icaf_conv2d. */
typedef struct icaf_bneck_args {
    icaf_conv_args conv;
    const void* w1;
    const float* bias1;
    long long w1_gs, bias1_gs; /* per-group strides (elements / floats) */
    int Kp1;
    int shape;
    const void* x2;
    long long x2_gs;
    int ldx2, reserved;
} icaf_bneck_args;
int icaf_bottleneck(ICAF_HOST const icaf_bneck_args* a, icaf_stream_t s);
/* name of the kernel instantiation icaf_conv2d would launch for these args (host string, for profiling) */
int icaf_conv2d_kernel_name(ICAF_HOST const icaf_conv_args* a, char* buf, int buf_len);
/* the launch configuration ids that are built, ascending: writes the first `cap` of them to ids (may be NULL), returns how many there are */
int icaf_conv2d_config_ids(ICAF_HOST int* ids, int cap);

/* ---- SPPF / upsample / copy ------------------------------------------------------------------------------
 * icaf_sppf_pool: the three chained k x k stride-1 max pools of SPPF.forward (models/common.py:262-267);
 *   y1 = mp(x), y2 = mp(y1), y3 = mp(y2) computed in one pass (-inf padding semantics).
 * icaf_upsample_nearest: nn.Upsample(None, scale, 'nearest') rows of the head (yaml rows 24, 28).
 * icaf_copy_channels: generic channel-slice copy (fallback for Concat, models/common.py:313-321).
 */
int icaf_sppf_pool(const void* x, int ldx, void* y1, void* y2, void* y3, int ldy, int dtype, int B, int H, int W,
                   int C, int k, icaf_stream_t s);
/* launch choice of icaf_sppf_pool for this geometry (SPPF.forward, models/common.py:262-267): *vpb = channel vectors per
 * workgroup of the LDS kernel (8 / 4 / 2 / 1, the probe knob "sppf_vpb" included), 0 = the global-memory kernel */
int icaf_sppf_config(int dtype, int H, int W, int C, ICAF_HOST int* vpb);
int icaf_upsample_nearest(const void* x, int ldx, void* y, int ldy, int dtype, int B, int H, int W, int C,
                          int scale, icaf_stream_t s);
/* nn.MaxPool2d(k, stride, pad) over an NHWC tensor (models/common.py:122: the 2 / 2 / 0 pool closing a VGGblock; 3 / 2 / 1 is ResNet's):
 * y[b][ho][wo][c] = max over the window's pixels INSIDE the image (padding never takes part: it acts as -inf), Ho = (H + 2 pad - k) /
 * stride + 1 (floor).  x / y may be channel slices (ldx, ldy >= C); a pair activation is 2 B images.  The bits are those of torch's CPU
 * kernel (same scan order and comparison, NaN propagates).  C must be a multiple of the 16-byte vector width (4 fp32 / 8 16-bit); 16-byte
 * loads and stores where ldx, ldy and both addresses allow, one element per thread otherwise.  Other windows: ICAF_ERR_UNSUPPORTED. */
int icaf_maxpool2d(const void* x, int ldx, void* y, int ldy, int dtype, int B, int H, int W, int C, int k, int stride, int pad,
                   icaf_stream_t s);
int icaf_copy_channels(const void* x, int ldx, void* y, int ldy, int dtype, long long rows, int C,
                       icaf_stream_t s);
/* icaf_axpby: y = a*x0 + b*x1 over `rows` pixels of C channels — the `Add` fusion block (models/common.py:324-331:
 * x[0]*w + x[1]*(1-w)) of the *_Add_* configs. */
int icaf_axpby(const void* x0, int ld0, const void* x1, int ld1, void* y, int ldy, int dtype, long long rows, int C,
               float a, float b, icaf_stream_t s);

/* ---- DMFF (TransformerFusionBlock, models/common.py:762-865) ---------------------------------------------
 * icaf_dmff_pool_tokens: AdaptivePool2d avg + max (models/common.py:868-891), LearnableWeights mix
 *   (:579-587) and positional embedding add (:817-823) for both modalities.
 *   tokens[g][b][n][c] = w1_g*avg + w2_g*max + pos_g[n][c],  g = 0 (RGB) / 1 (IR),  n = th*W' + tw.
 * icaf_layernorm: nn.LayerNorm(C), eps 1e-5 over the last dim, C <= 2048 in whole 16-byte vectors (fp32 rows wider than 1024 run an
 *   instantiation with eight vectors per lane; every other row the one it always ran); group g uses (gamma_g, beta_g)
 *   (CrossAttention.LN1/LN2 :646,:651; CrossTransformerBlock.LN2 applied to both groups :749-750).
 * icaf_cross_attention: the two crossed softmax(QK^T/sqrt(dk))V products of CrossAttention.forward (:670-685).
 *   qkv[g][row][3C] holds [q | k | v] of modality g; out[0] = softmax(q_1 k_0^T) v_0, out[1] = softmax(q_0 k_1^T) v_1
 *   with heads laid out as in .view(b, n, h, dk) (:647-649).
 * icaf_dmff_upsample_merge: eval-mode F.interpolate(bilinear, align_corners=False) of the token maps back to
 *   (H, W), residual add of the original features and channel concat (:827-840):
 *   out[b][h][w][g*C + c] = bilinear(tokens[g])[b][h][w][c] + fea_g[b][h][w][c].
 */
int icaf_dmff_pool_tokens(const void* fea_rgb, int ld_rgb, const void* fea_ir, int ld_ir, const float* pos_rgb,
                          const float* pos_ir, void* tokens, int dtype, int B, int H, int W, int C, int th, int tw,
                          int kh, int kw, int sh, int sw, float w1_rgb, float w2_rgb, float w1_ir, float w2_ir,
                          icaf_stream_t s);
/* launch choice of icaf_dmff_pool_tokens for this geometry (same argument checks): *kernel = 0 (one thread per token element) / 1 (separable
 * rows kernel, overlapping windows whose token row fits the LDS); rows kernel: *R = input rows in flight per item (4 / 8 / 12), *TR = token rows
 * per workgroup (1 / 2), else 0; element kernel: *index64 = 1 when the 64-bit-index instantiation runs (the probe knob "index64" included) */
int icaf_dmff_pool_config(int dtype, int B, int H, int W, int C, int th, int tw, int kh, int kw, int sh, int sw, ICAF_HOST int* kernel, ICAF_HOST int* R,
                          ICAF_HOST int* TR, ICAF_HOST int* index64);
int icaf_layernorm(const void* x, void* y, const float* gamma0, const float* beta0, const float* gamma1,
                   const float* beta1, int dtype, long long rows_per_group, int C, int groups, float eps,
                   icaf_stream_t s);
int icaf_cross_attention(const void* qkv, void* out, int dtype, int B, int N, int C, int heads, icaf_stream_t s);
/* launch choice of icaf_cross_attention (CrossAttention.forward :670-685): *dkp = padded head dimension of the kernel instance,
 * *qsplit = query splits per head (the probe knob "attn_qsplit" included), *remap = 1 when the one-dimensional XCD-grouped grid is used */
int icaf_cross_attention_config(int dtype, int B, int N, int C, int heads, ICAF_HOST int* dkp, ICAF_HOST int* qsplit, ICAF_HOST int* remap);
/* Which kernel icaf_cross_attention launches for this shape (same argument checks): *form = 0, the resident form — K and V^T of a head stay in
 * LDS for the workgroup's lifetime: d_k <= 128 and at most 160 KiB, unchanged; *form = 1, the key-streaming form — K and V^T pass through LDS
 * in double-buffered 32-key tiles, same online softmax and key order: 128 < d_k <= 256 (a multiple of the 16-byte vector) and every shape whose
 * resident K / V^T exceed 160 KiB (fp32 at N = 256, d_k = 128), or everything with the probe knob "attn_stream".  For form 1
 * icaf_cross_attention_config reports the streaming instance's padded head dimension (64 / 128 / 256; d_k = 192 runs the 256 instance), its query
 * splits (a workgroup round is four query tiles, two at 256, where a pair of waves shares a query tile and splits the head's d rows) and remap. */
int icaf_cross_attention_form(int dtype, int B, int N, int C, int heads, ICAF_HOST int* form);
int icaf_dmff_upsample_merge(const void* tokens, const void* fea_rgb, int ld_rgb, const void* fea_ir, int ld_ir,
                             void* out, int ldo, int dtype, int B, int H, int W, int C, int th, int tw,
                             icaf_stream_t s);

/* ---- Detect decode (models/yolo_test.py:43-65, eval branch) -----------------------------------------------
 * p: fp32 output of the level's 1x1 conv, NHWC [B][ny][nx][ldp] with channel = a*no + o.
 * Writes z[b][row_offset + (a*ny + y)*nx + x][o] (sigmoid + grid/anchor decode), logits (raw class scores,
 * may be NULL) and raw[b][a][y][x][o] (the permuted pre-sigmoid map the reference also returns, may be NULL).
 * anchors_px: host pointer to na*2 floats = anchor sizes in pixels (anchor_grid).
 */
int icaf_detect_decode(const float* p, int ldp, float* z, float* logits, float* raw, int B, int ny, int nx, int na,
                       int no, long long rows_total, long long row_offset, float stride, ICAF_HOST const float* anchors_px,
                       icaf_stream_t s);
/* which kernel icaf_detect_decode launches for these arguments (models/yolo_test.py:43-65): *kernel = 0 one thread per pixel
 * (3 anchors, no in {6, 8, 14}, 8-byte aligned rows), 1 one thread per element (every other head, or the probe knob
 * "detect_elementwise").  Pointers, not shapes: their alignment is part of the choice; nothing is read through them. */
int icaf_detect_decode_kernel(const float* p, int ldp, const float* z, const float* raw, int B, int ny, int nx, int na,
                              int no, ICAF_HOST int* kernel);
/* A Detect level in ONE launch (16-bit feature maps, 3 anchors, no in {6, 8, 14}): the level's 1x1 output convolution
 * (models/yolo_test.py:50; `a` describes it as for icaf_conv2d: 1x1, no activation, groups 1, Cout = na * no; a->y is ignored)
 * with the decode above as the epilogue of the persistent streaming GEMM — the fp32 conv map is never written.  z / logits / raw
 * are bit-identical to icaf_conv2d (fp32 out) followed by icaf_detect_decode. */
int icaf_detect_conv(ICAF_HOST const icaf_conv_args* a, float* z, float* logits, float* raw, int na, int no, long long rows_total,
                     long long row_offset, float stride, ICAF_HOST const float* anchors_px, icaf_stream_t s);

/* ---- fused DMFF block (16-bit token types) -------------------------------------------------------------------
 * One CrossTransformerBlock iteration (models/common.py:737-759) in two launches:
 *   icaf_dmff_ln_qkv    qkv[g] = LayerNorm_g(x[g]) W_qkv,g^T + b   — CrossAttention.LN1 / LN2 (:661-662) fused in front of the
 *                       six Linear(C, C) projections (:664-669); qkv[g][row][3C] = [que | key | val] of modality g.
 *   icaf_dmff_attn_mlp  per 64 token rows of one (image, modality g): the crossed attention of those rows over all heads
 *                       (softmax(q_{1-g} k_g^T / sqrt(dk)) v_g, :670-681), out-projection and coefficient mix
 *                       x_att = coef_res_attn[g] * x + coef_acc_attn[g] * (att W_o,g^T + b) (:682-685, :745-746), the block's shared
 *                       LayerNorm LN2 (:749-750), MLP Linear(C, 4C) -> GELU(erf) -> Linear(4C, C) (:704-709) and
 *                       y = coef_res_mlp[g] * x_att + coef_acc_mlp[g] * (mlp + b) (:751-752).  Attention output, x_att, the
 *                       normalised tile and the hidden activations stay in LDS / registers.
 * x: tokens [2][B*N][C] (group stride x_gs elements); y: element (g, row, c) at y + g*y_gs + row*ldy + c (may alias neither x
 * nor qkv).  Weights are packed [2][Np][Kp] (Np multiple of 128, Kp of 64; *_gs = per-modality strides), biases fp32 [2][Np].
 * Requirements: dtype bf16 / f16, C % 64 == 0, head dim % 8 == 0, hidden % 128 == 0; icaf_dmff_attn_mlp additionally C <= 512
 * (icaf_dmff_attn_mlp_lds_bytes returns the LDS bytes a launch needs, or (size_t)-1 when the shape is not covered: callers
 * then run the per-layer entry points above).  Rounding points equal those of the per-layer launches. */
typedef struct icaf_dmff_args {
    const void* x; void* qkv; void* y;
    const void* wqkv; const float* bqkv;
    const void* wo; const float* bo;
    const void* w1; const float* b1;
    const void* w2; const float* b2;
    const float* ln_attn_gamma[2]; const float* ln_attn_beta[2];   /* CrossAttention.LN1 (RGB tokens), LN2 (IR tokens) */
    const float* ln_mlp_gamma; const float* ln_mlp_beta;           /* CrossTransformerBlock.LN2, both modalities */
    long long wqkv_gs, bqkv_gs, wo_gs, bo_gs, w1_gs, b1_gs, w2_gs, b2_gs, x_gs, y_gs;
    int dtype, B, N, C, heads, Kp, Kp4, hidden, ldy, reserved;
    float eps_attn, eps_mlp;
    float coef_res_attn[2], coef_acc_attn[2], coef_res_mlp[2], coef_acc_mlp[2];   /* coefficient1/3, 2/4, 5/7, 6/8 */
    void* debug_clock;   /* NULL, or 8 int64 slots: workgroup (0,0,0) of icaf_dmff_attn_mlp stores the shader clock at its phase boundaries */
    /* reserved: icaf_dmff_wide_ln_qkv reads it as "output-channel passes per workgroup": 1 = one (A/B switch; measured slower), anything else =
     * three; other entry points ignore it */
    /* fp32 RESIDUAL STREAM across the shared-weight iterations (models/common.py:744-752 run `loops` times: x = block(x)); read by
     * icaf_dmff_wide_proj_mlp / _split / icaf_dmff_wide_reduce only.  y32 != NULL: this iteration's tokens are ALSO written in fp32 to
     * y32 [2][B*N][C] (x_att is then kept in fp32 inside the step); x32 != NULL: the residual x of this iteration is read from the previous
     * iteration's fp32 tokens instead of the 16-bit x (LayerNorm + QKV keep reading the 16-bit tokens).  16-bit dtypes, 16-byte aligned. */
    const float* x32; float* y32;
} icaf_dmff_args;
int icaf_dmff_ln_qkv(ICAF_HOST const icaf_dmff_args* a, icaf_stream_t s);
int icaf_dmff_attn_mlp(ICAF_HOST const icaf_dmff_args* a, icaf_stream_t s);
/* The three-launch block (dmff_wide.hip: C = 128, 256 or 512 in the 16-bit types, and the fp32 parity build at C = 128): one iteration =
 * icaf_dmff_wide_ln_qkv, icaf_cross_attention, icaf_dmff_wide_proj_mlp.
 *   icaf_dmff_wide_ln_qkv    as icaf_dmff_ln_qkv (LayerNorm :661-662 + the six projections :664-669);
 *   icaf_dmff_wide_proj_mlp  out-projection + coefficient mix (:682-685, :745-746), the shared LayerNorm (:749-750), MLP + mix
 *                            (:704-709, :751-752) of 64 token rows per workgroup; att = the attention output tokens [2][B*N][C]
 *                            (contiguous, as icaf_cross_attention writes them); a->qkv / wqkv / bqkv are not read.
 * DIFFERENT WEIGHT LAYOUT: a->wqkv / wo / w1 / w2 point at FRAGMENT-MAJOR copies of the packed [2][Np][Kp] matrices,
 * [2][Np/32][Kp/16][64][8] (lane (hi*32 + r) of block (nb, ks) = w[nb*32 + r][ks*16 + hi*8 .. +8], the layout of icaf_conv_args.wf;
 * same *_gs strides): each wavefront streams its MFMA weight operands straight from L2 into registers.  hidden % 256 == 0. */
int icaf_dmff_wide_ln_qkv(ICAF_HOST const icaf_dmff_args* a, icaf_stream_t s);
int icaf_dmff_wide_proj_mlp(ICAF_HOST const icaf_dmff_args* a, const void* att, icaf_stream_t s);
/* The same step with the MLP's hidden columns split over `ksplit` (2 or 4) workgroups per 64-row tile — for levels with fewer tiles
 * than CUs and more weight bytes than an XCD's L2 (P5: 100 tokens x 32 images at C = 512): every workgroup repeats out-projection +
 * LayerNorm (:682-685, :745-750), runs Linear(C, 4C) -> GELU -> Linear(4C, C) (:704-709) over ITS hidden slice, parks x_att in y and
 * writes fp32 partial sums into partial [ksplit][2][B*N][C].  icaf_dmff_wide_reduce (the next launch on the stream) adds them in slice
 * order (deterministic: no atomics, no in-kernel fences) and applies bias + the coefficient mix (:751-752) in place on y.  Same operands
 * and fragment-major weight layout as icaf_dmff_wide_proj_mlp; hidden % (256 * ksplit) == 0. */
int icaf_dmff_wide_proj_mlp_split(ICAF_HOST const icaf_dmff_args* a, const void* att, float* partial, int ksplit, icaf_stream_t s);
int icaf_dmff_wide_reduce(ICAF_HOST const icaf_dmff_args* a, const float* partial, int ksplit, icaf_stream_t s);
int icaf_dmff_attn_mlp_lds_bytes(int C, int N, int heads, int dtype, ICAF_HOST size_t* bytes);
/* Which forms of a block iteration are built for a shape.  Pure host code (no HIP call: usable without a GPU) that runs the resolve and the
 * table lookup of the launches themselves, so a form reported here is a form the entry points above launch, and one refused here they refuse
 * with ICAF_ERR_UNSUPPORTED.  *two_launch: icaf_dmff_ln_qkv + icaf_dmff_attn_mlp cover (dtype, C, N, heads, hidden), the 160 KiB LDS limit
 * included.  *three_launch: icaf_dmff_wide_ln_qkv + icaf_cross_attention + icaf_dmff_wide_proj_mlp (ksplit = 1) or _split + icaf_dmff_wide_reduce
 * (ksplit = 2 / 4) are built for it, stream32 != 0: with the fp32 token stream (x32 / y32). */
int icaf_dmff_block_forms(int dtype, int C, int N, int heads, int hidden, int ksplit, int stream32, ICAF_HOST int* two_launch,
                          ICAF_HOST int* three_launch);

/* ---- test-time augmentation (models/yolo_test.py:116-131, utils/torch_utils.py:257-267) ---------------------
 * Model.forward(augment=True) runs three passes, (scale, flip) = (1, -), (0.83, left-right), (0.67, -), and concatenates their decoded
 * rows.  The reference's loop scales only `x` and calls forward_once(xi) without the second image (:122-123, a TypeError for the
 * two-stream model); built here is what it plainly means: the SAME flip and scale for both modalities.
 *
 * icaf_tta_stage: scale_img (utils/torch_utils.py:257-267) of `x.flip(3) if flip else x` for both modalities and up to
 *   ICAF_TTA_MAX_PASSES scaled passes in ONE launch: F.interpolate(size = (Hr, Wr), 'bilinear', align_corners=False) followed by
 *   F.pad(right, bottom, value = 0.447) up to (Hp, Wp), written as the fp32 NCHW [2][B][3][Hp][Wp] input of the pass's plan.
 *   src: fp32 [2][B][3][H][W] (both modalities adjacent), or src_u8 != 0: the dataloader's uint8 [B][ctot][H][W] batch, modality m =
 *   channels [3m, 3m + 3), value = (float)u8 / 255.0f exactly as icaf_preprocess_u8 (the result equals staging from u8.float() / 255
 *   bit for bit).  Arithmetic of torch's CPU kernel, all fp32: scale = (float)in / (float)out, src = fmaf(scale, d + 0.5f, -0.5f)
 *   clamped below at 0, i0 = min((int)src, in - 1), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1,
 *   v = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11), no contraction; the flip is folded into the source column.
 *   Wp % 4 == 0 and 16-byte aligned dst (one 16-byte store per thread and row); Hr <= Hp, Wr <= Wp.
 * icaf_tta_merge: the de-scale / de-flip and torch.cat(y, 1) of :125-131.  z[i]: [B][rows[i]][no] fp32 (the pass's decoded rows),
 *   out: [B][sum rows][no]; out[..., :4] = z / scale[i] (a correctly rounded fp32 division, as torch's `/=`: never a reciprocal
 *   multiply), then for flip[i] != 0 out[..., 0] = width - out[..., 0]; columns >= 4 are copied.  z / rows / scale / flip are HOST arrays
 *   of npass <= ICAF_TTA_MAX_PASSES + 1 entries (z[i] device pointers). */
enum { ICAF_TTA_MAX_PASSES = 3 };
typedef struct icaf_tta_pass {
    float* dst;        /* [2][B][3][Hp][Wp] fp32 */
    int Hr, Wr;        /* resized size: (int)(H * ratio), (int)(W * ratio) */
    int Hp, Wp;        /* padded size: ceil(H * ratio / gs) * gs, ceil(W * ratio / gs) * gs */
    int flip;          /* != 0: x.flip(3) before the resize */
    int reserved;
} icaf_tta_pass;
int icaf_tta_stage(const void* src, int src_u8, int ctot, int B, int H, int W, ICAF_HOST const icaf_tta_pass* passes, int npass,
                   icaf_stream_t s);
int icaf_tta_merge(ICAF_HOST const float* const* z, ICAF_HOST const long long* rows, ICAF_HOST const float* scale, ICAF_HOST const int* flip, int npass, float* out,
                   int B, int no, float width, icaf_stream_t s);

/* ---- native camera frames (utils/datasets.py: letterbox; detect_twostream.py:70-80) ---------------------------------------
 * icaf_letterbox_frames: the host letterbox on the device, byte for byte.  arena: decoder-layout frames, h0 x w0 x ch interleaved uint8
 *   (ch = 3, or 1: the one channel feeds all three planes), each with its own row pitch; geom: DEVICE table of nstreams * B descriptors,
 *   entry modality * B + image, so that one static launch serves frames whose sizes change from step to step.  dst: the plan's uint8
 *   [B][ctot][H][W] input, modality m = channels [3m, 3m + 3); every byte of those planes is written exactly once: rows [top, top + nh) x
 *   columns [left, left + nw) the bilinear resize (half-pixel centres, edge clamp) of the frame, 114 elsewhere.  swap_rb != 0: source
 *   channel 2 - c feeds plane c (BGR frames -> RGB planes).  Arithmetic of utils/datasets.py resize_bilinear, fp32, nothing fused:
 *   s = (j + 0.5f) * scale - 0.5f (two rounded operations), i0 = floor(s) (may be -1), frac = s - i0 BEFORE i0 and i0 + 1 are clamped into
 *   the frame, top = a00 * (1 - fx) + a01 * fx, bot likewise, out = top * (1 - fy) + bot * fy, result floor(out + 0.5f) clipped to 0..255;
 *   sx = (float)(w0 / (double)nw), sy likewise, computed by the host (the kernel does not divide).  One workgroup per 32 x 64 output tile:
 *   if the source rectangle a tile of that descriptor can tap fits ICAF_LETTERBOX_LDS_BYTES — at most ((int)(32 sy) + 4 capped at h0)
 *   rows of ((int)(64 sx) + 4 capped at w0) * ch + 30 bytes, rounded down to whole 16-byte vectors — it is staged in LDS with aligned 16-byte
 *   loads, otherwise (or with the probe knob "letterbox_direct") every tap is a clamped global load: any scale works.  No load leaves
 *   the frame's h0 * pitch bytes.  The host guarantees (icafusion_amd/ops.py validates): offset % 16 == 0, pitch >= w0 * ch,
 *   offset + h0 * pitch inside the arena, top + nh <= H, left + nw <= W; W % 16 == 0, arena and dst 16-byte aligned.
 * icaf_scale_detections: scale_coords + clip_coords (utils/general.py:386-407) of an NMS output block on the device.  det
 *   [B][max_det][6], count [B], scale [B][5] = {gain, pad_x, pad_y, w0, h0} (device rows, as icaf_match_predictions takes them);
 *   out [B][max_det][6] may alias det.  Rows < count[b]: x = clamp((x - pad_x) / gain, 0, w0), y likewise with pad_y / h0 (an IEEE
 *   division; the SAME device function icaf_match_predictions maps its boxes with), round != 0: then round-half-even (torch.round);
 *   conf and cls copied.  Rows >= count[b] are written as zeros. */
enum { ICAF_LETTERBOX_LDS_BYTES = 20480 };
typedef struct icaf_frame_geom {
    long long offset;      /* first byte of the frame in the arena (16-byte aligned) */
    int h0, w0;            /* native size */
    int pitch, ch;         /* bytes per row (>= w0 * ch); interleaved channels: 3 or 1 */
    int nh, nw;            /* resized size (letterbox's new_unpad) */
    int top, left;         /* where the resized block starts in the H x W output */
    float sx, sy;          /* w0 / nw, h0 / nh rounded to fp32 */
} icaf_frame_geom;
int icaf_letterbox_frames(const void* arena, const icaf_frame_geom* geom, int nstreams, int B, void* dst, int ctot, int H, int W,
                          int swap_rb, icaf_stream_t s);
int icaf_scale_detections(const float* det, const int* count, int B, int max_det, const float* scale, int round, float* out,
                          icaf_stream_t s);

/* ---- native YUV 4:2:0 camera frames (utils/datasets.py: yuv420_to_bgr, then letterbox) ----------------------------------------
 * icaf_letterbox_yuv_frames: icaf_letterbox_frames for the surfaces a video decoder delivers (NV12 / NV21: a Y plane and one plane of
 *   interleaved chroma; I420 / YV12: three planes), byte for byte equal to letterbox(yuv420_to_bgr(y, cb, cr, matrix)) followed by the
 *   BGR -> RGB planes: CONVERT AT NATIVE RESOLUTION, THEN LETTERBOX.  arena, dst, nstreams, B, ctot, H, W, the grid, the 32 x 64 tile, the
 *   alignment rules, the refusals and "every byte of the planes written exactly once, 114 outside the block" are icaf_letterbox_frames';
 *   geom: DEVICE table of nstreams * B 80-byte rows, entry modality * B + image.
 *   kind 0: g is exactly icaf_letterbox_frames' row (ch 3 or 1) and the tile produces exactly its bytes, swap_rb included; the other
 *     fields are not read.  A thermal stream that arrives as NV12 is such a row on its Y plane (offset, pitch, ch 1): luma taken as is.
 *   kind 1: g.offset / g.pitch describe the Y plane (h0 rows, g.ch is 1); the chroma planes hold ceil(h0 / 2) rows of ceil(w0 / 2) samples,
 *     sample (i, j) of Cb at arena byte cb_offset + i * c_pitch + j * c_step, of Cr likewise from cr_offset; c_step 2 is interleaved
 *     chroma (the two offsets one byte apart), c_step 1 planar.  Pixel (y, x) uses chroma sample (y >> 1, x >> 1): nearest replication,
 *     no chroma filtering; odd h0 / w0 are legal.  swap_rb is not read: planes [3m, 3m + 3) are always R, G, B.
 *     Each of the four bilinear taps of an output pixel is converted to three bytes, then icaf_letterbox_frames' fp32 tap arithmetic
 *     (s, i0, frac, top, bot, out, floor(out + 0.5f), clip) runs on those bytes per channel.  Conversion in 32-bit integers, >> an
 *     arithmetic (flooring) shift, clip8 clamping to 0..255, c = Y - 16, d = Cb - 128, e = Cr - 128:
 *       matrix 0, BT.601 limited range:  R = clip8((298 c + 409 e + 128) >> 8)   G = clip8((298 c - 100 d - 208 e + 128) >> 8)
 *                                        B = clip8((298 c + 516 d + 128) >> 8)
 *       matrix 1, BT.709 limited range:  R = clip8((298 c + 459 e + 128) >> 8)   G = clip8((298 c - 55 d - 136 e + 128) >> 8)
 *                                        B = clip8((298 c + 541 d + 128) >> 8)
 *       matrix 2, BT.601 full range (JFIF):  R = clip8(Y + ((91881 e + 32768) >> 16))   G = clip8(Y + ((-22554 d - 46802 e + 32768) >> 16))
 *                                            B = clip8(Y + ((116130 d + 32768) >> 16))
 *   Budget rule of a kind-1 row: with rows = (int)(32 sy) + 4 capped at h0 and cols = (int)(64 sx) + 4 capped at w0 (the luma rectangle a
 *   tile can tap), crows = rows / 2 + 1 capped at ceil(h0 / 2) and ccols = cols / 2 + 1 capped at ceil(w0 / 2) (the chroma samples under
 *   it), a tile stages rows luma rows of (cols + 30) / 16 vectors and, for c_step 2, crows rows of (2 ccols + 30) / 16 vectors, for c_step 1
 *   twice crows rows of (ccols + 30) / 16 vectors (16-byte vectors, integer divisions) if that fits ICAF_YUV_LDS_BYTES and sx, sy < 1024;
 *   otherwise, or with the probe knob "letterbox_direct", every tap is three clamped global byte loads.  Staging reads aligned 16-byte
 *   vectors where they lie inside a plane and single bytes where a vector crosses a plane's first or last byte (chroma planes need no
 *   alignment).  No load leaves the h0 * pitch bytes of the Y plane or the bytes from a chroma plane's first sample to its last.
 *   The host guarantees (icafusion_amd/ops.py validate_yuv_frames): everything icaf_letterbox_frames asks of g; for kind 1 also ch == 1,
 *   c_step 1 or 2, c_pitch >= ceil(w0 / 2) * c_step, both chroma planes inside the arena, |cb_offset - cr_offset| == 1 for c_step 2,
 *   matrix 0..2. */
enum { ICAF_YUV_LDS_BYTES = 40960 };     /* a 1080 x 1920 NV12 frame letterboxed to 640 (3 x) stages: (100 * 14 + 51 * 14) vectors = 33,824 bytes */
typedef struct icaf_yuv_geom {
    icaf_frame_geom g;     /* kind 0: exactly icaf_letterbox_frames' row (ch 3 or 1).  kind 1: offset / pitch describe the Y plane, ch is 1 */
    long long cb_offset, cr_offset;   /* first Cb / Cr byte in the arena */
    int c_pitch, c_step;   /* bytes per chroma row; bytes between chroma samples: 2 = interleaved (NV12: cr = cb + 1, NV21: cb = cr + 1), 1 = planar (I420 / YV12) */
    int matrix, kind;
} icaf_yuv_geom;           /* 80 bytes */
int icaf_letterbox_yuv_frames(const void* arena, const icaf_yuv_geom* geom, int nstreams, int B, void* dst, int ctot, int H, int W,
                              int swap_rb, icaf_stream_t s);

/* ---- calibrated RGB / IR pairs (utils/datasets.py: warp_perspective, then letterbox) -----------------------------------------
 * icaf_letterbox_warp_frames: icaf_letterbox_frames for a pair whose two cameras are registered by a homography, byte for byte equal
 *   to letterbox(warp_perspective(frame, m, (h0, w0), border)): WARP AT THE TAPS, the aligned frame never exists in memory.  arena, dst,
 *   nstreams, B, ctot, H, W, the grid, the 32 x 64 tile, the alignment rules, the refusals and "every byte of the planes written exactly
 *   once, 114 outside the block" are icaf_letterbox_frames'; geom: DEVICE table of nstreams * B 104-byte rows, entry modality * B + image.
 *   kind 0: g is exactly icaf_letterbox_frames' row and the tile produces exactly its bytes (the same device function), swap_rb
 *     included; the other fields are not read.
 *   kind 1: g.h0 / g.w0 are the ALIGNED size (the other modality's native size) and nh / nw / top / left / sx / sy its letterbox;
 *     g.offset / g.pitch / g.ch describe the SOURCE frame of hs x ws pixels.  The letterbox's four taps of an output pixel are ALIGNED
 *     pixels (y, x), its clamped tap indices; each is evaluated from the source and rounded to a byte per channel, then
 *     icaf_letterbox_frames' fp32 tap arithmetic runs on those bytes.  Aligned pixel (x, y), all fp32, every operation rounded on its
 *     own (built with fp contraction off), m row-major and mapping aligned -> source pixel coordinates (integers are pixel centres):
 *       X = (m[0] x + m[1] y) + m[2], Y = (m[3] x + m[4] y) + m[5], Z = (m[6] x + m[7] y) + m[8], u = X / Z, v = Y / Z (IEEE divisions);
 *       ok = Z > 0 && u > -1 && u < ws && v > -1 && v < hs (false on NaN); not ok: the pixel is `border` in every channel;
 *       i0 = floor(u), fu = u - i0, j0 / fv likewise; a tap (j, i) inside the source frame is its byte, a tap outside is `border`;
 *       top = a00 (1 - fu) + a01 fu, bot likewise, out = top (1 - fv) + bot fv, the byte floor(out + 0.5f) clipped to 0..255.
 *     A pixel's coordinates are computed once for its channels; a letterbox tap whose weight is +0 is not evaluated (it adds +0).
 *     `border` fills aligned pixels the source does not cover; the padding outside the resized block stays 114.
 *   Stage rule of a kind-1 tile: the aligned rectangle the tile's resized pixels tap (lb_tap at its first and last resized row and
 *   column: first index of the first, second index of the last) has four corners; each is warped by the rule above.  If all four have
 *   Z > 0 and finite u, v, the box [floor(min u) - 1, floor(max u) + 2] x [floor(min v) - 1, floor(max v) + 2] (fp32), cut to the frame,
 *   is not empty and its rows of (ncols * ch + 30) / 16 16-byte vectors fit ICAF_WARP_LDS_BYTES, the box is staged in LDS with aligned
 *   16-byte loads (single bytes in the frame's last, partial vector) and taps read LDS; a tap outside the box reads global memory, so the
 *   bytes do not depend on the box.  Otherwise, or with the probe knob "letterbox_direct", every in-frame tap is a global byte load.  No
 *   load leaves the source frame's hs * pitch bytes.
 *   The host guarantees (icafusion_amd/ops.py validate_warp_frames): kind 0 rows as icaf_letterbox_frames asks; kind 1: ch 1 or 3,
 *   hs, ws, h0, w0, nh, nw >= 1, pitch >= ws * ch, offset % 16 == 0, offset + hs * pitch inside the arena, the block inside H x W,
 *   sx, sy > 0, border 0..255, nine finite matrix entries. */
enum { ICAF_WARP_LDS_BYTES = 20480 };    /* a 512 x 640 grey source under a 1080 x 1920 aligned frame letterboxed to 640 stages about 52 rows of 6 vectors: 5 KB */
typedef struct icaf_warp_geom {
    icaf_frame_geom g;     /* kind 0: exactly icaf_letterbox_frames' row.  kind 1: h0 / w0 = the ALIGNED size, nh / nw / top / left / sx / sy its
                              letterbox; offset / pitch / ch describe the SOURCE frame */
    int kind;              /* 0 plain, 1 warped */
    int hs, ws;            /* source size (kind 1) */
    int border;            /* 0..255 */
    float m[9];            /* row-major, aligned -> source */
    int reserved;
} icaf_warp_geom;          /* 104 bytes */
int icaf_letterbox_warp_frames(const void* arena, const icaf_warp_geom* geom, int nstreams, int B, void* dst, int ctot, int H, int W,
                               int swap_rb, icaf_stream_t s);

/* ---- 16-bit thermal frames (utils/datasets.py: agc_window, agc_u16_to_u8, then letterbox) ---------------------------------------
 * Uncooled LWIR cameras deliver 14- or 16-bit raw counts (Y16).  Automatic gain control picks a window [lo, hi] from the frame's
 * histogram and maps it linearly onto 0..255; both steps are stated here in integers, no floating point anywhere in them.
 *   Frame: h0 x w0 little-endian uint16; g.pitch in BYTES, even, >= 2 * w0; g.offset 16-byte aligned; g.ch is 1.
 *   Window (mode 1), clip_lo / clip_hi in basis points, 0..4999: n = h0 * w0, C(v) = pixels <= v, D(v) = pixels >= v;
 *     lo = the smallest v with 10000 * C(v) > clip_lo * n, hi = the largest v with 10000 * D(v) > clip_hi * n (64-bit products, both
 *     inequalities strict; clip (0, 0) gives the frame's minimum and maximum; clip_lo + clip_hi < 10000 implies lo <= hi).  Row padding
 *     never enters the histogram.  Mode 0: the caller's (lo, hi), 0 <= lo <= hi <= 65535, taken as is.
 *   Mapping: d = max(hi - lo, 1), out(v) = min(255, ((max(v, lo) - lo) * 255 + (d >> 1)) / d), a flooring integer division, no special
 *     cases: v <= lo gives 0, v >= hi gives 255 when hi > lo, a flat frame maps to 0.  The numerator x is at most 65535 * 255 + 32767 <
 *     2^24.  The kernels multiply instead of dividing: with m = 2^40 / d + 1 (flooring), m * d = 2^40 + e with 1 <= e <= d, so
 *     x * m / 2^40 = x / d + x * e / (d * 2^40); x = q * d + r with r <= d - 1 leaves a gap of at least 1 / d to q + 1, and
 *     x * e / (d * 2^40) < 1 / d because x * e < 2^24 * 2^16: (x * m) >> 40 == x / d for every numerator and divisor in range, and
 *     x * m < 2^24 * (2^40 + 1) fits 64 bits.
 *   Composition: MAP AT NATIVE RESOLUTION, THEN LETTERBOX — the output equals letterbox(grey -> 3 planes of agc_u16_to_u8(frame, lo,
 *     hi)); each of the four bilinear taps of an output pixel is mapped to a byte, then icaf_letterbox_frames' fp32 tap arithmetic runs
 *     on those bytes.  The 8-bit thermal frame never exists in memory.
 * icaf_y16_window: fills window[nstreams * B][2] (DEVICE int32 lo, hi; entry modality * B + image) for every kind-1 row of geom: mode 0
 *   copies the row's lo / hi, mode 1 runs the select above.  Rows of kind 0 leave their entry untouched.  One workgroup per frame, two
 *   passes over it: 256 bins of v >> 8, then 256 bins of v & 255 inside the high byte that holds the lo rank and inside the one that
 *   holds the hi rank; every wave counts into its own LDS copy and equal values of a wave are counted with one addition.  Counts are
 *   integers: the result does not depend on the order of the additions.  No host synchronisation, nothing read back.
 * icaf_letterbox_y16_frames: icaf_letterbox_frames for tables that hold Y16 rows.  arena, dst, nstreams, B, ctot, H, W, the grid, the
 *   32 x 64 tile, the alignment rules, the refusals and "every byte of the planes written exactly once, 114 outside the block" are
 *   icaf_letterbox_frames'; geom: DEVICE table of nstreams * B 72-byte rows; window: the table icaf_y16_window filled (4-byte aligned).
 *   kind 0: g is exactly icaf_letterbox_frames' row (ch 3 or 1) and the tile produces exactly its bytes (the same device function),
 *     swap_rb included; the other fields and `window` are not read.
 *   kind 1: a Y16 frame, mapped with its row of `window` whatever its mode; the three planes hold the same bytes, swap_rb is not read.
 *   Budget rule of a kind-1 row: the MAPPED bytes are staged, so the rule is icaf_letterbox_frames' for a grey frame — with rows =
 *   (int)(32 sy) + 4 capped at h0 and cols = (int)(64 sx) + 4 capped at w0, a tile stages rows rows of (cols + 30) / 16 16-byte vectors
 *   if that fits ICAF_Y16_LDS_BYTES and sx, sy < 1024.  A staged vector is 16 pixels from a pixel index (row * pitch / 2 + column) that is
 *   a multiple of 16: two aligned 16-byte loads (single pixels where a load would cross the frame's last byte), each pixel mapped
 *   once while it is written to LDS.  Otherwise, or with the probe knob "letterbox_direct", every tap is one clamped 2-byte load plus
 *   the mapping.  No load leaves the frame's h0 * pitch bytes.
 *   The host guarantees (icafusion_amd/ops.py validate_y16_frames): everything icaf_letterbox_frames asks of g of a kind-0 row; for
 *   kind 1 ch == 1, offset % 16 == 0, pitch even and >= 2 * w0, offset + h0 * pitch inside the arena, the block inside H x W, mode 0 or
 *   1, clip_lo and clip_hi in 0..4999, 0 <= lo <= hi <= 65535 for mode 0. */
enum { ICAF_Y16_LDS_BYTES = 20480 };     /* the mapped bytes of a grey frame: icaf_letterbox_frames' own budget */
typedef struct icaf_y16_geom {
    icaf_frame_geom g;     /* kind 0: exactly icaf_letterbox_frames' row (ch 3 or 1).  kind 1: ch is 1, pitch in bytes over 2-byte pixels */
    int kind, mode;        /* kind 0 plain, 1 Y16; mode 0 = window (lo, hi) given, 1 = percentile */
    int lo, hi;            /* mode 0: the window */
    int clip_lo, clip_hi;  /* mode 1: basis points clipped at either end */
} icaf_y16_geom;           /* 72 bytes */
int icaf_y16_window(const void* arena, const icaf_y16_geom* geom, int nstreams, int B, int* window, icaf_stream_t s);
int icaf_letterbox_y16_frames(const void* arena, const icaf_y16_geom* geom, const int* window, int nstreams, int B, void* dst, int ctot,
                              int H, int W, int swap_rb, icaf_stream_t s);

/* ---- native validation frames(utils/datasets.py:1116-1122, load_image_rgb_ir: longest side to img_size, then letterbox's padding) ----
 * icaf_resize_frames: icaf_letterbox_frames with a resize mode per descriptor, so that one launch serves a rectangular validation batch
 *   that mixes frames that shrink, frames that grow and frames that are copied.  arena, geom (DEVICE table, 48-byte rows), dst, swap_rb
 *   and the rule "every byte of the planes written exactly once, 114 outside the block" are icaf_letterbox_frames'.  mode: DEVICE int
 *   array parallel to geom, or NULL = every row 0.
 *   mode 0: the bilinear arithmetic of icaf_letterbox_frames (the same device functions; sx / sy as there).
 *   mode 1: the pixel-area average of utils.datasets.resize_area_scalar, byte for byte; needs nh <= h0 and nw <= w0 (the host checks:
 *     icafusion_amd/ops.py resize_frames); sx / sy are not read.  Per axis s = n_in / (double)n_out on the device; output j covers
 *     [lo, hi) = [j * s, j * s + s) in fp64, the weight of source pixel px < n_in is (float)(max(min(hi, px + 1) - max(lo, px), 0) / s),
 *     pixels floor(lo) .. floor(lo) + (int)s + 1 are looked at and a weight of 0 is skipped.  Vertical pass first,
 *     v[o][x][c] = sum_h wy[o][h] * f[h][x][c] in ascending h, then the horizontal pass over v in ascending x: fp32 accumulator from 0,
 *     each product rounded to fp32 and then added (no FMA); result floor(out + 0.5f) clipped to 0..255.
 *   One workgroup per 32 x 64 output tile.  A mode-1 tile tabulates its weights in LDS (at most ICAF_RESIZE_MAX_TAPS per output, i.e.
 *   s < 7 on both axes) and works through its resized rows in sub-tiles of R rows: threads own four source byte columns of one output
 *   row and run the vertical taps down the frame (one aligned 32-bit load per tap where pitch % 4 == 0, bytes inside w0 * ch otherwise;
 *   no load leaves h0 * pitch), the fp32 v rows go to LDS, and after a barrier one lane per output column runs the horizontal taps from
 *   there.  R = min(32, ICAF_RESIZE_LDS_BYTES / (4 * F)), F = (min(w0, (int)(64 * s_x) + 2) * ch rounded up to 4) + 4 floats per v row.
 *   Descriptors with R < 2 or more taps than the tables hold — or every one, with the probe knob "area_direct" — take the direct path:
 *   the same operations in the same order without LDS, each horizontal tap recomputing its vertical sum from the frame. */
enum { ICAF_RESIZE_LDS_BYTES = 20480, ICAF_RESIZE_MAX_TAPS = 8 };
int icaf_resize_frames(const void* arena, const icaf_frame_geom* geom, const int* mode, int nstreams, int B, void* dst, int ctot, int H,
                       int W, int swap_rb, icaf_stream_t s);

/* ---- NMS (utils/general.py:518-607 + torchvision.ops.nms semantics) ----------------------------------------
 * pred: [B][rows][5+nc] fp32 (cx, cy, w, h, obj, cls...).  Per image: obj > conf filter, conf = obj*cls, best
 * class or multi-label expansion, optional class filter (host int array), top max_nms by score (stable),
 * class-offset boxes, greedy IoU suppression in descending score order (ties: ascending candidate index), first
 * max_det survivors.
 * det: [B][max_det][6] (x1,y1,x2,y2,conf,cls), count: [B], keep_idx: [B][max_det] = indices into the image's
 * candidate list exactly as torchvision.ops.nms would return them (may be NULL: one small launch less).
 * No candidate list and no full sort are materialised: the workspace (icaf_nms_workspace_bytes; 256-byte aligned, contents
 * irrelevant on entry) holds one 32-bit score key per candidate slot, per-image score histograms and per-chunk candidate counts;
 * only the score ranges the greedy walk actually reaches are gathered and sorted, in LDS (nms.hip).  Enqueues a memset and
 * 2-3 kernels on `s`; max_det <= 1024, nc <= 65535, class filter ids 0..255. */
/* Validation statistics of test.py:196-230 on the device, one workgroup per image: the NMS output block det
 * [B][max_det][6] / count[B] (letterboxed pixel space) is mapped to native image space with scale[b] = {gain, pad_x,
 * pad_y, w0, h0} (scale_coords + clip_coords, utils/general.py:386-407; NULL = already native), every detection is paired
 * with the best-IoU label of its class (labels [L][5] = cls, x1, y1, x2, y2 in native space, image b owning rows
 * [label_off[b], label_off[b+1])), and claims it in index order if its IoU exceeds iouv[0]:
 * correct[b][i][t] = claimed && iou > iouv[t] (uint8).  predn (optional) receives the native-space boxes [B][max_det][4]. */
int icaf_match_predictions(const float* det, const int* count, int B, int max_det, const float* labels, const int* label_off,
                           int max_labels_per_image, const float* scale, const float* iouv, int T, unsigned char* correct,
                           float* predn, icaf_stream_t s);
int icaf_nms_workspace_bytes(int B, long long rows, int nc, int multi_label, ICAF_HOST size_t* bytes);
int icaf_nms(const float* pred, int B, long long rows, int nc, float conf_thres, float iou_thres, int multi_label,
             int agnostic, ICAF_HOST const int* classes_host, int n_classes, int max_det, int max_nms, float max_wh,
             float* det, int* count, int* keep_idx, void* workspace, size_t workspace_bytes, icaf_stream_t s);
/* icaf_nms_ex: icaf_nms with the two modes of the reference that it cannot express; with labels = NULL (or max_labels = 0) and merge = 0 it
 * enqueues exactly what icaf_nms enqueues (icaf_nms is this call with those values) and the workspace is icaf_nms_workspace_bytes'.
 * APRIORI LABELS (utils/general.py:545-552; test.py --save-hybrid): labels [L][5] fp32 rows cls, cx, cy, w, h in the prediction's pixel space,
 *   label_off [B+1] int32 (both device memory): image b owns rows [label_off[b], label_off[b+1]), the convention of icaf_match_predictions, at
 *   most max_labels of them (the host-known capacity that sizes the workspace; rows beyond it are not read).  A label row is a candidate with
 *   obj = 1 and class confidence 1 for (int)cls, 0 for the other classes: it passes the obj test by construction (:543 runs before :546), then
 *   conf = obj * cls > conf_thres and the class filter like any row.  The label rows FOLLOW the image's prediction rows in candidate order —
 *   candidate row rows + r, slot (rows + r) * ncm + class with ncm = nc under multi_label and 1 otherwise — so "descending score, ties by
 *   ascending candidate index" holds unchanged and keep_idx indexes the concatenated candidate list.  The boxes are read where they lie; no
 *   concatenated tensor is built.  cls must be in [0, nc) (the host wrapper checks; the kernels skip such a row rather than index with it).
 * MERGE-NMS (:594-600, the reference's `merge = True`), after the walk, per image.  n = the image's candidates after the class filter and
 *   before the max_nms cap.  Unless 1 < n < 3000 the image's plain result stands, silently, as in the reference; merge with max_nms < 3000 is
 *   ICAF_ERR_ARG (the reference would merge over a truncated list).  For every kept box i and candidate j: hit = box_iou(boxes[i], boxes[j])
 *   > iou_thres on the class-offset boxes, fp32 without contraction in the order of :455-477 (areas, clamp(0), inter / (a1 + a2 - inter)), so
 *   every decision is bit-exact.  New box = sum_j hit * score_j * xyxy_j / sum_j hit * score_j over the un-offset xyxy.  THE SUMMATION RULE (the
 *   reference leaves the order to its BLAS): products and sums in fp64 (fp32 x fp32 is exact there); partial sum l, l = 0..63, takes the hits
 *   j = l, l + 64, l + 128, ... in ascending j from 0.0; the 64 partial sums are combined by v[l] += v[l ^ o] for o = 32, 16, 8, 4, 2, 1; each of
 *   the five sums is rounded to fp32 once and the division is fp32.  Two calls give the same bits.  redundant != 0 (:599-600): a kept box with
 *   fewer than two hits is removed; det, keep_idx and count are compacted in order, and the rows at or behind the new count hold what
 *   icaf_nms leaves there (the walk's plain rows up to its count, untouched memory behind).  No special case for degenerate boxes: a
 *   zero-area box has IoU NaN with every box, itself included, hence no hit and 0 / 0 = NaN coordinates, exactly as the reference.
 * `classes` is HOST memory (n_classes ints); every other pointer is device memory.  One more small kernel per mode on `s`. */
enum { ICAF_NMS_MERGE_LIMIT = 3000, ICAF_NMS_MAX_LABELS = 65536 };
typedef struct icaf_nms_args {
    const float* pred;        /* [B][rows][5+nc] */
    const int* classes;       /* HOST: class filter, n_classes ids in 0..255, or NULL */
    const float* labels;      /* [L][5] cls, cx, cy, w, h; NULL: none */
    const int* label_off;     /* [B+1] */
    float* det;               /* [B][max_det][6] */
    int* count;               /* [B] */
    int* keep_idx;            /* [B][max_det] or NULL */
    void* workspace;          /* icaf_nms_ex_workspace_bytes, 256-byte aligned */
    size_t workspace_bytes;
    long long rows;
    int B, nc;
    float conf_thres, iou_thres;
    int multi_label, agnostic;
    int n_classes, max_det;
    int max_nms, max_labels;
    float max_wh;
    int merge, redundant;
    int reserved;
} icaf_nms_args;
int icaf_nms_ex_workspace_bytes(ICAF_HOST const icaf_nms_args* a, ICAF_HOST size_t* bytes);
int icaf_nms_ex(ICAF_HOST const icaf_nms_args* a, icaf_stream_t s);

/* ---- KAIST log-average miss rate, per-image half (evaluation_script/evaluation_script.py:46-79, 119-179, 181-294, 478-497) ----------
 * The reference evaluator's nine passes (All / Day / Night on set-up 0, near / medium / far / none / partial / heavy on set-ups 1-6) share
 * their per-image work up to the set-up, so one launch matches every image under all seven set-ups; the FPPI sweep (:296-395, 432-475)
 * runs on the host (icafusion_amd/utils/missrate.py).
 * Set-ups (KAISTParams, :478-497): HtRng = [55,1e10] [115,1e10] [45,115] [1,45] [1,1e10] [1,1e10] [1,1e10], OccRng = {0,1} {0} {0} {0} {0} {1}
 *   {2}, IoU threshold 0.5, maxDets 1000, bndRng = 5, 5, 635, 507.
 * icaf_missrate_stage: one validation batch into the detection store.  predn [B][max_det][4] native-space xyxy and det [B][max_det][6]
 *   (score in column 4) as icaf_match_predictions leaves them, count [B], image_index [B] (DEVICE ints: the image's row in the store, i.e.
 *   frame - 1 of the result files).  Row i < min(count[b], max_det, cap) of dt[image_index[b]] becomes {x1, y1, x2 - x1, y2 - y1, score}:
 *   the subtraction in fp32 (as the result-file writer's), then widened to fp64; dt_count[image_index[b]] = that bound.  An index outside
 *   [0, I) writes nothing.  One launch, no host synchronisation.
 * icaf_missrate_match: one workgroup per image.  Labels in annotation order: gt_box [G][4] fp64 (x, y, w, h), gt_height [G] fp64,
 *   gt_occlusion [G], gt_ignore_base [G] (the file's `ignore`, 0 if absent), image i owning rows [gt_off[i], gt_off[i + 1]); detections
 *   dt [I][cap][5] fp64 (x, y, w, h, score; an image's rows in arrival order) and dt_count [I]; max_labels_per_image is the HOST's
 *   maximum of gt_off[i + 1] - gt_off[i].
 *   gt_ignore [G]: bit s = ignored in set-up s (:59-71): the base flag, or height < lo, height > hi, occlusion not in OccRng[s], x < 5,
 *     y < 5, x + w > 635 or y + h > 507.
 *   order [I][cap]: sorted position -> arrival index, descending score, equal scores in arrival order (np.argsort(-score, 'mergesort'),
 *     :129, :207); only the first 1000 positions are matched (:208).
 *   dt_gt [I][cap][7], dt_ignore [I][cap]: per sorted position and set-up the matched row of the label table or -1, and bit s = matched to
 *     an ignored label.  Labels are walked non-ignored first, then ignored, each group in annotation order (:205), with best = 0.5 (:229-250):
 *     a taken non-ignored label is skipped; the walk stops at the first ignored label once anything has matched; a label with iou < best
 *     is skipped; otherwise it is taken and best = iou.  Hence the maximal IoU >= 0.5 among the free non-ignored labels, the LATER label on a
 *     tie; failing that the FIRST ignored label with IoU >= 0.5 (not the best one).  Only a non-ignored match consumes its label (:257-258).
 *   IoU (:148-179) in fp64 without contraction: dx2 = dx + dw, iw = min(dx2, gx2) - max(dx1, gx1), zero overlap if iw <= 0, ih likewise,
 *     t = iw * ih, union = dw * dh for an ignored label and (dw * dh + gw * gh) - t otherwise, iou = t / union (IEEE division).
 *   Rows at or beyond dt_count[i] (and positions >= 1000) of the three per-detection outputs are left as they were; nothing is read or
 *   written outside the tables.  ICAF_ERR_UNSUPPORTED before any device call for more than ICAF_MISSRATE_MAX_LABELS labels in an image or
 *   cap > ICAF_MISSRATE_MAX_DET, ICAF_ERR_ARG for null pointers.  Scores must be finite (the host wrappers check before upload). */
enum { ICAF_MISSRATE_MAX_DET = 1024, ICAF_MISSRATE_KEEP = 1000, ICAF_MISSRATE_MAX_LABELS = 256, ICAF_MISSRATE_SETUPS = 7 };
int icaf_missrate_stage(const float* predn, const float* det, const int* count, const int* image_index, int B, int max_det, double* dt,
                        int* dt_count, int I, int cap, icaf_stream_t s);
int icaf_missrate_match(const double* gt_box, const double* gt_height, const int* gt_occlusion, const int* gt_ignore_base,
                        const int* gt_off, int I, int max_labels_per_image, const double* dt, const int* dt_count, int cap, int* order,
                        int* dt_gt, unsigned char* dt_ignore, unsigned char* gt_ignore, icaf_stream_t s);

/* ---- Confluence suppression (utils/confluence.py:50-193; the reference's alternative to NMS, test.py:139-140) ----------------------
 * confluence (:109-193), per class 0 .. nc-1 on a candidate list [x1, y1, x2, y2, conf, cls] (fp32 values, arithmetic in fp64), candidates of a
 * class in their original order; while any is alive:
 *   p(i, j) (:141-162): lo / hi = min / max of i.x1, i.x2, j.x1, j.x2, every value normalised on its own as (v - lo) / (hi - lo) (one
 *     subtraction, one IEEE division), likewise y; p = ((|n(i.x1) - n(j.x1)| + |n(i.x2) - n(j.x2)|) + |n(i.y1) - n(j.y1)|) + |n(i.y2) - n(j.y2)|.
 *     hi == lo gives NaN: such a pair is no neighbour and never suppresses.
 *   value(i) (:166-173) = min over the alive j != i with p(i, j) < 2 of p(i, j) / conf_i, 0 when there is none.
 *   pick (:133-178) = the first i whose value is below a running minimum starting at 10000; the reference crashes when no value is, hence
 *     the PRECONDITION conf > 2e-4 on every candidate (p < 2, so p / conf < 10000).  Here a value that is not below 10000 counts as 10000
 *     and the lowest alive index wins among those: the launch always ends.  conf must be positive.
 *   remove (:180-190) the pick and every alive j with p(pick, j) < p_thres (strict; p_thres is the reference's Python float: a double).
 * The result is the picked candidates in ascending candidate index (np.unique, :192).
 * The select entry point — cand [B][max_cand][6] fp32, n [B] (device): det [B][max_cand][6] receives the kept rows in ascending candidate
 *   index and zeros behind them, count [B] their number, keep_idx [B][max_cand] (may be NULL) their candidate indices and -1 behind them.  Rows
 *   whose class is not an integer in [0, nc) are never kept (no class loop of the reference visits them).  n[b] < 0 counts as 0; n[b] > max_cand
 *   refuses the image as below.  Rows of cand at or beyond n[b] are never read.  Two kernels on `s`: one workgroup per (image, class) with its
 *   members in LDS, then one per image; det doubles as scratch in between.
 * The whole path (confluence_process, :50-106) — pred [B][rows][5+nc] fp32 (cx, cy, w, h, obj, cls...): obj > conf_thres, conf = cls * obj
 *   (fp32), xywh -> xyxy (fp32), one candidate per (box, class) with conf > conf_thres in row-major order (for nc == 1 the best-class branch
 *   of :89-91 is the same list); no class offset, no max_nms, no max_det.  Then the select.  The reference has no cap and a silent top-k would
 *   be another algorithm, so an image with more than max_cand candidates is REFUSED, not truncated: count[b] = -(its candidate number), its
 *   det rows zero; the other images of the batch are unaffected and the host decides.  conf_thres < 2e-4 is ICAF_ERR_ARG (the precondition
 *   above).  Workspace: icaf_confluence_workspace_bytes, 256-byte aligned, contents irrelevant on entry (the candidate list and the initial
 *   sweep's minimum / neighbour per candidate).  Four kernels on `s`, no host synchronisation.
 * ICAF_CONFLUENCE_MAX_CAND = 4096: a class's members stay in the LDS of one CU for all its picks at 35 bytes each (box 16, value 8, conf 4,
 *   neighbour 2, candidate index 2, re-sweep list 2, alive 1): 140 KiB of the 160 KiB; candidate and member indices fit 16 bits.
 * ICAF_ERR_ARG for null pointers, B / nc / rows < 1, max_cand outside [1, ICAF_CONFLUENCE_MAX_CAND], a NaN p_thres, a short or misaligned
 *   workspace. */
enum { ICAF_CONFLUENCE_MAX_CAND = 4096 };
int icaf_confluence_select(const float* cand, const int* n, int B, int max_cand, int nc, double p_thres, float* det, int* count,
                           int* keep_idx, icaf_stream_t s);
int icaf_confluence_workspace_bytes(int B, long long rows, int nc, int max_cand, ICAF_HOST size_t* bytes);
int icaf_confluence(const float* pred, int B, long long rows, int nc, float conf_thres, double p_thres, int max_cand, float* det,
                    int* count, int* keep_idx, void* workspace, size_t workspace_bytes, icaf_stream_t s);

/* ---- Validation loss: the forward value of ComputeLoss (utils/loss.py:325-463; test.py:112,132-133,364-367) -------------------------
 * The box / objectness / class loss of a batch from the raw Detect maps p[i] [B][na][ny_i][nx_i][5+nc] fp32 and the target table [nt][6] fp32
 * (image, class, x, y, w, h; normalised) — the VALUE only: no gradient is computed and nothing is kept for one.
 * Target assignment (build_targets, :409-463), level i, gain = [nx_i, ny_i, nx_i, ny_i] (p[i].shape[[3, 2, 3, 2]]), separate fp32 operations
 *   in the reference's order: t = targets * gain; r = t.wh / anchors[i][a]; target t joins anchor a when max(r, 1 / r).max() < anchor_t (fp32);
 *   gxy = t.xy, gxi = gain.xy - gxy; j, k = (gxy % 1. < 0.5) & (gxy > 1.), l, m likewise on gxi; the row is repeated for the offsets
 *   off = {(0, 0), (0.5, 0), (0, 0.5), (-0.5, 0), (0, -0.5)} that hold (the first always); gij = (gxy - off).long() truncates.
 * SLOT LAYOUT: level i has 5 * na * nt slots, slot index (off * na + a) * nt + t; a slot is valid or not.  The valid slots of a level in slot
 *   order are the reference's rows in the reference's order (targets.repeat(na, 1, 1)[j] is (anchor, target)-major, t.repeat((5, 1, 1))[j]
 *   puts the offset outermost).  A slot record is ICAF_LOSS_SLOT_INTS = 10 32-bit words {valid, b, a, gj, gi, tbox[4] (fp32 bits), tcls}, zeros
 *   when not valid; level i's records start at slots_off[i] of the workspace.
 * CLAMP TRAP: :457 clamps gj / gi in place on views of gij, so tbox = gxy - gij (:458) uses the CLAMPED indices (a centre at x or y = 1.0).
 * Per valid slot (:362-388), in fp64 on the fp32 logits: pxy = sigmoid * 2 - 0.5, pwh = (sigmoid * 2)^2 * anchor, CIoU against tbox
 *   (bbox_iou(x1y1x2y2=False, CIoU=True), utils/general.py:410-452, eps 1e-7); lbox = sum over levels with a match of mean(1 - iou); for nc > 1
 *   lcls = sum over those levels of mean over matches x classes of BCE-with-logits(pos_weight cls_pw) against cn everywhere, cp at tcls.
 * Objectness: tobj[b, a, gj, gi] = (1 - gr) + gr * max(iou, 0) (fp32).  DUPLICATE RULE: several slots may hit one cell; the reference sorts by
 *   iou ascending before the scatter (:379-382), so the LARGEST value stays — here an integer atomic max on the float's bits into the zeroed
 *   dense map, which needs non-negative values: gr outside [0, 1] is refused.  lobj = sum_i balance[i] * mean(BCE-with-logits(p_i[..., 4],
 *   tobj_i; pos_weight obj_pw)); level i's tobj map [B][na][ny_i][nx_i] fp32 starts at tobj_off[i] of the workspace.
 * out[4] = {lbox * box, lobj * obj, lcls * cls, 0} fp32 (the rank loss is never accumulated, :391), counts[nl] the matches per level.  Sums are
 *   fp64, two-stage, in a fixed order (no float atomics): two calls on the same inputs give the same bits.  anchors [nl][na][2] (grid units) and
 *   prm are HOST memory; maps is a host array of nl device pointers; everything else lives on the device.  anchor_t is compared in fp32.
 * Departures: a target whose image index is outside [0, B) is skipped and a class outside [0, nc) marks no positive (the reference raises).
 * REFUSALS, all before any launch, outputs and workspace untouched, nothing is ever truncated: ICAF_ERR_UNSUPPORTED for nl outside [1, 5], na
 *   outside [1, 8], nt > ICAF_LOSS_MAX_TARGETS = 4096, a level of more than 2^31 cells; ICAF_ERR_ARG for null pointers (a null map included),
 *   nc < 1, B < 1, nt < 0, an empty map, gr outside [0, 1] (NaN included), a short or misaligned workspace.  nt = 0 is valid (:444-446):
 *   lbox = lcls = 0 and lobj against an all-zero tobj.  Workspace: icaf_loss_workspace_bytes (tobj_off / slots_off [nl], bytes from its start,
 *   may be NULL; tobj_off does not depend on nt), 256-byte aligned, contents irrelevant on entry (the call zeroes its own tobj).  One memset
 *   and three kernels on `s`, no host synchronisation. */
enum { ICAF_LOSS_MAX_LEVELS = 5, ICAF_LOSS_MAX_ANCHORS = 8, ICAF_LOSS_MAX_TARGETS = 4096, ICAF_LOSS_SLOT_INTS = 10 };
typedef struct icaf_loss_params {
    double box, obj, cls, cls_pw, obj_pw, anchor_t, gr, cp, cn, balance[5];
} icaf_loss_params;
int icaf_loss_workspace_bytes(int nl, ICAF_HOST const int* ny, ICAF_HOST const int* nx, int B, int na, int nt, ICAF_HOST size_t* bytes, ICAF_HOST size_t* tobj_off, ICAF_HOST size_t* slots_off);
int icaf_loss(ICAF_HOST const float* const* maps, ICAF_HOST const int* ny, ICAF_HOST const int* nx, int nl, int B, int na, int nc, ICAF_HOST const float* anchors,
              const float* targets, int nt, ICAF_HOST const icaf_loss_params* prm, float* out, int* counts, void* workspace, size_t workspace_bytes,
              icaf_stream_t s);

/* ---- Validation statistics: store, ap_per_class, ConfusionMatrix (test.py:144-230, 287-321; utils/metrics.py:18-82, 85-110, 113-159) ---
 * icaf_stats_stage (test.py:198-230, the `stats.append` of every image): one validation batch into a data-set-wide store.  correct [B][max_det][T]
 *   uint8 as icaf_match_predictions leaves it, det [B][max_det][6], count [B].  Row i < min(max(count[b], 0), max_det) of image b lands at
 *   cursor + (rows of the images before b) + i: image order, then row order.  store_mask [capacity] uint16 (bit t = correct[b][i][t] != 0),
 *   store_conf [capacity] fp32 (det column 4), store_cls [capacity] int32 ((int) of det column 5); cursor [1] int32 is advanced by the batch's
 *   rows, any_tp [1] int32 becomes 1 if any stored bit is set.  One launch of one workgroup: it forms the prefix, reads and advances the cursor,
 *   so no atomic decides an order; calls on one stream append in call order.  Nothing is written at or beyond `capacity`: a batch that does not
 *   fit still advances the cursor past the capacity (the host sees the overflow), after which every further call writes nothing.  Rows of
 *   correct / det at or beyond count[b] are never read.  ICAF_ERR_UNSUPPORTED before any launch: T outside [1, ICAF_STATS_MAX_T], capacity
 *   outside [1, ICAF_STATS_MAX_ROWS], B outside [1, ICAF_STATS_MAX_BATCH].
 * icaf_ap_per_class (utils/metrics.py:18-82 with compute_ap, :85-110): mask / conf / cls [n] as the store holds them, unique_classes [nc] int32
 *   (DEVICE; ascending, from the labels) and n_l [nc] int32 (DEVICE; their label counts); all arithmetic the reference does in float64 is fp64
 *   without contraction, in its operation order.
 *   ORDER (the reference's np.argsort(-conf) leaves ties to the numpy build): class ascending, confidence descending, equal confidences in
 *     arrival order — a stable LSD radix sort over the bit pattern of the fp32 confidence and one 8-bit class pass, ICAF_STATS_SORT_TILE rows
 *     per workgroup.  PRECONDITIONS: conf finite and >= 0, classes in [0, 256) (a class outside is sorted as 0 / 255).  perm [n] (may be NULL)
 *     receives the arrival index of every sorted position.
 *   Per class ci with predictions and labels: tpc[t][i] the inclusive count of bit t over the class's rows (workspace, at tpc_off: int32 [T][n]
 *     indexed by sorted position; fpc = (row in class + 1) - tpc); recall = tpc / (n_l + 1e-16), precision = tpc / (tpc + fpc);
 *     r[ci] = interp(-px, -conf, recall[:, 0], left = 0), p[ci] likewise with left = 1, px = linspace(0, 1, 1000); ap[ci][t] = trapezoid sum in
 *     index order of interp(linspace(0, 1, 101), [0, recall, recall[-1] + 0.01], envelope([1, precision, 0])).  interp is np.interp: below xp[0]
 *     `left`, above xp[-1] fp[-1], otherwise j = the LARGEST index with xp[j] <= x and fp[j] if j is the last index or xp[j] == x, else
 *     ((fp[j+1] - fp[j]) / (xp[j+1] - xp[j])) * (x - xp[j]) + fp[j].  A class without predictions (or with n_l <= 0) keeps zero rows; predictions
 *     of a class that is not in unique_classes are ignored.
 *   f1 = 2 p r / (p + r + 1e-16); best [1] = the first argmax over the 1000 points of the class mean (classes summed in order, then divided);
 *     report [nc][3] fp64 = {tp, fp, fn} at that index: tp = rint(r * n), fn = n - tp, fp = rint(tp / (p + 1e-16) - tp) with n = n_l[nc - 1]
 *     for EVERY class (the reference's loop variable, :45, read after the loop, :78-80), rounding half to even.
 *   Outputs ap [nc][T], p / r / f1 [nc][1000] fp64.  Integer scans and fixed-order sums: two calls give the same bits.  n = 0 is valid.
 *   ICAF_ERR_UNSUPPORTED before any launch: nc > ICAF_STATS_MAX_CLASSES, T outside [1, ICAF_STATS_MAX_T], n > ICAF_STATS_MAX_ROWS;
 *   ICAF_ERR_ARG for null pointers, nc < 1, a short or misaligned (256 bytes) workspace (icaf_ap_workspace_bytes; contents irrelevant on entry).
 * icaf_confusion_matrix (ConfusionMatrix.process_batch, :121-159), one workgroup per image, integer atomics into matrix [(nc+1)][(nc+1)] int32
 *   (accumulated, never cleared here; rows = predicted class, columns = true class, index nc = background).  predn [B][max_det][4] native-space
 *   boxes as icaf_match_predictions writes them, det (conf column 4, class column 5), count, labels [L][5] (cls, x1, y1, x2, y2), label_off [B+1].
 *   Detections with conf > `conf` (fp32) are kept, classes truncated to int; (label, detection) is a candidate when the fp32 box_iou
 *   (utils/general.py:455-477: inter / (area_label + area_det - inter)) is > iou_thres; every detection keeps its highest-IoU label, every label
 *   the highest-IoU detection among those that chose it; a matched label adds matrix[cls(det)][cls(label)], an unmatched one
 *   matrix[nc][cls(label)]; ONLY IF the image has a match, every kept detection that matched no label adds matrix[cls(det)][nc] (the
 *   reference's `if n:`).  IoU TIES: the reference's order comes from an unstable argsort; here the lowest label index wins, then the lowest
 *   detection index.  An image with no detections or no labels contributes nothing (test.py never calls process_batch for it).  A class outside
 *   [0, nc) adds nothing (the reference raises).  Bounds come from count / label_off only; rows at or beyond count[b] are never read.
 *   max_det above 1024 is ICAF_ERR_UNSUPPORTED. */
enum { ICAF_STATS_MAX_T = 16, ICAF_STATS_MAX_ROWS = 16777216, ICAF_STATS_MAX_CLASSES = 256, ICAF_STATS_MAX_BATCH = 4096,
       ICAF_STATS_SORT_TILE = 4096, ICAF_AP_CURVE_POINTS = 1000 };
int icaf_stats_stage(const unsigned char* correct, const float* det, const int* count, int B, int max_det, int T, void* store_mask,
                     float* store_conf, int* store_cls, int capacity, int* cursor, int* any_tp, icaf_stream_t s);
int icaf_ap_workspace_bytes(int n, int T, ICAF_HOST size_t* bytes, ICAF_HOST size_t* tpc_off);
int icaf_ap_per_class(const void* mask, const float* conf, const int* cls, int n, int T, const int* unique_classes, const int* n_l, int nc,
                      double* ap, double* p, double* r, double* f1, int* best, double* report, int* perm, void* workspace,
                      size_t workspace_bytes, icaf_stream_t s);
int icaf_confusion_matrix(const float* predn, const float* det, const int* count, int B, int max_det, const float* labels,
                          const int* label_off, int nc, float conf, float iou_thres, int* matrix, icaf_stream_t s);

/* ---- HIP graph capture / events (so the Python host never needs a tracing compiler) ------------------------ */
int icaf_graph_begin(icaf_stream_t s);
int icaf_graph_end(icaf_stream_t s, ICAF_HOST void** graph_exec);
int icaf_graph_launch(void* graph_exec, icaf_stream_t s);
int icaf_graph_destroy(void* graph_exec);
int icaf_event_create(ICAF_HOST void** ev);
int icaf_event_record(void* ev, icaf_stream_t s);
int icaf_stream_wait_event(icaf_stream_t s, void* ev);         /* hipStreamWaitEvent: fork / join of capture branches */
int icaf_event_elapsed_ms(void* start, void* stop, ICAF_HOST float* ms); /* synchronises on `stop` */
int icaf_event_destroy(void* ev);
int icaf_stream_sync(icaf_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* ICAF_H */
