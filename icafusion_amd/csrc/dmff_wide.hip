// DMFF block kernels for the WIDE levels (C = 256 / 512, 16-bit types) on gfx950 — one CrossTransformerBlock iteration (reference
// models/common.py:737-759, CrossAttention :641-687, MLP :704-709) as THREE launches:
//
//   dmff_wide_ln_qkv_kernel    LayerNorm (CrossAttention.LN1 / LN2, :661-662) + the six Linear(C, C) projections (:664-669); a workgroup
//                              = 64 rows x three passes of output channels, or ONE pass where the tiles alone do not fill the chip
//   cross_attn_kernel          (dmff.hip) softmax(q_other k^T / sqrt(dk)) v per (image, direction, head) (:670-681)
//   dmff_wide_proj_mlp_kernel  out-projection + coefficient mix (:682-685, :745-746), the block's shared LayerNorm (:749-750),
//                              MLP Linear(C, 4C) -> GELU(erf) -> Linear(4C, C) and the final mix (:704-709, :751-752)
//
// Why not the two-launch form of dmff_fused.hip: with C >= 256 its 64-row tile + K / V^T of two heads leave ONE four-wave
// workgroup per CU, and its weight stream — through LDS, one barrier per 16 KB slice — measured 1200-1850 cycles per slice against
// 256 cycles of MFMAs (phase clocks at batch 32; the same stream by LDS-DMA with a 4-stage ring and eight waves: still 1200: every
// MFMA needs two fragment reads, 64 KB of LDS reads per 16 KB slice).  Here the GEMMs are organised around what is scarce:
//   * the 64-row token tile is RESIDENT in LDS (read-only during a pass);
//   * EIGHT wavefronts, wave w owns output channels [32 w, 32 w + 32) of a 256-channel pass and BOTH 32-row halves of the tile:
//     one weight fragment feeds two MFMAs;
//   * the weights never touch LDS: a wave reads ITS fragments straight from L2 into registers, from a FRAGMENT-MAJOR copy of the
//     packed matrix ([Np/32][Kp/16][64 lanes][8 elements]: one coalesced 16-byte load per lane = one MFMA A operand), four K slices
//     (64 K elements each) ahead, as one continuous per-wave stream across the passes and phases of the kernel — no ring, no DMA
//     issue slots, NO barrier inside a pass;
//   * LDS traffic per 32 KB of weights: 64 KB of token-fragment reads (8 waves x 8 b128 reads), against 128 + 32 KB before.
// Rounding points are those of the per-layer launches (activations rounded to the storage type between layers, fp32 accumulate,
// two-pass LayerNorm statistics on the rounded values); only fp32 summation orders differ.
//
// Round 4 — hidden split (icaf_dmff_wide_proj_mlp_split): at P5 of yolov5s (C = 512, 100 tokens x 32 images) there are only 100 tiles
// of 64 rows for 256 CUs, and every workgroup streams all 4.7 MB of its modality's weights, which do not stay in a 4 MB L2: PMC showed
// 106 MB fetched per launch for 56.6 MB of distinct bytes and 53 GB/s per CU, the latency of the fabric.  With KS = 2 / 4 a tile is
// shared by KS workgroups, each owning 1/KS of the hidden columns (its slices of W1 and W2 — the XCDs of a modality are dealt over
// the hidden slices, so an XCD's L2 holds W_o + ONE slice: 2.6 MB at KS = 2); every one repeats the cheap front (out-projection +
// LayerNorm: 1/9 of the FLOPs), writes its fc2 partial sums in fp32, and a second, tiny launch (dmff_wide_reduce_kernel) adds the
// partials in FIXED order (deterministic, no atomics, no in-kernel fences: the agent-scope release / acquire of round 3's one-launch
// attempt emptied the L2 of the very weights being streamed) and applies bias + coefficient mix.
#include <type_traits>
#include "icaf_common.h"
#include "conv_common.h"
#include "wide_cursor.h"
#include "dmff_args.h"

namespace icaf {

struct WideP {
    const void* x;            // tokens [2][rows][C]: LN + QKV input / residual of the attention mix
    const void* att;          // proj_mlp: attention output [2][rows][C]
    float* part;              // hidden split: fc2 partial sums [KS][2][rows][C] fp32
    const float* x32;         // R32 (round 5): the token stream of the PREVIOUS iteration in fp32 [2][rows][C] (NULL: first iteration, x is all there is)
    float* y32;               // R32: this iteration's tokens in fp32 [2][rows][C] (the 16-bit y is written as well: LayerNorm + QKV read it)
    void* qkv;                // ln_qkv: [2][rows][3C]
    void* y;                  // proj_mlp: element (g, row, c) at y + g * y_gs + row * ldy + c
    const void* wqkv; const float* bqkv;      // FRAGMENT-MAJOR weights [2][Np/32][Kp/16][64][8]; biases fp32 [2][Np]
    const void* wo; const float* bo;
    const void* w1; const float* b1;
    const void* w2; const float* b2;
    const float* ln_a_g[2]; const float* ln_a_b[2];
    const float* ln_m_g; const float* ln_m_b;
    long long wqkv_gs, bqkv_gs, wo_gs, bo_gs, w1_gs, b1_gs, w2_gs, b2_gs, x_gs, y_gs;
    long long rows;
    int C, Kp, Kp4, hid, ldy;
    int qkv_npass;            // ln_qkv: passes (of WPASS output channels) per workgroup, 3 or 1
    float eps_a, eps_m;
    float c_res_a[2], c_acc_a[2], c_res_m[2], c_acc_m[2];
};

constexpr int WROWS = 64;            // token rows per workgroup
constexpr int WDEPTH = 4;            // slices in flight per wave (register ring; every pass is a multiple of it)
// Geometry of a build: NW wavefronts per workgroup, wave w owning output channels [32 w, 32 w + 32) of a pass of 32 NW channels, and
// SL MFMA K steps (16 elements each) per slice of the weight stream.
//   wide levels (C = 256 / 512):  NW = 8, SL = 4  -> 256-channel passes, 64-element slices
//   C = 128 (P3 of yolov5s):      NW = 4, SL = 2  -> 128-channel passes, 32-element slices (a pass over K = 128 is again 4 slices)
template <int NW_, int SL_> struct WG {
    static constexpr int NW = NW_, SL = SL_;
    static constexpr int WT = 64 * NW;           // threads per workgroup
    static constexpr int WPASS = 32 * NW;        // output channels per pass
    // (an MFMA K step is 32 BYTES of a row in every type: 16 elements of a 16-bit type, 8 of fp32 — the parity instantiation)
    template <int DT> static constexpr int kstep() { return 32 / Elem<DT>::BYTES; }          // K elements per MFMA step
    template <int DT> static constexpr int ksl() { return kstep<DT>() * SL; }                // K elements per slice
    template <int DT> static constexpr int nsl2() { return WPASS / ksl<DT>(); }              // slices of an fc2 pass over one hidden chunk
    static constexpr int TPR = WT / WROWS;       // threads per row in the tile LayerNorm
};
using WG8 = WG<8, 4>;
using WG4 = WG<4, 2>;

// One wave's weight stream.  A SEGMENT is one pass's fragments for this wave's 32 channels: n slices of WSL consecutive K steps,
// 64 lanes x 16 bytes each, contiguous in the fragment-major copy.  Which segment follows which, and where its slices lie, is the
// integer arithmetic of wide_cursor.h (checked on the host); `mats(m)` is the wave-uniform base of matrix m, the lane offset is added last.
//
// A refill is UNCONDITIONAL: WSL loads per slot, always, the cursor arithmetic behind them scalar code with no load in a branch.  With
// the refill in a branch (`if (left == 0) return;`, the first form of this file) the compiler could not count the loads younger than a slot and waited
// vmcnt(0) once per rotation — for the refill it had issued a few MFMAs earlier: a ring of four slices that held one (docs/HISTORY.md
// section 21).  Now a slot is waited for with (WDEPTH - 1) * WSL + (WSL - 1 - k) loads still travelling.  Past the end of the kernel's
// stream the cursor stays on its last valid slice: WDEPTH refills of an address already read, never consumed.
template <int WSL, class SEGS, class MATS>
__device__ __forceinline__ void wfetch(u32x4 (&w)[WSL], WCursor& c, const SEGS& segs, const MATS& mats) {
    const u32x4* b = mats(c.mat) + c.frag * 64 + (threadIdx.x & 63);
#pragma unroll
    for (int k = 0; k < WSL; ++k) w[k] = b[k * 64];
    wcursor_advance(c, WSL, segs);
}

// acc[t] += W[32 wn + i][k] * A[32 t + j][k] over the next n slices (n % WDEPTH == 0) of the wave's stream; A: LDS tile, row stride SA
template <int DT, int WSL, class SEGS, class MATS>
__device__ __forceinline__ void wpass(f32x16 (&acc)[2], const unsigned char* A, int SA, int n, u32x4 (&wq)[WDEPTH][WSL], WCursor& c, const SEGS& segs, const MATS& mats) {
    const int lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
    const unsigned char* a0 = A + (size_t)l31 * SA + hi * 16;
    const unsigned char* a1 = a0 + (size_t)32 * SA;
    int s = 0;
    do {                                         // (n >= WDEPTH: a loop that runs at least once tells the compiler that a load requested before the pass is
                                                 //  older than WDEPTH * WSL refills when the pass ends — its wait there is counted, the ring stays full)
#pragma unroll
        for (int u = 0; u < WDEPTH; ++u) {
#pragma unroll
            for (int k = 0; k < WSL; ++k) {
                const int off = ((s + u) * WSL + k) * 32;
                const u32x4 x0 = *(const u32x4*)(a0 + off);
                const u32x4 x1 = *(const u32x4*)(a1 + off);
                mma_step<DT>(acc[0], wq[u][k], x0);
                mma_step<DT>(acc[1], wq[u][k], x1);
            }
            wfetch<WSL>(wq[u], c, segs, mats);
            __builtin_amdgcn_sched_barrier(0);             // (left alone the scheduler hoists the token-fragment reads of all four slices: 128 registers)
        }
        s += WDEPTH;
    } while (s < n);
}

// LayerNorm of the 64 rows of an LDS tile in place: TPR (8 or 4) threads per row, two-pass statistics in fp32 on the stored values
// (the arithmetic of layernorm_kernel, dmff.hip).  gam / bet: C floats each IN LDS (the kernel's prologue fetched them with the tile: read from
// global memory here, inside the third loop, they cost one dependent round trip per iteration).
template <int DT, int TPR>
__device__ __forceinline__ void wide_tile_layernorm(unsigned char* tile, int S, int C, const float* gam, const float* bet, float eps) {
    using E = Elem<DT>;
    const int tid = threadIdx.x, row = tid / TPR, part = tid % TPR;
    const int nv = C / E::VEC;
    unsigned char* r = tile + (size_t)row * S;
    float s = 0.0f;
    for (int v = part; v < nv; v += TPR) {
        float t[E::VEC];
        unpack16<DT>(*(const u32x4*)(r + v * 16), t);
#pragma unroll
        for (int j = 0; j < E::VEC; ++j) s += t[j];
    }
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2);
    if constexpr (TPR == 8) s += __shfl_xor(s, 4);
    const float mean = s / (float)C;
    float q = 0.0f;
    for (int v = part; v < nv; v += TPR) {
        float t[E::VEC];
        unpack16<DT>(*(const u32x4*)(r + v * 16), t);
#pragma unroll
        for (int j = 0; j < E::VEC; ++j) { const float d = t[j] - mean; q += d * d; }
    }
    q += __shfl_xor(q, 1); q += __shfl_xor(q, 2);
    if constexpr (TPR == 8) q += __shfl_xor(q, 4);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
    for (int v = part; v < nv; v += TPR) {
        float t[E::VEC], o[E::VEC];
        unpack16<DT>(*(const u32x4*)(r + v * 16), t);
#pragma unroll
        for (int j = 0; j < E::VEC; ++j) o[j] = (t[j] - mean) * rstd * gam[v * E::VEC + j] + bet[v * E::VEC + j];
        *(u32x4*)(r + v * 16) = pack16<DT>(o);
    }
}

// workgroup id -> (modality, index): XCDs 0-3 take modality 0, XCDs 4-7 modality 1 (hardware deals consecutive ids round-robin
// over the 8 XCDs), so an XCD's L2 holds ONE modality's weights — at C = 512 that is 4.7 of the 9.4 MB of a block
__device__ __forceinline__ void wide_place(int bid, int& g, int& idx) { g = (bid & 7) >> 2; idx = (bid >> 3) * 4 + (bid & 3); }
// ... and with the hidden columns split KS ways, the 4 XCDs of a modality are dealt over the hidden slices: an XCD's L2 holds W_o and
// ONE slice of W1 / W2
template <int KS> __device__ __forceinline__ void wide_place_ks(int bid, int& g, int& ks, int& idx) {
    const int x = bid & 7, per = 4 / KS;            // XCDs per (modality, slice)
    g = x >> 2;
    ks = (x & 3) / per;
    idx = (bid >> 3) * per + (x & 3) % per;
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm + QKV projection: a workgroup = 64 token rows x three passes (768 output channels with eight wavefronts, 384 with
// four) of one modality.  grid = 8 * ceil(tiles * C / WPASS / 4)
// ---------------------------------------------------------------------------------------------------------------
// NT: 16-byte vectors of the token tile per thread (64 rows x C elements over the workgroup's threads: 4, or 8 at C = 512 and in fp32) — a
// compile-time count, so that the prologue is ONE batch of loads: the tile, then one quad of gamma | beta and one of this workgroup's biases
// per thread (from clamped indices, stored to LDS under the predicate), then the first WDEPTH weight slices; the LDS writes follow, waiting
// for the older loads only.  Read in a `for (i = tid; ...)` loop the tile cost one memory round trip per iteration, and the first of them
// drained the weight prefetch issued "to travel meanwhile".
template <int DT, class G = WG8, int NT = 4>
__global__ __launch_bounds__(G::WT) void dmff_wide_ln_qkv_kernel(const WideP p) {
    using E = Elem<DT>;
    using T = typename E::type;
    constexpr int VEC = E::VEC, EB = E::BYTES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int C = p.C, SA = C * EB + 16;
    unsigned char* tile = smem;
    float* lnp = (float*)(tile + (size_t)WROWS * SA);               // gamma [C], beta [C]
    float* bs = lnp + 2 * C;                                        // bias of this workgroup's passes [npass][WPASS]
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int npass = p.qkv_npass;                                    // 3: a workgroup writes q, k AND v columns of its group; 1: one pass each
    const int ngrp = 3 * (C / G::WPASS) / npass;                      // column groups per tile
    const int ntiles = (int)((p.rows + WROWS - 1) / WROWS);
    int g, idx;
    wide_place(blockIdx.x, g, idx);
    if (idx >= ntiles * ngrp) return;
    const int tile_i = idx / ngrp, grp = idx - tile_i * ngrp;
    const long long r0 = (long long)tile_i * WROWS;
    const int ks_row = p.Kp / G::template kstep<DT>(), nsl = C / G::template ksl<DT>();

    // ---- prologue: every global load of the workgroup's front in one batch, the weight ring last (youngest) ----
    u32x4 tl[NT];
    const int nv = C / VEC;
    {
        const T* xg = (const T*)p.x + g * p.x_gs;
#pragma unroll
        for (int it = 0; it < NT; ++it) {                            // raw tokens (rows beyond the tensor: clamped, never stored)
            const int i = tid + it * G::WT, row = i / nv, v = i - row * nv;
            long long r = r0 + row;
            r = r < p.rows ? r : p.rows - 1;
            tl[it] = *(const u32x4*)(xg + r * C + v * VEC);
        }
    }
    const int nlq = C / 2, nbq = npass * (G::WPASS / 4);             // quads of gamma | beta, of the workgroup's biases (both < threads)
    const int lqi = tid < nlq ? tid : nlq - 1, bqi = tid < nbq ? tid : nbq - 1;
    const f32x4 lq = *(const f32x4*)(lqi < C / 4 ? p.ln_a_g[g] + 4 * lqi : p.ln_a_b[g] + 4 * lqi - C);
    const f32x4 bq = *(const f32x4*)(p.bqkv + g * p.bqkv_gs + grp * npass * G::WPASS + 4 * bqi);

    const u32x4* wf = (const u32x4*)((const T*)p.wqkv + g * p.wqkv_gs);
    const WQkvSegs segs{npass, grp, G::NW, wn, ks_row, nsl};
    auto mats = [&](int) { return wf; };
    WCursor cur;
    wcursor_start(cur, G::SL, segs);
    u32x4 wq[WDEPTH][G::SL];
#pragma unroll
    for (int u = 0; u < WDEPTH; ++u) wfetch<G::SL>(wq[u], cur, segs, mats);      // the first weight slices travel while the tokens are normalised

#pragma unroll
    for (int it = 0; it < NT; ++it) {
        const int i = tid + it * G::WT, row = i / nv, v = i - row * nv;
        *(u32x4*)(tile + (size_t)row * SA + v * 16) = tl[it];
    }
    if (tid < nlq) *(f32x4*)(lnp + 4 * tid) = lq;
    if (tid < nbq) *(f32x4*)(bs + 4 * tid) = bq;
    lds_barrier();
    wide_tile_layernorm<DT, G::TPR>(tile, SA, C, lnp, lnp + C, p.eps_a);
    lds_barrier();

    const int nout = 3 * C;
    T* out = (T*)p.qkv + (long long)g * p.rows * nout;
    for (int j = 0; j < npass; ++j) {
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        wpass<DT, G::SL>(acc, tile, SA, nsl, wq, cur, segs, mats);
        const int nb = (grp * npass + j) * G::WPASS + wn * 32;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = nb + 8 * q + 4 * hi;
            const f32x4 b = *(const f32x4*)(bs + j * G::WPASS + wn * 32 + 8 * q + 4 * hi);      // (LDS: no global load inside the predicated store)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const long long row = r0 + t * 32 + l31;
                if (row < p.rows)
                    *(typename Quad<DT>::type*)(out + row * nout + n) =
                        pack4<DT>(acc[t][4 * q] + b[0], acc[t][4 * q + 1] + b[1], acc[t][4 * q + 2] + b[2], acc[t][4 * q + 3] + b[3]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// out-projection + LayerNorm + MLP: a workgroup = 64 token rows of one modality.  grid = 8 * ceil(tiles / 4)
// ---------------------------------------------------------------------------------------------------------------
// R32 (round 5, blocks with loops > 1): the residual chain x -> x_att -> x' stays in FP32 across iterations — x is read from p.x32 where it exists,
// x_att is kept (and parked) in fp32, x' is written to p.y32 beside the 16-bit y.  Without it every iteration rounds the token stream twice to the
// storage type, and three iterations had used up the 16-bit parity margin of the 3-iteration configuration (0.91 x the reference's own bf16 error).
template <int DT, int NPW, int KS = 1, class G = WG8, bool R32 = false>          // NPW = C / WPASS passes per C-wide product; KS = workgroups sharing a tile (hidden split)
__global__ __launch_bounds__(G::WT) void dmff_wide_proj_mlp_kernel(const WideP p) {
    using E = Elem<DT>;
    using T = typename E::type;
    constexpr int VEC = E::VEC, EB = E::BYTES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int C = p.C, SA = C * EB + 16;
    constexpr int WPASS = G::WPASS, WT = G::WT, NSL2 = G::template nsl2<DT>(), KST = G::template kstep<DT>();
    constexpr int SH = WPASS * EB + 16;
    unsigned char* T0 = smem;                                      // attention output -> later the LayerNorm'ed MLP input
    unsigned char* Hb = T0 + (size_t)WROWS * SA;                   // hidden chunk [64][256]
    float* red = (float*)(Hb + (size_t)WROWS * SH);                // [NW][64] row partial sums of the channel groups
    float* prm = red + G::NW * 64;                                 // ln_m gamma [C], ln_m beta [C], b_o [C], b2 [C]: fetched with the tile
    constexpr int NT = WROWS * (NPW * WPASS / VEC) / WT;           // 16-byte vectors of the attention tile per thread (C = NPW * WPASS)

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntiles = (int)((p.rows + WROWS - 1) / WROWS);
    int g, tile_i, ksl = 0;
    if constexpr (KS == 1) wide_place(blockIdx.x, g, tile_i);
    else wide_place_ks<KS>(blockIdx.x, g, ksl, tile_i);
    if (tile_i >= ntiles) return;
    const long long r0 = (long long)tile_i * WROWS;
    const int ks_row = p.Kp / KST, ks_row4 = p.Kp4 / KST, nsl = C / G::template ksl<DT>(), nchunk = p.hid / WPASS / KS, chunk0 = ksl * nchunk;

    // the wave's stream: NPW out-projection passes, then per hidden chunk one fc1 pass and NPW fc2 passes
    // ---- prologue: the attention tile and one quad of the four parameter vectors per thread in ONE batch of loads (clamped indices,
    //      stored to LDS under the predicate), then the first WDEPTH weight slices; the LDS writes wait for the older loads only ----
    u32x4 tl[NT];
    constexpr int NV = NPW * WPASS / VEC;
    {
        const T* att = (const T*)p.att + (long long)g * p.rows * C;
#pragma unroll
        for (int it = 0; it < NT; ++it) {                          // (rows beyond the tensor: clamped, never stored)
            const int i = tid + it * WT, row = i / NV, v = i - row * NV;
            long long r = r0 + row;
            r = r < p.rows ? r : p.rows - 1;
            tl[it] = *(const u32x4*)(att + r * C + v * VEC);
        }
    }
    const int pqi = tid < C ? tid : C - 1, pw = pqi / (C / 4), po = 4 * pqi - pw * C;        // C quads (<= threads): vector pw, element po
    const f32x4 pq = *(const f32x4*)((pw == 0 ? p.ln_m_g : pw == 1 ? p.ln_m_b : pw == 2 ? p.bo + g * p.bo_gs : p.b2 + g * p.b2_gs) + po);

    const u32x4* wof = (const u32x4*)((const T*)p.wo + g * p.wo_gs);
    const u32x4* w1f = (const u32x4*)((const T*)p.w1 + g * p.w1_gs);
    const u32x4* w2f = (const u32x4*)((const T*)p.w2 + g * p.w2_gs);
    const WMlpSegs segs{NPW, G::NW, wn, ks_row, ks_row4, nsl, NSL2, nchunk, chunk0, WPASS / KST};
    auto mats = [&](int m) { return m == 0 ? wof : m == 1 ? w1f : w2f; };
    WCursor cur;
    wcursor_start(cur, G::SL, segs);
    u32x4 wq[WDEPTH][G::SL];
#pragma unroll
    for (int u = 0; u < WDEPTH; ++u) wfetch<G::SL>(wq[u], cur, segs, mats);      // the first weight slices travel while the tile is stored

#pragma unroll
    for (int it = 0; it < NT; ++it) {
        const int i = tid + it * WT, row = i / NV, v = i - row * NV;
        *(u32x4*)(T0 + (size_t)row * SA + v * 16) = tl[it];
    }
    if (tid < C) *(f32x4*)(prm + 4 * tid) = pq;
    lds_barrier();

    bool rok[2];
    const T* xres[2];
    T* yrow[2];
    const float* x32row[2];
    float* y32row[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const long long row = r0 + t * 32 + l31;
        rok[t] = row < p.rows;
        const long long grow = rok[t] ? row : p.rows - 1;
        xres[t] = (const T*)p.x + g * p.x_gs + grow * C;
        yrow[t] = (T*)p.y + g * p.y_gs + grow * p.ldy;
        y32row[t] = R32 ? p.y32 + ((long long)g * p.rows + grow) * C : nullptr;
        // (first iteration, no x32: the fp32 residual load below still goes out — to this lane's row of y32, any mapped address — and is discarded)
        x32row[t] = R32 ? (p.x32 ? p.x32 + ((long long)g * p.rows + grow) * C : y32row[t]) : nullptr;
    }
    const bool has32 = R32 && p.x32 != nullptr;
    using XQ = typename std::conditional<R32, f32x4, typename Quad<DT>::type>::type;      // x_att per (pass, row half, channel quad): fp32, or rounded to the storage type
    auto xq_pack = [](float a, float b, float c, float d) -> XQ {
        if constexpr (R32) return f32x4{a, b, c, d};
        else return pack4<DT>(a, b, c, d);
    };
    auto xq_unpack = [](const XQ& q, float* f) {
        if constexpr (R32) { f[0] = q[0]; f[1] = q[1]; f[2] = q[2]; f[3] = q[3]; }
        else unpack4<DT>(q, f);
    };

    // ---- out-projection + coefficient mix: x_att = c_res * x + c_acc * (att W_o^T + b), rounded to the storage type, in registers ----
    constexpr bool PARK = NPW >= 2 || KS > 1;          // (hidden split: the reduce launch reads x_att from the output rows)
    XQ xatt[NPW][2][4];
    {
        const float* bias = prm + 2 * C;                              // b_o (LDS)
        const float ca = p.c_acc_a[g], cr = p.c_res_a[g];
#pragma unroll
        for (int i = 0; i < NPW; ++i) {
            // the residual rows this pass's result meets: requested BEFORE the pass (unconditionally: the rows are clamped), so that they
            // travel under its MFMAs and are older than its refills — the wait behind the pass leaves the weight ring alone
            // (the fp32 stream at C = 512 has no 48 registers to spare across the pass: its rows are requested behind it, still as one batch)
            constexpr bool AHEAD = !(R32 && NPW > 1);
            typename Quad<DT>::type xr[2][4];
            f32x4 xr32[R32 ? 2 : 1][R32 ? 4 : 1];
            auto request = [&]() {
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int n = i * WPASS + wn * 32 + 8 * q + 4 * hi;
                        xr[t][q] = *(const typename Quad<DT>::type*)(xres[t] + n);
                        if constexpr (R32) xr32[t][q] = *(const f32x4*)(x32row[t] + n);
                    }
            };
            if constexpr (AHEAD) request();
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
            wpass<DT, G::SL>(acc, T0, SA, nsl, wq, cur, segs, mats);
            if constexpr (!AHEAD) request();
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    asm volatile("" : "+v"(xr[t][q]));                // (consumed here, behind the pass: the loads stay where they were written)
                    if constexpr (R32) asm volatile("" : "+v"(xr32[t][q]));
                }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = i * WPASS + wn * 32 + 8 * q + 4 * hi;
                    const f32x4 bv = *(const f32x4*)(bias + n);
                    float rv[4], v[4];
                    unpack4<DT>(xr[t][q], rv);
                    if constexpr (R32) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) rv[j] = has32 ? xr32[t][q][j] : rv[j];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf(cr, rv[j], (acc[t][4 * q + j] + bv[j]) * ca);
                    xatt[i][t][q] = xq_pack(v[0], v[1], v[2], v[3]);
                }
        }
    }
    // ---- the block's shared LayerNorm over x_att, from registers: row sums = this lane's channels + the other lane half (shuffle) +
    //      the other channel groups (LDS); the normalised tile overwrites T0 — every wave has passed a barrier after its last
    //      out-projection read by then ----
    {
        float mean[2], rstd[2];
        float sum[2] = {0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < NPW; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[4];
                    xq_unpack(xatt[i][t][q], v);
                    sum[t] += (v[0] + v[1]) + (v[2] + v[3]);
                }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            sum[t] += __shfl_xor(sum[t], 32);
            if (hi == 0) red[wn * 64 + t * 32 + l31] = sum[t];
        }
        lds_barrier();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < G::NW; ++w) s += red[w * 64 + t * 32 + l31];
            mean[t] = s / (float)C;
        }
        lds_barrier();
        float sq[2] = {0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < NPW; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[4];
                    xq_unpack(xatt[i][t][q], v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float d = v[j] - mean[t]; sq[t] += d * d; }
                }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            sq[t] += __shfl_xor(sq[t], 32);
            if (hi == 0) red[wn * 64 + t * 32 + l31] = sq[t];
        }
        lds_barrier();
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < G::NW; ++w) s += red[w * 64 + t * 32 + l31];
            rstd[t] = 1.0f / sqrtf(s / (float)C + p.eps_m);
        }
#pragma unroll
        for (int i = 0; i < NPW; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = i * WPASS + wn * 32 + 8 * q + 4 * hi;
                const f32x4 gv = *(const f32x4*)(prm + n), bv = *(const f32x4*)(prm + C + n);          // (LDS)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float v[4], o[4];
                    xq_unpack(xatt[i][t][q], v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = (v[j] - mean[t]) * rstd[t] * gv[j] + bv[j];
                    *(typename Quad<DT>::type*)(T0 + (size_t)(t * 32 + l31) * SA + n * EB) = pack4<DT>(o[0], o[1], o[2], o[3]);
                    // C = 512: x_att is needed once more, as the residual of the final mix — parked in the workgroup's own rows of the
                    // output tensor (read back by the same lane) instead of holding 32 more registers through the MLP (spills otherwise)
                    if constexpr (PARK) {
                        if (rok[t] && ksl == 0) {
                            if constexpr (R32) *(f32x4*)(y32row[t] + n) = xatt[i][t][q];          // (fp32 x_att parks in the fp32 output rows)
                            else *(typename Quad<DT>::type*)(yrow[t] + n) = xatt[i][t][q];
                        }
                    }
                }
            }
        lds_barrier();
    }
    // ---- MLP in 256-column hidden chunks: H = GELU(n2 W1_chunk^T + b1) -> LDS, then acc2 += H W2[:, chunk]^T ----
    f32x16 acc2[NPW][2];
#pragma unroll
    for (int i = 0; i < NPW; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[i][t][r] = 0.0f;
    const float* b1 = p.b1 + g * p.b1_gs + (long long)chunk0 * WPASS + wn * 32 + 4 * hi;
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        f32x4 b1q[4];                                              // this lane's fc1 biases of the chunk: requested before the pass, as the residual rows above
#pragma unroll
        for (int q = 0; q < 4; ++q) b1q[q] = *(const f32x4*)(b1 + chunk * WPASS + 8 * q);
        f32x16 acc[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        wpass<DT, G::SL>(acc, T0, SA, nsl, wq, cur, segs, mats);
#pragma unroll
        for (int q = 0; q < 4; ++q) asm volatile("" : "+v"(b1q[q]));
        lds_barrier();                                             // every wave is done with the previous chunk's H
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nl = wn * 32 + 8 * q + 4 * hi;
                const f32x4 bv = b1q[q];
                *(typename Quad<DT>::type*)(Hb + (size_t)(t * 32 + l31) * SH + nl * EB) =
                    pack4<DT>(apply_act<ICAF_ACT_GELU, DT>(acc[t][4 * q] + bv[0]), apply_act<ICAF_ACT_GELU, DT>(acc[t][4 * q + 1] + bv[1]),
                              apply_act<ICAF_ACT_GELU, DT>(acc[t][4 * q + 2] + bv[2]), apply_act<ICAF_ACT_GELU, DT>(acc[t][4 * q + 3] + bv[3]));
            }
        lds_barrier();
#pragma unroll
        for (int i = 0; i < NPW; ++i) wpass<DT, G::SL>(acc2[i], Hb, SH, NSL2, wq, cur, segs, mats);
    }
    // ---- output: x' = c_res2 * x_att + c_acc2 * (mlp + b2) ----
    if constexpr (KS > 1) {                            // hidden split: this workgroup's share of the fc2 sums, fp32; dmff_wide_reduce_kernel finishes
        float* part = p.part + ((long long)(ksl * 2 + g) * p.rows) * C;
#pragma unroll
        for (int i = 0; i < NPW; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = i * WPASS + wn * 32 + 8 * q + 4 * hi;
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    if (rok[t])
                        *(f32x4*)(part + (r0 + t * 32 + l31) * C + n) = f32x4{acc2[i][t][4 * q], acc2[i][t][4 * q + 1], acc2[i][t][4 * q + 2], acc2[i][t][4 * q + 3]};
            }
    } else {
        const float* b2 = prm + 3 * C;                            // (LDS)
        const float ca = p.c_acc_m[g], cr = p.c_res_m[g];
#pragma unroll
        for (int i = 0; i < NPW; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = i * WPASS + wn * 32 + 8 * q + 4 * hi;
                const f32x4 bv = *(const f32x4*)(b2 + n);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    float rv[4], v[4];
                    if constexpr (PARK && R32) { const f32x4 r4 = *(const f32x4*)(y32row[t] + n); rv[0] = r4[0]; rv[1] = r4[1]; rv[2] = r4[2]; rv[3] = r4[3]; }
                    else if constexpr (PARK) unpack4<DT>(*(const typename Quad<DT>::type*)(yrow[t] + n), rv);     // (clamped row when !rok: never stored)
                    else xq_unpack(xatt[i][t][q], rv);
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf(cr, rv[j], (acc2[i][t][4 * q + j] + bv[j]) * ca);
                    if (rok[t]) {
                        *(typename Quad<DT>::type*)(yrow[t] + n) = pack4<DT>(v[0], v[1], v[2], v[3]);
                        if constexpr (R32) *(f32x4*)(y32row[t] + n) = f32x4{v[0], v[1], v[2], v[3]};
                    }
                }
            }
    }
}

// y = c_res2 * x_att + c_acc2 * (sum_ks part[ks] + b2): x_att was parked in y by the ks = 0 workgroups; the partial sums are added in
// slice order (a fixed association: the result does not depend on which workgroup finished first).  One thread = 4 channels of one row.
template <int DT, int KS, bool R32 = false>
__global__ __launch_bounds__(256) void dmff_wide_reduce_kernel(const WideP p) {
    using T = typename Elem<DT>::type;
    const int C = p.C, nq = C >> 2;
    const long long total = 2 * p.rows * nq;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int qn = (int)(idx % nq);
        const long long gr = idx / nq;
        const int g = (int)(gr / p.rows);
        const long long row = gr - (long long)g * p.rows;
        const int n = qn * 4;
        f32x4 sum = *(const f32x4*)(p.part + ((long long)g * p.rows + row) * C + n);
#pragma unroll
        for (int k = 1; k < KS; ++k) {
            const f32x4 v = *(const f32x4*)(p.part + ((long long)(k * 2 + g) * p.rows + row) * C + n);
            sum[0] += v[0]; sum[1] += v[1]; sum[2] += v[2]; sum[3] += v[3];
        }
        const f32x4 bv = *(const f32x4*)(p.b2 + g * p.b2_gs + n);
        T* y = (T*)p.y + g * p.y_gs + row * p.ldy + n;
        float* y32 = R32 ? p.y32 + ((long long)g * p.rows + row) * C + n : nullptr;
        float rv[4], v[4];
        if constexpr (R32) { const f32x4 r4 = *(const f32x4*)y32; rv[0] = r4[0]; rv[1] = r4[1]; rv[2] = r4[2]; rv[3] = r4[3]; }      // x_att parked in fp32
        else unpack4<DT>(*(const typename Quad<DT>::type*)y, rv);
        const float ca = p.c_acc_m[g], cr = p.c_res_m[g];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf(cr, rv[j], (sum[j] + bv[j]) * ca);
        *(typename Quad<DT>::type*)y = pack4<DT>(v[0], v[1], v[2], v[3]);
        if constexpr (R32) *(f32x4*)y32 = f32x4{v[0], v[1], v[2], v[3]};
    }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
template <int DT, class G, int NT>
static int launch_wide_ln_qkv(const WideP& p, hipStream_t s) {
    const size_t lds = (size_t)WROWS * (p.C * Elem<DT>::BYTES + 16) + (size_t)(2 * p.C + 3 * G::WPASS) * sizeof(float);      // tile, gamma | beta, biases
    ICAF_LDS_OPTIN((dmff_wide_ln_qkv_kernel<DT, G, NT>), lds);        // (size checked on EVERY call, attribute raised per device as needed)
    const long long work = ((p.rows + WROWS - 1) / WROWS) * (3 * (p.C / G::WPASS) / p.qkv_npass);
    hipLaunchKernelGGL((dmff_wide_ln_qkv_kernel<DT, G, NT>), dim3((unsigned)(8 * ((work + 3) / 4))), dim3(G::WT), lds, s, p);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

template <int DT, int NPW, int KS, class G, bool R32>
static int launch_wide_proj_mlp(const WideP& p, hipStream_t s) {
    // tile, hidden chunk, row sums, the four parameter vectors
    const size_t eb = Elem<DT>::BYTES, lds = (size_t)WROWS * (p.C * eb + 16) + (size_t)WROWS * (G::WPASS * eb + 16) + G::NW * 64 * sizeof(float) + (size_t)4 * p.C * sizeof(float);
    ICAF_LDS_OPTIN((dmff_wide_proj_mlp_kernel<DT, NPW, KS, G, R32>), lds);
    const long long ntiles = (p.rows + WROWS - 1) / WROWS, per = 4 / KS;          // KS workgroups share a tile
    hipLaunchKernelGGL((dmff_wide_proj_mlp_kernel<DT, NPW, KS, G, R32>), dim3((unsigned)(8 * ((ntiles + per - 1) / per))), dim3(G::WT), lds, s, p);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

template <int DT, int KS, bool R32>
static int launch_wide_reduce(const WideP& p, hipStream_t s) {
    const long long items = 2 * p.rows * (p.C / 4);
    long long blocks = (items + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((dmff_wide_reduce_kernel<DT, KS, R32>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    ICAF_LAUNCH_CHECK();
    return ICAF_OK;
}

// THE statement of which three-launch instantiations exist: one row per (C, type class, ksplit, fp32 token stream) with its launchers.  The four
// entry points and icaf_dmff_block_forms find their row through wide_find, so the query's verdict is the launch's verdict.
using WideFn = int (*)(const WideP&, hipStream_t);
struct WideRow {
    int C, f32, ksplit, r32, wpass;                      // f32: the fp32 parity build (else the 16-bit types); wpass: output channels per pass
    WideFn ln_qkv[2], proj_mlp[2], reduce[2];            // [0] bf16 (fp32 in the parity row), [1] f16; reduce: the split rows only
};
// G: geometry, NT: 16-byte loads per thread that fill the token tile, NPW: passes per C-wide product (C = NPW * G::WPASS)
template <class G, int NT, int NPW, int KS, bool R32>
constexpr WideRow wide_row16() {
    static_assert(WROWS * (NPW * G::WPASS / Elem<ICAF_BF16>::VEC) == NT * G::WT, "NT is not the width this geometry loads its tile for");
    WideRow r = {NPW * G::WPASS, 0, KS, R32, G::WPASS,
                 {launch_wide_ln_qkv<ICAF_BF16, G, NT>, launch_wide_ln_qkv<ICAF_F16, G, NT>},
                 {launch_wide_proj_mlp<ICAF_BF16, NPW, KS, G, R32>, launch_wide_proj_mlp<ICAF_F16, NPW, KS, G, R32>}, {nullptr, nullptr}};
    if constexpr (KS > 1) r.reduce[0] = launch_wide_reduce<ICAF_BF16, KS, R32>, r.reduce[1] = launch_wide_reduce<ICAF_F16, KS, R32>;
    return r;
}
// NOT a second statement of what is built (WIDE_ROWS below is the only one the lookup reads; an entry missing here changes nothing): the device
// module numbers its kernels in the order the host code first names their launchers, and the basic-block labels of a kernel carry that number.
// Naming them here in the order this file has always had keeps tools/kernel_fingerprint.py, which compares assembly text, able to tell a
// host-only change from a change to a kernel.
#define WIDE_PROJ_OF(DT) launch_wide_proj_mlp<DT, 1, 1, WG4, true>, launch_wide_proj_mlp<DT, 1, 1, WG8, true>, launch_wide_proj_mlp<DT, 1, 1, WG4, false>, \
                         launch_wide_proj_mlp<DT, 1, 1, WG8, false>, launch_wide_proj_mlp<DT, 2, 1, WG8, false>
#define WIDE_SPLIT_OF(DT) launch_wide_proj_mlp<DT, 1, 2, WG8, true>, launch_wide_proj_mlp<DT, 2, 2, WG8, true>, launch_wide_proj_mlp<DT, 1, 2, WG8, false>, \
                          launch_wide_proj_mlp<DT, 1, 4, WG8, false>, launch_wide_proj_mlp<DT, 2, 2, WG8, false>, launch_wide_proj_mlp<DT, 2, 4, WG8, false>
#define WIDE_REDUCE_OF(DT) launch_wide_reduce<DT, 2, true>, launch_wide_reduce<DT, 2, false>, launch_wide_reduce<DT, 4, false>
#define WIDE_LN_QKV_OF(DT) launch_wide_ln_qkv<DT, WG4, 4>, launch_wide_ln_qkv<DT, WG8, 4>, launch_wide_ln_qkv<DT, WG8, 8>
[[maybe_unused]] static const WideFn WIDE_KERNEL_ORDER[] = {
    launch_wide_ln_qkv<ICAF_F32, WG4, 8>, WIDE_LN_QKV_OF(ICAF_BF16), WIDE_LN_QKV_OF(ICAF_F16),
    launch_wide_proj_mlp<ICAF_F32, 1, 1, WG4, false>, WIDE_PROJ_OF(ICAF_BF16), WIDE_PROJ_OF(ICAF_F16), WIDE_SPLIT_OF(ICAF_BF16), WIDE_SPLIT_OF(ICAF_F16),
    WIDE_REDUCE_OF(ICAF_BF16), WIDE_REDUCE_OF(ICAF_F16)};

static const WideRow WIDE_ROWS[] = {
    // C = 128: four wavefronts, 128-channel passes; its weights are 0.3 MB: no hidden split
    wide_row16<WG4, 4, 1, 1, false>(), wide_row16<WG4, 4, 1, 1, true>(),
    // fp32: the PARITY instantiation of the C = 128 build (v_mfma_f32_32x32x2_f32, erff): the same indexing, masks, LayerNorm and hidden-chunk loop as the
    // 16-bit kernels the bench runs, held to the reference's DMFF goldens at fp32 accuracy (tests/test_gpu_dmff_fused.py)
    {128, 1, 1, 0, WG4::WPASS, {launch_wide_ln_qkv<ICAF_F32, WG4, 8>, nullptr}, {launch_wide_proj_mlp<ICAF_F32, 1, 1, WG4, false>, nullptr}, {nullptr, nullptr}},
    // C = 256 / 512: eight wavefronts, 256-channel passes.  The fp32 token stream (loops > 1) is built for ksplit <= 2, and at C = 512 for the
    // split only (unsplit with fp32 x_att: 258 registers)
    wide_row16<WG8, 4, 1, 1, false>(), wide_row16<WG8, 4, 1, 1, true>(), wide_row16<WG8, 4, 1, 2, false>(), wide_row16<WG8, 4, 1, 2, true>(),
    wide_row16<WG8, 4, 1, 4, false>(),
    wide_row16<WG8, 8, 2, 1, false>(), wide_row16<WG8, 8, 2, 2, false>(), wide_row16<WG8, 8, 2, 2, true>(), wide_row16<WG8, 8, 2, 4, false>(),
};

static const WideRow* wide_find(const char* who, int dtype, int C, int ksplit, bool r32) {
    const int f32 = dtype == ICAF_F32;
    bool shape = false;                                  // some row has this C in this type class
    if (dtype == ICAF_BF16 || dtype == ICAF_F16 || f32)
        for (const WideRow& r : WIDE_ROWS) {
            if (r.C != C || r.f32 != f32) continue;
            shape = true;
            if (r.ksplit == ksplit && r.r32 == (int)r32) return &r;
        }
    if (!shape) fail(ICAF_ERR_UNSUPPORTED, "%s: C=%d, dtype %d: built for C = 128 [four wavefronts, 128-channel passes] and 256 / 512 [eight, 256-channel passes] in the 16-bit types (fp32: the C = 128 parity build only)", who, C, dtype);
    else fail(ICAF_ERR_UNSUPPORTED, "%s: C=%d is not built for ksplit = %d %s the fp32 residual stream", who, C, ksplit, r32 ? "with" : "without");
    return nullptr;
}

// what a row asks of the shape beyond C: the head-dimension rule of the attention launch between its two, whole passes of hidden columns per workgroup
static int wide_shape(const char* who, const WideRow& r, int heads, int hidden) {
    if (heads < 1 || r.C % heads || (r.C / heads) % 8) return fail(ICAF_ERR_UNSUPPORTED, "%s: %d heads at C=%d (head dim must be a multiple of 8)", who, heads, r.C);
    if (hidden < 1 || hidden % (r.wpass * r.ksplit)) return fail(ICAF_ERR_UNSUPPORTED, "%s: hidden width %d must be a multiple of %d", who, hidden, r.wpass * r.ksplit);
    return ICAF_OK;
}

// argument checks + the fields every launch reads; mlp: the launch reads att, the MLP weights and y
static int wide_fill(const icaf_dmff_args* a, const void* att, float* partial, int ksplit, bool mlp, WideP& p, const WideRow*& row, const char* who) {
    if (!a || !a->x) return fail(ICAF_ERR_ARG, "%s: null pointer", who);
    if (!(row = wide_find(who, a->dtype, a->C, ksplit, (mlp || partial) && a->y32))) return ICAF_ERR_UNSUPPORTED;       // (LN + QKV reads no fp32 stream)
    if (a->x32 && !a->y32) return fail(ICAF_ERR_ARG, "%s: x32 without y32 (the fp32 residual stream is read AND written by every iteration but the first)", who);
    if (a->y32 && a->dtype == ICAF_F32) return fail(ICAF_ERR_ARG, "%s: the fp32 residual stream belongs to the 16-bit builds", who);
    if ((a->x32 && ((uintptr_t)a->x32 & 15)) || (a->y32 && ((uintptr_t)a->y32 & 15))) return fail(ICAF_ERR_ARG, "%s: x32 / y32 must be 16-byte aligned", who);
    if (a->B < 1 || a->N < 1) return fail(ICAF_ERR_ARG, "%s: bad B/N", who);
    if (a->Kp < a->C || a->Kp % (row->f32 ? 32 : 64)) return fail(ICAF_ERR_ARG, "%s: Kp=%d", who, a->Kp);
    if (mlp) {
        if (!att || !a->y || !a->wo || !a->bo || !a->w1 || !a->b1 || !a->w2 || !a->b2 || !a->ln_mlp_gamma || !a->ln_mlp_beta) return fail(ICAF_ERR_ARG, "%s: null pointer", who);
        const int st = wide_shape(who, *row, a->heads, a->hidden);
        if (st) return st;
        if (a->Kp4 < a->hidden || a->Kp4 % (row->f32 ? 32 : 64)) return fail(ICAF_ERR_UNSUPPORTED, "%s: Kp4=%d for hidden width %d", who, a->Kp4, a->hidden);
    }
    if ((mlp || partial) && (a->ldy < a->C || a->ldy % 4)) return fail(ICAF_ERR_ARG, "%s: ldy=%d", who, a->ldy);
    dmff_fill_common(a, p);
    p.att = att; p.part = partial; p.x32 = a->x32; p.y32 = a->y32;
    p.rows = (long long)a->B * a->N;
    // LN + QKV: three output-channel passes per workgroup by default.  One pass per workgroup (three times the workgroups for the levels whose
    // tiles alone do not fill the chip) was measured and LOSES at every level — P5 of yolov5s 26.7 -> 34.4 us, P4 19.6 -> 25.5, yolov5l P4
    // 48.9 -> 65.5: the repeated LayerNorm and workgroup prologues cost more than the idle CUs.  a->reserved = 1 keeps it reachable for A/B.
    p.qkv_npass = a->reserved == 1 ? 1 : 3;
    return ICAF_OK;
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_dmff_block_forms(int dtype, int C, int N, int heads, int hidden, int ksplit, int stream32, int* two_launch, int* three_launch) {
    if (!two_launch || !three_launch) return fail(ICAF_ERR_ARG, "icaf_dmff_block_forms: null pointer");
    *two_launch = dmff_fused_covered(dtype, C, N, heads, hidden);
    const WideRow* row = N >= 1 ? wide_find("icaf_dmff_block_forms", dtype, C, ksplit, stream32 != 0) : nullptr;
    *three_launch = row && wide_shape("icaf_dmff_block_forms", *row, heads, hidden) == ICAF_OK;
    return ICAF_OK;
}

extern "C" int icaf_dmff_wide_ln_qkv(const icaf_dmff_args* a, icaf_stream_t s) {
    WideP p{};          // (value-initialised: a field a later edit forgets to fill is zero, not stack garbage)
    const WideRow* row;
    int st = wide_fill(a, nullptr, nullptr, 1, false, p, row, "icaf_dmff_wide_ln_qkv");
    if (st) return st;
    if (!a->qkv || !a->wqkv || !a->bqkv || !a->ln_attn_gamma[0] || !a->ln_attn_gamma[1] || !a->ln_attn_beta[0] || !a->ln_attn_beta[1])
        return fail(ICAF_ERR_ARG, "icaf_dmff_wide_ln_qkv: null pointer");
    return row->ln_qkv[a->dtype == ICAF_F16](p, S(s));
}

extern "C" int icaf_dmff_wide_proj_mlp(const icaf_dmff_args* a, const void* att, icaf_stream_t s) {
    WideP p{};
    const WideRow* row;
    int st = wide_fill(a, att, nullptr, 1, true, p, row, "icaf_dmff_wide_proj_mlp");
    return st ? st : row->proj_mlp[a->dtype == ICAF_F16](p, S(s));
}

extern "C" int icaf_dmff_wide_proj_mlp_split(const icaf_dmff_args* a, const void* att, float* partial, int ksplit, icaf_stream_t s) {
    if (!partial) return fail(ICAF_ERR_ARG, "icaf_dmff_wide_proj_mlp_split: null pointer");
    if (ksplit != 2 && ksplit != 4) return fail(ICAF_ERR_ARG, "icaf_dmff_wide_proj_mlp_split: ksplit %d (2 or 4)", ksplit);
    WideP p{};
    const WideRow* row;
    int st = wide_fill(a, att, partial, ksplit, true, p, row, "icaf_dmff_wide_proj_mlp_split");
    return st ? st : row->proj_mlp[a->dtype == ICAF_F16](p, S(s));
}

extern "C" int icaf_dmff_wide_reduce(const icaf_dmff_args* a, const float* partial, int ksplit, icaf_stream_t s) {
    if (!partial || !a || !a->y || !a->b2) return fail(ICAF_ERR_ARG, "icaf_dmff_wide_reduce: null pointer");
    if (ksplit != 2 && ksplit != 4) return fail(ICAF_ERR_ARG, "icaf_dmff_wide_reduce: ksplit %d (2 or 4)", ksplit);
    WideP p{};
    const WideRow* row;
    int st = wide_fill(a, nullptr, const_cast<float*>(partial), ksplit, false, p, row, "icaf_dmff_wide_reduce");
    return st ? st : row->reduce[a->dtype == ICAF_F16](p, S(s));
}
