// Host check of the weight-stream cursor of the DMFF token kernels (icafusion_amd/csrc/wide_cursor.h), over every geometry of the
// instantiation table of dmff_wide.hip: C 128 (four wavefronts, slices of two K steps; 16-bit and fp32) / 256 / 512 (eight wavefronts,
// slices of four), K padded or not, LayerNorm + QKV with three passes or one and every column group, out-projection + MLP with NPW 1 / 2
// and the hidden columns split 1 / 2 / 4 ways with every hidden slice, hidden = 4 C, every wavefront.
//   (i)  the slices CONSUMED, in ring order (slot = index mod WDEPTH), are the sequence the kernels' GEMM passes expect — written out
//        below as the plain nested loops of the passes, independently of the cursor;
//   (ii) every slice REQUESTED — the WDEPTH refills past the end of the stream included, which must repeat the last valid slice — lies
//        inside its fragment-major matrix.
// Meant to be built with -fsanitize=address,undefined: the ring and the expected sequence live in exactly sized heap arrays.
#include "wide_cursor.h"
#include <cstdio>
#include <vector>

using namespace icaf;

namespace {
constexpr int WDEPTH = 4;
struct Slice { int mat; long long frag; };
long long g_checked = 0;

template <class SEGS>
bool run(const SEGS& segs, int WSL, const std::vector<Slice>& want, const long long (&size)[3], const char* what) {
    if (want.empty() || want.size() % WDEPTH) return std::printf("FAIL %s: %zu slices, not a multiple of the ring depth\n", what, want.size()), false;
    std::vector<Slice> ring(WDEPTH);
    WCursor c;
    wcursor_start(c, WSL, segs);
    size_t fetched = 0;
    auto fetch = [&](int slot) {
        if (c.mat < 0 || c.mat > 2 || c.frag < 0 || c.frag + WSL > size[c.mat])
            return std::printf("FAIL %s: request %zu reads fragments [%lld, %lld) of matrix %d (%lld fragments)\n", what, fetched, c.frag, c.frag + WSL, c.mat, size[c.mat]), false;
        if (fetched >= want.size() && (c.mat != want.back().mat || c.frag != want.back().frag))
            return std::printf("FAIL %s: tail request %zu is not the last valid slice\n", what, fetched), false;
        ring.at(slot) = Slice{c.mat, c.frag};
        ++fetched;
        wcursor_advance(c, WSL, segs);
        return true;
    };
    for (int u = 0; u < WDEPTH; ++u)
        if (!fetch(u)) return false;
    for (size_t i = 0; i < want.size(); ++i) {
        const Slice got = ring.at(i % WDEPTH);
        if (got.mat != want[i].mat || got.frag != want[i].frag)
            return std::printf("FAIL %s: slice %zu is (%d, %lld), expected (%d, %lld)\n", what, i, got.mat, got.frag, want[i].mat, want[i].frag), false;
        if (!fetch((int)(i % WDEPTH))) return false;
    }
    if (fetched != want.size() + WDEPTH) return std::printf("FAIL %s: %zu requests\n", what, fetched), false;
    ++g_checked;
    return true;
}
}  // namespace

int main() {
    struct Build { int C, NW, SL, eb; };
    const Build builds[] = {{128, 4, 2, 2}, {128, 4, 2, 4}, {256, 8, 4, 2}, {512, 8, 4, 2}};
    char what[256];
    for (const Build& b : builds) {
        const int C = b.C, NW = b.NW, SL = b.SL, WPASS = 32 * NW, kst = 32 / b.eb, ksl = kst * SL;
        const int nsl = C / ksl, nsl2 = WPASS / ksl, NPW = C / WPASS, hid = 4 * C, kpad = b.eb == 4 ? 32 : 64;
        for (int pad = 0; pad < 2; ++pad) {
            const int Kp = C + pad * kpad, Kp4 = hid + pad * kpad, ks_row = Kp / kst, ks_row4 = Kp4 / kst;
            // ---- LayerNorm + QKV ----
            for (int npass : {3, 1}) {
                const int ngrp = 3 * (C / WPASS) / npass;
                const long long size[3] = {(long long)(3 * C / 32) * ks_row, 0, 0};
                for (int grp = 0; grp < ngrp; ++grp)
                    for (int wn = 0; wn < NW; ++wn) {
                        std::vector<Slice> want;
                        for (int j = 0; j < npass; ++j)
                            for (int s = 0; s < nsl; ++s) want.push_back(Slice{0, (long long)((grp * npass + j) * NW + wn) * ks_row + s * SL});
                        std::snprintf(what, sizeof what, "ln_qkv C=%d eb=%d Kp=%d npass=%d grp=%d wave=%d", C, b.eb, Kp, npass, grp, wn);
                        if (!run(WQkvSegs{npass, grp, NW, wn, ks_row, nsl}, SL, want, size, what)) return 1;
                    }
            }
            // ---- out-projection + MLP ----
            for (int KS : {1, 2, 4}) {
                if (KS > 1 && NW != 8) continue;                      // (the hidden split is built for the eight-wave geometry)
                const int nchunk = hid / WPASS / KS;
                const long long size[3] = {(long long)(C / 32) * ks_row, (long long)(hid / 32) * ks_row, (long long)(C / 32) * ks_row4};
                for (int ks = 0; ks < KS; ++ks)
                    for (int wn = 0; wn < NW; ++wn) {
                        const int chunk0 = ks * nchunk;
                        std::vector<Slice> want;
                        for (int i = 0; i < NPW; ++i)
                            for (int s = 0; s < nsl; ++s) want.push_back(Slice{0, (long long)(i * NW + wn) * ks_row + s * SL});
                        for (int ch = 0; ch < nchunk; ++ch) {
                            for (int s = 0; s < nsl; ++s) want.push_back(Slice{1, (long long)((chunk0 + ch) * NW + wn) * ks_row + s * SL});
                            for (int i = 0; i < NPW; ++i)
                                for (int s = 0; s < nsl2; ++s)
                                    want.push_back(Slice{2, (long long)(i * NW + wn) * ks_row4 + (long long)(chunk0 + ch) * (WPASS / kst) + s * SL});
                        }
                        std::snprintf(what, sizeof what, "proj_mlp C=%d eb=%d Kp=%d Kp4=%d KS=%d slice=%d wave=%d", C, b.eb, Kp, Kp4, KS, ks, wn);
                        if (!run(WMlpSegs{NPW, NW, wn, ks_row, ks_row4, nsl, nsl2, nchunk, chunk0, WPASS / kst}, SL, want, size, what)) return 1;
                    }
            }
        }
    }
    std::printf("wide cursor ok (%lld streams)\n", g_checked);
    return 0;
}
