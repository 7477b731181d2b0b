// The per-wave weight stream of the DMFF token kernels (dmff_wide.hip) as plain integer arithmetic, shared by the device code and a host
// check (tests/native/wide_cursor_check.cpp): which segment follows which, where a slice lies in its fragment-major matrix, and what a
// refill reads once the kernel's stream has ended.
//
// Units.  A FRAGMENT is one MFMA K step of one 32-channel block: 64 lanes x 16 bytes, fragment (nb, ks) of a matrix with ks_row K steps
// per row block at index nb * ks_row + ks.  A SLICE is WSL consecutive fragments of one row block — what one slot of the register ring
// holds.  A SEGMENT is the n slices one wave consumes in one GEMM pass.
//
// Every refill is UNCONDITIONAL (dmff_wide.hip, wfetch): the ring always holds WDEPTH slices in flight, so the count of younger loads in
// front of a slot is a constant the wait can be written against.  After its last segment the cursor stays on the last slice of that
// segment: the WDEPTH refills issued while the last slices are consumed re-read an address the wave has already read (in bounds, an L2
// hit) and their values are never consumed.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ICAF_HD __host__ __device__ __forceinline__
#else
#define ICAF_HD inline
#endif

namespace icaf {

struct WSeg {
    int mat;                 // which matrix of the kernel (ln_qkv: 0 = W_qkv; proj_mlp: 0 = W_o, 1 = W1, 2 = W2)
    long long first;         // first fragment of the segment
    int n;                   // slices
};

// LayerNorm + QKV: workgroup (tile, column group grp) runs npass passes; pass j covers output channels [(grp * npass + j) * 32 NW, + 32 NW)
struct WQkvSegs {
    int npass, grp, NW, wn, ks_row, nsl;
    ICAF_HD int count() const { return npass; }
    ICAF_HD WSeg at(int s) const { return WSeg{0, (long long)((grp * npass + s) * NW + wn) * ks_row, nsl}; }
};

// out-projection + MLP: NPW out-projection passes, then per hidden chunk one fc1 pass (K = C) and NPW fc2 passes (K = the chunk's
// 32 NW hidden columns: nsl2 slices starting at K step (chunk0 + chunk) * kst_pass of a row of ks_row4 steps)
struct WMlpSegs {
    int NPW, NW, wn, ks_row, ks_row4, nsl, nsl2, nchunk, chunk0, kst_pass;
    ICAF_HD int count() const { return NPW + nchunk * (1 + NPW); }
    ICAF_HD WSeg at(int s) const {
        if (s < NPW) return WSeg{0, (long long)(s * NW + wn) * ks_row, nsl};
        const int m = s - NPW, chunk = m / (1 + NPW), r = m - chunk * (1 + NPW);
        if (r == 0) return WSeg{1, (long long)((chunk0 + chunk) * NW + wn) * ks_row, nsl};
        return WSeg{2, (long long)((r - 1) * NW + wn) * ks_row4 + (long long)(chunk0 + chunk) * kst_pass, nsl2};
    }
};

struct WCursor {
    long long frag;          // next slice to fetch: fragments [frag, frag + WSL) of matrix mat
    int mat, left, seg;
};

template <class SEGS>
ICAF_HD void wcursor_enter(WCursor& c, int WSL, const SEGS& segs) {          // c.seg -> (mat, frag, left); past the last segment: its last slice, again and again
    const int last = segs.count() - 1;
    const bool end = c.seg > last;
    const WSeg s = segs.at(end ? last : c.seg);
    c.mat = s.mat;
    c.frag = end ? s.first + (long long)(s.n - 1) * WSL : s.first;
    c.left = end ? 1 : s.n;
}

template <class SEGS>
ICAF_HD void wcursor_start(WCursor& c, int WSL, const SEGS& segs) { c.seg = 0; wcursor_enter(c, WSL, segs); }

template <class SEGS>
ICAF_HD void wcursor_advance(WCursor& c, int WSL, const SEGS& segs) {        // after the slice at c.frag has been requested
    c.frag += WSL;
    if (--c.left == 0) {
        if (c.seg < segs.count()) ++c.seg;           // (stays at count(): the tail never overflows the counter)
        wcursor_enter(c, WSL, segs);
    }
}

}  // namespace icaf
