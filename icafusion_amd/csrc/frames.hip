// Device letterbox of native camera frames (utils/datasets.py: letterbox = resize_bilinear to new_unpad + grey padding), byte for byte:
// decoder-layout frames (H0 x W0 x ch interleaved uint8, own row pitch) -> the plan's uint8 [B][ctot][H][W] input planes.  Built with fp
// contraction off (build.py): every product and sum rounds like resize_bilinear's separate fp32 numpy operations.  The tile itself
// (lb_tile) and the entry point's checks and launch (frames_launch) are in frames_core.h, shared with resize.hip; this kernel stays beside
// resize_frames_kernel's mode-0 branch because it is the faster of the two on staged tiles (profiles/frames_tile_ab.json).
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
    lb_tile(frame, g, lds, d, plane_stride, H, W, swap_rb, force_direct);
}

}  // namespace icaf

using namespace icaf;

extern "C" int icaf_letterbox_frames(const void* arena, const icaf_frame_geom* geom, int nstreams, int B, void* dst, int ctot, int H, int W,
                                     int swap_rb, icaf_stream_t s) {
    return frames_launch("icaf_letterbox_frames", letterbox_frames_kernel, arena, geom, nullptr, dst, nstreams, B, ctot, H, W, swap_rb, s);
}
