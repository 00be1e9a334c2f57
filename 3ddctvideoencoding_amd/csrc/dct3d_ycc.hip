// dct3d_ycc.hip -- the YCbCr colour transform fused into the packed RGB24 stream calls and the rate probe
// (DCT3D_OPT_COLOUR = DCT3D_COLOUR_YCBCR): the CT = 1 instances of encode_eg_kernel and
// decode_eg_rgb_kernel (dct3d_eg_fused_dev.h) under every table mode (QT = 0, 1, 2: the StreamYcc unit's ladders)
// and of rate_kernel (dct3d_rate_dev.h).
// The transform sits where a channel's bytes are picked out of a lane's 24 (ycc_pick8: the row loads and the exact
// replay's reload) and, in the decode, on the merged bytes in registers before the one store (ycc_to_rgb4): no
// launch and no memory traffic is added.  A translation unit of its own: no other code object changes, and a
// context that does not set the option never comes here.
#include "dct3d_launch.h"
#include "dct3d_rate_dev.h"

namespace dct3d {

template int launch_encode_eg_in<StreamYcc>(const Variant&, const EncodeParams&, const EgFusedParams&, const VqParams*, hipStream_t);
// (no grey variant is in StreamYcc: this ladder launches nothing and answers -1)
template int launch_decode_eg_in<StreamYcc>(const Variant&, const DecodeParamsQ&, const EgDecParams&, int, const VqParams*, hipStream_t);
template int launch_decode_eg_rgb_in<StreamYcc>(const Variant&, const DecodeParamsQ&, const EgDecRgbParams&, const VqParams*, uint32_t, hipStream_t);

int launch_rate_ycc(int D, int edge, const EncodeParams& P, const RateParams& R, hipStream_t st) {
    return probe_dispatch(D, 3, edge, P, R, [&](auto d, auto, auto e) {
        const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
        hipLaunchKernelGGL((rate_kernel<decltype(d)::value, 3, decltype(e)::value, 1>), grid, dim3(kBlock), 0, st, P, R);
    });
}

}  // namespace dct3d
