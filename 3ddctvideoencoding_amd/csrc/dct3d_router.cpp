// dct3d_router.cpp -- the five variant launchers: each hands its call to the unit of its family that holds the
// variant (dct3d_variant.h), whose translation unit instantiates the family's ladder for exactly its variants
// (dct3d_launch.h).  A variant no unit holds (a value outside an axis): -1.
#include "dct3d_kernels.h"

namespace dct3d {

int launch_encode(const Variant& v, const EncodeParams& P, hipStream_t st) {
    return RasterUnits::route(v, [&](auto u) { return launch_encode_in<decltype(u)>(v, P, st); });
}
int launch_decode(const Variant& v, const DecodeParamsQ& P, hipStream_t st) {
    return RasterUnits::route(v, [&](auto u) { return launch_decode_in<decltype(u)>(v, P, st); });
}
int launch_encode_eg(const Variant& v, const EncodeParams& P, const EgFusedParams& E, const VqParams* V, hipStream_t st) {
    return StreamUnits::route(v, [&](auto u) { return launch_encode_eg_in<decltype(u)>(v, P, E, V, st); });
}
int launch_decode_eg(const Variant& v, const DecodeParamsQ& P, const EgDecParams& E, int groups_per_wave, const VqParams* V,
                     hipStream_t st) {
    return StreamUnits::route(v, [&](auto u) { return launch_decode_eg_in<decltype(u)>(v, P, E, groups_per_wave, V, st); });
}
// (no packed RGB24 variant is in StreamPlain, which builds no such ladder)
int launch_decode_eg_rgb(const Variant& v, const DecodeParamsQ& P, const EgDecRgbParams& E, const VqParams* V, uint32_t vq_ch_stride,
                         hipStream_t st) {
    using RgbUnits = Units<StreamFrames, StreamQuant, StreamVq, StreamYcc>;
    return RgbUnits::route(v, [&](auto u) { return launch_decode_eg_rgb_in<decltype(u)>(v, P, E, V, vq_ch_stride, st); });
}

}  // namespace dct3d
