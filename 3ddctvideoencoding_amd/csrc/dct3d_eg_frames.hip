// dct3d_eg_frames.hip -- the fused Exp-Golomb calls for frames of any size and packed RGB24
// (dct3d_encode_eg_frames* / dct3d_decode_eg_frames*): raster -> one Exp-Golomb stream per channel and back,
// with no int32 cube-major intermediate.  The device code is the fused kernels' (dct3d_eg_fused_dev.h) with
// the edge padding / crop (EDGE = 1) and the channel pick / mix (PX = 3) in its
// addressing.  A translation unit of its own: the other kernels' code objects do not change with it, and a
// grey geometry whose width and height are multiples of 8 never comes here.
#include "dct3d_launch.h"

namespace dct3d {

template int launch_encode_eg_in<StreamFrames>(const Variant&, const EncodeParams&, const EgFusedParams&, const VqParams*, hipStream_t);
template int launch_decode_eg_in<StreamFrames>(const Variant&, const DecodeParamsQ&, const EgDecParams&, int, const VqParams*, hipStream_t);
template int launch_decode_eg_rgb_in<StreamFrames>(const Variant&, const DecodeParamsQ&, const EgDecRgbParams&, const VqParams*, uint32_t, hipStream_t);

}  // namespace dct3d
