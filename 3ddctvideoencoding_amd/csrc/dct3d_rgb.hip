// dct3d_rgb.hip -- packed RGB24 video (the upstream capture format: uint8 [frame][y][x][3], R, G, B): the
// fused colour encode and decode kernels' instantiations and launchers.  The device code is the grey
// kernels' (dct3d_encode_dev.h / dct3d_decode_dev.h) with the packed addressing: a wave owns the three
// channels of its tile, reads or writes each packed byte once, and splits / interleaves the channels in
// registers with byte permutes.  The int32 side is laid out [stack][channel][cube]: each (stack, channel)
// block is what the grey path gives for that plane's stack.  A translation unit of its own: the grey
// kernels' code objects do not change with it.
#include "dct3d_launch.h"

namespace dct3d {

// Packed RGB24: the same geometry over the RGB cubes (P.n_cubes of them), each wave encoding the three channels
// of its tile (encode16_rgb_kernel / encode_rgb_kernel) or decoding them in turn (decode_rgb_kernel)
template int launch_encode_in<RasterRgb>(const Variant&, const EncodeParams&, hipStream_t);
template int launch_decode_in<RasterRgb>(const Variant&, const DecodeParamsQ&, hipStream_t);

}  // namespace dct3d
