// dct3d_edge.hip -- frames of any size (dct3d_encode_frames* / dct3d_decode_frames*): the encode and decode
// kernels' instantiations with the edge padding and the crop in their addressing (EDGE = 1), grey and packed
// RGB24, and their launchers.  The device code is the product kernels' (dct3d_encode_dev.h /
// dct3d_decode_dev.h): the cubes tile the padded raster, which repeats each frame's last column and last row
// and exists nowhere in memory; only the row loads (encode, its rare paths' reloads included) and the raster
// stores (decode) differ.  A translation unit of its own: the other kernels' code objects do not change with
// it, and a geometry whose width and height are multiples of 8 never comes here (the runtime launches the
// existing kernels for it).
#include "dct3d_launch.h"

namespace dct3d {

template int launch_encode_in<RasterEdge>(const Variant&, const EncodeParams&, hipStream_t);
template int launch_decode_in<RasterEdge>(const Variant&, const DecodeParamsQ&, hipStream_t);

}  // namespace dct3d
