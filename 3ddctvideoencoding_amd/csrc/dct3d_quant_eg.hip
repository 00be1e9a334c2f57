// dct3d_quant_eg.hip -- quantiser tables through the fused Exp-Golomb calls (dct3d_encode_eg* /
// dct3d_decode_eg*, the _frames calls included): the QT = 1 instantiations of the fused kernels
// (dct3d_eg_fused_dev.h) for every geometry, and their launchers.  As dct3d_quant.hip: the encode differs in
// its DC and its exact replay's divisor, the decode in where its steps come from (decode_tile<CODES>: the
// lane's 11 steps as integers for the |q| * step products; the stream re-parse of the exact replay).  The
// grey stream decode is built at 8 groups per wave only, the product's default.  A translation unit of its
// own: no other code object changes, and a context with the reference table never comes here.
#include "dct3d_launch.h"

namespace dct3d {

template int launch_encode_eg_in<StreamQuant>(const Variant&, const EncodeParams&, const EgFusedParams&, const VqParams*, hipStream_t);
template int launch_decode_eg_in<StreamQuant>(const Variant&, const DecodeParamsQ&, const EgDecParams&, int, const VqParams*, hipStream_t);
template int launch_decode_eg_rgb_in<StreamQuant>(const Variant&, const DecodeParamsQ&, const EgDecRgbParams&, const VqParams*, uint32_t, hipStream_t);

}  // namespace dct3d
