// dct3d_quant.hip -- quantiser tables (dct3d_ctx_set_quant): the int32 encode and decode kernels'
// instantiations that take the step of each s = kx + ky + kz from the context's table (QT = 1), grey and
// packed RGB24, multiples of 8 and frames of any size, both depths, and their launchers.  The device code is
// the product kernels' (dct3d_encode_dev.h / dct3d_decode_dev.h): the encode's main path reads the same
// {1 / step_s, G_s, 0.5 - E_s} table either way, so only its DC and its rare paths (enc4_replay, the second
// certificate's quotient, the exact fold) differ, by the divisor; the decode reads its 11 steps per lane
// from the table where the product kernels compute sb + 5 j.  A translation unit of its own: the other
// kernels' code objects do not change with it, and a context whose table is the reference's never comes
// here (the runtime launches the existing kernels for it).
#include "dct3d_launch.h"

namespace dct3d {

template int launch_encode_in<RasterQuant>(const Variant&, const EncodeParams&, hipStream_t);
template int launch_decode_in<RasterQuant>(const Variant&, const DecodeParamsQ&, hipStream_t);

}  // namespace dct3d
