// dct3d_vq_dec.hip -- the fused stream decode with a quantiser table per stack (dct3d_decode_eg_frames_vq*;
// DESIGN 4m, 4n, 4p): the StreamVq unit's two decode ladders, decode_eg_kernel<D, 8, EDGE, QT = 2> and
// decode_eg_rgb_kernel<D, EDGE, QT = 2> (dct3d_eg_fused_dev.h: the shared bodies, the per-lane step pointer as
// their QT = 2 arm).  The sync, scan and mark passes do not depend on the table.
// A translation unit of its own: no other code object changes.
#include "dct3d_launch.h"

namespace dct3d {

template int launch_decode_eg_in<StreamVq>(const Variant&, const DecodeParamsQ&, const EgDecParams&, int, const VqParams*, hipStream_t);
template int launch_decode_eg_rgb_in<StreamVq>(const Variant&, const DecodeParamsQ&, const EgDecRgbParams&, const VqParams*, uint32_t, hipStream_t);

}  // namespace dct3d
