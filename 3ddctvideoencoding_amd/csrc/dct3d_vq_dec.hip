// dct3d_vq_dec.hip -- the fused stream decode with a quantiser table per stack (dct3d_decode_eg_frames_vq*;
// DESIGN 4m, 4n): the launchers of decode_eg_kernel<D, 8, EDGE, QT = 2> and decode_eg_rgb_kernel<D, EDGE, QT = 2>
// (dct3d_eg_fused_dev.h: the shared bodies, the per-lane step pointer as their QT = 2 arm).  The sync, scan and
// mark passes do not depend on the table.
// A translation unit of its own: no other code object changes.
#include "dct3d_eg_fused_dev.h"

namespace dct3d {

int launch_decode_eg_vq(int D, int edge, const DecodeParams& P, const EgDecParams& E, const VqParams& V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!V.steps || !V.map) return -1;
    int rc = -1;
    with_variant(D, 1, edge, [&](auto d, auto, auto e) {
        const dim3 grid(dec_grid(d, P.n_cubes - P.cube_base, 8));  // cube_base: a multiple of the cubes per wave
        hipLaunchKernelGGL((decode_eg_kernel<d, 8, e, 2, VqParams>), grid, dim3(kBlock), 0, st, P, E, V);
        rc = launched();
    });
    return rc;
}

int launch_decode_eg_rgb_vq(int D, int edge, const DecodeParams& P, const EgDecRgbParams& E, const VqParams& V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!V.steps || !V.map) return -1;
    int rc = -1;
    with_variant(D, 3, edge, [&](auto d, auto, auto e) {
        const dim3 grid(dec_grid(d, P.n_cubes - P.cube_base));
        hipLaunchKernelGGL((decode_eg_rgb_kernel<d, e, 2, 0, VqParams>), grid, dim3(kBlock), 0, st, P, E, V);
        rc = launched();
    });
    return rc;
}

}  // namespace dct3d
