// dct3d_edge.hip -- frames of any size (dct3d_encode_frames* / dct3d_decode_frames*): the encode and decode
// kernels' instantiations with the edge padding and the crop in their addressing (EDGE = 1), grey and packed
// RGB24, and their launchers.  The device code is the product kernels' (dct3d_encode_dev.h /
// dct3d_decode_dev.h): the cubes tile the padded raster, which repeats each frame's last column and last row
// and exists nowhere in memory; only the row loads (encode, its rare paths' reloads included) and the raster
// stores (decode) differ.  A translation unit of its own: the other kernels' code objects do not change with
// it, and a geometry whose width and height are multiples of 8 never comes here (the runtime launches the
// existing kernels for it).
#include "dct3d_encode_dev.h"
#include "dct3d_decode_dev.h"

namespace dct3d {

int launch_encode_edge(int D, int px, const EncodeParams& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    const dim3 grid(enc_grid(D, P));
    if (D == 8) {
        if (px == 1) hipLaunchKernelGGL((encode16_kernel<0, 1>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((encode16_rgb_kernel<1>), grid, dim3(kBlock), 0, st, P);
    } else {
        if (px == 1) hipLaunchKernelGGL((encode_kernel<1>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((encode_rgb_kernel<1>), grid, dim3(kBlock), 0, st, P);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_decode_edge(int D, int px, const DecodeParams& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    const dim3 grid(dec_grid(D, P.n_cubes));
    if (D == 8) {
        if (px == 1) hipLaunchKernelGGL((decode_kernel<8, 1>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((decode_rgb_kernel<8, 1>), grid, dim3(kBlock), 0, st, P);
    } else {
        if (px == 1) hipLaunchKernelGGL((decode_kernel<4, 1>), grid, dim3(kBlock), 0, st, P);
        else hipLaunchKernelGGL((decode_rgb_kernel<4, 1>), grid, dim3(kBlock), 0, st, P);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace dct3d
