// dct3d_quant.hip -- quantiser tables (dct3d_ctx_set_quant): the int32 encode and decode kernels'
// instantiations that take the step of each s = kx + ky + kz from the context's table (QT = 1), grey and
// packed RGB24, multiples of 8 and frames of any size, both depths, and their launchers.  The device code is
// the product kernels' (dct3d_encode_dev.h / dct3d_decode_dev.h): the encode's main path reads the same
// {1 / step_s, G_s, 0.5 - E_s} table either way, so only its DC and its rare paths (enc4_replay, the second
// certificate's quotient, the exact fold) differ, by the divisor; the decode reads its 11 steps per lane
// from the table where the product kernels compute sb + 5 j.  A translation unit of its own: the other
// kernels' code objects do not change with it, and a context whose table is the reference's never comes
// here (the runtime launches the existing kernels for it).
#include "dct3d_encode_dev.h"
#include "dct3d_decode_dev.h"

namespace dct3d {

int launch_encode_qt(int D, int px, int edge, const EncodeParams& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (px != 1 && px != 3) return -1;
    const dim3 grid(enc_grid(D, P)), blk(kBlock);
    switch ((D == 8 ? 4 : 0) + (px == 3 ? 2 : 0) + (edge ? 1 : 0)) {
        case 7: hipLaunchKernelGGL((encode16_rgb_kernel<1, 1>), grid, blk, 0, st, P); break;
        case 6: hipLaunchKernelGGL((encode16_rgb_kernel<0, 1>), grid, blk, 0, st, P); break;
        case 5: hipLaunchKernelGGL((encode16_kernel<0, 1, 1>), grid, blk, 0, st, P); break;
        case 4: hipLaunchKernelGGL((encode16_kernel<0, 0, 1>), grid, blk, 0, st, P); break;
        case 3: hipLaunchKernelGGL((encode_rgb_kernel<1, 1>), grid, blk, 0, st, P); break;
        case 2: hipLaunchKernelGGL((encode_rgb_kernel<0, 1>), grid, blk, 0, st, P); break;
        case 1: hipLaunchKernelGGL((encode_kernel<1, 1>), grid, blk, 0, st, P); break;
        default: hipLaunchKernelGGL((encode_kernel<0, 1>), grid, blk, 0, st, P); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_decode_qt(int D, int px, int edge, const DecodeParamsQ& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if ((px != 1 && px != 3) || !P.steps) return -1;
    const dim3 grid(dec_grid(D, P.n_cubes)), blk(kBlock);
    switch ((D == 8 ? 4 : 0) + (px == 3 ? 2 : 0) + (edge ? 1 : 0)) {
        case 7: hipLaunchKernelGGL((decode_rgb_kernel<8, 1, 1>), grid, blk, 0, st, P); break;
        case 6: hipLaunchKernelGGL((decode_rgb_kernel<8, 0, 1>), grid, blk, 0, st, P); break;
        case 5: hipLaunchKernelGGL((decode_kernel<8, 1, 1>), grid, blk, 0, st, P); break;
        case 4: hipLaunchKernelGGL((decode_kernel<8, 0, 1>), grid, blk, 0, st, P); break;
        case 3: hipLaunchKernelGGL((decode_rgb_kernel<4, 1, 1>), grid, blk, 0, st, P); break;
        case 2: hipLaunchKernelGGL((decode_rgb_kernel<4, 0, 1>), grid, blk, 0, st, P); break;
        case 1: hipLaunchKernelGGL((decode_kernel<4, 1, 1>), grid, blk, 0, st, P); break;
        default: hipLaunchKernelGGL((decode_kernel<4, 0, 1>), grid, blk, 0, st, P); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace dct3d
