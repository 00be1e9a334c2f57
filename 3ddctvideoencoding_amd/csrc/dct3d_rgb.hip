// dct3d_rgb.hip -- packed RGB24 video (the upstream capture format: uint8 [frame][y][x][3], R, G, B): the
// fused colour encode and decode kernels' instantiations and launchers.  The device code is the grey
// kernels' (dct3d_encode_dev.h / dct3d_decode_dev.h) with the packed addressing: a wave owns the three
// channels of its tile, reads or writes each packed byte once, and splits / interleaves the channels in
// registers with byte permutes.  The int32 side is laid out [stack][channel][cube]: each (stack, channel)
// block is what the grey path gives for that plane's stack.  A translation unit of its own: the grey
// kernels' code objects do not change with it.
#include "dct3d_encode_dev.h"
#include "dct3d_decode_dev.h"

namespace dct3d {

// Packed RGB24: the same geometry over the RGB cubes (P.n_cubes of them), each wave encoding the three
// channels of its tile (encode16_rgb_kernel / encode_rgb_kernel).
int launch_encode_rgb(int D, const EncodeParams& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    const dim3 grid(enc_grid(D, P));
    if (D == 8) hipLaunchKernelGGL((encode16_rgb_kernel<>), grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL((encode_rgb_kernel<>), grid, dim3(kBlock), 0, st, P);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Packed RGB24: one wave per tile of RGB cubes, its three channels in turn (decode_rgb_kernel)
int launch_decode_rgb(int D, const DecodeParams& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    const dim3 grid(dec_grid(D, P.n_cubes));
    if (D == 8) hipLaunchKernelGGL((decode_rgb_kernel<8>), grid, dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL((decode_rgb_kernel<4>), grid, dim3(kBlock), 0, st, P);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace dct3d
