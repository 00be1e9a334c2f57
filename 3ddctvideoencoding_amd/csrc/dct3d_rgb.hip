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
    if (D == 8) {
        const uint32_t groups = (P.n_cubes - P.g_base + kE16CPW - 1) / kE16CPW;
        const uint32_t blocks = (groups + kWavesPerBlock - 1) / kWavesPerBlock;
        hipLaunchKernelGGL((encode16_rgb_kernel<true>), dim3(blocks), dim3(kBlock), 0, st, P);
    } else {
        const uint32_t groups = (P.n_cubes - P.g_base + kCubesPerWave - 1) / kCubesPerWave;
        const uint32_t blocks = (groups + kWavesPerBlock - 1) / kWavesPerBlock;
        hipLaunchKernelGGL((encode_rgb_kernel<4, true>), dim3(blocks), dim3(kBlock), 0, st, P);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Packed RGB24: one wave per tile of RGB cubes, its three channels in turn (decode_rgb_kernel)
int launch_decode_rgb(int D, const DecodeParams& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    const uint32_t per = (D == 8 ? DecGeom<8>::CPW : DecGeom<4>::CPW) * kWavesPerBlock;
    const uint32_t groups = (uint32_t)((P.n_cubes + per - 1) / per);
    if (D == 8) hipLaunchKernelGGL((decode_rgb_kernel<8, 1>), dim3(groups), dim3(kBlock), 0, st, P);
    else hipLaunchKernelGGL((decode_rgb_kernel<4, 1>), dim3(groups), dim3(kBlock), 0, st, P);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace dct3d
