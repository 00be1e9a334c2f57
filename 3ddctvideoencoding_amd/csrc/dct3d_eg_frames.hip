// dct3d_eg_frames.hip -- the fused Exp-Golomb calls for frames of any size and packed RGB24
// (dct3d_encode_eg_frames* / dct3d_decode_eg_frames*): raster -> one Exp-Golomb stream per channel and back,
// with no int32 cube-major intermediate.  The device code is the fused kernels' (dct3d_eg_fused_dev.h) with
// the edge padding / crop (EDGE = 1) and the channel pick / mix (PX = 3) in its
// addressing.  A translation unit of its own: the other kernels' code objects do not change with it, and a
// grey geometry whose width and height are multiples of 8 never comes here.
#include "dct3d_eg_fused_dev.h"

namespace dct3d {

namespace {
template <int D, int PX, int EDGE>
void launch_enc_egf_t(const EncodeParams& P, const EgFusedParams& E, hipStream_t st) {
    const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
    hipLaunchKernelGGL((encode_eg_kernel<D, PX, EDGE>), grid, dim3(kBlock), 0, st, P, E);
}
template <int D>
void launch_enc_egf_d(int px, int edge, const EncodeParams& P, const EgFusedParams& E, hipStream_t st) {
    if (px == 1) launch_enc_egf_t<D, 1, 1>(P, E, st);
    else if (edge) launch_enc_egf_t<D, 3, 1>(P, E, st);
    else launch_enc_egf_t<D, 3, 0>(P, E, st);
}
template <int D, int NG>
void launch_dec_ege_t(const DecodeParams& P, const EgDecParams& E, hipStream_t st) {
    const dim3 grid(dec_grid(D, P.n_cubes - P.cube_base, NG));  // cube_base: a multiple of the cubes per wave
    hipLaunchKernelGGL((decode_eg_kernel<D, NG, 1>), grid, dim3(kBlock), 0, st, P, E);
}
template <int D, int EDGE>
void launch_dec_egr_t(const DecodeParams& P, const EgDecRgbParams& E, hipStream_t st) {
    const dim3 grid(dec_grid(D, P.n_cubes - P.cube_base));
    hipLaunchKernelGGL((decode_eg_rgb_kernel<D, EDGE>), grid, dim3(kBlock), 0, st, P, E);
}
}  // namespace

int launch_encode_eg_frames(int D, int px, int edge, const EncodeParams& P, const EgFusedParams& E, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if ((px != 1 && px != 3) || (px == 1 && !edge)) return -1;
    if (D == 8) launch_enc_egf_d<8>(px, edge, P, E, st);
    else launch_enc_egf_d<4>(px, edge, P, E, st);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_decode_eg_edge(int D, const DecodeParams& P, const EgDecParams& E, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (D == 8) launch_dec_ege_t<8, 8>(P, E, st);
    else launch_dec_ege_t<4, 8>(P, E, st);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_decode_eg_rgb(int D, int edge, const DecodeParams& P, const EgDecRgbParams& E, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (D == 8) {
        if (edge) launch_dec_egr_t<8, 1>(P, E, st);
        else launch_dec_egr_t<8, 0>(P, E, st);
    } else {
        if (edge) launch_dec_egr_t<4, 1>(P, E, st);
        else launch_dec_egr_t<4, 0>(P, E, st);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace dct3d
