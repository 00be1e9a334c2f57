// dct3d_quant_eg.hip -- quantiser tables through the fused Exp-Golomb calls (dct3d_encode_eg* /
// dct3d_decode_eg*, the _frames calls included): the QT = 1 instantiations of the fused kernels
// (dct3d_eg_fused_dev.h) for every geometry, and their launchers.  As dct3d_quant.hip: the encode differs in
// its DC and its exact replay's divisor, the decode in where its steps come from (decode_tile<CODES>: the
// lane's 11 steps as integers for the |q| * step products; the stream re-parse of the exact replay).  The
// grey stream decode is built at 8 groups per wave only, the product's default.  A translation unit of its
// own: no other code object changes, and a context with the reference table never comes here.
#include "dct3d_eg_fused_dev.h"

namespace dct3d {

namespace {
template <int D, int PX, int EDGE>
void launch_enc_egq_t(const EncodeParams& P, const EgFusedParams& E, hipStream_t st) {
    const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
    hipLaunchKernelGGL((encode_eg_kernel<D, PX, EDGE, 1>), grid, dim3(kBlock), 0, st, P, E);
}
template <int D>
void launch_enc_egq_d(int px, int edge, const EncodeParams& P, const EgFusedParams& E, hipStream_t st) {
    if (px == 1 && !edge) launch_enc_egq_t<D, 1, 0>(P, E, st);
    else if (px == 1) launch_enc_egq_t<D, 1, 1>(P, E, st);
    else if (edge) launch_enc_egq_t<D, 3, 1>(P, E, st);
    else launch_enc_egq_t<D, 3, 0>(P, E, st);
}
template <int D, int EDGE>
void launch_dec_egq_t(const DecodeParamsQ& P, const EgDecParams& E, hipStream_t st) {
    const dim3 grid(dec_grid(D, P.n_cubes - P.cube_base, 8));  // cube_base: a multiple of the cubes per wave
    hipLaunchKernelGGL((decode_eg_kernel<D, 8, EDGE, 1>), grid, dim3(kBlock), 0, st, P, E);
}
template <int D, int EDGE>
void launch_dec_egrq_t(const DecodeParamsQ& P, const EgDecRgbParams& E, hipStream_t st) {
    const dim3 grid(dec_grid(D, P.n_cubes - P.cube_base));
    hipLaunchKernelGGL((decode_eg_rgb_kernel<D, EDGE, 1>), grid, dim3(kBlock), 0, st, P, E);
}
}  // namespace

int launch_encode_eg_qt(int D, int px, int edge, const EncodeParams& P, const EgFusedParams& E, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (px != 1 && px != 3) return -1;
    if (D == 8) launch_enc_egq_d<8>(px, edge, P, E, st);
    else launch_enc_egq_d<4>(px, edge, P, E, st);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_decode_eg_qt(int D, int edge, const DecodeParamsQ& P, const EgDecParams& E, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!P.steps) return -1;
    if (D == 8) {
        if (edge) launch_dec_egq_t<8, 1>(P, E, st);
        else launch_dec_egq_t<8, 0>(P, E, st);
    } else {
        if (edge) launch_dec_egq_t<4, 1>(P, E, st);
        else launch_dec_egq_t<4, 0>(P, E, st);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_decode_eg_rgb_qt(int D, int edge, const DecodeParamsQ& P, const EgDecRgbParams& E, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!P.steps) return -1;
    if (D == 8) {
        if (edge) launch_dec_egrq_t<8, 1>(P, E, st);
        else launch_dec_egrq_t<8, 0>(P, E, st);
    } else {
        if (edge) launch_dec_egrq_t<4, 1>(P, E, st);
        else launch_dec_egrq_t<4, 0>(P, E, st);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace dct3d
