// dct3d_distortion.h -- the distortion probe's kernel parameters and launchers (dct3d_distortion.hip; DESIGN
// 4j), shared with the C-ABI runtime.
#pragma once
#include "dct3d_rate.h"

namespace dct3d {

constexpr int kDistStepN = 32;  // fp64 steps per table, s = kx + ky + kz (as DecodeParamsQ::steps)

// distortion_kernel codes channel `ch` of the cubes of EncodeParams P (as launch_rate's) under n_tables tables
// and decodes them again: per table and cube the squared error of the decoded bytes against the source bytes
// inside the frame, and optionally the cube's Exp-Golomb bits.
struct DistParams : RateParams {  // (cube_bits may be nullptr here)
    const double* steps;       // [n_tables][kDistStepN] the decode's steps
    uint32_t* cube_sse;        // [n_tables][table_stride]: cube g of channel ch at enc_out_cube
    const double* inv_coef_t;  // the decode's certificate and replay (as DecodeParams)
    double dec_G, dec_E;
    float dec_l1_max;
};

// px = 1 grey | 3 packed RGB24, edge = 0 | 1 (frames of any size)
int launch_distortion(int D, int px, int edge, const EncodeParams& P, const DistParams& R, hipStream_t st);
// out[r] = the sum of cube_sse[r * run .. r * run + run), r < n_runs
int launch_distortion_sum(const uint32_t* cube_sse, uint32_t run, uint64_t n_runs, uint64_t* out, hipStream_t st);

}  // namespace dct3d
