// dct3d_rate.h -- the rate probe's kernel parameters and launchers (dct3d_rate.hip), shared with
// the probes' host unit (dct3d_probes.cpp).
#pragma once
#include "dct3d_kernels.h"

namespace dct3d {

constexpr int kRateTables = 8;   // quantiser tables priced by one launch (their rows live in the block's LDS)
constexpr int kRateTabN = 24;    // rows per table, s = kx + ky + kz < 22 (== kTabN, dct3d_encode_dev.h)

// rate_kernel prices channel `ch` of the cubes of EncodeParams P (as launch_encode_eg's: raster and
// address fields, the fold tables ngroups / coef / group_of, coef_dc, the counter slots) under n_tables tables.
struct RateParams {
    const float4* tabs;     // [n_tables][kRateTabN] {fp32(1 / step_s), G_s, 0.5 - E_s, step_s}
    uint16_t* cube_bits;    // [n_tables][table_stride]: bits of cube g of channel ch at enc_out_cube
                            // ([stack][channel][cube] within a table)
    uint64_t table_stride;  // cubes of one table: channels * P.n_cubes
    int n_tables;           // 1 .. kRateTables
    int ch;
};

// px = 1 grey | 3 packed RGB24, edge = 0 | 1 (frames of any size)
int launch_rate(int D, int px, int edge, const EncodeParams& P, const RateParams& R, hipStream_t st);
// packed RGB24 with the YCbCr colour transform: channel R.ch of the Y, Cb, Cr planes (dct3d_ycc.hip)
int launch_rate_ycc(int D, int edge, const EncodeParams& P, const RateParams& R, hipStream_t st);
// out[r] = the sum of cube_bits[r * run .. r * run + run), r < n_runs
int launch_rate_sum(const uint16_t* cube_bits, uint32_t run, uint64_t n_runs, uint64_t* out, hipStream_t st);

}  // namespace dct3d
