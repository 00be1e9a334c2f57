// dct3d_distortion.h -- the distortion probe's kernel parameters and launchers (dct3d_distortion.hip; DESIGN
// 4j), shared with the probes' host unit (dct3d_probes.cpp).
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

// The SSIM probe's arm of distortion_kernel (dct3d_ssim_frames*): besides the above (cube_sse may be
// nullptr here) the moments of every 4 x 4 block of the frames, block (frame f of P's stacks, by, bx) at
// (f * nby + by) * nbx + bx.  blk_y per table: Sy | Syy << 12 | Sxy << 32 over the block's samples inside the
// frame (16 x 255 < 2^12, 16 x 255^2 < 2^20); blk_x once: Sx | Sxx << 12.
struct SsimParams : DistParams {
    uint64_t* blk_y;      // [n_tables][blk_stride]
    uint32_t* blk_x;      // [blk_stride]
    uint64_t blk_stride;  // >= frames x nby x nbx
    uint32_t nbx, nby;    // ceil(w / 4), ceil(h / 4)
};

// ssim_window_kernel: the windows of channel ch of ns stacks under n_tables tables from the block records; window
// i of a stack is (frame z, row j, column x) at (z * nwy + j) * nwx + x
constexpr uint32_t kSsimWinPerBlock = 1024;  // windows a block takes where a stack has that many (4 per thread)
constexpr uint32_t kSsimMaxBpr = 1024;
struct SsimWinParams {
    const uint64_t* blk_y;
    const uint32_t* blk_x;
    uint64_t blk_stride;
    int32_t* win;  // nullptr | the v of window i of table t, stack s at win[t * win_t + s * win_s + i]
    uint64_t win_t, win_s;
    int64_t* part;  // [n_tables][ns][bpr] the blocks' sums of v
    uint32_t w, h, nbx, nby, nwx, nwy, depth;
    uint32_t ns, n_tables, bpr;  // bpr: blocks per (table, stack)
};

// px = 1 grey | 3 packed RGB24, edge = 0 | 1 (frames of any size)
int launch_distortion(int D, int px, int edge, const EncodeParams& P, const DistParams& R, hipStream_t st);
int launch_distortion_ssim(int D, int px, int edge, const EncodeParams& P, const SsimParams& R, hipStream_t st);
int launch_ssim_window(const SsimWinParams& W, hipStream_t st);
// out[(t * out_t + s) * out_s] = the sum of part[t][s][0 .. bpr), t < n_tables, s < ns
int launch_ssim_sum(const int64_t* part, uint32_t bpr, uint32_t ns, uint32_t n_tables, int64_t* out, uint64_t out_t,
                    uint64_t out_s, hipStream_t st);
// out[r] = the sum of cube_sse[r * run .. r * run + run), r < n_runs
int launch_distortion_sum(const uint32_t* cube_sse, uint32_t run, uint64_t n_runs, uint64_t* out, hipStream_t st);

}  // namespace dct3d
