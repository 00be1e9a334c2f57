// dct3d_distortion_rgb.h -- the RGB-domain distortion probe's kernel parameters and launchers
// (dct3d_distortion_rgb.hip; dct3d_distortion_rgb_frames*), shared with the probes' host unit
// (dct3d_probes.cpp).
#pragma once
#include "dct3d_distortion.h"

namespace dct3d {

// Pass 1, one plane of the YCbCr transform of packed RGB24 frames: distortion_kernel's work on plane R.ch (ct = 1:
// the plane at the frames' size; ct = 2: the 4:2:0 subsampled plane R.ch = 1 | 2, P as launch_rate_c420's), with
// the decoded samples inside the plane kept: table t of the launch writes the dense plane
// uint8 [stack * D + frame][ph][pw] at planes + t * plane_stride (C420Planes' layout).  cube_sse and cube_bits hold
// the plane's cubes alone: cube g of table t at t * table_stride + g.
struct DistPlaneParams : DistParams {
    uint8_t* planes;
    uint64_t plane_stride;  // bytes from one table's plane to the next
    uint32_t pw, ph;        // the plane's samples: the mask of the squared error and the bounds of the stores
};
// edge: ct = 1: pw or ph is no multiple of 8; ct = 2: the frames' width or height is no multiple of 16
int launch_distortion_plane(int D, int edge, int ct, const EncodeParams& P, const DistPlaneParams& R, hipStream_t st);

// Pass 2: per candidate c and cube g of the frames' grid, the squared error of the source pixels against
// ycc_to_rgb of the decoded planes Y = y + slot[c][0] * y_stride, Cb = cb + slot[c][1] * c_stride, Cr = cr +
// slot[c][2] * c_stride, over the cube's pixels inside the frame.  The chroma sample of pixel (row, col) is
// (row >> shift, col >> shift) of a cw x chh plane (shift = 0: 4:4:4, the planes at the frames' size; 1: 4:2:0).
struct RgbCombineParams {
    const uint8_t* frames;  // packed RGB24 [stack * D + frame][h][w][3]
    const uint8_t *y, *cb, *cr;
    uint64_t y_stride, c_stride;
    uint32_t w, h, cw, chh, shift;
    uint32_t nbx, cubes_per_stack, n_cubes;  // the frames' padded grid; n_cubes < 2^31
    FastDiv div_cps, div_nbx;
    const uint8_t* slots;  // device [n_cand][3]
    uint32_t n_cand;
    uint32_t* cube_sse;    // candidate c, cube g at c * cand_stride + g
    uint64_t cand_stride;
};
int launch_distortion_rgb_combine(int D, const RgbCombineParams& C, hipStream_t st);

// The RGB and luma SSIM probe's pass 2: C as above (cube_sse and cand_stride unused) and, in the SSIM
// probe's record formats (SsimParams), the 4 x 4 blocks' moments of planes R, G, B (and, luma = 1, plane 3: the
// source's luma against the decoded Y) between the source pixels and the candidate's decoded pixels.  Block
// (frame f of C's stacks, by, bx) at i = (f * nby4 + by) * nbx4 + bx: blk_y[(k * n_cand + c) * blk_stride + i],
// blk_x[k * blk_stride + i] (candidate 0's threads write it).
struct SsimRgbParams {
    RgbCombineParams C;
    uint64_t* blk_y;
    uint32_t* blk_x;
    uint64_t blk_stride;   // >= frames x nby4 x nbx4
    uint32_t nbx4, nby4;   // ceil(w / 4), ceil(h / 4)
};
int launch_ssim_rgb_block(int D, int luma, const SsimRgbParams& S, hipStream_t st);

// Planes mode: out[c * out_stride + s * cps + g] = sum over k < 3 of in[slots[c][k] * in_stride + (3 s + k) * cps + g]
// (in: the distortion probe's per-cube buffer of one table, [stack][channel][cube])
int launch_distortion_rgb_gather(const uint32_t* in, uint64_t in_stride, const uint8_t* slots, uint32_t n_cand, uint32_t cps,
                                 uint32_t n_stacks, uint32_t* out, uint64_t out_stride, hipStream_t st);

}  // namespace dct3d
