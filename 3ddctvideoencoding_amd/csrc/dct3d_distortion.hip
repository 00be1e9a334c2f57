// dct3d_distortion.hip -- the distortion probe (dct3d_distortion_frames*): the exact squared error
// of encode + decode under several quantiser tables, from one row load and one forward transform per cube.
// Per table the wave quantises and certifies its cubes as the encode does, puts the integers where the decode
// expects its staged input, runs the certified fp64 decode tile with the bytes kept in registers, and compares
// them with the rows it started from.  No coefficient and no decoded raster exists in memory.  The kernel's body
// is distortion_body (dct3d_distortion_dev.h), shared with the RGB-domain probe's colour planes.  A
// translation unit of its own: no other kernel's code object changes with it.
// The SSIM probe (dct3d_ssim_frames*) is an arm of the same kernel -- the moments of the frames' 4 x 4
// blocks from the same bytes -- and two small kernels that turn the blocks' records into the windows' values.
#include "dct3d_distortion.h"
#include "dct3d_distortion_dev.h"
#include <type_traits>

namespace dct3d {

// distortion_body (dct3d_distortion_dev.h) on channel R.ch of the frames; SSIM = 1: with the block moments
template <int SSIM>
using DistKernelParams = std::conditional_t<SSIM != 0, SsimParams, DistParams>;
template <int D, int PX, int EDGE, int SSIM = 0>
__global__ __launch_bounds__(kBlock, 2) void distortion_kernel(EncodeParams P, DistKernelParams<SSIM> R) {
    distortion_body<D, PX, EDGE, SSIM, 0>(P, R);
}

// One block per run of `run` cubes (a table's stack and channel): their sum (rate_sum_kernel for uint32)
__global__ __launch_bounds__(kBlock) void distortion_sum_kernel(const uint32_t* cube_sse, uint32_t run, uint64_t* out) {
    const uint32_t* p = cube_sse + (size_t)blockIdx.x * run;
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < run; i += kBlock) s += p[i];
    const uint64_t r = probe_block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

template <int SSIM>
static int launch_distortion_t(int D, int px, int edge, const EncodeParams& P, const DistKernelParams<SSIM>& R, hipStream_t st) {
    return probe_dispatch(D, px, edge, P, R, [&](auto d, auto p, auto e) {
        const dim3 grid(grid_blocks(P.n_cubes, DecGeom<decltype(d)::value>::CPW));
        hipLaunchKernelGGL((distortion_kernel<decltype(d)::value, decltype(p)::value, decltype(e)::value, SSIM>), grid, dim3(kBlock), 0, st, P, R);
    });
}
int launch_distortion(int D, int px, int edge, const EncodeParams& P, const DistParams& R, hipStream_t st) {
    return launch_distortion_t<0>(D, px, edge, P, R, st);
}
int launch_distortion_ssim(int D, int px, int edge, const EncodeParams& P, const SsimParams& R, hipStream_t st) {
    return launch_distortion_t<1>(D, px, edge, P, R, st);
}

int launch_distortion_sum(const uint32_t* cube_sse, uint32_t run, uint64_t n_runs, uint64_t* out, hipStream_t st) {
    if (n_runs == 0) return 0;
    if (n_runs > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(distortion_sum_kernel, dim3((uint32_t)n_runs), dim3(kBlock), 0, st, cube_sse, run, out);
    return launched();
}

// ---- the SSIM probe's windows (dct3d.h states the definition) ----
// One thread per window of (table blockIdx.z, stack blockIdx.y): the moments of its 1, 2 or 4 blocks, n from the
// geometry, A, B, C, D in int64, s = fl(fl(A B) / fl(C D)), v = floor(s 2^24); the block's sum of v
__global__ __launch_bounds__(kBlock) void ssim_window_kernel(SsimWinParams W) {
    const uint32_t t = blockIdx.z, s = blockIdx.y;
    const uint32_t per_frame = W.nwx * W.nwy, per_stack = per_frame * W.depth;
    const uint64_t* const by_ = W.blk_y + (size_t)t * W.blk_stride;
    int64_t sum = 0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < per_stack; i += W.bpr * kBlock) {
        const uint32_t z = i / per_frame, r = i - z * per_frame;
        const uint32_t j = r / W.nwx, x = r - j * W.nwx;
        const uint32_t x1 = min(x + 1u, W.nbx - 1u), j1 = min(j + 1u, W.nby - 1u);
        const size_t f0 = ((size_t)s * W.depth + z) * W.nby;
        int64_t Sx = 0, Sy = 0, Sxx = 0, Syy = 0, Sxy = 0;
        for (uint32_t bj = j; bj <= j1; bj++)
            for (uint32_t bi = x; bi <= x1; bi++) {
                const size_t b = (f0 + bj) * W.nbx + bi;
                const uint64_t my = by_[b];
                const uint32_t mx = W.blk_x[b];
                Sx += mx & 0xFFFu;
                Sxx += mx >> 12;
                Sy += (uint32_t)my & 0xFFFu;
                Syy += (uint32_t)my >> 12;
                Sxy += (uint32_t)(my >> 32);
            }
        const int64_t n = (int64_t)(min(4u * x + 8u, W.w) - 4u * x) * (int64_t)(min(4u * j + 8u, W.h) - 4u * j);
        const int64_t n2 = n * n, xy = Sx * Sy, xx = Sx * Sx, yy = Sy * Sy;
        const int64_t A = 20000 * xy + 65025 * n2;
        const int64_t B = 20000 * (n * Sxy - xy) + 585225 * n2;
        const int64_t Cc = 10000 * (xx + yy) + 65025 * n2;
        const int64_t Dd = 10000 * (n * Sxx - xx + n * Syy - yy) + 585225 * n2;
        const double q = __ddiv_rn(__dmul_rn((double)A, (double)B), __dmul_rn((double)Cc, (double)Dd));
        const int32_t v = (int32_t)floor(__dmul_rn(q, 16777216.0));
        if (W.win) W.win[(size_t)t * W.win_t + (size_t)s * W.win_s + i] = v;
        sum += v;
    }
    const uint64_t r = probe_block_sum((uint64_t)sum);
    if (threadIdx.x == 0) W.part[((size_t)t * W.ns + s) * W.bpr + blockIdx.x] = (int64_t)r;
}

// One block per (stack blockIdx.x, table blockIdx.y): the sum of its bpr partial sums
__global__ __launch_bounds__(kBlock) void ssim_sum_kernel(const int64_t* part, uint32_t bpr, int64_t* out, uint64_t out_t,
                                                          uint64_t out_s) {
    const int64_t* p = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * bpr;
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < bpr; i += kBlock) s += (uint64_t)p[i];
    const uint64_t r = probe_block_sum(s);
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * out_t + (size_t)blockIdx.x * out_s] = (int64_t)r;
}

int launch_ssim_window(const SsimWinParams& W, hipStream_t st) {
    if (W.ns == 0 || W.n_tables == 0) return 0;
    if (W.ns > 65535u || W.n_tables > 65535u || W.bpr == 0) return -1;
    hipLaunchKernelGGL(ssim_window_kernel, dim3(W.bpr, W.ns, W.n_tables), dim3(kBlock), 0, st, W);
    return launched();
}

int launch_ssim_sum(const int64_t* part, uint32_t bpr, uint32_t ns, uint32_t n_tables, int64_t* out, uint64_t out_t,
                    uint64_t out_s, hipStream_t st) {
    if (ns == 0 || n_tables == 0) return 0;
    if (n_tables > 65535u) return -1;
    hipLaunchKernelGGL(ssim_sum_kernel, dim3(ns, n_tables), dim3(kBlock), 0, st, part, bpr, out, out_t, out_s);
    return launched();
}

}  // namespace dct3d
