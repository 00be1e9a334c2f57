// dct3d_rate.hip -- the rate probe (dct3d_rate_frames*): the exact Exp-Golomb size of every cube
// under several quantiser tables, from one transform per cube.  The width of a code does not depend on its
// place in the stream, so a cube's cost is a plain sum over its coefficients: nothing is staged in diagonal
// order, emitted or compacted, and the fp32 transform does not depend on the table.  A translation unit of
// its own: no other kernel's code object changes with it.
#include "dct3d_rate_dev.h"

namespace dct3d {

// One block per run of `run` cubes (a table's stack and channel): their sum.  The body goes as 8-byte loads
// from the first 8-byte boundary; the few values before and after it one by one.
__global__ __launch_bounds__(kBlock) void rate_sum_kernel(const uint16_t* cube_bits, uint32_t run, uint64_t* out) {
    const uint16_t* p = cube_bits + (size_t)blockIdx.x * run;
    const uint32_t head = min(run, (uint32_t)(((8u - ((uintptr_t)p & 7u)) & 7u) / 2u));
    const uint32_t nvec = (run - head) / 4u;
    const uint2* v = (const uint2*)(p + head);
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < nvec; i += kBlock) {
        const uint2 t = v[i];
        s += (t.x & 0xFFFFu) + (t.x >> 16) + (t.y & 0xFFFFu) + (t.y >> 16);
    }
    if (threadIdx.x < head) s += p[threadIdx.x];
    for (uint32_t i = head + nvec * 4u + threadIdx.x; i < run; i += kBlock) s += p[i];
    const uint64_t r = probe_block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

int launch_rate(int D, int px, int edge, const EncodeParams& P, const RateParams& R, hipStream_t st) {
    return probe_dispatch(D, px, edge, P, R, [&](auto d, auto p, auto e) {
        const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
        hipLaunchKernelGGL((rate_kernel<decltype(d)::value, decltype(p)::value, decltype(e)::value>), grid, dim3(kBlock), 0, st, P, R);
    });
}

int launch_rate_sum(const uint16_t* cube_bits, uint32_t run, uint64_t n_runs, uint64_t* out, hipStream_t st) {
    if (n_runs == 0) return 0;
    if (n_runs > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(rate_sum_kernel, dim3((uint32_t)n_runs), dim3(kBlock), 0, st, cube_bits, run, out);
    return launched();
}

}  // namespace dct3d
