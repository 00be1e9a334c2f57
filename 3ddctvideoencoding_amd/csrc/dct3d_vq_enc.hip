// dct3d_vq_enc.hip -- the fused stream encode with a quantiser table per stack (dct3d_encode_eg_frames_vq*;
// DESIGN 4m, 4n): the launcher of encode_eg_kernel<D, PX, EDGE, QT = 2> (dct3d_eg_fused_dev.h: the shared body,
// the per-stack table as its QT = 2 arms) and the copy kernel that brings a call's block to the device.
// A translation unit of its own: no other code object changes.
#include "dct3d_eg_fused_dev.h"

namespace dct3d {

__global__ __launch_bounds__(kBlock) void vq_upload_kernel(const uint4* src, uint4* dst, uint32_t n16) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}

int launch_vq_upload(const void* src, void* dst, uint32_t n16, hipStream_t st) {
    if (n16 == 0) return 0;
    if (!src || !dst) return -1;
    hipLaunchKernelGGL(vq_upload_kernel, dim3((n16 + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const uint4*)src, (uint4*)dst, n16);
    return launched();
}

int launch_encode_eg_vq(int D, int px, int edge, const EncodeParams& P, const EgFusedParams& E, const VqParams& V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!V.tabs || !V.map) return -1;
    int rc = -1;
    with_variant(D, px, edge, [&](auto d, auto p, auto e) {
        const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
        hipLaunchKernelGGL((encode_eg_kernel<d, p, e, 2, 0, VqParams>), grid, dim3(kBlock), 0, st, P, E, V);
        rc = launched();
    });
    return rc;
}

}  // namespace dct3d
