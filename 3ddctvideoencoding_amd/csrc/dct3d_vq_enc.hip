// dct3d_vq_enc.hip -- the fused stream encode with a quantiser table per stack (dct3d_encode_eg_frames_vq*;
// DESIGN 4m, 4n, 4p): the StreamVq unit's encode ladder, encode_eg_kernel<D, PX, EDGE, QT = 2> (dct3d_eg_fused_dev.h:
// the shared body, the per-stack table as its QT = 2 arms), and the copy kernel that brings a call's block to the
// device.
// A translation unit of its own: no other code object changes.
#include "dct3d_launch.h"

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

template int launch_encode_eg_in<StreamVq>(const Variant&, const EncodeParams&, const EgFusedParams&, const VqParams*, hipStream_t);

}  // namespace dct3d
