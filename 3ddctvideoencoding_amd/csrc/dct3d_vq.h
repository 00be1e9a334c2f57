// dct3d_vq.h -- per-stack quantiser tables in the fused stream calls (dct3d_encode_eg_frames_vq* /
// dct3d_decode_eg_frames_vq*): the kernels' extra parameter and the upload of a call's block,
// shared with the C-ABI runtime.  The kernels are the QT = 2 instances of the shared stream kernels
// (dct3d_eg_fused_dev.h, which includes this header for VqParams): qt = 2 of the variant (dct3d_variant.h), launched
// by the stream ladders (dct3d_launch.h) in the StreamVq unit, with the colour transform in StreamYcc.
#pragma once
#include "dct3d_kernels.h"

namespace dct3d {

constexpr int kVqMaxTables = 32;  // == DCT3D_RATE_MAX_TABLES: the palette's size
constexpr int kVqTabN = 24;       // rows per table (== kTabN: asserted in dct3d_eg_fused_dev.h)
constexpr int kVqStepN = 32;      // fp64 steps per table (the decode kernels' layout, as distortion_kernel's)

// The palette and the map of one call.  Cube g (global index: the encode's from 0, the decode's from
// P.cube_base on) lies in stack g / cubes_per_stack and is coded with table map[that stack].
// In device memory the steps are a block of kVqMaxTables tables whatever n_tables is, followed by the FastDiv of
// cubes_per_stack and then the map itself (vq_div_behind, vq_map_behind): the decode's rare exact replay finds
// all three from `steps` alone, so its reload functor is no larger than the QT = 1 kernels' (one more member
// and it no longer travels in registers into the replay's out-of-line body: the kernel would take scratch).
struct VqParams {
    const float4* tabs;   // encode: [n_tables][kVqTabN] {fp32(1 / step_s), G_s, 0.5 - E_s, step_s}
    const double* steps;  // decode: [kVqMaxTables][kVqStepN] step_s (the first n_tables filled)
    const uint8_t* map;   // [n_stacks] table of each stack, < n_tables; == vq_map_behind(steps)
};
// A table per (stack, channel) (the _vqc calls): every channel has a block {steps, FastDiv, map column} of
// its own and a launch is handed its channel's VqParams -- but for decode_eg_rgb_kernel, which walks the three
// channels itself.  Its _vqc instances take this: channel ch's block begins ch * ch_stride bytes behind `steps`
// (`map`: channel 0's column).  The _vq calls keep the VqParams instances, whose text is as it was.
struct VqcParams : VqParams {
    uint32_t ch_stride;
};
constexpr size_t kVqStepsBytes = (size_t)kVqMaxTables * kVqStepN * sizeof(double);
__host__ __device__ inline const FastDiv* vq_div_behind(const double* steps) {
    return (const FastDiv*)((const char*)steps + kVqStepsBytes);
}
__host__ __device__ inline const uint8_t* vq_map_behind(const double* steps) {
    return (const uint8_t*)steps + kVqStepsBytes + sizeof(FastDiv);
}

// A call's block (steps, FastDiv, map, rows: some KiB) from the context's pinned host copy -- src, its device-side
// address -- to device memory, as a kernel on the call's stream: a copy-engine transfer in front of the first
// kernel cost the call a hand-over between two queues, longer than the transfer itself.
// n16: 16-byte words; both buffers hold that many.
int launch_vq_upload(const void* src, void* dst, uint32_t n16, hipStream_t st);

}  // namespace dct3d
