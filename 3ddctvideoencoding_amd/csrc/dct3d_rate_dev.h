// dct3d_rate_dev.h -- device code the probes share (dct3d_rate.hip, dct3d_distortion.hip): the width of an
// Exp-Golomb code and the Java fold of one coefficient up to the division by a table's step.
#pragma once
#include "dct3d_encode_dev.h"

namespace dct3d {

// Bits of the signed order-0 Exp-Golomb code of q (ExpGolomb.c:32-64): code = max(2q, 1 - 2q), 2n - 1 bits for
// a code of n bits
__device__ __forceinline__ uint32_t rate_width(int q) {
    const uint32_t code = (uint32_t)(q > 0 ? 2 * q : 1 - 2 * q);
    return 63u - 2u * (uint32_t)__builtin_clz(code);
}

// The Java fold of one coefficient (replay_fold's sums, products and fold order: DCT.java:44-52) up to the
// division: the folded value itself, valid in lane 0.  It does not depend on the table; the caller divides it
// by each table's step.
__device__ __forceinline__ double rate_fold(const ReplayIn& in, int cs, int lane, int* ssum, double* prod) {
    ssum[lane] = 0;
    wave_lds_sync();
    if (lane * 8 < cs) {
#pragma unroll
        for (int bb = 0; bb < 4; bb++) {
            const uint32_t g0 = (in.gr.x >> (8 * bb)) & 0xFF, g1 = (in.gr.y >> (8 * bb)) & 0xFF;
            if (g0 < kMaxGroupsDev) atomicAdd(&ssum[g0], (int)((in.px.x >> (8 * bb)) & 0xFF));
            if (g1 < kMaxGroupsDev) atomicAdd(&ssum[g1], (int)((in.px.y >> (8 * bb)) & 0xFF));
        }
    }
    wave_lds_sync();
    prod[lane] = __dmul_rn((double)ssum[lane], lane < in.ng ? in.cf : 0.0);
    wave_lds_sync();
    double acc = 0.0;
    if (lane == 0) {
#pragma unroll 1
        for (int gi = 0; gi < in.ng; gi++) acc = __dadd_rn(acc, prod[gi]);  // DCT.java:50, in order
    }
    wave_lds_sync();
    return acc;
}

}  // namespace dct3d
