// dct3d_launch.h -- the five kernel families' launch ladders, each written once.  launch_*_in<Unit> walks the
// variant's picks (dct3d_variant.h) and launches under `if constexpr (Unit::holds(...))`: a unit that
// instantiates a ladder builds exactly the kernels its predicate admits, and answers -1 for any other variant
// (a value outside an axis included).  The three stream ladders walk the stream pick (with_stream_variant): the
// table axis to 2 and the colour axis.  A unit's launcher section is one explicit instantiation per family.
#pragma once
#include "dct3d_eg_fused_dev.h"

namespace dct3d {

template <class Unit>
int launch_encode_in(const Variant& v, const EncodeParams& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    int rc = -1;
    with_variant(v, [&](auto d, auto p, auto e, auto q) {
        if constexpr (Unit::holds(d, p, e, q)) {
            hipLaunchKernelGGL((encode_kernel_of<d, p, e, q>()), dim3(enc_grid(d, P)), dim3(kBlock), 0, st, P);
            rc = launched();
        }
    });
    return rc;
}

// (QT = 0: the kernel takes P's DecodeParams part)
template <class Unit>
int launch_decode_in(const Variant& v, const DecodeParamsQ& P, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    int rc = -1;
    with_variant(v, [&](auto d, auto p, auto e, auto q) {
        if constexpr (Unit::holds(d, p, e, q)) {
            if (q && !P.steps) return;
            hipLaunchKernelGGL((decode_kernel_of<d, p, e, q>()), dim3(dec_grid(d, P.n_cubes)), dim3(kBlock), 0, st, P);
            rc = launched();
        }
    });
    return rc;
}

// The three stream ladders walk the table axis to 2, a table per stack: V is then the call's VqParams (null for
// qt < 2) and the kernel's trailing argument.
template <class Unit>
int launch_encode_eg_in(const Variant& v, const EncodeParams& P, const EgFusedParams& E, const VqParams* V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    int rc = -1;
    with_stream_variant(v, [&](auto d, auto p, auto e, auto q, auto ct) {
        if constexpr (Unit::holds(d, p, e, q, ct)) {
            const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
            if constexpr (q == 2) {
                if (!V || !V->tabs || !V->map) return;
                hipLaunchKernelGGL((encode_eg_kernel<d, p, e, 2, ct, VqParams>), grid, dim3(kBlock), 0, st, P, E, *V);
            } else {
                hipLaunchKernelGGL((encode_eg_kernel<d, p, e, q, ct>), grid, dim3(kBlock), 0, st, P, E);
            }
            rc = launched();
        }
    });
    return rc;
}

// grey streams; groups_per_wave: Unit's pick (with_groups).  (QT = 0 and 2: the kernel takes P's DecodeParams part)
template <class Unit>
int launch_decode_eg_in(const Variant& v, const DecodeParamsQ& P, const EgDecParams& E, int groups_per_wave,
                        const VqParams* V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    int rc = -1;
    with_stream_variant(v, [&](auto d, auto p, auto e, auto q, auto ct) {
        if constexpr (p == 1 && Unit::holds(d, p, e, q, ct)) {
            if (q == 2 ? !V || !V->steps || !V->map : q && !P.steps) return;
            with_groups<Unit>(groups_per_wave, [&](auto ng) {
                const dim3 grid(dec_grid(d, P.n_cubes - P.cube_base, ng));  // cube_base: a multiple of the cubes per wave
                if constexpr (q == 2) hipLaunchKernelGGL((decode_eg_kernel<d, ng, e, 2, VqParams>), grid, dim3(kBlock), 0, st, P, E, *V);
                else hipLaunchKernelGGL((decode_eg_kernel<d, ng, e, q>), grid, dim3(kBlock), 0, st, P, E);
            });
            rc = launched();
        }
    });
    return rc;
}

// packed RGB24: three streams.  vq_ch_stride != 0 (a _vqc call, qt = 2): the instances that take a block per channel
// (VqcParams); the _vq calls keep theirs
template <class Unit>
int launch_decode_eg_rgb_in(const Variant& v, const DecodeParamsQ& P, const EgDecRgbParams& E, const VqParams* V,
                            uint32_t vq_ch_stride, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    int rc = -1;
    with_stream_variant(v, [&](auto d, auto p, auto e, auto q, auto ct) {
        if constexpr (p == 3 && Unit::holds(d, p, e, q, ct)) {
            if (q == 2 ? !V || !V->steps || !V->map : q && !P.steps) return;
            const dim3 grid(dec_grid(d, P.n_cubes - P.cube_base));
            if constexpr (q == 2) {
                if (vq_ch_stride)
                    hipLaunchKernelGGL((decode_eg_rgb_kernel<d, e, 2, ct, VqcParams>), grid, dim3(kBlock), 0, st, P, E,
                                       VqcParams{*V, vq_ch_stride});
                else
                    hipLaunchKernelGGL((decode_eg_rgb_kernel<d, e, 2, ct, VqParams>), grid, dim3(kBlock), 0, st, P, E, *V);
            } else {
                hipLaunchKernelGGL((decode_eg_rgb_kernel<d, e, q, ct>), grid, dim3(kBlock), 0, st, P, E);
            }
            rc = launched();
        }
    });
    return rc;
}

}  // namespace dct3d
