// dct3d_c420.h -- 4:2:0 chroma subsampling in the YCbCr stream calls and the rate probe (dct3d_ctx_set_chroma;
// DESIGN 4q): the launchers of dct3d_c420.hip and the decode's extra parameter, shared with the C-ABI runtime.
// The kernels are keyed (D, edge, qt) here and are no variant of the stream family (dct3d_variant.h): the colour
// axis keeps its two values.
#pragma once
#include "dct3d_kernels.h"
#include "dct3d_rate.h"

namespace dct3d {

// The decoded chroma planes of a call (or of a chunk of its stacks, rebased like the raster): S(Cb) and S(Cr),
// uint8 [stack * D + frame][ceil(h / 2)][ceil(w / 2)], dense, written by the grey stream decode at that geometry.
struct C420Planes {
    const uint8_t* cb;
    const uint8_t* cr;
};

// Channel E.ch = 1 | 2 of a packed RGB24 call under 4:2:0.  P: the cube fields (n_cubes, cubes_per_stack, nbx, the
// FastDivs) of the chroma plane, the address fields (width, height, plane, stack_stride) of the frames, height set
// whatever the edge.  edge: the width or the height is no multiple of 16.  qt, V: as launch_encode_eg's.
int launch_encode_eg_c420(int D, int edge, int qt, const EncodeParams& P, const EgFusedParams& E, const VqParams* V, hipStream_t st);
// the rate probe's chroma launch (P likewise; R.cube_bits: the plane's cubes alone)
int launch_rate_c420(int D, int edge, const EncodeParams& P, const RateParams& R, hipStream_t st);
// Stream 0 (Y) of E -> the packed frames, with the chroma of C upsampled by replication and the inverse colour
// transform before the one store; nothing is stored unless all three fronts of E are good.  P: as
// launch_decode_eg_rgb's, height set whatever the edge.  edge: the width or the height is no multiple of 8.
int launch_decode_eg_y420(int D, int edge, int qt, const DecodeParamsQ& P, const EgDecRgbParams& E, const C420Planes& C,
                          const VqParams* V, hipStream_t st);

}  // namespace dct3d
