// tests/native/emulate_float.cpp -- TEST ONLY: host emulations of the two float kernels' fp64 arithmetic, written from
// the kernels' text and sharing no code with them but the butterfly source (csrc/dct_butterfly.h):
//   * cube_f32_kernel<D, INV> (csrc/dct3d_kernels.hip), drop-in (A): float -> double, passes Y, X, Z with
//     fdct8<false, false>(x, 0.0) / fdctN<D, false, false>, or idct8 / idctN<D>; the inverse's clamp as the kernel
//     writes it; the (float) cast;
//   * fwd64_raster_kernel<D> (csrc/dct3d_kernels_f.hip), the dct_opt output of dct3d_encode_stacks: u8 -> double,
//     passes X, Z, Y.
// The layout changes between the kernels' passes move values and round nothing, so the pass order and the butterfly
// source fix every bit.  Built by the tests with g++ -O2 -ffp-contract=off -fno-fast-math; never linked into the
// product.
#include <cstddef>
#include <cstdint>

#include "dct_butterfly.h"

using namespace dct3d;

namespace {

template <int N, bool INV>
void line(double (&r)[N]) {
    if (INV) idctN<N>(r);
    else fdctN<N, false, false>(r, 0.0);
}

// one pass over a cube b[z][y][x]: AXIS 0 = X, 1 = Y, 2 = Z (N values along it)
template <int D, int AXIS, bool INV>
void pass(double (&b)[D][8][8]) {
    constexpr int N = (AXIS == 2) ? D : 8;
    constexpr int NU = (AXIS == 2) ? 8 : D;  // the slowest of the two other axes
    for (int u = 0; u < NU; u++)
        for (int v = 0; v < 8; v++) {
            double r[N];
            for (int i = 0; i < N; i++) r[i] = AXIS == 0 ? b[u][v][i] : AXIS == 1 ? b[u][i][v] : b[i][u][v];
            line<N, INV>(r);
            for (int i = 0; i < N; i++) (AXIS == 0 ? b[u][v][i] : AXIS == 1 ? b[u][i][v] : b[i][u][v]) = r[i];
        }
}

// order: 0 = the kernel's Y, X, Z; 1 = X, Y, Z (a test of the tests only: another order of the same passes)
template <int D, bool INV>
void cube_f32(const float* in, float* out, double* pre, size_t n, int order) {
    constexpr int CS = 64 * D;
    for (size_t g = 0; g < n; g++) {
        double b[D][8][8];
        for (int i = 0; i < CS; i++) (&b[0][0][0])[i] = (double)in[g * CS + i];
        if (order == 0) {
            pass<D, 1, INV>(b);
            pass<D, 0, INV>(b);
        } else {
            pass<D, 0, INV>(b);
            pass<D, 1, INV>(b);
        }
        pass<D, 2, INV>(b);
        for (int i = 0; i < CS; i++) {
            double t = (&b[0][0][0])[i];
            if (pre) pre[g * CS + i] = t;
            if (INV) t = t > 255.0 ? 255.0 : (t < 0.0 ? 0.0 : t);
            out[g * CS + i] = (float)t;
        }
    }
}

// order: 0 = the kernel's X, Z, Y; 1 = X, Y, Z (as above)
template <int D>
void fwd64(const uint8_t* in, double* out, size_t n, int order) {
    constexpr int CS = 64 * D;
    for (size_t g = 0; g < n; g++) {
        double b[D][8][8];
        for (int i = 0; i < CS; i++) (&b[0][0][0])[i] = (double)in[g * CS + i];
        pass<D, 0, false>(b);
        if (order == 0) {
            pass<D, 2, false>(b);
            pass<D, 1, false>(b);
        } else {
            pass<D, 1, false>(b);
            pass<D, 2, false>(b);
        }
        for (int i = 0; i < CS; i++) out[g * CS + i] = (&b[0][0][0])[i];
    }
}

}  // namespace

// in, out: cube-major float [n][D][8][8]; pre (may be null): the fp64 values before the clamp and the cast, same
// layout; 0 on success, -1 for a depth other than 8 and 4
extern "C" int emulate_cube_f32(const float* in, long long n, int D, int inverse, int order, float* out, double* pre) {
    const size_t m = (size_t)n;
    if (D == 8) inverse ? cube_f32<8, true>(in, out, pre, m, order) : cube_f32<8, false>(in, out, pre, m, order);
    else if (D == 4) inverse ? cube_f32<4, true>(in, out, pre, m, order) : cube_f32<4, false>(in, out, pre, m, order);
    else return -1;
    return 0;
}

// in: cube-major u8 [n][D][8][8] (the cubes of the raster); out: fp64 in the same layout
extern "C" int emulate_fwd64(const uint8_t* in, long long n, int D, int order, double* out) {
    if (D == 8) fwd64<8>(in, out, (size_t)n, order);
    else if (D == 4) fwd64<4>(in, out, (size_t)n, order);
    else return -1;
    return 0;
}
