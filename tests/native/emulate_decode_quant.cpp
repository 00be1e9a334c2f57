// tests/native/emulate_decode_quant.cpp -- TEST ONLY: emulate_decode.cpp's host emulation of the decode kernel's
// fp64 arithmetic (csrc/dct3d_decode_dev.h, decode_tile) with the quantiser's table in place of
// max(1, 5 (x + y + z)): the exact dequantisation q * steps[x + y + z], the per-cube L1, then the same butterfly
// source (csrc/dct_butterfly.h) in the kernel's pass order -- inverse Y, X, Z, the last pass with the
// fixed-point offset, which the emulation subtracts again (exactly while |v| < 2^19).  Built by the tests with
// g++ -O2 -ffp-contract=off; never linked into the product.
// emulate_decode_quant_w (cert_common.py) returns w = v + kFixMagic itself, the last pass's output bit for bit: the
// word whose low half the kernel's certificate reads (lo_min / lo_max) and whose high half gives the byte.
#include <cmath>
#include <cstdint>

#include "dct_butterfly.h"

using namespace dct3d;

constexpr double kFix = 1572864.0;  // the kernel's fixed-point offset (kFixMagic)

// q: cube-major int32 [n][D][8][8]; steps: [8 + 8 + D - 2]; v_out: the kernel's fp64 values [n][D][8][8];
// l1_out: sum |q * step| per cube
static int run(const int32_t* q, int n_cubes, int D, const int32_t* steps, double* v_out, double* l1_out,
               bool keep_fix) {
    const int CS = 64 * D;
    for (int g = 0; g < n_cubes; g++) {
        double b[8][8][8];  // [z][y][x]
        double l1 = 0.0;
        for (int z = 0; z < D; z++)
            for (int y = 0; y < 8; y++)
                for (int x = 0; x < 8; x++) {
                    b[z][y][x] = (double)q[(size_t)g * CS + (z * 8 + y) * 8 + x] * (double)steps[x + y + z];
                    l1 += std::fabs(b[z][y][x]);
                }
        for (int z = 0; z < D; z++)
            for (int x = 0; x < 8; x++) {  // pass Y
                double r[8];
                for (int y = 0; y < 8; y++) r[y] = b[z][y][x];
                idct8(r);
                for (int y = 0; y < 8; y++) b[z][y][x] = r[y];
            }
        for (int z = 0; z < D; z++)
            for (int y = 0; y < 8; y++) {  // pass X
                double r[8];
                for (int x = 0; x < 8; x++) r[x] = b[z][y][x];
                idct8(r);
                for (int x = 0; x < 8; x++) b[z][y][x] = r[x];
            }
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 8; x++) {  // pass Z
                if (D == 8) {
                    double r[8];
                    for (int z = 0; z < 8; z++) r[z] = b[z][y][x];
                    idct8_fix(r, kFix);
                    for (int z = 0; z < 8; z++) b[z][y][x] = r[z];
                } else {
                    double r[4];
                    for (int z = 0; z < 4; z++) r[z] = b[z][y][x];
                    idct4_fix(r, kFix);
                    for (int z = 0; z < 4; z++) b[z][y][x] = r[z];
                }
            }
        for (int z = 0; z < D; z++)
            for (int y = 0; y < 8; y++)
                for (int x = 0; x < 8; x++) v_out[(size_t)g * CS + (z * 8 + y) * 8 + x] = keep_fix ? b[z][y][x] : b[z][y][x] - kFix;
        l1_out[g] = l1;
    }
    return 0;
}

extern "C" int emulate_decode_quant(const int32_t* q, int n_cubes, int D, const int32_t* steps, double* v_out,
                                    double* l1_out) {
    return run(q, n_cubes, D, steps, v_out, l1_out, false);
}

// w_out: w = v + kFixMagic [n][D][8][8], the kernel's cz after pass Z
extern "C" int emulate_decode_quant_w(const int32_t* q, int n_cubes, int D, const int32_t* steps, double* w_out,
                                      double* l1_out) {
    return run(q, n_cubes, D, steps, w_out, l1_out, true);
}
