// dct3d_kernels.hip -- CDNA4 (gfx950) kernels of the 3D-DCT hot path (the device templates live in
// dct3d_encode_dev.h / dct3d_decode_dev.h; this file instantiates them, adds the fused Exp-Golomb
// kernels and the launchers).
//
// Work decomposition.  8x8x8 encode (encode16_kernel), decode, float drop-ins: 16 lanes per cube (2 D
// lanes at 8x8x4 decode), 32 values per lane, the permlane16 pair (l, l ^ 16) splitting each cube.
// 8x8x4 encode and the fused encode + Exp-Golomb: 8 lanes per cube, 8 cubes per wave ("row layout"
// lane (c, y) holds a[z][x]; "face layout" lane (c, kz[, h]) holds b[y][x]).  Layout changes are
// permlane16 swaps or a wave-private LDS transpose (no workgroup barrier: LDS ops of a wave execute in
// order); cube-major int32 / fp64 traffic is staged through the same region so that every global
// access of the wave is a contiguous 1 KiB (16 B per lane) burst.
//
// Encode (raster u8 -> quantised int32 cube-major), fp32, certified: rows -> S, m, A = max|x - m| ->
// pass X (exact integer front, centring folded into X0) -> pass Z -> pass Y -> q = v * fp32(1/step),
// n = rint(q), certified iff |q - n| < 0.5 - (A*G_s + E_s) (dct3d_plan.cpp).  DC = JavaRound(fp64(S) *
// coef_dc) exactly.  Open coefficients: 8x8x8 settles them in the wave (fp64 second certificate, then
// the exact Java fold); 8x8x4 folds them exactly in the wave, its 8 cubes in parallel (enc4_replay).
// Decode (quantised int32 cube-major -> raster u8), fp64, certified: staged loads -> fp64 dequantise +
// L1 -> inverse passes Y, X, Z (the last one adds the fixed-point offset) -> certificate on the low
// words, 16-bit floors saturated to bytes -> raster stores; uncertified cubes are replayed whole in the
// wave (exact Java InverseDCT fold) before the stores.
#include "dct3d_launch.h"

namespace dct3d {

// =============================================================================================
// Drop-in (A): float cube-major -> float cube-major, fp64 internal (3dDCT.cl:43-143 / 164-265)
// =============================================================================================
// The decode kernel's geometry (2*D lanes per cube, 32 doubles per lane, staged 1 KiB loads, the
// lane-pair swap and the two LDS rounds), with the forward (DCT-II) or inverse (DCT-III, clamped to
// [0,255] as 3dDCT.cl:257-261) butterflies along Y, X, Z.  Layout C stores f32 cube-major directly:
// for D = 8 a store instruction covers one 256-byte z face of each of the wave's 4 cubes.
template <bool INV>
__device__ __forceinline__ void f64_line8(double (&x)[8]) {
    if constexpr (INV) idct8(x);
    else fdct8<false, false>(x, 0.0);
}
template <int D, bool INV>
__global__ __launch_bounds__(kBlock, 4) void cube_f32_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                             uint32_t n_cubes) {
    using G = DecGeom<D>;
    constexpr int CPW = G::CPW;
    constexpr int NXC = (D == 8) ? 4 : 8;
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * kDecWaveLds];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* wl = lds + wave * kDecWaveLds;
    const uint32_t cube0 = (xcd_tile() * kWavesPerBlock + wave) * CPW;
    if (cube0 >= n_cubes) return;  // wave-uniform
    {
        int4 v[8];
        __builtin_amdgcn_s_setprio(3);
        dec_load_tile_p<D>((const char*)in, n_cubes, cube0, lane, v);
        __builtin_amdgcn_s_setprio(0);
        dec_stage_tile<D>(wl, lane, v);
    }
    wave_lds_sync();
    const int h = (lane >> 4) & 1, k = lane & (D - 1);
    const int c = (lane >> 5) * (CPW / 2) + ((lane & 15) / D);
    const uint32_t g = cube0 + c;

    // layout A: lane (c, z = k, h) holds face k, rows y, x = 4h + e
    double b[8][4];
    {
        const char* src = wl + c * G::SA_C + k * G::SA_F + h * 16;
        float4 raw[8];
#pragma unroll
        for (int y = 0; y < 8; y++) raw[y] = *(const float4*)(src + y * 32);
#pragma unroll
        for (int y = 0; y < 8; y++) {
            b[y][0] = raw[y].x; b[y][1] = raw[y].y; b[y][2] = raw[y].z; b[y][3] = raw[y].w;
        }
    }
    // pass Y
#pragma unroll
    for (int e = 0; e < 4; e++) {
        double col[8];
#pragma unroll
        for (int y = 0; y < 8; y++) col[y] = b[y][e];
        pin(col);
        f64_line8<INV>(col);
        pin(col);
#pragma unroll
        for (int y = 0; y < 8; y++) b[y][e] = col[y];
    }
    // A -> B: lane-pair swap of the off-diagonal 4x4 blocks
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int e = 0; e < 4; e++) swap16(b[r][e], b[4 + r][e]);
    // pass X
#pragma unroll
    for (int r = 0; r < 4; r++) {
        double row[8];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            row[e] = b[r][e];
            row[4 + e] = b[4 + r][e];
        }
        pin(row);
        f64_line8<INV>(row);
        pin(row);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            b[r][e] = row[e];
            b[4 + r][e] = row[4 + e];
        }
    }
    double cz[D][NXC];
    dec_b_to_c<D>(b, cz, wl, c, k, h);
    // pass Z
#pragma unroll
    for (int e = 0; e < NXC; e++) {
        double col[D];
#pragma unroll
        for (int z = 0; z < D; z++) col[z] = cz[z][e];
        pin(col);
        if constexpr (INV) idctN<D>(col);
        else fdctN<D, false, false>(col, 0.0);
        pin(col);
#pragma unroll
        for (int z = 0; z < D; z++) cz[z][e] = col[z];
    }
    if (g < n_cubes) {
        const int y = (D == 8) ? k : (4 * h + k);
        const int x0 = (D == 8) ? 4 * h : 0;
        float* o = out + (size_t)g * G::CS + y * 8 + x0;
#pragma unroll
        for (int z = 0; z < D; z++) {
            float v[NXC];
#pragma unroll
            for (int e = 0; e < NXC; e++) {
                double t = cz[z][e];
                if constexpr (INV) t = t > 255.0 ? 255.0 : (t < 0.0 ? 0.0 : t);  // 3dDCT.cl:257-261
                v[e] = (float)t;
            }
#pragma unroll
            for (int e = 0; e < NXC; e += 4) {  // non-temporal: whole 128-byte lines, written once
                typedef float f32x4_t __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(f32x4_t{v[e], v[e + 1], v[e + 2], v[e + 3]}, (f32x4_t*)(o + z * 64 + e));
            }
        }
    }
}

int launch_cube_f32(int D, bool inverse, const float* in, float* out, uint32_t n_cubes, hipStream_t st) {
    const uint32_t blocks = dec_grid(D, n_cubes);
    if (!blocks) return 0;
    return with_depth(D, [&](auto d) {
        if (inverse) hipLaunchKernelGGL((cube_f32_kernel<d, true>), dim3(blocks), dim3(kBlock), 0, st, in, out, n_cubes);
        else hipLaunchKernelGGL((cube_f32_kernel<d, false>), dim3(blocks), dim3(kBlock), 0, st, in, out, n_cubes);
    }) ? launched() : -1;
}


// =============================================================================================
// Launchers
// =============================================================================================
// Encode: 8x8x8 = encode16_kernel (16 lanes per cube, in-wave exact replay, one launch per call);
// 8x8x4 = encode_kernel (8 lanes per cube, in-wave exact replay, one launch).  Both store the int32
// output non-temporally.  The variants that lost (8 lanes per cube at 8x8x8, plain stores, NT loads,
// LDS-padded occupancy) are recorded in profiles/r01/encode_variant_sweep.txt, not built.
// Decode: one butterfly per pin group (pin groups 1 / 2 / 4 / none measured within 1 %; non-temporal dword
// output stores were 26 % slower: profiles/r01/decode_variant_sweep.txt).
template int launch_encode_in<RasterPlain>(const Variant&, const EncodeParams&, hipStream_t);
template int launch_decode_in<RasterPlain>(const Variant&, const DecodeParamsQ&, hipStream_t);
template int launch_encode_eg_in<StreamPlain>(const Variant&, const EncodeParams&, const EgFusedParams&, const VqParams*, hipStream_t);
template int launch_decode_eg_in<StreamPlain>(const Variant&, const DecodeParamsQ&, const EgDecParams&, int, const VqParams*, hipStream_t);

}  // namespace dct3d
