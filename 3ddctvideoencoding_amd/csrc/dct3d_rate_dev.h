// dct3d_rate_dev.h -- the rate probe's kernel (dct3d_rate_frames*), shared by the units that instantiate
// it: dct3d_rate.hip (the planes as they are) and dct3d_ycc.hip (CT = 1: the YCbCr planes).
#pragma once
#include "dct3d_rate.h"
#include "dct3d_probe_dev.h"

namespace dct3d {

// encode_eg_kernel's geometry: one wave owns 8 cubes, 8 lanes per cube; rows -> statistics -> transform as
// there.  The coefficients then stay in registers, and a rolled loop over the launch's tables quantises and
// certifies them exactly as encode_eg_kernel does (the same products, thresholds and DC), adding the code
// widths of the certified values instead of staging codes.  The width of a value n held as an fp32 integer
// comes from the exponent of its code c = max(2n, 1 - 2n), exact in fp32 (c < 2^14): 2 (e - 126) - 1 bits
// for the biased exponent e, so a lane sums exponents and converts once.  The coefficients a table leaves
// open go to the table's mask in LDS; after the loop the wave folds each coefficient that is open under any
// table once (the Java fold does not depend on the table) and rounds the fold over the step of every table
// that left it open.  Per cube and table one uint16 goes out (a cube costs < 2^15 bits: 512 codes of <= 27).
// The wave's LDS region, free after the transform: the fold's scratch, the cubes' sums per table, the masks.
// CT = 1 (dct3d_ycc.hip): the rows and the fold's reload are channel R.ch of the YCbCr planes (ycc_pick8).
// CT = 2 (dct3d_c420.hip): the cubes of the 4:2:0 subsampled plane R.ch = 1 | 2 (c420_row8; P as
// encode_eg_kernel's CT = 2), and cube_bits holds that plane alone: cube g at g.
template <int D, int PX, int EDGE, int CT = 0>
__global__ __launch_bounds__(kBlock, 4) void rate_kernel(EncodeParams P, RateParams R) {
    constexpr int CS = 64 * D;
    constexpr int NB = (D == 8) ? 8 : 4;
    constexpr int NI = 7 + NB;
    constexpr int NV = CS / 8;  // coefficients per lane
    constexpr int MW = (D == 8) ? 2 : 1;  // mask words per lane
    constexpr int RS_B = kMaxGroupsDev * (4 + 8);
    constexpr int SUM_B = kRateTables * 8 * 4;
    static_assert(RS_B + SUM_B + kRateTables * 64 * MW * 4 <= enc_wave_lds<D>(), "scratch, sums and masks fit the wave's region");
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * enc_wave_lds<D>()];
    __shared__ float4 s_tab[kRateTables * kTabN];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cube0 = (blockIdx.x * kWavesPerBlock + wave) * kCubesPerWave;
    uint2 raw[D];
    __builtin_amdgcn_s_setprio(3);  // the rows in flight first (as encode_eg_kernel)
    load_channel_rows<D, 0, PX, EDGE, CT>(P, cube0 + (lane >> 3), cube0 + (lane >> 3) < P.n_cubes, lane & 7, 0, R.ch, raw);
    __builtin_amdgcn_s_setprio(0);
    if (blockIdx.x == 0 && P.replay_clear) enc_clear_next_slot(P);  // the next call's counter slot
    if (cube0 >= P.n_cubes) return;  // wave-uniform
    const int nt = R.n_tables;
    probe_fill_tabs(s_tab, R, lane);
    char* wl = lds + wave * enc_wave_lds<D>();
    int* const ssum = (int*)wl;
    double* const prod = (double*)(wl + kMaxGroupsDev * 4);
    uint32_t* const sums = (uint32_t*)(wl + RS_B);         // [table][cube]
    uint32_t* const msk = (uint32_t*)(wl + RS_B + SUM_B);  // [table][word][lane]
    const ProbeLane L = probe_lane8<D>(lane);
    const int c = L.c, j = lane & 7;
    const bool valid = cube0 + c < P.n_cubes;

    float a[D][8];
    to_float<D>(raw, a);
    uint32_t S;
    int m;
    float A;
    cube_stats<D>(raw, a, S, m, A);
    asm volatile("" : "+v"(S), "+v"(m), "+v"(A));
    float b[8][NB];
    forward_cube<D, NB>(a, m, c, j, wl, b);

    uint32_t fm[MW];  // open under any table: bit ky * NB + x
#pragma unroll
    for (int w = 0; w < MW; w++) fm[w] = 0u;
#pragma unroll 1
    for (int t = 0; t < nt; t++) {
        const float4* tab = s_tab + t * kTabN;
        uint32_t es, e00, om[MW];  // the sum of the codes' exponents; the fp32 DC's; open under this table
        probe_quantise<NB, NI, MW>(tab, L.kz + L.kx0, A, b, es, e00, om, [](int, const float (&)[NB]) {});
        uint32_t bits = probe_lane_bits<NV, MW>(es, e00, om, L.dc(), L.dc() ? probe_dc(S, P.coef_dc, tab) : 0);
        if (!valid) {
            bits = 0u;
#pragma unroll
            for (int w = 0; w < MW; w++) om[w] = 0u;
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) bits += __shfl_xor(bits, o, 64);
        if (j == 0) sums[t * 8 + c] = bits;
#pragma unroll
        for (int w = 0; w < MW; w++) {
            msk[(t * MW + w) * 64 + lane] = om[w];
            fm[w] |= om[w];
        }
    }
    wave_lds_sync();

    // the coefficients some table left open, one at a time by the whole wave (rare): one fold each, one
    // division and rounding per table that left it open.  (The distortion probe folds per table instead, before
    // that table's decode, which needs the value.)
    {
        const ReplayGeom G = probe_replay_geom<PX, (CT == 2 ? 1 : EDGE)>(P, R.ch);  // (CT = 2: the height whatever EDGE)
        uint32_t nrep = 0;
        for (;;) {
            uint32_t any = fm[0];
            if constexpr (MW == 2) any |= fm[1];
            const unsigned long long who = __ballot(any != 0u);
            if (who == 0ull) break;
            const int src = __builtin_ctzll(who);
            int mybit = fm[0] ? __builtin_ctz(fm[0]) : 0;
            if constexpr (MW == 2) mybit = fm[0] ? mybit : (fm[1] ? 32 + __builtin_ctz(fm[1]) : 0);
            const int bit = __shfl(mybit, src, 64);
            const ProbeLane SL = probe_lane8<D>(src);
            const int sc = SL.c;
            int ss;
            const uint32_t k = SL.template coef<NB>(bit, ss);
            const double acc = rate_fold(replay_load<D, PX, EDGE, CT>(G, cube0 + sc, k, lane), CS, lane, ssum, prod);
#pragma unroll 1
            for (int t = 0; t < nt; t++) {
                const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)msk[(t * MW + (bit >> 5)) * 64 + src]);
                if ((w >> (bit & 31)) & 1u) {  // wave-uniform
                    if (lane == 0) {
                        const int q = java_round_dev(__ddiv_rn(acc, (double)s_tab[t * kTabN + ss].w));
                        sums[t * 8 + sc] += rate_width(q);
                    }
                    nrep++;
                }
            }
            if (lane == src) {
                if (fm[0]) fm[0] &= fm[0] - 1u;
                else if constexpr (MW == 2) fm[1] &= fm[1] - 1u;
            }
            wave_lds_sync();
        }
        if (nrep && lane == 0 && P.replay_count) atomicAdd(P.replay_count + (blockIdx.x & (kCountSpread - 1)), nrep);
    }

    // lane 8 t + cc: cube cc's bits under table t (its place as the encode's [stack][channel][cube] blocks)
    const uint32_t ot = (uint32_t)lane >> 3, og = cube0 + ((uint32_t)lane & 7u);
    if constexpr (CT == 2) {  // a chroma plane's cubes alone, [stack][cube] within a table
        if (ot < (uint32_t)nt && og < P.n_cubes) R.cube_bits[(size_t)ot * R.table_stride + og] = (uint16_t)sums[lane];
    } else {
        if (ot < (uint32_t)nt && og < P.n_cubes)
            R.cube_bits[(size_t)ot * R.table_stride + enc_out_cube<PX>(P, og, R.ch)] = (uint16_t)sums[lane];
    }
}

}  // namespace dct3d
