// dct3d_probe_dev.h -- device code the probes share (dct3d_rate.hip, dct3d_distortion.hip): a
// table's quantise-and-certify pass, the lane's bits from it, the Java fold of one coefficient up to the
// division by a table's step, the lanes' places in the two encode geometries, the sum kernels' block
// reduction and the dispatch from the runtime's (D, px, edge) to a kernel instance.
#pragma once
#include "dct3d_encode_dev.h"
#include "dct3d_rate.h"

namespace dct3d {

static_assert(kRateTabN == kTabN, "a table's rows as the encode kernels'");

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

// A lane's place after the forward transform: cube c of the wave, coefficients (kz, ky, kx0 + x), x < NB, bit
// ky * NB + x of its masks.  The two encode geometries: 8 lanes per cube (encode_body, encode_eg_kernel: NB = 8
// at 8x8x8, 4 at 8x8x4) and 16 lanes per cube (encode16_kernel, 8x8x8: NB = 4).
struct ProbeLane {
    int c, kz, kx0;
    __device__ __forceinline__ bool dc() const { return kz == 0 && kx0 == 0; }  // the lane of the cube's DC
    template <int NB>
    __device__ __forceinline__ uint32_t coef(int bit, int& s) const {  // the coefficient's index; s = kx + ky + kz
        const int ky = bit / NB, kx = kx0 + bit % NB;
        s = kx + ky + kz;
        return (uint32_t)((kz * 8 + ky) * 8 + kx);
    }
};
template <int D>
__device__ __forceinline__ ProbeLane probe_lane8(int lane) {
    const int j = lane & 7;
    return {lane >> 3, (D == 8) ? j : (j >> 1), (D == 8) ? 0 : (j & 1) * 4};
}
__device__ __forceinline__ ProbeLane probe_lane16(int lane) {
    return {(lane >> 5) * 2 + ((lane & 15) >> 3), lane & 7, 4 * ((lane >> 4) & 1)};
}

// the launch's table rows into the block's LDS: every wave writes the block's whole copy (identical bits) and
// reads only after its own writes (enc_tables)
__device__ __forceinline__ void probe_fill_tabs(float4* s_tab, const RateParams& R, int lane) {
    for (int i = lane; i < R.n_tables * kTabN; i += kWave) s_tab[i] = R.tabs[i];
}

template <int PX, int EDGE>
__device__ __forceinline__ ReplayGeom probe_replay_geom(const EncodeParams& P, int ch) {
    ReplayGeom G{P.raster, P.cubes_per_stack, P.nbx, P.width, P.plane, P.stack_stride, P.ngroups, P.coef, P.group_of};
    if constexpr (PX != 1) G.ch = ch;
    if constexpr (EDGE != 0) G.height = P.height;
    return G;
}

// One table's quantise-and-certify pass over the lane's b[ky][x] (s = so + ky + x), exactly as encode_eg_kernel
// does it (the same products, thresholds and slow re-scan).  sink(ky, n) receives the rounded values of row ky.
// es: the sum of the exponents of the certified values' codes.  The width of a value n held as an fp32 integer
// comes from the exponent of its code c = max(2n, 1 - 2n), exact in fp32 (c < 2^14): 2 (e - 126) - 1 bits for
// the biased exponent e, so a lane sums exponents and converts once (probe_lane_bits).  e00: the exponent of
// b[0][0]'s (the fp32 DC's in the DC lane).  om: the coefficients left open, bit ky * NB + x.
template <int NB, int NI, int MW, class Sink>
__device__ __forceinline__ void probe_quantise(const float4* tab, int so, float A, const float (&b)[8][NB], uint32_t& es,
                                               uint32_t& e00, uint32_t (&om)[MW], Sink&& sink) {
    int sz = so;
    float rr[NI], thr[NI];
    es = 0;
    e00 = 0;
#pragma unroll
    for (int w = 0; w < MW; w++) om[w] = 0u;
#pragma unroll
    for (int ky = 0; ky < 8; ky++) {
        tab_window<NB, NI>(tab, sz, ky, A, rr, thr);
        bool f = false;
        float qq[NB], n[NB];
        uint32_t e[NB];
#pragma unroll
        for (int x = 0; x < NB; x++) {
            qq[x] = b[ky][x] * rr[ky + x];
            n[x] = __builtin_rintf(qq[x]);
            f |= __builtin_fabsf(qq[x] - n[x]) >= thr[ky + x];
            const float n2 = n[x] + n[x];
            e[x] = __float_as_uint(__builtin_fmaxf(n2, 1.0f - n2)) >> 23;
            es += e[x];
        }
        if (ky == 0) e00 = e[0];
        if (__builtin_expect(f, 0)) {
            uint32_t bits = 0;
#pragma unroll
            for (int x = 0; x < NB; x++)
                if (__builtin_fabsf(qq[x] - __builtin_rintf(qq[x])) >= thr[ky + x]) {
                    bits |= 1u << x;
                    es -= e[x];
                }
            om[(ky * NB) >> 5] |= bits << ((ky * NB) & 31);
        }
        sink(ky, n);
        asm volatile("" : "+v"(es), "+v"(om[0]));
    }
}

// the exact DC: from the integer cube sum S, over the table's step 0
__device__ __forceinline__ int probe_dc(uint32_t S, double coef_dc, const float4* tab) {
    return java_round_dev(__ddiv_rn((double)S * coef_dc, (double)tab[0].w));
}

// The bits of the lane's certified values after probe_quantise (all NV but the open ones): the sum of
// 2 (e - 126) - 1.  In the cube's DC lane (dcq: probe_dc) the exact DC's width replaces the fp32 DC's; the DC is
// never left open (its threshold is +inf), and were it, it is exact already.
template <int NV, int MW>
__device__ __forceinline__ uint32_t probe_lane_bits(uint32_t es, uint32_t e00, uint32_t (&om)[MW], bool dc_lane, int dcq) {
    if (dc_lane && (om[0] & 1u)) {
        om[0] &= ~1u;
        es += e00;
    }
    uint32_t open = (uint32_t)__builtin_popcount(om[0]);
    if constexpr (MW == 2) open += (uint32_t)__builtin_popcount(om[1]);
    uint32_t bits = 2u * es - 253u * ((uint32_t)NV - open);
    if (dc_lane) bits += rate_width(dcq) - (2u * e00 - 253u);
    return bits;
}

// The sum kernels' tail: the block's sum of every thread's s (the shuffles move 64-bit values as two halves),
// valid in thread 0
__device__ __forceinline__ uint64_t probe_block_sum(uint64_t s) {
    __shared__ uint64_t s_part[kWavesPerBlock];
    uint32_t lo = (uint32_t)s, hi = (uint32_t)(s >> 32);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const uint64_t t = ((uint64_t)(uint32_t)__shfl_xor((int)hi, o, 64) << 32) | (uint32_t)__shfl_xor((int)lo, o, 64);
        s += t;
        lo = (uint32_t)s;
        hi = (uint32_t)(s >> 32);
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    uint64_t r = 0;
#pragma unroll
    for (int i = 0; i < kWavesPerBlock; i++) r += s_part[i];
    return r;
}

// Host: the runtime's (D, px, edge) -> f(<D>, <PX>, <EDGE>) as integral constants; the launchers' argument check
template <class F>
int probe_dispatch(int D, int px, int edge, const EncodeParams& P, const RateParams& R, F&& f) {
    if (P.n_cubes == 0) return 0;
    if (R.n_tables < 1 || R.n_tables > kRateTables) return -1;
    return with_variant(D, px, edge, f) ? launched() : -1;
}

}  // namespace dct3d
