// dct3d_distortion.hip -- the distortion probe (dct3d_distortion_frames*): the exact squared error
// of encode + decode under several quantiser tables, from one row load and one forward transform per cube.
// Per table the wave quantises and certifies its cubes as the encode does, puts the integers where the decode
// expects its staged input, runs the certified fp64 decode tile with the bytes kept in registers, and compares
// them with the rows it started from.  No coefficient and no decoded raster exists in memory.  A translation
// unit of its own: no other kernel's code object changes with it.
// The SSIM probe (dct3d_ssim_frames*) is an arm of the same kernel -- the moments of the frames' 4 x 4
// blocks from the same bytes -- and two small kernels that turn the blocks' records into the windows' values.
#include "dct3d_distortion.h"
#include "dct3d_probe_dev.h"
#include "dct3d_decode_dev.h"
#include <type_traits>

namespace dct3d {

// The decode's rare replay re-reads a cube's quantised values: the int16 copy of the tile beside the decode
// region (|q| < 2^15 for 8-bit frames and steps >= 1, so the copy is exact, whatever the cube's L1)
template <int D>
struct ReloadQ16 {
    const int16_t* q16;   // [CPW][CS], the wave's tile
    const double* steps;  // the table's fp64 steps
    uint32_t cube0;
    __device__ __forceinline__ void operator()(uint32_t g, double* cf, int lane) const {
        constexpr int CS = 64 * D;
        const int16_t* q = q16 + (size_t)(g - cube0) * CS;
#pragma unroll
        for (int i = 0; i < CS / 64; i++) {
            const int k = lane + 64 * i;
            const int kz = k / 64, ky = (k / 8) & 7, kx = k & 7;
            cf[k] = (double)q[k] * steps[kx + ky + kz];
        }
    }
};

// e16_body (dct3d_encode_dev.h) up to its quantiser: the statistics over the cube's 16 lanes (S: the sum, A: max
// |x - mean|) and passes X / Z / Y, operation for operation, so the coefficients and the certificate's bounds
// are encode16_kernel's.  Lane (c, kz = k, h) ends with b[ky][e], kx = 4h + e.  (A copy: splitting e16_body
// itself changes the register allocation of the encode16 kernels, whose code objects stay as they are.)
__device__ __forceinline__ void e16_forward(const uint2 (&raw)[4], char* wl, int lane, uint32_t& S, float& A,
                                            float (&b)[8][4]) {
    constexpr int CS = 512;
    const int k = lane & 7, h = (lane >> 4) & 1;
    const int c = (lane >> 5) * 2 + ((lane & 15) >> 3);
    float a[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            a[r][e] = byte_of(raw[r].x, e);
            a[r][e + 4] = byte_of(raw[r].y, e);
        }
    uint32_t mx = 0u, mn = 0x7F800000u;
    S = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        S = __builtin_amdgcn_udot4(raw[r].x, 0x01010101u, S, false);
        S = __builtin_amdgcn_udot4(raw[r].y, 0x01010101u, S, false);
#pragma unroll
        for (int x = 0; x < 8; x += 2) {
            const uint32_t u0 = __float_as_uint(a[r][x]), u1 = __float_as_uint(a[r][x + 1]);
            asm("v_max3_u32 %0, %1, %2, %3" : "=v"(mx) : "v"(mx), "v"(u0), "v"(u1));
            asm("v_min3_u32 %0, %1, %2, %3" : "=v"(mn) : "v"(mn), "v"(u0), "v"(u1));
        }
    }
#pragma unroll
    for (int o = 1; o <= 16; o <<= 1) {
        if (o == 8) continue;  // the cube's lanes: k bits (1, 2, 4) and h (16)
        S += __shfl_xor(S, o, 64);
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
        mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
    }
    const int m = (int)((S + CS / 2) / CS);
    A = fmaxf(__uint_as_float(mx) - (float)m, (float)m - __uint_as_float(mn));
    asm volatile("" : "+v"(S), "+v"(A));
    // pass X (exact integer front, centring folded into X0)
    const float dcsub = 8.0f * (float)m;
    pin(a[0]);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        fdct8<true, true>(a[r], dcsub);
        if (r + 1 < 4) pin2(a[r], a[r + 1]);
        else pin(a[r]);
    }
    // the lane pair's off-diagonal 4x4 blocks swapped: lines along z; pass Z
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(a[r][e]), __float_as_uint(a[r][4 + e]),
                                                             false, false);
            a[r][e] = __uint_as_float((uint32_t)sw[0]);
            a[r][4 + e] = __uint_as_float((uint32_t)sw[1]);
        }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float col[8];
#pragma unroll
        for (int z = 0; z < 4; z++) {
            col[z] = a[z][e];
            col[4 + z] = a[z][4 + e];
        }
        pin(col);
        fdct8<false, false>(col, 0.f);
        pin(col);
#pragma unroll
        for (int z = 0; z < 4; z++) {
            a[z][e] = col[z];
            a[z][4 + e] = col[4 + z];
        }
    }
    // LDS transpose in two y halves: lane (c, y = k, h) -> lane (c, kz = k, h); pass Y
#pragma unroll
    for (int rd = 0; rd < 2; rd++) {
        if ((k >> 2) == rd) {
            char* dst = wl + c * kE16TC + h * 64 + (k & 3) * 16;
#pragma unroll
            for (int kz = 0; kz < 8; kz++) {
                const float* v = kz < 4 ? &a[kz][0] : &a[kz - 4][4];
                *(float4*)(dst + kz * kE16TZ) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
        wave_lds_sync();
        const char* src = wl + c * kE16TC + k * kE16TZ + h * 64;
#pragma unroll
        for (int yy = 0; yy < 4; yy++) {
            const float4 t = *(const float4*)(src + yy * 16);
            b[4 * rd + yy][0] = t.x; b[4 * rd + yy][1] = t.y; b[4 * rd + yy][2] = t.z; b[4 * rd + yy][3] = t.w;
        }
        wave_lds_sync();
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float col[8];
#pragma unroll
        for (int y = 0; y < 8; y++) col[y] = b[y][e];
        pin(col);
        fdct8<false, false>(col, 0.f);
        pin(col);
#pragma unroll
        for (int y = 0; y < 8; y++) b[y][e] = col[y];
    }
}

// The encode tile and the decode tile own the same cubes: 4 cubes x 16 lanes at 8x8x8 (e16_forward's lanes are
// the decode's), 8 cubes x 8 lanes at 8x8x4 (encode_body's lanes; the decode's lanes of a cube are others, and
// the integers cross over in the staging).  Encode side: lane (ec, kz, kx0) holds b[ky][x], kx = kx0 + x.
// Decode side (layout C): lane (dc, y, x0) holds the bytes of x0 .. x0 + NXC - 1 of row y of every plane.
// The wave's LDS region: the decode's region (first the forward transform's transposes, then per table the
// staged integers, the decode's own transposes and replay scratch), the int16 copy of the staged integers
// (ReloadQ16), the fold's scratch, the cubes' bits.
// SSIM = 1 (the SSIM probe): a word of the decode side is one row of a 4 x 4 block of one frame, the
// block's four rows are the lanes dk ^ 1, dk ^ 2.  Per table the lane takes Sy, Syy and Sxy of each word, the four
// rows add up as two packed words (quad permutes), and the lane of the block's first row stores the record.
template <int SSIM>
using DistKernelParams = std::conditional_t<SSIM != 0, SsimParams, DistParams>;
// the sum over the lane's quad partner x (1 | 2): both are quad permutes
template <int X>
__device__ __forceinline__ uint32_t quad_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, X == 1 ? 0xB1 : 0x4E, 0xF, 0xF, false);
}
template <int D, int PX, int EDGE, int SSIM = 0>
__global__ __launch_bounds__(kBlock, 2) void distortion_kernel(EncodeParams P, DistKernelParams<SSIM> R) {
    using G = DecGeom<D>;
    constexpr int CS = 64 * D, CPW = G::CPW;
    constexpr int NXC = (D == 8) ? 4 : 8, NW = NXC / 4;
    constexpr int NV = 32;  // coefficients per lane
    constexpr int Q16_OFF = kDecWaveLds;
    constexpr int RS_OFF = Q16_OFF + CPW * CS * 2;
    constexpr int SUM_OFF = RS_OFF + kMaxGroupsDev * (4 + 8);
    constexpr int WLDS = SUM_OFF + 8 * 4;
    static_assert(kE16Lds <= kDecWaveLds && enc_wave_lds<4>() <= kDecWaveLds, "the forward transform fits the decode's region");
    static_assert(WLDS % 16 == 0 && Q16_OFF % 16 == 0, "aligned regions");
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * WLDS];
    __shared__ float4 s_tab[kRateTables * kTabN];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t cube0 = (blockIdx.x * kWavesPerBlock + wave) * CPW;
    // encode side
    const auto enc_lane = [](int ln) { return (D == 8) ? probe_lane16(ln) : probe_lane8<4>(ln); };
    const ProbeLane L = enc_lane(lane);
    const int ec = L.c, kz = L.kz, kx0 = L.kx0;
    const bool dcl = L.dc();  // the cube's DC lane
    const bool evalid = cube0 + ec < P.n_cubes;
    uint2 raw[4];
    __builtin_amdgcn_s_setprio(3);  // the rows in flight first (as the encode kernels)
    if constexpr (D == 8) load_channel_rows<4, 4, PX, EDGE>(P, cube0 + ec, evalid, lane & 7, (lane >> 4) & 1, R.ch, raw);
    else load_channel_rows<4, 0, PX, EDGE>(P, cube0 + ec, evalid, lane & 7, 0, R.ch, raw);
    __builtin_amdgcn_s_setprio(0);
    if (blockIdx.x == 0 && P.replay_clear) enc_clear_next_slot(P);  // the next call's counter slot
    if (cube0 >= P.n_cubes) return;  // wave-uniform
    const int nt = R.n_tables;
    probe_fill_tabs(s_tab, R, lane);
    char* const wl = lds + wave * WLDS;
    int16_t* const q16 = (int16_t*)(wl + Q16_OFF);
    int* const ssum = (int*)(wl + RS_OFF);
    double* const prod = (double*)(wl + RS_OFF + kMaxGroupsDev * 4);
    uint32_t* const sums = (uint32_t*)(wl + SUM_OFF);  // [cube] bits under the current table

    // decode side: the lane's source bytes in layout C (sw[z][wd] beside the decode's outw[z][wd]), the
    // samples outside the frame masked out of both sides
    const int dh = (lane >> 4) & 1, dk = lane & (D - 1);
    const int dc = dec_cube_of_lane<D>(lane);
    const int dy = (D == 8) ? dk : 4 * dh + dk, dx0 = (D == 8) ? 4 * dh : 0;
    const bool dvalid = cube0 + dc < P.n_cubes;
    uint32_t sw[D][NW];
    if constexpr (D == 8) {  // rows y = k of frames 4h .. 4h + 3 -> x 4h .. 4h + 3 of all 8 (the lane pair's swap)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const auto t = __builtin_amdgcn_permlane16_swap(raw[r].x, raw[r].y, false, false);
            sw[r][0] = (uint32_t)t[0];
            sw[4 + r][0] = (uint32_t)t[1];
        }
    } else {  // the rows of encode lane (dc, j = y)
#pragma unroll
        for (int z = 0; z < 4; z++) {
            sw[z][0] = (uint32_t)__shfl((int)raw[z].x, dc * 8 + dy, 64);
            sw[z][1] = (uint32_t)__shfl((int)raw[z].y, dc * 8 + dy, 64);
        }
    }
    uint32_t saa = 0;
    uint32_t bmask[NW];
    {
        uint32_t npx = dvalid ? (uint32_t)NXC : 0u;
        if constexpr (EDGE) {
            const CubePos cp = cube_pos(P, min(cube0 + (uint32_t)dc, P.n_cubes - 1u));
            const uint32_t row = cp.by * 8 + (uint32_t)dy, col = cp.bx * 8 + (uint32_t)dx0;
            if (row >= P.height || col >= P.width) npx = 0u;
            else npx = min(npx, P.width - col);
        }
#pragma unroll
        for (int wd = 0; wd < NW; wd++) {
            const uint32_t n = npx > 4u * wd ? min(npx - 4u * wd, 4u) : 0u;
            bmask[wd] = n >= 4u ? 0xFFFFFFFFu : (1u << (8u * n)) - 1u;
        }
#pragma unroll
        for (int z = 0; z < D; z++)
#pragma unroll
            for (int wd = 0; wd < NW; wd++) {
                sw[z][wd] &= bmask[wd];
                saa = __builtin_amdgcn_udot4(sw[z][wd], sw[z][wd], saa, false);
            }
    }
    // SSIM: the lane's blocks (word wd of frame z at blk0 + z * blkz + wd) and, once, the source's moments
    [[maybe_unused]] size_t blk0 = 0, blkz = 0;
    [[maybe_unused]] bool bst[NW] = {};
    if constexpr (SSIM) {
        const CubePos cp = cube_pos(P, min(cube0 + (uint32_t)dc, P.n_cubes - 1u));
        const uint32_t by4 = cp.by * 2 + ((uint32_t)dy >> 2), bx4 = cp.bx * 2 + ((uint32_t)dx0 >> 2);
        blkz = (size_t)R.nby * R.nbx;
        blk0 = ((size_t)cp.s * D * R.nby + by4) * R.nbx + bx4;
#pragma unroll
        for (int wd = 0; wd < NW; wd++) bst[wd] = dvalid && (dk & 3) == 0 && by4 < R.nby && bx4 + wd < R.nbx;
#pragma unroll
        for (int z = 0; z < D; z++)
#pragma unroll
            for (int wd = 0; wd < NW; wd++) {
                uint32_t m = __builtin_amdgcn_udot4(sw[z][wd], 0x01010101u, 0u, false) |
                             (__builtin_amdgcn_udot4(sw[z][wd], sw[z][wd], 0u, false) << 12);
                m = quad_add<2>(quad_add<1>(m));
                if (bst[wd]) R.blk_x[blk0 + z * blkz + wd] = m;
            }
    }

    // ---- statistics and the forward transform, once ----
    uint32_t S;
    float A;
    float b[8][4];
    if constexpr (D == 8) {
        e16_forward(raw, wl, lane, S, A, b);
    } else {
        float a[4][8];
        to_float<4>(raw, a);
        int m;
        cube_stats<4>(raw, a, S, m, A);
        asm volatile("" : "+v"(S), "+v"(m), "+v"(A));
        forward_cube<4, 4>(a, m, ec, lane & 7, wl, b);
    }

    DecodeParams DP = {};
    DP.n_cubes = P.n_cubes;
    DP.dec_G = R.dec_G;
    DP.dec_E = R.dec_E;
    DP.dec_l1_max = R.dec_l1_max;
    DP.inv_coef_t = R.inv_coef_t;
    DP.replay_count = P.replay_count;
    const ReplayGeom RG = probe_replay_geom<PX, EDGE>(P, R.ch);
    const size_t ocube = enc_out_cube<PX>(P, min(cube0 + (uint32_t)dc, P.n_cubes - 1u), R.ch);  // the decode lane's cube
    uint32_t nrep = 0;

#pragma unroll 1
    for (int t = 0; t < nt; t++) {
        const float4* tab = s_tab + t * kTabN;
        const double* steps = R.steps + t * kDistStepN;
        // ---- quantise + certify with the encode's products and thresholds (probe_quantise); the integers, the
        //      exact DC among them, to the decode's staging and to the int16 copy ----
        uint32_t es, e00, om[1];  // om: open under this table, bit 4 ky + x
        const int dcq = probe_dc(S, P.coef_dc, tab);
        char* const stg = wl + ec * G::SA_C + kz * G::SA_F + kx0 * 4;
        int16_t* const s16 = q16 + ec * CS + kz * 64 + kx0;
        probe_quantise<4, 11, 1>(tab, kz + kx0, A, b, es, e00, om, [&](int ky, const float (&n)[4]) {
            int qi[4];
#pragma unroll
            for (int x = 0; x < 4; x++) qi[x] = (int)n[x];
            if (ky == 0 && dcl) qi[0] = dcq;
            *(int4*)(stg + ky * 32) = make_int4(qi[0], qi[1], qi[2], qi[3]);
            *(uint2*)(s16 + ky * 8) = make_uint2(__builtin_amdgcn_perm(qi[1], qi[0], 0x05040100u),
                                                 __builtin_amdgcn_perm(qi[3], qi[2], 0x05040100u));
        });
        uint32_t bits = probe_lane_bits<NV, 1>(es, e00, om, dcl, dcq);
        if (!evalid) {
            bits = 0u;
            om[0] = 0u;
        }
        bits += __shfl_xor(bits, 1, 64);
        bits += __shfl_xor(bits, 2, 64);
        bits += __shfl_xor(bits, 4, 64);
        if constexpr (D == 8) bits += __shfl_xor(bits, 16, 64);
        if (dcl) sums[ec] = bits;
        wave_lds_sync();

        // ---- the coefficients the certificate left open, one at a time by the whole wave (rare): the Java fold,
        //      divided by this table's step, written over the provisional value in both copies.  (Per table and
        //      before the decode, which needs the value; the rate probe folds once for all tables after its loop.) ----
        for (;;) {
            const unsigned long long who = __ballot(om[0] != 0u);
            if (who == 0ull) break;
            const int src = __builtin_ctzll(who);
            const int bit = __shfl(om[0] ? __builtin_ctz(om[0]) : 0, src, 64);
            const ProbeLane SL = enc_lane(src);
            const int sc = SL.c;
            int ss;
            const uint32_t k = SL.template coef<4>(bit, ss);
            const double acc = rate_fold(replay_load<D, PX, EDGE>(RG, cube0 + sc, k, lane), CS, lane, ssum, prod);
            if (lane == 0) {
                const int q = java_round_dev(__ddiv_rn(acc, (double)tab[ss].w));
                *(int*)(wl + sc * G::SA_C + (k >> 6) * G::SA_F + (k & 63) * 4) = q;
                q16[sc * CS + k] = (int16_t)q;
                sums[sc] += rate_width(q);
            }
            nrep++;
            if (lane == src) om[0] &= om[0] - 1u;
            wave_lds_sync();
        }
        if (R.cube_bits && lane < CPW && cube0 + lane < P.n_cubes)
            R.cube_bits[(size_t)t * R.table_stride + enc_out_cube<PX>(P, cube0 + lane, R.ch)] = (uint16_t)sums[lane];

        // ---- the decode tile on the staged integers, its bytes kept; the squared error inside the frame:
        //      sum (x - y)^2 = sum x^2 + sum y^2 - 2 sum x y, three byte dot products per word ----
        uint32_t outw[D][NW];
        bool kv;
        decode_tile<D, false, false, true, 0, 1>(DP, wl, lane, cube0, [] {}, ReloadQ16<D>{q16, steps, cube0}, &outw[0][0],
                                                 &kv, steps);
        uint32_t sbb = 0, sab = 0;
#pragma unroll
        for (int z = 0; z < D; z++)
#pragma unroll
            for (int wd = 0; wd < NW; wd++) {
                const uint32_t y = outw[z][wd] & bmask[wd];
                if constexpr (SSIM) {
                    const uint32_t syy = __builtin_amdgcn_udot4(y, y, 0u, false);
                    const uint32_t sxy = __builtin_amdgcn_udot4(sw[z][wd], y, 0u, false);
                    sbb += syy;
                    sab += sxy;
                    const uint32_t lo = quad_add<2>(quad_add<1>(__builtin_amdgcn_udot4(y, 0x01010101u, 0u, false) | (syy << 12)));
                    const uint32_t hi = quad_add<2>(quad_add<1>(sxy));
                    if (bst[wd]) R.blk_y[(size_t)t * R.blk_stride + blk0 + z * blkz + wd] = ((uint64_t)hi << 32) | lo;
                } else {
                    sbb = __builtin_amdgcn_udot4(y, y, sbb, false);
                    sab = __builtin_amdgcn_udot4(sw[z][wd], y, sab, false);
                }
            }
        uint32_t sse = saa + sbb - 2u * sab;  // < 2^32 for the cube: 512 x 255^2
        sse += __shfl_xor(sse, 1, 64);
        sse += __shfl_xor(sse, 2, 64);
        if constexpr (D == 8) sse += __shfl_xor(sse, 4, 64);
        sse += __shfl_xor(sse, 16, 64);
        if (dk == 0 && dh == 0 && dvalid && (!SSIM || R.cube_sse)) R.cube_sse[(size_t)t * R.table_stride + ocube] = sse;
        wave_lds_sync();  // the next table rewrites the staging
    }
    if (nrep && lane == 0 && P.replay_count) atomicAdd(P.replay_count + (blockIdx.x & (kCountSpread - 1)), nrep);
}

// One block per run of `run` cubes (a table's stack and channel): their sum (rate_sum_kernel for uint32)
__global__ __launch_bounds__(kBlock) void distortion_sum_kernel(const uint32_t* cube_sse, uint32_t run, uint64_t* out) {
    const uint32_t* p = cube_sse + (size_t)blockIdx.x * run;
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < run; i += kBlock) s += p[i];
    const uint64_t r = probe_block_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

int launch_distortion(int D, int px, int edge, const EncodeParams& P, const DistParams& R, hipStream_t st) {
    return probe_dispatch(D, px, edge, P, R, [&](auto d, auto p, auto e) {
        const dim3 grid(grid_blocks(P.n_cubes, DecGeom<decltype(d)::value>::CPW));
        hipLaunchKernelGGL((distortion_kernel<decltype(d)::value, decltype(p)::value, decltype(e)::value>), grid, dim3(kBlock), 0, st, P, R);
    });
}

int launch_distortion_ssim(int D, int px, int edge, const EncodeParams& P, const SsimParams& R, hipStream_t st) {
    return probe_dispatch(D, px, edge, P, R, [&](auto d, auto p, auto e) {
        const dim3 grid(grid_blocks(P.n_cubes, DecGeom<decltype(d)::value>::CPW));
        hipLaunchKernelGGL((distortion_kernel<decltype(d)::value, decltype(p)::value, decltype(e)::value, 1>), grid, dim3(kBlock), 0, st, P, R);
    });
}

int launch_distortion_sum(const uint32_t* cube_sse, uint32_t run, uint64_t n_runs, uint64_t* out, hipStream_t st) {
    if (n_runs == 0) return 0;
    if (n_runs > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(distortion_sum_kernel, dim3((uint32_t)n_runs), dim3(kBlock), 0, st, cube_sse, run, out);
    return launched();
}

// ---- the SSIM probe's windows (dct3d.h states the definition) ----
// One thread per window of (table blockIdx.z, stack blockIdx.y): the moments of its 1, 2 or 4 blocks, n from the
// geometry, A, B, C, D in int64, s = fl(fl(A B) / fl(C D)), v = floor(s 2^24); the block's sum of v
__global__ __launch_bounds__(kBlock) void ssim_window_kernel(SsimWinParams W) {
    const uint32_t t = blockIdx.z, s = blockIdx.y;
    const uint32_t per_frame = W.nwx * W.nwy, per_stack = per_frame * W.depth;
    const uint64_t* const by_ = W.blk_y + (size_t)t * W.blk_stride;
    int64_t sum = 0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < per_stack; i += W.bpr * kBlock) {
        const uint32_t z = i / per_frame, r = i - z * per_frame;
        const uint32_t j = r / W.nwx, x = r - j * W.nwx;
        const uint32_t x1 = min(x + 1u, W.nbx - 1u), j1 = min(j + 1u, W.nby - 1u);
        const size_t f0 = ((size_t)s * W.depth + z) * W.nby;
        int64_t Sx = 0, Sy = 0, Sxx = 0, Syy = 0, Sxy = 0;
        for (uint32_t bj = j; bj <= j1; bj++)
            for (uint32_t bi = x; bi <= x1; bi++) {
                const size_t b = (f0 + bj) * W.nbx + bi;
                const uint64_t my = by_[b];
                const uint32_t mx = W.blk_x[b];
                Sx += mx & 0xFFFu;
                Sxx += mx >> 12;
                Sy += (uint32_t)my & 0xFFFu;
                Syy += (uint32_t)my >> 12;
                Sxy += (uint32_t)(my >> 32);
            }
        const int64_t n = (int64_t)(min(4u * x + 8u, W.w) - 4u * x) * (int64_t)(min(4u * j + 8u, W.h) - 4u * j);
        const int64_t n2 = n * n, xy = Sx * Sy, xx = Sx * Sx, yy = Sy * Sy;
        const int64_t A = 20000 * xy + 65025 * n2;
        const int64_t B = 20000 * (n * Sxy - xy) + 585225 * n2;
        const int64_t Cc = 10000 * (xx + yy) + 65025 * n2;
        const int64_t Dd = 10000 * (n * Sxx - xx + n * Syy - yy) + 585225 * n2;
        const double q = __ddiv_rn(__dmul_rn((double)A, (double)B), __dmul_rn((double)Cc, (double)Dd));
        const int32_t v = (int32_t)floor(__dmul_rn(q, 16777216.0));
        if (W.win) W.win[(size_t)t * W.win_t + (size_t)s * W.win_s + i] = v;
        sum += v;
    }
    const uint64_t r = probe_block_sum((uint64_t)sum);
    if (threadIdx.x == 0) W.part[((size_t)t * W.ns + s) * W.bpr + blockIdx.x] = (int64_t)r;
}

// One block per (stack blockIdx.x, table blockIdx.y): the sum of its bpr partial sums
__global__ __launch_bounds__(kBlock) void ssim_sum_kernel(const int64_t* part, uint32_t bpr, int64_t* out, uint64_t out_t,
                                                          uint64_t out_s) {
    const int64_t* p = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * bpr;
    uint64_t s = 0;
    for (uint32_t i = threadIdx.x; i < bpr; i += kBlock) s += (uint64_t)p[i];
    const uint64_t r = probe_block_sum(s);
    if (threadIdx.x == 0) out[(size_t)blockIdx.y * out_t + (size_t)blockIdx.x * out_s] = (int64_t)r;
}

int launch_ssim_window(const SsimWinParams& W, hipStream_t st) {
    if (W.ns == 0 || W.n_tables == 0) return 0;
    if (W.ns > 65535u || W.n_tables > 65535u || W.bpr == 0) return -1;
    hipLaunchKernelGGL(ssim_window_kernel, dim3(W.bpr, W.ns, W.n_tables), dim3(kBlock), 0, st, W);
    return launched();
}

int launch_ssim_sum(const int64_t* part, uint32_t bpr, uint32_t ns, uint32_t n_tables, int64_t* out, uint64_t out_t,
                    uint64_t out_s, hipStream_t st) {
    if (ns == 0 || n_tables == 0) return 0;
    if (n_tables > 65535u) return -1;
    hipLaunchKernelGGL(ssim_sum_kernel, dim3(ns, n_tables), dim3(kBlock), 0, st, part, bpr, out, out_t, out_s);
    return launched();
}

}  // namespace dct3d
