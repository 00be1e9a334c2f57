// dct3d_distortion_dev.h -- the device code the distortion probes share (dct3d_distortion.hip, the plane probe and
// its SSIM arm; dct3d_distortion_rgb.hip, the colour planes of the RGB-domain probes, DESIGN 4s / 4u;
// DESIGN 4w): the replay's reload source, the 8x8x8 forward transform, the quad sum, and distortion_body, the one
// body of pass 1 that distortion_kernel and distortion_plane_kernel instantiate.
#pragma once
#include "dct3d_probe_dev.h"
#include "dct3d_decode_dev.h"

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
// are encode16_kernel's.  Lane (c, kz = k, h) ends with b[ky][e], kx = 4h + e.  (The one copy of it:
// splitting e16_body itself changes the register allocation of the encode16 kernels, whose code objects stay as
// they are.)
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

// the sum over the lane's quad partner x (1 | 2): both are quad permutes
template <int X>
__device__ __forceinline__ uint32_t quad_add(uint32_t v) {
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, X == 1 ? 0xB1 : 0x4E, 0xF, 0xF, false);
}

// Pass 1 of every distortion probe, the body of distortion_kernel (CT = 0: channel R.ch of the frames, R a DistParams
// or, SSIM = 1, a SsimParams) and of distortion_plane_kernel (PX = 3, SSIM = 0, R a DistPlaneParams: plane R.ch of the
// colour transform of packed frames.  CT = 1: the rows and the replay reload through ycc_pick8, the plane at the
// frames' size.  CT = 2: through c420_row8, P's cube fields the chroma plane's and its address fields the frames',
// launch_rate_c420's).
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
// CT != 0: the mask and the stores go by the plane's own (R.pw, R.ph), the cubes' figures lie densely, and each lane
// stores its own row piece of the decoded samples (dec_store_tile's EDGE arm): the kernel has early-returning waves
// and a rolled table loop, so the block store and its barrier are not taken.
template <int D, int PX, int EDGE, int SSIM, int CT, class Params>
__device__ __forceinline__ void distortion_body(EncodeParams P, Params R) {
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
    static_assert(CT == 0 || (PX == 3 && SSIM == 0), "a colour plane: packed frames, no block moments");
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
    if constexpr (D == 8) load_channel_rows<4, 4, PX, EDGE, CT>(P, cube0 + ec, evalid, lane & 7, (lane >> 4) & 1, R.ch, raw);
    else load_channel_rows<4, 0, PX, EDGE, CT>(P, cube0 + ec, evalid, lane & 7, 0, R.ch, raw);
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
    // samples outside the frame (CT != 0: the plane) masked out of both sides
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
    const uint32_t dg = min(cube0 + (uint32_t)dc, P.n_cubes - 1u);  // the decode lane's cube
    uint32_t saa = 0;
    uint32_t bmask[NW];
    uint32_t npx = dvalid ? (uint32_t)NXC : 0u;  // the lane's samples inside the frame
    [[maybe_unused]] size_t poff = 0;            // CT != 0: its first sample in a table's plane (frame 0 of its stack)
    {
        if constexpr (EDGE || CT != 0) {
            uint32_t mw, mh;  // the mask's bounds
            if constexpr (CT != 0) mw = R.pw, mh = R.ph;
            else mw = P.width, mh = P.height;
            const CubePos cp = cube_pos(P, dg);
            const uint32_t row = cp.by * 8 + (uint32_t)dy, col = cp.bx * 8 + (uint32_t)dx0;
            if constexpr (EDGE) {
                if (row >= mh || col >= mw) npx = 0u;
                else npx = min(npx, mw - col);
            }
            if constexpr (CT != 0) poff = ((size_t)cp.s * D * R.ph + row) * R.pw + col;
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
    // a cube's place in cube_bits and cube_sse
    const auto out_cube = [&](uint32_t g) -> uint32_t {
        if constexpr (CT != 0) return g;
        else return enc_out_cube<PX>(P, g, R.ch);
    };
    // SSIM: the lane's blocks (word wd of frame z at blk0 + z * blkz + wd) and, once, the source's moments
    [[maybe_unused]] size_t blk0 = 0, blkz = 0;
    [[maybe_unused]] bool bst[NW] = {};
    if constexpr (SSIM) {
        const CubePos cp = cube_pos(P, dg);
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
    [[maybe_unused]] size_t pframe = 0;
    if constexpr (CT != 0) pframe = (size_t)R.ph * R.pw;

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
    const ReplayGeom RG = probe_replay_geom<PX, (CT == 2 ? 1 : EDGE)>(P, R.ch);  // (CT = 2: the height whatever EDGE)
    const size_t ocube = out_cube(dg);
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
            const double acc = rate_fold(replay_load<D, PX, EDGE, CT>(RG, cube0 + sc, k, lane), CS, lane, ssum, prod);
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
            R.cube_bits[(size_t)t * R.table_stride + out_cube(cube0 + lane)] = (uint16_t)sums[lane];

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
        if constexpr (CT != 0) {  // the samples inside the plane to table t's plane
            if (npx) {            // (npx <= pw - col and row < ph: no store leaves the plane)
                uint8_t* dst = R.planes + (size_t)t * R.plane_stride + poff;
#pragma unroll
                for (int z = 0; z < D; z++, dst += pframe) {
                    if (npx == (uint32_t)NXC) {
#pragma unroll
                        for (int i = 0; i < NW; i++) *(dec_u32_u_t*)(dst + 4 * i) = outw[z][i];
                    } else {
#pragma unroll
                        for (int bb = 0; bb < NXC - 1; bb++)
                            if (bb < (int)npx) dst[bb] = (uint8_t)(outw[z][bb >> 2] >> (8 * (bb & 3)));
                    }
                }
            }
        }
        wave_lds_sync();  // the next table rewrites the staging
    }
    if (nrep && lane == 0 && P.replay_count) atomicAdd(P.replay_count + (blockIdx.x & (kCountSpread - 1)), nrep);
}

}  // namespace dct3d
