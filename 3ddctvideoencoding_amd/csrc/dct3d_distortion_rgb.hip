// dct3d_distortion_rgb.hip -- the RGB-domain distortion probe (dct3d_distortion_rgb_frames*): the exact
// squared error, in the RGB pixels, of the YCbCr (and 4:2:0) stream encode + decode under a list of (Y, Cb, Cr)
// table triples.  Pass 1 is the distortion probe's kernel (dct3d_distortion.hip) on one plane of the colour
// transform with the rate kernel's colour axis: per table it quantises, certifies, folds and decodes as there,
// keeps the plane's squared error and bits, and stores the decoded samples inside the plane into a dense plane
// the context owns.  Pass 2 reads a candidate's three decoded planes beside the source pixels, upsamples the chroma
// by replication, runs ycc_to_rgb4 and takes the squared error per cube of the frames' grid.  The RGB and luma SSIM
// probe (dct3d_ssim_rgb_frames*) is pass 1 as it is and a pass 2 of its own, ssim_rgb_block_kernel.  A
// translation unit of its own: no other kernel's code object changes with it.
#include "dct3d_distortion_rgb.h"
#include "dct3d_probe_dev.h"
#include "dct3d_decode_dev.h"
#include "dct3d_eg_fused_dev.h"

namespace dct3d {

// (copies of dct3d_distortion.hip's: that unit's code object stays as it is)
template <int D>
struct ReloadPlaneQ16 {
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

// e16_body (dct3d_encode_dev.h) up to its quantiser, operation for operation (dct3d_distortion.hip's e16_forward)
__device__ __forceinline__ void plane_e16_forward(const uint2 (&raw)[4], char* wl, int lane, uint32_t& S, float& A,
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
    const float dcsub = 8.0f * (float)m;
    pin(a[0]);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        fdct8<true, true>(a[r], dcsub);
        if (r + 1 < 4) pin2(a[r], a[r + 1]);
        else pin(a[r]);
    }
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

// distortion_kernel's body (dct3d_distortion.hip: the lanes, the LDS regions, the table loop) on plane R.ch of the
// colour transform of packed frames.  CT = 1: the rows and the replay reload through ycc_pick8, the plane at the
// frames' size.  CT = 2: through c420_row8, P's cube fields the chroma plane's and its address fields the frames'
// (launch_rate_c420's).  The in-plane mask and the stores go by the plane's own (R.pw, R.ph).  Each lane stores its
// own row piece (dec_store_tile's EDGE arm): the kernel has early-returning waves and a rolled table loop, so the
// block store and its barrier are not taken.
template <int D, int EDGE, int CT>
__global__ __launch_bounds__(kBlock, 2) void distortion_plane_kernel(EncodeParams P, DistPlaneParams R) {
    using G = DecGeom<D>;
    constexpr int PX = 3;
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
    const bool dcl = L.dc();
    const bool evalid = cube0 + ec < P.n_cubes;
    uint2 raw[4];
    __builtin_amdgcn_s_setprio(3);
    if constexpr (D == 8) load_channel_rows<4, 4, PX, EDGE, CT>(P, cube0 + ec, evalid, lane & 7, (lane >> 4) & 1, R.ch, raw);
    else load_channel_rows<4, 0, PX, EDGE, CT>(P, cube0 + ec, evalid, lane & 7, 0, R.ch, raw);
    __builtin_amdgcn_s_setprio(0);
    if (blockIdx.x == 0 && P.replay_clear) enc_clear_next_slot(P);
    if (cube0 >= P.n_cubes) return;  // wave-uniform
    const int nt = R.n_tables;
    probe_fill_tabs(s_tab, R, lane);
    char* const wl = lds + wave * WLDS;
    int16_t* const q16 = (int16_t*)(wl + Q16_OFF);
    int* const ssum = (int*)(wl + RS_OFF);
    double* const prod = (double*)(wl + RS_OFF + kMaxGroupsDev * 4);
    uint32_t* const sums = (uint32_t*)(wl + SUM_OFF);

    // decode side: the lane's source samples in layout C, the samples outside the plane masked out of both sides
    const int dh = (lane >> 4) & 1, dk = lane & (D - 1);
    const int dc = dec_cube_of_lane<D>(lane);
    const int dy = (D == 8) ? dk : 4 * dh + dk, dx0 = (D == 8) ? 4 * dh : 0;
    const bool dvalid = cube0 + dc < P.n_cubes;
    uint32_t sw[D][NW];
    if constexpr (D == 8) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const auto t = __builtin_amdgcn_permlane16_swap(raw[r].x, raw[r].y, false, false);
            sw[r][0] = (uint32_t)t[0];
            sw[4 + r][0] = (uint32_t)t[1];
        }
    } else {
#pragma unroll
        for (int z = 0; z < 4; z++) {
            sw[z][0] = (uint32_t)__shfl((int)raw[z].x, dc * 8 + dy, 64);
            sw[z][1] = (uint32_t)__shfl((int)raw[z].y, dc * 8 + dy, 64);
        }
    }
    const uint32_t dg = min(cube0 + (uint32_t)dc, P.n_cubes - 1u);  // the decode lane's cube
    uint32_t saa = 0;
    uint32_t bmask[NW];
    uint32_t npx = dvalid ? (uint32_t)NXC : 0u;  // the lane's samples inside the plane
    size_t poff;                                 // its first sample in a table's plane (frame 0 of its stack)
    {
        const CubePos cp = cube_pos(P, dg);
        const uint32_t row = cp.by * 8 + (uint32_t)dy, col = cp.bx * 8 + (uint32_t)dx0;
        if constexpr (EDGE) {
            if (row >= R.ph || col >= R.pw) npx = 0u;
            else npx = min(npx, R.pw - col);
        }
        poff = ((size_t)cp.s * D * R.ph + row) * R.pw + col;
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
    const size_t pframe = (size_t)R.ph * R.pw;

    // ---- statistics and the forward transform, once ----
    uint32_t S;
    float A;
    float b[8][4];
    if constexpr (D == 8) {
        plane_e16_forward(raw, wl, lane, S, A, b);
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
    uint32_t nrep = 0;

#pragma unroll 1
    for (int t = 0; t < nt; t++) {
        const float4* tab = s_tab + t * kTabN;
        const double* steps = R.steps + t * kDistStepN;
        uint32_t es, e00, om[1];
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

        // the coefficients the certificate left open (rare): the Java fold, per table and before the decode
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
            R.cube_bits[(size_t)t * R.table_stride + cube0 + lane] = (uint16_t)sums[lane];

        // ---- the decode tile on the staged integers, its bytes kept: the plane's squared error, and the samples
        //      inside the plane to table t's plane ----
        uint32_t outw[D][NW];
        bool kv;
        decode_tile<D, false, false, true, 0, 1>(DP, wl, lane, cube0, [] {}, ReloadPlaneQ16<D>{q16, steps, cube0}, &outw[0][0],
                                                 &kv, steps);
        uint32_t sbb = 0, sab = 0;
#pragma unroll
        for (int z = 0; z < D; z++)
#pragma unroll
            for (int wd = 0; wd < NW; wd++) {
                const uint32_t y = outw[z][wd] & bmask[wd];
                sbb = __builtin_amdgcn_udot4(y, y, sbb, false);
                sab = __builtin_amdgcn_udot4(sw[z][wd], y, sab, false);
            }
        uint32_t sse = saa + sbb - 2u * sab;
        sse += __shfl_xor(sse, 1, 64);
        sse += __shfl_xor(sse, 2, 64);
        if constexpr (D == 8) sse += __shfl_xor(sse, 4, 64);
        sse += __shfl_xor(sse, 16, 64);
        if (dk == 0 && dh == 0 && dvalid) R.cube_sse[(size_t)t * R.table_stride + dg] = sse;
        if (npx) {  // (npx <= pw - col and row < ph: no store leaves the plane)
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
        wave_lds_sync();  // the next table rewrites the staging
    }
    if (nrep && lane == 0 && P.replay_count) atomicAdd(P.replay_count + (blockIdx.x & (kCountSpread - 1)), nrep);
}

// Pass 2.  Thread (cube, y) of a block of 32 cubes x 8 rows takes row y of its cube: 8 pixels of D frames.  A row
// piece that lies inside the frame loads whole words (byte aligned); any other loads its pixels one at a time, the
// column clamped into the frame, and masks what lies outside.  blockIdx.y: the candidate.
typedef unsigned rgbc_u32_u_t __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t rgbc_byte(uint32_t w, int i) { return (w >> (8 * i)) & 0xFFu; }
template <int D>
__global__ __launch_bounds__(kBlock) void distortion_rgb_combine_kernel(RgbCombineParams C) {
    const uint32_t g = blockIdx.x * (kBlock / 8) + (threadIdx.x >> 3);
    const uint32_t y = threadIdx.x & 7u;
    const uint32_t cand = blockIdx.y;
    const bool valid = g < C.n_cubes;
    uint32_t sse = 0;
    const uint32_t gg = min(g, C.n_cubes - 1u);
    const uint32_t s = fdiv(gg, C.div_cps);
    const uint32_t rr = gg - s * C.cubes_per_stack;
    const uint32_t by = fdiv(rr, C.div_nbx), bx = rr - by * C.nbx;
    const uint32_t row = by * 8 + y, col = bx * 8;
    if (valid && row < C.h && col < C.w) {
        const uint32_t npx = min(8u, C.w - col);
        const uint8_t* const sl = C.slots + 3 * (size_t)cand;
        const uint8_t* yp = C.y + (size_t)sl[0] * C.y_stride + ((size_t)s * D * C.h + row) * C.w + col;
        const uint32_t crow = row >> C.shift, ccol = col >> C.shift;  // < chh, < cw: the pixel is inside the frame
        const size_t coff = ((size_t)s * D * C.chh + crow) * C.cw + ccol;
        const uint8_t* cbp = C.cb + (size_t)sl[1] * C.c_stride + coff;
        const uint8_t* crp = C.cr + (size_t)sl[2] * C.c_stride + coff;
        const uint8_t* src = C.frames + ((size_t)s * D * C.h + row) * C.w * 3 + (size_t)col * 3;
        const size_t yframe = (size_t)C.h * C.w, cframe = (size_t)C.chh * C.cw;
        for (int z = 0; z < D; z++, yp += yframe, cbp += cframe, crp += cframe, src += 3 * yframe) {
            uint32_t x3[6], yw[2], cbv[8], crv[8];
            if (npx == 8u) {
#pragma unroll
                for (int i = 0; i < 6; i++) x3[i] = *(const rgbc_u32_u_t*)(src + 4 * i);
                yw[0] = *(const rgbc_u32_u_t*)yp;
                yw[1] = *(const rgbc_u32_u_t*)(yp + 4);
                if (C.shift) {  // 4 samples per plane: (col + 7) >> 1 < cw
                    const uint32_t b4 = *(const rgbc_u32_u_t*)cbp, r4 = *(const rgbc_u32_u_t*)crp;
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        cbv[i] = rgbc_byte(b4, i >> 1);
                        crv[i] = rgbc_byte(r4, i >> 1);
                    }
                } else {
                    const uint32_t b0 = *(const rgbc_u32_u_t*)cbp, b1 = *(const rgbc_u32_u_t*)(cbp + 4);
                    const uint32_t r0 = *(const rgbc_u32_u_t*)crp, r1 = *(const rgbc_u32_u_t*)(crp + 4);
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        cbv[i] = rgbc_byte(i < 4 ? b0 : b1, i & 3);
                        crv[i] = rgbc_byte(i < 4 ? r0 : r1, i & 3);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < 6; i++) x3[i] = 0u;
                yw[0] = yw[1] = 0u;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const uint32_t xi = min((uint32_t)i, npx - 1u);  // clamped into the row
                    const uint32_t ci = ((col + xi) >> C.shift) - ccol;
                    cbv[i] = cbp[ci];
                    crv[i] = crp[ci];
                    if ((uint32_t)i < npx) {
                        yw[i >> 2] |= (uint32_t)yp[i] << (8 * (i & 3));
#pragma unroll
                        for (int k = 0; k < 3; k++) x3[(3 * i + k) >> 2] |= (uint32_t)src[3 * i + k] << (8 * ((3 * i + k) & 3));
                    }
                }
            }
#pragma unroll
            for (int hw = 0; hw < 2; hw++) {
                const uint32_t y4 = yw[hw];
                const uint32_t* cb = cbv + 4 * hw;
                const uint32_t* cr = crv + 4 * hw;
                uint32_t a = rgbc_byte(y4, 0) | (cb[0] << 8) | (cr[0] << 16) | (rgbc_byte(y4, 1) << 24);
                uint32_t b = cb[1] | (cr[1] << 8) | (rgbc_byte(y4, 2) << 16) | (cb[2] << 24);
                uint32_t c = cr[2] | (rgbc_byte(y4, 3) << 8) | (cb[3] << 16) | (cr[3] << 24);
                ycc_to_rgb4(a, b, c);
                const uint32_t o[3] = {a, b, c};
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    // bytes 12 hw + 4 i .. + 3 of the row piece: inside the frame below 3 npx
                    const uint32_t first = 12u * hw + 4u * i, lim = 3u * npx;
                    const uint32_t n = lim > first ? min(lim - first, 4u) : 0u;
                    const uint32_t m = n >= 4u ? 0xFFFFFFFFu : (1u << (8u * n)) - 1u;
                    const uint32_t xs = x3[3 * hw + i] & m, ys = o[i] & m;
                    sse += __builtin_amdgcn_udot4(xs, xs, 0u, false) + __builtin_amdgcn_udot4(ys, ys, 0u, false) -
                           2u * __builtin_amdgcn_udot4(xs, ys, 0u, false);
                }
            }
        }
    }
    sse += __shfl_xor(sse, 1, 64);
    sse += __shfl_xor(sse, 2, 64);
    sse += __shfl_xor(sse, 4, 64);
    if (valid && y == 0) C.cube_sse[(size_t)cand * C.cand_stride + g] = sse;  // 512 x 3 x 255^2 < 2^32
}

// The RGB and luma SSIM probe's pass 2 (dct3d_ssim_rgb_frames*): the combine kernel's threads, loads,
// upsampling and ycc_to_rgb4, with the SSIM probe's block moments in the place of the cube's squared
// error.  A half row piece (4 pixels) of one frame is one row of a 4 x 4 block; its 12 bytes of either side split
// into one word per channel, the moments are byte dot products, the block's four rows are the lanes y ^ 1, y ^ 2
// (two quad permutes), and the lane of the block's first row stores the records ssim_window_kernel reads.  Every
// lane runs the moments and the permutes; a lane outside the frame loads nothing and contributes zeros.
// LUMA: plane 3, the source's luma (ycc_pick8's arithmetic, channel 0) against the decoded Y bytes.
template <int K>
__device__ __forceinline__ uint32_t rgbc_pick4(uint32_t d0, uint32_t d1, uint32_t d2) {  // byte K + 3 p of 12, p < 4
    return __builtin_amdgcn_perm(d2, __builtin_amdgcn_perm(d1, d0, rgb_pick_sel1(K)), rgb_pick_sel2(K));
}
__device__ __forceinline__ uint32_t rgbc_luma4(uint32_t d0, uint32_t d1, uint32_t d2) {
    const uint32_t d[3] = {d0, d1, d2};
    uint32_t n[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        int b[3];
#pragma unroll
        for (int i = 0; i < 3; i++) b[i] = (int)((d[(3 * p + i) >> 2] >> (8 * ((3 * p + i) & 3))) & 0xFFu);
        n[p] = (uint32_t)(__mul24(19595, b[0]) + __mul24(38470, b[1]) + __mul24(7471, b[2]) + 32768);
    }
    constexpr uint32_t kPair = 0x0c0c0602u, kJoin = 0x05040100u;  // byte 2 of the numerators
    return __builtin_amdgcn_perm(__builtin_amdgcn_perm(n[3], n[2], kPair), __builtin_amdgcn_perm(n[1], n[0], kPair), kJoin);
}
// (dct3d_distortion.hip's quad_add, copied: that unit's code object stays as it is)
template <int X>
__device__ __forceinline__ uint32_t rgbc_quad_add(uint32_t v) {  // the sum over the lane's quad partner X (1 | 2)
    return v + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, X == 1 ? 0xB1 : 0x4E, 0xF, 0xF, false);
}
template <int D, int LUMA>
__global__ __launch_bounds__(kBlock) void ssim_rgb_block_kernel(SsimRgbParams S) {
    const RgbCombineParams& C = S.C;
    constexpr int NP = 3 + LUMA;
    const uint32_t g = blockIdx.x * (kBlock / 8) + (threadIdx.x >> 3);
    const uint32_t y = threadIdx.x & 7u;
    const uint32_t cand = blockIdx.y;
    const bool valid = g < C.n_cubes;
    const uint32_t gg = min(g, C.n_cubes - 1u);
    const uint32_t s = fdiv(gg, C.div_cps);
    const uint32_t rr = gg - s * C.cubes_per_stack;
    const uint32_t by = fdiv(rr, C.div_nbx), bx = rr - by * C.nbx;
    const uint32_t row = by * 8 + y, col = bx * 8;
    const bool live = valid && row < C.h && col < C.w;
    const uint32_t npx = live ? min(8u, C.w - col) : 0u;  // the lane's pixels inside the frame
    // the lane's blocks: half hw of frame z at blk0 + z * blkz + hw.  A block that does not exist stores nothing
    // (by4 < nby4 is row < h for the storing lane; bx4 + hw < nbx4 is col + 4 hw < w)
    const uint32_t by4 = by * 2 + (y >> 2), bx4 = bx * 2;
    const size_t blkz = (size_t)S.nby4 * S.nbx4;
    const size_t blk0 = ((size_t)s * D * S.nby4 + by4) * S.nbx4 + bx4;
    bool bst[2];
    uint32_t bm[2];
#pragma unroll
    for (int hw = 0; hw < 2; hw++) {
        bst[hw] = valid && (y & 3u) == 0u && by4 < S.nby4 && bx4 + hw < S.nbx4;
        const uint32_t n = npx > 4u * hw ? min(npx - 4u * hw, 4u) : 0u;
        bm[hw] = n >= 4u ? 0xFFFFFFFFu : (1u << (8u * n)) - 1u;
    }
    const uint8_t* const sl = C.slots + 3 * (size_t)cand;
    const uint32_t crow = row >> C.shift, ccol = col >> C.shift;
    const size_t yframe = (size_t)C.h * C.w, cframe = (size_t)C.chh * C.cw;
    const uint8_t *yp = nullptr, *cbp = nullptr, *crp = nullptr, *src = nullptr;
    if (live) {
        yp = C.y + (size_t)sl[0] * C.y_stride + ((size_t)s * D * C.h + row) * C.w + col;
        const size_t coff = ((size_t)s * D * C.chh + crow) * C.cw + ccol;
        cbp = C.cb + (size_t)sl[1] * C.c_stride + coff;
        crp = C.cr + (size_t)sl[2] * C.c_stride + coff;
        src = C.frames + ((size_t)s * D * C.h + row) * C.w * 3 + (size_t)col * 3;
    }
    uint64_t* const rec_y = S.blk_y + (size_t)cand * S.blk_stride + blk0;
    uint32_t* const rec_x = S.blk_x + blk0;
    const size_t plane_y = (size_t)C.n_cand * S.blk_stride;  // from plane to plane
    for (int z = 0; z < D; z++) {
        uint32_t x3[6], yw[2], cbv[8], crv[8];
#pragma unroll
        for (int i = 0; i < 6; i++) x3[i] = 0u;
        yw[0] = yw[1] = 0u;
#pragma unroll
        for (int i = 0; i < 8; i++) cbv[i] = crv[i] = 0u;
        if (npx == 8u) {
#pragma unroll
            for (int i = 0; i < 6; i++) x3[i] = *(const rgbc_u32_u_t*)(src + 4 * i);
            yw[0] = *(const rgbc_u32_u_t*)yp;
            yw[1] = *(const rgbc_u32_u_t*)(yp + 4);
            if (C.shift) {  // 4 samples per plane: (col + 7) >> 1 < cw
                const uint32_t b4 = *(const rgbc_u32_u_t*)cbp, r4 = *(const rgbc_u32_u_t*)crp;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    cbv[i] = rgbc_byte(b4, i >> 1);
                    crv[i] = rgbc_byte(r4, i >> 1);
                }
            } else {
                const uint32_t b0 = *(const rgbc_u32_u_t*)cbp, b1 = *(const rgbc_u32_u_t*)(cbp + 4);
                const uint32_t r0 = *(const rgbc_u32_u_t*)crp, r1 = *(const rgbc_u32_u_t*)(crp + 4);
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    cbv[i] = rgbc_byte(i < 4 ? b0 : b1, i & 3);
                    crv[i] = rgbc_byte(i < 4 ? r0 : r1, i & 3);
                }
            }
        } else if (npx) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t xi = min((uint32_t)i, npx - 1u);  // clamped into the row
                const uint32_t ci = ((col + xi) >> C.shift) - ccol;
                cbv[i] = cbp[ci];
                crv[i] = crp[ci];
                if ((uint32_t)i < npx) {
                    yw[i >> 2] |= (uint32_t)yp[i] << (8 * (i & 3));
#pragma unroll
                    for (int k = 0; k < 3; k++) x3[(3 * i + k) >> 2] |= (uint32_t)src[3 * i + k] << (8 * ((3 * i + k) & 3));
                }
            }
        }
#pragma unroll
        for (int hw = 0; hw < 2; hw++) {
            const uint32_t y4 = yw[hw];
            const uint32_t* cb = cbv + 4 * hw;
            const uint32_t* cr = crv + 4 * hw;
            uint32_t a = rgbc_byte(y4, 0) | (cb[0] << 8) | (cr[0] << 16) | (rgbc_byte(y4, 1) << 24);
            uint32_t b = cb[1] | (cr[1] << 8) | (rgbc_byte(y4, 2) << 16) | (cb[2] << 24);
            uint32_t c = cr[2] | (rgbc_byte(y4, 3) << 8) | (cb[3] << 16) | (cr[3] << 24);
            ycc_to_rgb4(a, b, c);
            const uint32_t x0 = x3[3 * hw], x1 = x3[3 * hw + 1], x2 = x3[3 * hw + 2];
            uint32_t xs[NP], ys[NP];
            xs[0] = rgbc_pick4<0>(x0, x1, x2);
            xs[1] = rgbc_pick4<1>(x0, x1, x2);
            xs[2] = rgbc_pick4<2>(x0, x1, x2);
            ys[0] = rgbc_pick4<0>(a, b, c);
            ys[1] = rgbc_pick4<1>(a, b, c);
            ys[2] = rgbc_pick4<2>(a, b, c);
            if constexpr (LUMA) {
                xs[3] = rgbc_luma4(x0, x1, x2);
                ys[3] = y4;
            }
#pragma unroll
            for (int k = 0; k < NP; k++) {
                const uint32_t xv = xs[k] & bm[hw], yv = ys[k] & bm[hw];
                uint32_t lo = __builtin_amdgcn_udot4(yv, 0x01010101u, 0u, false) | (__builtin_amdgcn_udot4(yv, yv, 0u, false) << 12);
                uint32_t hi = __builtin_amdgcn_udot4(xv, yv, 0u, false);
                uint32_t mx = __builtin_amdgcn_udot4(xv, 0x01010101u, 0u, false) | (__builtin_amdgcn_udot4(xv, xv, 0u, false) << 12);
                lo = rgbc_quad_add<2>(rgbc_quad_add<1>(lo));
                hi = rgbc_quad_add<2>(rgbc_quad_add<1>(hi));
                mx = rgbc_quad_add<2>(rgbc_quad_add<1>(mx));
                if (bst[hw]) {
                    rec_y[(size_t)k * plane_y + z * blkz + hw] = ((uint64_t)hi << 32) | lo;
                    if (cand == 0u) rec_x[(size_t)k * S.blk_stride + z * blkz + hw] = mx;  // (the same under every candidate)
                }
            }
        }
        yp += yframe;
        cbp += cframe;
        crp += cframe;
        src += 3 * yframe;
    }
}

__global__ __launch_bounds__(kBlock) void distortion_rgb_gather_kernel(const uint32_t* in, uint64_t in_stride, const uint8_t* slots,
                                                                        uint32_t cps, uint32_t n_stacks, uint32_t* out,
                                                                        uint64_t out_stride) {
    const uint64_t per = (uint64_t)cps * n_stacks;
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= per) return;
    const uint32_t cand = blockIdx.y;
    const uint32_t s = (uint32_t)(i / cps), g = (uint32_t)(i - (uint64_t)s * cps);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) v += in[(size_t)slots[3 * cand + k] * in_stride + ((size_t)3 * s + k) * cps + g];
    out[(size_t)cand * out_stride + i] = v;
}

int launch_distortion_plane(int D, int edge, int ct, const EncodeParams& P, const DistPlaneParams& R, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (R.n_tables < 1 || R.n_tables > kRateTables || !R.planes || !R.cube_sse || R.pw == 0 || R.ph == 0) return -1;
    if (ct == 2 ? (R.ch != 1 && R.ch != 2) : (ct != 1 || R.ch < 0 || R.ch > 2)) return -1;
    int rc = -1;
    with_depth(D, [&](auto d) { with_flag(edge, [&](auto e) {
        constexpr int Dv = decltype(d)::value, Ev = decltype(e)::value;
        const dim3 grid(grid_blocks(P.n_cubes, DecGeom<Dv>::CPW));
        if (ct == 2) hipLaunchKernelGGL((distortion_plane_kernel<Dv, Ev, 2>), grid, dim3(kBlock), 0, st, P, R);
        else hipLaunchKernelGGL((distortion_plane_kernel<Dv, Ev, 1>), grid, dim3(kBlock), 0, st, P, R);
        rc = launched();
    }); });
    return rc;
}

int launch_distortion_rgb_combine(int D, const RgbCombineParams& C, hipStream_t st) {
    if (C.n_cubes == 0 || C.n_cand == 0) return 0;
    if (C.n_cand > 65535u || C.shift > 1u) return -1;
    int rc = -1;
    with_depth(D, [&](auto d) {
        const dim3 grid((C.n_cubes + kBlock / 8 - 1) / (kBlock / 8), C.n_cand);
        hipLaunchKernelGGL((distortion_rgb_combine_kernel<decltype(d)::value>), grid, dim3(kBlock), 0, st, C);
        rc = launched();
    });
    return rc;
}

int launch_ssim_rgb_block(int D, int luma, const SsimRgbParams& S, hipStream_t st) {
    const RgbCombineParams& C = S.C;
    if (C.n_cubes == 0 || C.n_cand == 0) return 0;
    if (C.n_cand > 65535u || C.shift > 1u || !S.blk_y || !S.blk_x || S.nbx4 == 0 || S.nby4 == 0) return -1;
    if (S.nbx4 != (C.w + 3u) / 4u || S.nby4 != (C.h + 3u) / 4u) return -1;  // the records' grid is the frames'
    if (S.blk_stride < (uint64_t)(C.n_cubes / C.cubes_per_stack) * D * S.nby4 * S.nbx4) return -1;
    int rc = -1;
    with_depth(D, [&](auto d) {
        constexpr int Dv = decltype(d)::value;
        const dim3 grid((C.n_cubes + kBlock / 8 - 1) / (kBlock / 8), C.n_cand);
        if (luma) hipLaunchKernelGGL((ssim_rgb_block_kernel<Dv, 1>), grid, dim3(kBlock), 0, st, S);
        else hipLaunchKernelGGL((ssim_rgb_block_kernel<Dv, 0>), grid, dim3(kBlock), 0, st, S);
        rc = launched();
    });
    return rc;
}

int launch_distortion_rgb_gather(const uint32_t* in, uint64_t in_stride, const uint8_t* slots, uint32_t n_cand, uint32_t cps,
                                 uint32_t n_stacks, uint32_t* out, uint64_t out_stride, hipStream_t st) {
    const uint64_t per = (uint64_t)cps * n_stacks;
    if (per == 0 || n_cand == 0) return 0;
    if (n_cand > 65535u || (per + kBlock - 1) / kBlock > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(distortion_rgb_gather_kernel, dim3((uint32_t)((per + kBlock - 1) / kBlock), n_cand), dim3(kBlock), 0, st, in,
                       in_stride, slots, cps, n_stacks, out, out_stride);
    return launched();
}

}  // namespace dct3d
