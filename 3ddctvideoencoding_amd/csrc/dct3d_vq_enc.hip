// dct3d_vq_enc.hip -- the fused stream encode with a quantiser table per stack (dct3d_encode_eg_frames_vq*;
// DESIGN 4m).  encode_eg_vq_kernel is encode_eg_kernel<D, PX, EDGE, QT = 1> (dct3d_eg_fused_dev.h), its body
// copied operation for operation -- the row loads, statistics, transform, quantise + certify, code staging,
// whole-wave exact replay and emission are the same calls in the same order -- with one difference: the table
// rows {1 / step, G, 0.5 - E, step} are chosen per cube.  Cube c of a wave lies in stack (cube0 + c) /
// cubes_per_stack and takes the palette entry the map names for that stack.
// Where the rows live: in the wave's own staging region, between the transform and the code staging.  After
// forward_cube the region is free (the coefficients are in registers) until the codes are staged, so the wave
// copies the rows of its (up to 8) cubes' tables there, 3 KiB of the region's 8.25 KiB (4.1 KiB at 8x8x4), and
// the quantise loop reads them through tab_window exactly as the QT = 1 kernel reads the block's copy.  No LDS
// is added (the block still fits a quarter of the CU's), no table register is held across the transform.  Cubes
// that share a table share a copy (the slot of the first such cube), so a wave inside one stack -- every wave
// but a few at 1080p -- reads one table at wave-uniform addresses, as the QT = 1 kernel does.  The DC's step
// is read before the codes overwrite the copy; the rare exact replay takes the source cube's rows from global
// memory.
// A translation unit of its own: no other code object changes.
#include "dct3d_eg_fused_dev.h"
#include "dct3d_vq.h"

namespace dct3d {

static_assert(kVqTabN == kTabN, "a table's rows as the encode kernels'");
// a cube's copy in the wave's region: 25 rows apart (400 B: the 8 copies' rows on distinct 4-bank groups)
constexpr int kVqSlot = kVqTabN + 1;

template <int D, int PX, int EDGE>
__global__ __launch_bounds__(kBlock, 4) void encode_eg_vq_kernel(EncodeParams P, EgFusedParams E, VqParams V) {
    constexpr int CS = 64 * D;
    constexpr int NB = (D == 8) ? 8 : 4;
    constexpr int NI = 7 + NB;
    constexpr int VPL = CS / 8;            // stream values per lane
    constexpr int FACE = 128;
    static_assert(FACE == 128, "k1_code_off's face stride");
    constexpr int CUBE_B = (D == 8) ? 1056 : 2 * CS + 16;
    static_assert(8 * CUBE_B <= enc_wave_lds<D>(), "int16 staging must fit the wave region");
    static_assert(8 * kVqSlot * (int)sizeof(float4) <= enc_wave_lds<D>(), "the wave's table copies fit its region");
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * enc_wave_lds<D>()];
    constexpr int RS_B = kMaxGroupsDev * (4 + 8);
    constexpr bool RS_TAIL = 8 * CUBE_B + RS_B <= enc_wave_lds<D>();
    __shared__ __attribute__((aligned(16))) char rs_extra[RS_TAIL ? 16 : kWavesPerBlock * RS_B];
    __shared__ __attribute__((aligned(16))) uint16_t s_pos[CS];  // stream position -> byte offset in a cube
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t wid = blockIdx.x * kWavesPerBlock + wave;  // segment index
    const uint32_t cube0 = wid * kCubesPerWave;
    uint2 raw[D];
    __builtin_amdgcn_s_setprio(3);
    load_channel_rows<D, 0, PX, EDGE>(P, cube0 + (lane >> 3), cube0 + (lane >> 3) < P.n_cubes, lane & 7, 0, E.ch, raw);
    // the table of the lane's cube (a cube past the end: entry 0, never used)
    uint32_t ti = 0;
    if (cube0 + (lane >> 3) < P.n_cubes) ti = V.map[fdiv(cube0 + (lane >> 3), P.div_cps)];
    __builtin_amdgcn_s_setprio(0);
    if constexpr (PX != 1 || EDGE != 0) {
        if (blockIdx.x == 0 && P.replay_clear) {
#pragma unroll
            for (int i = 0; i < 2 * kCountSpread / kBlock; i++) P.replay_clear[i * kBlock + threadIdx.x] = 0u;
        }
    }
    {  // both loads in flight before the LDS writes
        static_assert(CS % kBlock == 0, "whole passes");
        uint16_t t[CS / kBlock];
#pragma unroll
        for (int r = 0; r < CS / kBlock; r++) t[r] = E.diag[threadIdx.x + r * kBlock];
#pragma unroll
        for (int r = 0; r < CS / kBlock; r++) s_pos[threadIdx.x + r * kBlock] = (uint16_t)k1_code_off<D>(t[r]);
    }
    __syncthreads();
    if (cube0 >= P.n_cubes) return;  // wave-uniform, after the barrier
    char* wl = lds + wave * enc_wave_lds<D>();
    char* rs = RS_TAIL ? wl + 8 * CUBE_B : rs_extra + wave * RS_B;
    static_assert((8 * CUBE_B) % 8 == 0 && RS_B % 8 == 0, "replay scratch alignment");
    const int c = lane >> 3, j = lane & 7;
    const int kz = (D == 8) ? j : (j >> 1);
    const int kx0 = (D == 8) ? 0 : (j & 1) * 4;
    const int so = kz + kx0;
    const bool valid = cube0 + c < P.n_cubes;

    float a[D][8];
    to_float<D>(raw, a);
    uint32_t S;
    int m;
    float A;
    cube_stats<D>(raw, a, S, m, A);
    asm volatile("" : "+v"(S), "+v"(m), "+v"(A), "+v"(ti));
    float b[8][NB];
    forward_cube<D, NB>(a, m, c, j, wl, b);

    // the wave's tables into its region (free until the codes are staged): the copy of cube cc's table at slot
    // cc, 3 rows per lane; a cube reads the slot of the first cube of the wave with its table
    const float4* tab;
    {
        wave_lds_sync();  // the transform's last reads of the region
        float4 row[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int i = lane + 64 * r, cc = i / kVqTabN;  // 192 rows = 8 cubes x kVqTabN
            const uint32_t tc = (uint32_t)__shfl((int)ti, cc * 8, 64);
            row[r] = V.tabs[tc * kVqTabN + (uint32_t)(i - cc * kVqTabN)];
        }
        int slot = c;
#pragma unroll
        for (int cc = 7; cc >= 0; cc--) {
            const uint32_t tc = (uint32_t)__builtin_amdgcn_readlane((int)ti, cc * 8);
            if (tc == ti) slot = cc;
        }
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int i = lane + 64 * r, cc = i / kVqTabN;
            ((float4*)wl)[cc * kVqSlot + (i - cc * kVqTabN)] = row[r];
        }
        wave_lds_sync();
        tab = (const float4*)wl + slot * kVqSlot;
    }

    int sz = so;
    float rr[NI], thr[NI];
    int32_t qv[8][NB];
    uint32_t fm_lo = 0, fm_hi = 0;  // uncertified mask: bit ky*NB + x (64 bits for NB = 8)
#pragma unroll
    for (int ky = 0; ky < 8; ky++) {
        pin(b[ky]);
        tab_window<NB, NI>(tab, sz, ky, A, rr, thr);
        bool f = false;
        float qq[NB];
#pragma unroll
        for (int x = 0; x < NB; x++) {
            qq[x] = b[ky][x] * rr[ky + x];
            const float n = __builtin_rintf(qq[x]);
            f |= __builtin_fabsf(qq[x] - n) >= thr[ky + x];
            qv[ky][x] = (int32_t)n;
        }
        if (__builtin_expect(f, 0)) {
            uint32_t bits = 0;
#pragma unroll
            for (int x = 0; x < NB; x++)
                if (__builtin_fabsf(qq[x] - __builtin_rintf(qq[x])) >= thr[ky + x]) bits |= 1u << x;
            const int sh = ky * NB;
            if (sh < 32) fm_lo |= bits << sh;
            else fm_hi |= bits << (sh - 32);
        }
        pin(qv[ky]);
        asm volatile("" : "+v"(fm_lo), "+v"(fm_hi));
    }
    if (j == 0) {
        qv[0][0] = java_round_dev(__ddiv_rn((double)S * P.coef_dc, enc_step<1>(tab, 0)));  // the cube's step[0]
        fm_lo &= ~1u;
    }
    if (!valid) fm_lo = fm_hi = 0;
    wave_lds_sync();  // the last reads of the table copies: the codes overwrite them

    // stage the cubes' Exp-Golomb codes as uint16, cube-major (k = (kz*8 + ky)*8 + kx at byte 2k of cube c)
#pragma unroll
    for (int ky = 0; ky < 8; ky++) {
        char* row = wl + c * CUBE_B + kz * FACE + ((D == 8) ? (((ky + kz) & 7) << 4) : 2 * (ky * 8 + kx0));
        if constexpr (D == 8) {
            *(uint4*)row = make_uint4(eg_code_pair(qv[ky][1], qv[ky][0]), eg_code_pair(qv[ky][3], qv[ky][2]),
                                      eg_code_pair(qv[ky][5], qv[ky][4]), eg_code_pair(qv[ky][7], qv[ky][6]));
        } else {
            *(uint2*)row = make_uint2(eg_code_pair(qv[ky][1], qv[ky][0]), eg_code_pair(qv[ky][3], qv[ky][2]));
        }
    }
    wave_lds_sync();

    // exact replay of the uncertified coefficients, one at a time by the whole wave (rare), each under the
    // source cube's table (its rows from global memory: the region holds the codes now)
    {
        ReplayGeom R{P.raster, P.cubes_per_stack, P.nbx, P.width, P.plane, P.stack_stride,
                     E.ngroups, E.coef, E.group_of};
        if constexpr (PX != 1) R.ch = E.ch;
        if constexpr (EDGE != 0) R.height = P.height;
        uint32_t nrep = 0;  // (counted by the PX / EDGE instantiations only)
        for (;;) {
            const unsigned long long who = __ballot((fm_lo | fm_hi) != 0u);
            if (who == 0ull) break;
            const int src = __builtin_ctzll(who);
            const int mybit = fm_lo ? __builtin_ctz(fm_lo) : (fm_hi ? 32 + __builtin_ctz(fm_hi) : 0);
            const int bit = __shfl(mybit, src, 64);
            const uint32_t tsrc = (uint32_t)__shfl((int)ti, src, 64);
            const int sj = src & 7, sc = src >> 3;
            const int skz = (D == 8) ? sj : (sj >> 1), skx0 = (D == 8) ? 0 : (sj & 1) * 4;
            const uint32_t k = (uint32_t)((skz * 8 + bit / NB) * 8 + skx0 + bit % NB);
            const int q = exact_coef<D, PX, EDGE, 1>(R, cube0 + sc, k, lane, (int*)rs, (double*)(rs + kMaxGroupsDev * 4),
                                                     V.tabs + tsrc * kVqTabN);
            if constexpr (PX != 1 || EDGE != 0) nrep++;
            if (lane == 0) *(uint16_t*)(wl + sc * CUBE_B + k1_code_off<D>(k)) = (uint16_t)(q > 0 ? 2 * q : 1 - 2 * q);
            if (lane == src) {
                if (fm_lo) fm_lo &= fm_lo - 1;
                else fm_hi &= fm_hi - 1;
            }
            wave_lds_sync();
        }
        if constexpr (PX != 1 || EDGE != 0) {
            if (nrep && lane == 0 && P.replay_count) atomicAdd(P.replay_count + (blockIdx.x & (kCountSpread - 1)), nrep);
        }
    }

    // Exp-Golomb: lane (cp, part) codes stream positions part*VPL .. +VPL-1 of cube cp (eg_lane_emit)
    const int cp = lane >> 3, part = lane & 7;
    const bool lvalid = cube0 + cp < P.n_cubes;
    const char* cb = wl + cp * CUBE_B;
    uint32_t zs = 0;  // sum of the leading-zero counts of the lane's codes
    uint32_t cds[VPL / 2];  // the lane's codes, two per register, kept for the emission
    if (lvalid) {
#pragma unroll
        for (int i0 = 0; i0 < VPL; i0 += 8) {
            const uint4 pp = *(const uint4*)&s_pos[part * VPL + i0];
            const uint32_t pw[4] = {pp.x, pp.y, pp.z, pp.w};
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const uint32_t lo = *(const uint16_t*)(cb + (pw[e >> 1] & 0xFFFFu));
                const uint32_t hi = *(const uint16_t*)(cb + (pw[e >> 1] >> 16));
                cds[(i0 + e) / 2] = lo | (hi << 16);
                zs += __builtin_clz(lo) + __builtin_clz(hi);
            }
        }
    }
    eg_lane_emit<VPL>(E, cds, zs, lvalid, lane, wid);
}

__global__ __launch_bounds__(kBlock) void vq_upload_kernel(const uint4* src, uint4* dst, uint32_t n16) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}

int launch_vq_upload(const void* src, void* dst, uint32_t n16, hipStream_t st) {
    if (n16 == 0) return 0;
    if (!src || !dst) return -1;
    hipLaunchKernelGGL(vq_upload_kernel, dim3((n16 + kBlock - 1) / kBlock), dim3(kBlock), 0, st, (const uint4*)src, (uint4*)dst, n16);
    return launched();
}

int launch_encode_eg_vq(int D, int px, int edge, const EncodeParams& P, const EgFusedParams& E, const VqParams& V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!V.tabs || !V.map) return -1;
    int rc = -1;
    with_variant(D, px, edge, [&](auto d, auto p, auto e) {
        const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
        hipLaunchKernelGGL((encode_eg_vq_kernel<d, p, e>), grid, dim3(kBlock), 0, st, P, E, V);
        rc = launched();
    });
    return rc;
}

}  // namespace dct3d
