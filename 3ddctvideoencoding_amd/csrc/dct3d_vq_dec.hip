// dct3d_vq_dec.hip -- the fused stream decode with a quantiser table per stack (dct3d_decode_eg_frames_vq*;
// DESIGN 4m).  decode_eg_vq_kernel is decode_eg_kernel<D, 8, EDGE, QT = 1> and decode_eg_rgb_vq_kernel is
// decode_eg_rgb_kernel<D, EDGE, QT = 1> (dct3d_eg_fused_dev.h), their bodies copied operation for operation; the
// one difference is the step pointer handed to decode_tile<..., QT = 1>, which already takes the lane's steps
// from a pointer by plain cached global loads: here it is per lane, steps + 32 * map[stack of the lane's cube],
// into the palette's [n_tables][32] fp64 array.  CODES' integer |q| * step products and the exact replay's
// re-parse (ReloadStreamVq) use the same entry.  The sync, scan and mark passes do not depend on the table.
// A translation unit of its own: no other code object changes.
#include "dct3d_eg_fused_dev.h"
#include "dct3d_vq.h"

namespace dct3d {

// The step pointer decode_tile<..., QT = 1> takes, for the lane's cube g (g < n_cubes: whole stacks, so the stack
// is inside the map).  decode_tile reads qsteps[4 h + k + j], j < 11: the pointer is formed as the palette's
// wave-uniform base plus one 32-bit lane offset (< 2^11 entries: 32 tables of 32 steps) that already holds
// 4 h + k, so that the loads keep a scalar base and one offset register, as the QT = 1 kernel's do.
template <int D>
__device__ __forceinline__ const double* vq_lane_steps(const VqParams& V, const DecodeParams& P, uint32_t g, int lane) {
    const uint32_t hk = (uint32_t)(4 * ((lane >> 4) & 1) + (lane & (D - 1)));
    const uint32_t o = ((uint32_t)kVqStepN * V.map[fdiv(g, P.div_cps)] + hk) & 0x7FFu;
    return (V.steps + o) - hk;
}

template <int D>
struct ReloadStreamVq {  // ReloadStreamQ with the table of the replayed cube's stack (steps: VqParams::steps)
    const uint32_t* words;
    uint64_t n_words;
    const uint16_t* mark;
    const uint64_t* mark_base;
    const uint16_t* diag;
    const double* steps;
    __device__ __forceinline__ void operator()(uint32_t g, double* cf, int lane) const {
        constexpr int PARTS = 64 * D / 32;
        if (lane < PARTS) {
            const double* st = steps + (size_t)kVqStepN * vq_map_behind(steps)[fdiv(g, *vq_div_behind(steps))];
            BitReader<GlobalBits> r{GlobalBits{words, n_words}, 0, 0, 0, 0};
            r.seek(mark_serial(mark, mark_base, (uint64_t)g * PARTS + lane));
            for (int i = 0; i < 32; i++) {
                uint32_t code = 1u;
                (void)r.get(code);
                const int k = diag[lane * 32 + i];
                const int kz = k / 64, ky = (k / 8) & 7, kx = k & 7;
                cf[k] = (double)eg_value(code) * st[kx + ky + kz];
            }
        }
    }
};

template <int D, int EDGE>
__global__ __launch_bounds__(kBlock, 4) void decode_eg_vq_kernel(DecodeParams P, EgDecParams E, VqParams V) {
    using G = DecGeom<D>;
    constexpr int NG = 8;
    constexpr uint32_t CS = G::CS, PARTS = CS / 32, CPW = G::CPW;
    static_assert(CPW * CS == 2048 && PARTS * CPW == 64, "one wave = 64 marks");
    constexpr uint32_t WIN = kDecWaveLds / 4 - 1;
    constexpr int NWP = 4;
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * kDecWaveLds];
    __shared__ uint16_t s_diag[CS];
    constexpr uint32_t SOFF = 40;
    __shared__ __attribute__((aligned(16))) uint16_t s_soff[PARTS * SOFF];
    dec_clear_next_slot(P);
    if (blockIdx.x == 0 && threadIdx.x == 0 && E.status_host) {  // the verdict to the host: the words, the tag
        uint64_t w[6];
#pragma unroll
        for (int i = 0; i < 6; i++) E.status_host[i] = w[i] = E.status[i];
        const uint32_t fl = (uint32_t)(w[2] & 7u) | (w[4] < E.n_values ? 8u : 0u);  // flags, short by the scan
        __hip_atomic_store(E.status_host + 6, hand_off_tag(E.seq, w[1], fl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (blockIdx.x == 0 && threadIdx.x < 6 && E.status_clear) E.status_clear[threadIdx.x] = 0u;
    // corrupt / short / empty stream: reported by the mark pass (block-uniform)
    if (E.status[2] != 0 || E.n_words == 0) return;
    const bool long_codes = E.status[3] != 0;  // the stream holds a code of 33+ bits (the mark pass)
    {  // both loads in flight before the LDS writes
        static_assert(CS % kBlock == 0, "whole passes");
        uint16_t t[CS / kBlock];
#pragma unroll
        for (uint32_t r = 0; r < CS / kBlock; r++) t[r] = E.diag[threadIdx.x + r * kBlock];
#pragma unroll
        for (uint32_t r = 0; r < CS / kBlock; r++) {
            const uint32_t i = threadIdx.x + r * kBlock, k = t[r];
            s_diag[i] = t[r];
            s_soff[(i / 32) * SOFF + i % 32] = (uint16_t)((k >> 6) * G::SA_F + (k & 63) * 4);
        }
    }
    __syncthreads();
    const int lane0 = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* wl = lds + wave * kDecWaveLds;
    uint32_t* win = (uint32_t*)wl + 1;  // the window one word into the region: parse_step reads win[-1]
    const uint64_t n_marks = E.n_values / 32;
    const uint32_t row0 = xcd_tile() * NG;  // the block's first round of 4 groups
    auto cube_of = [&](int i) { return P.cube_base + ((row0 + (uint32_t)i) * kWavesPerBlock + wave) * CPW; };
    static_assert(kMarkGroup == 64, "a group = one mark group");
    auto load_marks = [&](int lane, uint32_t cube0, uint64_t& gb, uint32_t& myl, uint64_t& last) {
        const uint64_t m0 = (uint64_t)cube0 * CS / 32;
        gb = m0 < n_marks ? E.mark_base[m0 / kMarkGroup] : 0u;
        myl = m0 + lane < n_marks ? (uint32_t)E.mark[m0 + lane] : ~0u;
        last = m0 + 64 < n_marks ? E.mark_base[m0 / kMarkGroup + 1] : E.status[1];
    };
    auto open_window = [&](int lane, uint64_t gb, uint32_t myl, uint64_t last, uint64_t& w0, uint32_t& rel,
                           uint64_t& span, uint32_t (&t)[NWP]) {
        w0 = uniform_u64(gb >> 5);  // the group's first mark
        const uint32_t off = mark_offset(myl, (uint16_t)gb);
        rel = myl <= 0xFFFFu ? (uint32_t)(gb & 31) + off : 0u;
        const uint64_t lw = uniform_u64(last);
        span = (lw >> 5) + 5 - w0;
        const uint64_t wb = min(w0, E.n_words - 1);
        const uint32_t jmax = (uint32_t)min(E.n_words - 1 - wb, (uint64_t)0xFFFFFFFFu);
#pragma unroll
        for (int b = 0; b < NWP; b++) t[b] = E.words[wb + min((uint32_t)(b * 64 + lane), jmax)];
    };
    uint64_t w0, span;
    uint32_t rel;
    uint32_t pw[NWP];
    {
        uint64_t gb, last;
        uint32_t myl;
        __builtin_amdgcn_s_setprio(3);  // marks and window loads ahead of the computing waves
        load_marks(lane0, cube_of(0), gb, myl, last);
        open_window(lane0, gb, myl, last, w0, rel, span, pw);
        __builtin_amdgcn_s_setprio(0);
    }
    for (int i = 0; i < NG; i++) {
        const uint32_t cube0 = cube_of(i);
        if (cube0 >= P.n_cubes) break;  // wave-uniform; every later group of the wave is past the end too
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const bool fits = span <= WIN;  // wave-uniform; else the parse reads global memory (parse_codes)
        const uint32_t nwin = (uint32_t)(fits ? span : 0);
        __builtin_amdgcn_s_setprio(2);
        const uint32_t nlive = (uint32_t)min((uint64_t)nwin, E.n_words - w0);
        static_assert(NWP * 64 <= WIN, "look-ahead inside the region");
#pragma unroll
        for (int b = 0; b < NWP; b++) {
            const uint32_t j = b * 64 + lane;
            if (b * 64 < nwin) win[j] = j < nlive ? __builtin_bswap32(pw[b]) : 0u;
        }
        for (uint32_t i0 = NWP * 64; i0 < nwin; i0 += 256) {
            uint32_t t[4];
#pragma unroll
            for (int b = 0; b < 4; b++) t[b] = E.words[min(w0 + i0 + b * 64 + lane, E.n_words - 1)];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t j = i0 + b * 64 + lane;
                if (j < nwin) win[j] = j < nlive ? __builtin_bswap32(t[b]) : 0u;
            }
        }
        uint64_t gb_n = 0, last_n = 0;
        uint32_t myl_n = 0;
        __builtin_amdgcn_s_setprio(3);
        if (i + 1 < NG) load_marks(lane, cube_of(i + 1), gb_n, myl_n, last_n);  // in flight during the parse
        __builtin_amdgcn_s_setprio(2);
        wave_lds_sync();
        uint32_t v[32];  // codes: decode_tile<CODES> converts them in its dequantisation
        parse_codes<32>(E, win, nwin, w0, fits, long_codes, rel, v);
        __builtin_amdgcn_s_setprio(3);
        if (i + 1 < NG) open_window(lane, gb_n, myl_n, last_n, w0, rel, span, pw);  // in flight during the transform
        __builtin_amdgcn_s_setprio(2);
        wave_lds_sync();
        {  // each value to its diagonal position in the staging: 8 offsets per 16-byte table read
            const uint32_t c = lane / PARTS, part = lane % PARTS;
            char* cb = wl + c * G::SA_C;
            const uint4* so = (const uint4*)(s_soff + part * SOFF);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 o = so[q];
                const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                for (int e = 0; e < 8; e++)
                    *(uint32_t*)(cb + ((w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu)) = v[q * 8 + e];
            }
        }
        wave_lds_sync();
        __builtin_amdgcn_s_setprio(0);  // the transform
        // the steps of the lane's cube (a lane whose cube is past the end: the last cube's, its output unused),
        // looked up here and not earlier (the opaque lane: no register is held across the parse for it)
        int ql = lane;
        asm volatile("" : "+v"(ql));
        const double* const qs = vq_lane_steps<D>(V, P, min(cube0 + (uint32_t)dec_cube_of_lane<D>(ql), P.n_cubes - 1), ql);
        decode_tile<D, true, true, false, EDGE, 1>(
            P, wl, lane, cube0, [] {},
            ReloadStreamVq<D>{E.words, E.n_words, E.mark, E.mark_base, s_diag, V.steps}, nullptr, nullptr, qs);
        if (i + 1 < NG) {
            if (P.blk_store && cube0 - (uint32_t)wave * CPW + kWavesPerBlock * CPW <= P.n_cubes) __syncthreads();
            else wave_lds_sync();
        }
    }
}

template <int D, int EDGE>
__global__ __launch_bounds__(kBlock, 3) void decode_eg_rgb_vq_kernel(DecodeParams P, EgDecRgbParams E, VqParams V) {
    using G = DecGeom<D>;
    constexpr uint32_t CS = G::CS, PARTS = CS / 32, CPW = G::CPW;
    static_assert(CPW * CS == 2048 && PARTS * CPW == 64, "one wave = 64 marks");
    constexpr uint32_t WIN = kDecWaveLds / 4 - 1;
    constexpr int NW = (D == 8) ? 1 : 2;  // words per plane and channel
    __shared__ __attribute__((aligned(16))) char lds[kWavesPerBlock * kDecWaveLds];
    __shared__ uint16_t s_diag[CS];
    constexpr uint32_t SOFF = 40;  // (as decode_eg_kernel's)
    __shared__ __attribute__((aligned(16))) uint16_t s_soff[PARTS * SOFF];
    dec_clear_next_slot(P);
    // corrupt / short / empty / unresolved stream, any channel: reported by its mark pass (block-uniform)
    if (E.s[0].status[2] != 0 || E.s[1].status[2] != 0 || E.s[2].status[2] != 0 || E.s[0].n_words == 0 ||
        E.s[1].n_words == 0 || E.s[2].n_words == 0 || E.s[0].status[4] < E.s[0].n_values ||
        E.s[1].status[4] < E.s[1].n_values || E.s[2].status[4] < E.s[2].n_values)
        return;
    {
        static_assert(CS % kBlock == 0, "whole passes");
        uint16_t t[CS / kBlock];
#pragma unroll
        for (uint32_t r = 0; r < CS / kBlock; r++) t[r] = E.diag[threadIdx.x + r * kBlock];
#pragma unroll
        for (uint32_t r = 0; r < CS / kBlock; r++) {
            const uint32_t i = threadIdx.x + r * kBlock, k = t[r];
            s_diag[i] = t[r];
            s_soff[(i / 32) * SOFF + i % 32] = (uint16_t)((k >> 6) * G::SA_F + (k & 63) * 4);
        }
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    char* wl = lds + wave * kDecWaveLds;
    uint32_t* win = (uint32_t*)wl + 1;  // parse_step reads win[-1]
    const uint32_t cube0 = P.cube_base + (xcd_tile() * kWavesPerBlock + wave) * CPW;
    if (cube0 >= P.n_cubes) return;  // wave-uniform (a block with such a wave takes no block store: no barrier follows)
    uint32_t out3[D][3 * NW];
#pragma unroll
    for (int z = 0; z < D; z++)
#pragma unroll
        for (int i = 0; i < 3 * NW; i++) out3[z][i] = 0u;
    bool valid = false;
#pragma unroll 1
    for (int ch = 0; ch < 3; ch++) {
        int lane = threadIdx.x & 63;
        asm volatile("" : "+v"(lane));
        const EgDecStream S = E.s[ch];
        const bool long_codes = S.status[3] != 0;
        const uint64_t n_marks = S.n_values / 32;
        __builtin_amdgcn_s_setprio(3);  // marks and window loads ahead of the computing waves
        const uint64_t m0 = (uint64_t)cube0 * CS / 32;  // < n_marks: cube0 < n_cubes
        const uint64_t gb = S.mark_base[m0 / kMarkGroup];
        const uint32_t myl = m0 + lane < n_marks ? (uint32_t)S.mark[m0 + lane] : ~0u;
        const uint64_t last = m0 + 64 < n_marks ? S.mark_base[m0 / kMarkGroup + 1] : S.status[1];
        const uint64_t w0 = uniform_u64(gb >> 5);
        const uint32_t off = mark_offset(myl, (uint16_t)gb);
        const uint32_t rel = myl <= 0xFFFFu ? (uint32_t)(gb & 31) + off : 0u;
        const uint64_t span = (uniform_u64(last) >> 5) + 5 - w0;
        const bool fits = span <= WIN;  // wave-uniform; else the parse reads global memory (parse_codes)
        const uint32_t nwin = (uint32_t)(fits ? span : 0);
        const uint32_t nlive = (uint32_t)min((uint64_t)nwin, S.n_words - w0);  // w0 < n_words: a mark of the stream
        wave_lds_sync();  // the previous channel's use of the region is over
        for (uint32_t i0 = 0; i0 < nwin; i0 += 256) {  // 4 words per lane per round, the loads before the LDS writes
            uint32_t t[4];
#pragma unroll
            for (int b = 0; b < 4; b++) t[b] = S.words[min(w0 + i0 + b * 64 + lane, S.n_words - 1)];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t j = i0 + b * 64 + lane;
                if (j < nwin) win[j] = j < nlive ? __builtin_bswap32(t[b]) : 0u;
            }
        }
        __builtin_amdgcn_s_setprio(2);
        wave_lds_sync();
        uint32_t v[32];  // codes: decode_tile<CODES> converts them in its dequantisation
        {
            EgDecParams L{};  // (parse_codes reads the stream's words alone)
            L.words = S.words;
            L.n_words = S.n_words;
            parse_codes<32>(L, win, nwin, w0, fits, long_codes, rel, v);
        }
        wave_lds_sync();
        {  // each value to its diagonal position in the staging: 8 offsets per 16-byte table read
            const uint32_t c = lane / PARTS, part = lane % PARTS;
            char* cb = wl + c * G::SA_C;
            const uint4* so = (const uint4*)(s_soff + part * SOFF);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint4 o = so[q];
                const uint32_t w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                for (int e = 0; e < 8; e++)
                    *(uint32_t*)(cb + ((w[e >> 1] >> (16 * (e & 1))) & 0xFFFFu)) = v[q * 8 + e];
            }
        }
        wave_lds_sync();
        __builtin_amdgcn_s_setprio(0);  // the transform
        uint32_t outw[D][NW];
        // the steps of the lane's cube (all three channels of a stack share its table), looked up here and not
        // earlier (the opaque lane: no register is held across the parse for it)
        int ql = lane;
        asm volatile("" : "+v"(ql));
        const double* const qs = vq_lane_steps<D>(V, P, min(cube0 + (uint32_t)dec_cube_of_lane<D>(ql), P.n_cubes - 1), ql);
        decode_tile<D, false, true, true, 0, 1>(
            P, wl, lane, cube0, [] {},
            ReloadStreamVq<D>{S.words, S.n_words, S.mark, S.mark_base, s_diag, V.steps}, &outw[0][0], &valid, qs);
        const uint32_t s0 = ch == 0 ? rgb_put_sel(0, 0) : ch == 1 ? rgb_put_sel(1, 0) : rgb_put_sel(2, 0);
        const uint32_t s1 = ch == 0 ? rgb_put_sel(0, 1) : ch == 1 ? rgb_put_sel(1, 1) : rgb_put_sel(2, 1);
        const uint32_t s2 = ch == 0 ? rgb_put_sel(0, 2) : ch == 1 ? rgb_put_sel(1, 2) : rgb_put_sel(2, 2);
#pragma unroll
        for (int z = 0; z < D; z++)
#pragma unroll
            for (int wd = 0; wd < NW; wd++) {
                out3[z][3 * wd] = __builtin_amdgcn_perm(out3[z][3 * wd], outw[z][wd], s0);
                out3[z][3 * wd + 1] = __builtin_amdgcn_perm(out3[z][3 * wd + 1], outw[z][wd], s1);
                out3[z][3 * wd + 2] = __builtin_amdgcn_perm(out3[z][3 * wd + 2], outw[z][wd], s2);
            }
    }
    __builtin_amdgcn_s_setprio(2);  // the store phase ahead of the computing waves
    dec_store_tile<D, false, 3, EDGE>(P, wl, (int)(threadIdx.x & 63), cube0, out3, valid);
}

int launch_decode_eg_vq(int D, int edge, const DecodeParams& P, const EgDecParams& E, const VqParams& V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!V.steps || !V.map) return -1;
    int rc = -1;
    with_variant(D, 1, edge, [&](auto d, auto, auto e) {
        const dim3 grid(dec_grid(d, P.n_cubes - P.cube_base, 8));  // cube_base: a multiple of the cubes per wave
        hipLaunchKernelGGL((decode_eg_vq_kernel<d, e>), grid, dim3(kBlock), 0, st, P, E, V);
        rc = launched();
    });
    return rc;
}

int launch_decode_eg_rgb_vq(int D, int edge, const DecodeParams& P, const EgDecRgbParams& E, const VqParams& V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!V.steps || !V.map) return -1;
    int rc = -1;
    with_variant(D, 3, edge, [&](auto d, auto, auto e) {
        const dim3 grid(dec_grid(d, P.n_cubes - P.cube_base));
        hipLaunchKernelGGL((decode_eg_rgb_vq_kernel<d, e>), grid, dim3(kBlock), 0, st, P, E, V);
        rc = launched();
    });
    return rc;
}

}  // namespace dct3d
