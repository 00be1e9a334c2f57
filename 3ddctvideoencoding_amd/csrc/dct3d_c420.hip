// dct3d_c420.hip -- 4:2:0 chroma subsampling fused into the YCbCr stream calls and the rate probe
// (dct3d_ctx_set_chroma = DCT3D_CHROMA_420 on top of DCT3D_OPT_COLOUR = DCT3D_COLOUR_YCBCR).
// Encode and rate probe: the CT = 2 instances of encode_eg_kernel (dct3d_eg_fused_dev.h) and rate_kernel
// (dct3d_rate_dev.h), whose rows and replay reloads are the subsampled Cb or Cr plane made from the packed pixels
// on the way in (c420_row8, dct3d_encode_dev.h).  Channel 0 is the CT = 1 chain of dct3d_ycc.hip at the full
// geometry.  Decode: streams 1 and 2 go through the grey stream decode at the chroma geometry into two planes the
// context owns; decode_eg_y420_kernel below then decodes stream 0 as one channel pass of decode_eg_rgb_kernel
// does, fetches each pixel's Cb and Cr at (y >> 1, x >> 1) of those planes, and stores R, G, B once.
// A translation unit of its own: no other code object changes, and a context that does not set the mode never
// comes here.  The instances are keyed (D, edge, qt) by this unit's launchers; they are no value of the variant's
// colour axis (dct3d_variant.h).
#include "dct3d_c420.h"
#include "dct3d_eg_fused_dev.h"
#include "dct3d_rate_dev.h"

namespace dct3d {

// the 12 packed bytes {Y, Cb, Cr} x 4 pixels from a word of 4 Y samples and the chroma of its two pixel pairs
__device__ __forceinline__ void c420_merge4(uint32_t y4, uint32_t cb0, uint32_t cr0, uint32_t cb1, uint32_t cr1,
                                            uint32_t& a, uint32_t& b, uint32_t& c) {
    a = (y4 & 0xFFu) | (cb0 << 8) | (cr0 << 16) | ((y4 >> 8) << 24);
    b = cb0 | (cr0 << 8) | (((y4 >> 16) & 0xFFu) << 16) | (cb1 << 24);
    c = cr1 | ((y4 >> 24) << 8) | (cb1 << 16) | (cr1 << 24);
}

// Stream 0 of a packed RGB24 call under 4:2:0 -> the frames.  The marks, the window, the parse, the scatter and
// decode_tile<KEEP> are one channel pass of decode_eg_rgb_kernel on the Y stream (P: the frames' geometry, P.height
// set whatever EDGE).  Lane (c, y, h) then holds NXC = 4 | 8 pixels of row by * 8 + y from column bx * 8 + x0 of D
// frames: their chroma is sample (row >> 1, col >> 1 ..) of frame s * D + z of the planes C, NXC / 2 bytes per
// plane and frame, the indices clamped into the plane (a lane of the padding, which stores nothing, reads inside
// too; a lane whose cube is past the end reads nothing).  The bytes are merged, go through ycc_to_rgb4 in registers
// and leave by the one dec_store_tile<PX = 3>.  A launch whose three fronts are not all good writes nothing.
template <int D, int EDGE = 0, int QT = 0, class... VQ>
__global__ __launch_bounds__(kBlock, 3) void decode_eg_y420_kernel(typename DecodeArgs<QT>::type P, EgDecRgbParams E,
                                                                    C420Planes C, VQ... vq) {
    static_assert(sizeof...(VQ) == (QT == 2 ? 1 : 0), "the VqParams (vq_of) with QT = 2, and only then");
    using G = DecGeom<D>;
    constexpr uint32_t CS = G::CS, PARTS = CS / 32, CPW = G::CPW;
    static_assert(CPW * CS == 2048 && PARTS * CPW == 64, "one wave = 64 marks");
    constexpr uint32_t WIN = kDecWaveLds / 4 - 1;
    constexpr int NW = (D == 8) ? 1 : 2;  // words per plane and channel
    constexpr int NXC = 4 * NW;           // the lane's pixels per plane
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
    int lane = threadIdx.x & 63;
    asm volatile("" : "+v"(lane));
    const EgDecStream S = E.s[0];
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
    dec_scatter_codes<D, SOFF>(wl, s_soff, lane, v);
    wave_lds_sync();
    __builtin_amdgcn_s_setprio(0);  // the transform
    uint32_t outw[D][NW];
    bool valid = false;
    if constexpr (QT == 2) {
        const VqParams& V = vq_of(vq...);
        int ql = lane;
        asm volatile("" : "+v"(ql));
        const double* const qs = vq_lane_steps<D>(V, P, min(cube0 + (uint32_t)dec_cube_of_lane<D>(ql), P.n_cubes - 1), ql);
        decode_tile<D, false, true, true, 0, 1>(
            P, wl, lane, cube0, [] {},
            ReloadStreamVq<D>{S.words, S.n_words, S.mark, S.mark_base, s_diag, V.steps}, &outw[0][0], &valid, qs);
    } else if constexpr (QT)
        decode_tile<D, false, true, true, 0, 1>(P, wl, lane, cube0, [] {},
                                                ReloadStreamQ<D>{S.words, S.n_words, S.mark, S.mark_base, s_diag, dec_steps(P)},
                                                &outw[0][0], &valid, dec_steps(P));
    else
        decode_tile<D, false, true, true>(P, wl, lane, cube0, [] {},
                                          ReloadStream<D>{S.words, S.n_words, S.mark, S.mark_base, s_diag},
                                          &outw[0][0], &valid);
    // the lane's place in the frames (dec_store_tile's) and its chroma samples
    uint32_t out3[D][3 * NW];
#pragma unroll
    for (int z = 0; z < D; z++)
#pragma unroll
        for (int i = 0; i < 3 * NW; i++) out3[z][i] = 0u;
    if (valid) {
        int sl = (int)(threadIdx.x & 63);
        asm volatile("" : "+v"(sl));
        const int h = (sl >> 4) & 1, k = sl & (D - 1);
        const uint32_t y = (D == 8) ? k : (4 * h + k), x0 = (D == 8) ? 4 * h : 0;
        const uint32_t g = cube0 + (uint32_t)dec_cube_of_lane<D>(sl);
        const uint32_t s = fdiv(g, P.div_cps);
        const uint32_t rr = g - s * P.cubes_per_stack;
        const uint32_t by = fdiv(rr, P.div_nbx), bx = rr - by * P.nbx;
        const uint32_t cw = (P.width + 1) >> 1, chh = (P.height + 1) >> 1;
        const uint32_t crow = min((by * 8 + y) >> 1, chh - 1);
        uint32_t ccol[NXC / 2];
#pragma unroll
        for (int i = 0; i < NXC / 2; i++) ccol[i] = min(((bx * 8 + x0) >> 1) + (uint32_t)i, cw - 1);
        const size_t cplane = (size_t)chh * cw;
        const size_t c0 = ((size_t)s * D) * cplane + (size_t)crow * cw;
        uint32_t cbv[D][NXC / 2], crv[D][NXC / 2];
#pragma unroll
        for (int z = 0; z < D; z++)
#pragma unroll
            for (int i = 0; i < NXC / 2; i++) {
                cbv[z][i] = C.cb[c0 + (size_t)z * cplane + ccol[i]];
                crv[z][i] = C.cr[c0 + (size_t)z * cplane + ccol[i]];
            }
#pragma unroll
        for (int z = 0; z < D; z++)
#pragma unroll
            for (int wd = 0; wd < NW; wd++) {
                c420_merge4(outw[z][wd], cbv[z][2 * wd], crv[z][2 * wd], cbv[z][2 * wd + 1], crv[z][2 * wd + 1],
                            out3[z][3 * wd], out3[z][3 * wd + 1], out3[z][3 * wd + 2]);
                ycc_to_rgb4(out3[z][3 * wd], out3[z][3 * wd + 1], out3[z][3 * wd + 2]);
            }
    }
    __builtin_amdgcn_s_setprio(2);  // the store phase ahead of the computing waves
    dec_store_tile<D, false, 3, EDGE>(P, wl, (int)(threadIdx.x & 63), cube0, out3, valid);
}

int launch_encode_eg_c420(int D, int edge, int qt, const EncodeParams& P, const EgFusedParams& E, const VqParams* V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (E.ch != 1 && E.ch != 2) return -1;
    int rc = -1;
    with_depth(D, [&](auto d) { with_flag(edge, [&](auto e) {
        with_table(qt, [&](auto q) {
            constexpr int Dv = decltype(d)::value, Pv = 3, Ev = decltype(e)::value, Qv = decltype(q)::value;
            const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
            if constexpr (Qv == 2) {
                if (!V || !V->tabs || !V->map) return;
                hipLaunchKernelGGL((encode_eg_kernel<Dv, Pv, Ev, 2, 2, VqParams>), grid, dim3(kBlock), 0, st, P, E, *V);
            } else {
                hipLaunchKernelGGL((encode_eg_kernel<Dv, Pv, Ev, Qv, 2>), grid, dim3(kBlock), 0, st, P, E);
            }
            rc = launched();
        });
    }); });
    return rc;
}

int launch_rate_c420(int D, int edge, const EncodeParams& P, const RateParams& R, hipStream_t st) {
    if (R.ch != 1 && R.ch != 2) return -1;
    return probe_dispatch(D, 3, edge, P, R, [&](auto d, auto, auto e) {
        const dim3 grid(grid_blocks(P.n_cubes, kCubesPerWave));
        hipLaunchKernelGGL((rate_kernel<decltype(d)::value, 3, decltype(e)::value, 2>), grid, dim3(kBlock), 0, st, P, R);
    });
}

int launch_decode_eg_y420(int D, int edge, int qt, const DecodeParamsQ& P, const EgDecRgbParams& E, const C420Planes& C,
                          const VqParams* V, hipStream_t st) {
    if (P.n_cubes == 0) return 0;
    if (!C.cb || !C.cr) return -1;
    int rc = -1;
    with_depth(D, [&](auto d) { with_flag(edge, [&](auto e) {
        with_table(qt, [&](auto q) {
            constexpr int Dv = decltype(d)::value, Ev = decltype(e)::value, Qv = decltype(q)::value;
            if (Qv == 2 ? !V || !V->steps || !V->map : Qv && !P.steps) return;
            const dim3 grid(dec_grid(Dv, P.n_cubes - P.cube_base));
            if constexpr (Qv == 2) hipLaunchKernelGGL((decode_eg_y420_kernel<Dv, Ev, 2, VqParams>), grid, dim3(kBlock), 0, st, P, E, C, *V);
            else hipLaunchKernelGGL((decode_eg_y420_kernel<Dv, Ev, Qv>), grid, dim3(kBlock), 0, st, P, E, C);
            rc = launched();
        });
    }); });
    return rc;
}

}  // namespace dct3d
