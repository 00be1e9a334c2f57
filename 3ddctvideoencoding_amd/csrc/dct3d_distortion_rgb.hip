// dct3d_distortion_rgb.hip -- the RGB-domain distortion probe (dct3d_distortion_rgb_frames*): the exact
// squared error, in the RGB pixels, of the YCbCr (and 4:2:0) stream encode + decode under a list of (Y, Cb, Cr)
// table triples.  Pass 1 instantiates the distortion probes' one body (distortion_body, dct3d_distortion_dev.h) on
// one plane of the colour transform with the rate kernel's colour axis: per table it quantises, certifies, folds and
// decodes as the plane probe does, keeps the plane's squared error and bits, and stores the decoded samples inside
// the plane into a dense plane the context owns.  Pass 2 reads a candidate's three decoded planes beside the source pixels, upsamples the chroma
// by replication, runs ycc_to_rgb4 and takes the squared error per cube of the frames' grid.  The RGB and luma SSIM
// probe (dct3d_ssim_rgb_frames*) is pass 1 as it is and a pass 2 of its own, ssim_rgb_block_kernel.  A
// translation unit of its own: no other kernel's code object changes with it.
#include "dct3d_distortion_rgb.h"
#include "dct3d_distortion_dev.h"
#include "dct3d_eg_fused_dev.h"

namespace dct3d {

// Pass 1: distortion_body (dct3d_distortion_dev.h) on plane R.ch of the colour transform, CT = 1 | 2
template <int D, int EDGE, int CT>
__global__ __launch_bounds__(kBlock, 2) void distortion_plane_kernel(EncodeParams P, DistPlaneParams R) {
    distortion_body<D, 3, EDGE, 0, CT>(P, R);
}

// Pass 2.  Thread (cube, y) of a block of 32 cubes x 8 rows takes row y of its cube: 8 pixels of D frames.  A row
// piece that lies inside the frame loads whole words (byte aligned); any other loads its pixels one at a time, the
// column clamped into the frame, and masks what lies outside.  blockIdx.y: the candidate.  Both pass-2 kernels load
// through rgbc_load_row and merge through rgbc_rgb4; each keeps its own lane set-up (sharing it costs
// ssim_rgb_block_kernel<D, 0> a wave per SIMD), and they treat a lane outside the frame differently.
typedef unsigned rgbc_u32_u_t __attribute__((aligned(1)));
__device__ __forceinline__ uint32_t rgbc_byte(uint32_t w, int i) { return (w >> (8 * i)) & 0xFFu; }
// A lane's row piece in its current frame: where it starts in the candidate's three planes and in the source, its
// pixels inside the frame (npx) and its column in the frame and in the chroma planes
struct RgbcRow {
    const uint8_t *yp, *cbp, *crp, *src;
    size_t yframe, cframe;
    uint32_t npx, col, ccol;
    __device__ __forceinline__ void next_frame() {
        yp += yframe;
        cbp += cframe;
        crp += cframe;
        src += 3 * yframe;
    }
};
// The one loader of pass 2: the row piece's 24 source bytes (x3), 8 Y samples (yw) and the chroma samples of its 8
// pixels, upsampled (cbv, crv), of a lane with npx >= 1
__device__ __forceinline__ void rgbc_load_row(const RgbCombineParams& C, const RgbcRow& W, uint32_t (&x3)[6],
                                              uint32_t (&yw)[2], uint32_t (&cbv)[8], uint32_t (&crv)[8]) {
    if (W.npx == 8u) {
#pragma unroll
        for (int i = 0; i < 6; i++) x3[i] = *(const rgbc_u32_u_t*)(W.src + 4 * i);
        yw[0] = *(const rgbc_u32_u_t*)W.yp;
        yw[1] = *(const rgbc_u32_u_t*)(W.yp + 4);
        if (C.shift) {  // 4 samples per plane: (col + 7) >> 1 < cw
            const uint32_t b4 = *(const rgbc_u32_u_t*)W.cbp, r4 = *(const rgbc_u32_u_t*)W.crp;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                cbv[i] = rgbc_byte(b4, i >> 1);
                crv[i] = rgbc_byte(r4, i >> 1);
            }
        } else {
            const uint32_t b0 = *(const rgbc_u32_u_t*)W.cbp, b1 = *(const rgbc_u32_u_t*)(W.cbp + 4);
            const uint32_t r0 = *(const rgbc_u32_u_t*)W.crp, r1 = *(const rgbc_u32_u_t*)(W.crp + 4);
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
            const uint32_t xi = min((uint32_t)i, W.npx - 1u);  // clamped into the row
            const uint32_t ci = ((W.col + xi) >> C.shift) - W.ccol;
            cbv[i] = W.cbp[ci];
            crv[i] = W.crp[ci];
            if ((uint32_t)i < W.npx) {
                yw[i >> 2] |= (uint32_t)W.yp[i] << (8 * (i & 3));
#pragma unroll
                for (int k = 0; k < 3; k++) x3[(3 * i + k) >> 2] |= (uint32_t)W.src[3 * i + k] << (8 * ((3 * i + k) & 3));
            }
        }
    }
}
// The decoded RGB bytes of pixels 4 hw .. 4 hw + 3 of the row piece: three words, packed as the source's
__device__ __forceinline__ void rgbc_rgb4(int hw, const uint32_t (&yw)[2], const uint32_t (&cbv)[8], const uint32_t (&crv)[8],
                                          uint32_t& a, uint32_t& b, uint32_t& c) {
    const uint32_t y4 = yw[hw];
    const uint32_t* cb = cbv + 4 * hw;
    const uint32_t* cr = crv + 4 * hw;
    a = rgbc_byte(y4, 0) | (cb[0] << 8) | (cr[0] << 16) | (rgbc_byte(y4, 1) << 24);
    b = cb[1] | (cr[1] << 8) | (rgbc_byte(y4, 2) << 16) | (cb[2] << 24);
    c = cr[2] | (rgbc_byte(y4, 3) << 8) | (cb[3] << 16) | (cr[3] << 24);
    ycc_to_rgb4(a, b, c);
}

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
        RgbcRow W{yp, cbp, crp, src, yframe, cframe, npx, col, ccol};
        for (int z = 0; z < D; z++, W.next_frame()) {
            uint32_t x3[6], yw[2], cbv[8], crv[8];
            rgbc_load_row(C, W, x3, yw, cbv, crv);
#pragma unroll
            for (int hw = 0; hw < 2; hw++) {
                uint32_t a, b, c;
                rgbc_rgb4(hw, yw, cbv, crv, a, b, c);
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
    const uint8_t *yp = nullptr, *cbp = nullptr, *crp = nullptr, *src = nullptr;  // (stay null outside the frame)
    if (live) {
        yp = C.y + (size_t)sl[0] * C.y_stride + ((size_t)s * D * C.h + row) * C.w + col;
        const size_t coff = ((size_t)s * D * C.chh + crow) * C.cw + ccol;
        cbp = C.cb + (size_t)sl[1] * C.c_stride + coff;
        crp = C.cr + (size_t)sl[2] * C.c_stride + coff;
        src = C.frames + ((size_t)s * D * C.h + row) * C.w * 3 + (size_t)col * 3;
    }
    RgbcRow W{yp, cbp, crp, src, yframe, cframe, npx, col, ccol};
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
        if (npx) rgbc_load_row(C, W, x3, yw, cbv, crv);
#pragma unroll
        for (int hw = 0; hw < 2; hw++) {
            uint32_t a, b, c;
            rgbc_rgb4(hw, yw, cbv, crv, a, b, c);
            const uint32_t y4 = yw[hw];
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
                lo = quad_add<2>(quad_add<1>(lo));
                hi = quad_add<2>(quad_add<1>(hi));
                mx = quad_add<2>(quad_add<1>(mx));
                if (bst[hw]) {
                    rec_y[(size_t)k * plane_y + z * blkz + hw] = ((uint64_t)hi << 32) | lo;
                    if (cand == 0u) rec_x[(size_t)k * S.blk_stride + z * blkz + hw] = mx;  // (the same under every candidate)
                }
            }
        }
        W.next_frame();
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
