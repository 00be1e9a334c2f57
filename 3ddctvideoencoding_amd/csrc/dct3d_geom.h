// dct3d_geom.h -- a call's raster geometry and the kernel parameters' address fields derived from it: the one
// place that knows how w x h frames of px bytes per pixel become n_cubes, nbx, the FastDivs, plane, ...
// Plain C++ (no HIP include): the runtime, the diagnostics library and a CPU test (tests/test_geom.py) share it.
#pragma once
#include <cstdint>

namespace dct3d {

// n / d for n < 2^31 as one 32x32->64 multiply and a shift (Granlund-Montgomery: s = 31 + ceil(log2 d),
// m = ceil(2^s / d) < 2^32 gives floor(n m / 2^s) = floor(n / d) for every n < 2^31)
struct FastDiv {
    uint32_t m, s;
};
inline FastDiv fast_div(uint32_t d) {
    uint32_t l = 0;
    while ((1ull << l) < d) l++;
    FastDiv f;
    f.s = 31 + l;
    f.m = (uint32_t)(((1ull << f.s) + d - 1) / d);
    return f;
}

// w x h frames of px bytes per pixel (1 grey, 3 packed RGB24), dense.  The cubes tile the padded wp x hp raster
// (the next multiples of 8), which repeats each frame's last column and last row and exists nowhere in
// memory: the edge kernels clamp their row loads (encode) and crop their stores (decode).
struct Geom {
    int w, h, wp, hp, px;
    bool edge() const { return wp != w || hp != h; }
    uint64_t cps() const { return (uint64_t)(wp / 8) * (uint64_t)(hp / 8); }  // cubes per stack and channel
    uint64_t plane() const { return (uint64_t)px * w * h; }                   // bytes of a frame
};

// Checks a call's geometry and builds it; any_size = false: w and h must be multiples of 8 (the reference
// overruns silently there).  *n_cubes: cubes per channel; px * n_cubes must fit the kernels' 32-bit cube
// indices (the int32 side of a packed RGB24 call holds three cubes per RGB cube).
inline bool make_geom(int w, int h, int px, int n_stacks, bool any_size, Geom* g, uint64_t* n_cubes) {
    if (px != 1 && px != 3) return false;
    if (w <= 0 || h <= 0 || n_stacks < 0 || w > INT32_MAX - 7 || h > INT32_MAX - 7) return false;
    if (!any_size && (w % 8 || h % 8)) return false;
    *g = Geom{w, h, (w + 7) / 8 * 8, (h + 7) / 8 * 8, px};
    const uint64_t n = g->cps() * (uint64_t)n_stacks;
    if ((uint64_t)px * n >= (1ull << 31) / 8) return false;
    *n_cubes = n;
    return true;
}

// The address fields of EncodeParams / DecodeParams for cubes [.., n_cubes) of stacks `depth` frames deep:
// nbx and cubes_per_stack describe the padded raster, width, plane (bytes) and stack_stride the frames in
// memory; height only where the kernels pad or crop (0: the *_stacks* kernels).
template <class Params>
inline void set_address_fields(Params& P, const Geom& g, int depth, uint64_t n_cubes) {
    P.n_cubes = (uint32_t)n_cubes;
    P.cubes_per_stack = (uint32_t)g.cps();
    P.nbx = (uint32_t)(g.wp / 8);
    P.div_cps = fast_div(P.cubes_per_stack);
    P.div_nbx = fast_div(P.nbx);
    P.width = (uint32_t)g.w;
    P.height = g.edge() ? (uint32_t)g.h : 0u;
    P.plane = g.plane();
    P.stack_stride = g.plane() * (uint64_t)depth;
}

// DecodeParams::blk_store (dec_store_tile's 16-byte block stores): rows 16-byte aligned (no crop), nbx even
// (a 16-byte chunk -- two grey cubes, or part of a 48-byte pair of RGB cubes -- never straddles a block-row),
// 32-bit byte offsets within a stack
inline uint32_t blk_store(const Geom& g, int depth) {
    return !g.edge() && (g.wp / 8) % 2 == 0 && g.plane() * (uint64_t)depth < (1ull << 32) ? 1u : 0u;
}

}  // namespace dct3d
