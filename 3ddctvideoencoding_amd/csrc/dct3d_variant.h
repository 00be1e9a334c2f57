// dct3d_variant.h -- a kernel's variant (depth, pixel format, edge, quantiser table, colour transform), the picks
// that turn the runtime's values into template arguments, and which translation unit holds which variant: the one place that
// says so.  A unit instantiates what its predicate admits (dct3d_launch.h) and the router sends a variant to
// the unit whose predicate admits it (dct3d_router.cpp), so the two cannot disagree.
// Plain C++ (no HIP include): the units, the router, the runtime and a CPU test (tests/test_variant.py) share it.
#pragma once
#include <type_traits>

namespace dct3d {

// D: 8 | 4 frames per cube.  px: 1 grey | 3 packed RGB24.  edge: 1 = the width or the height is no multiple of 8
// (padding and crop in the addressing).  qt: 1 = the steps come from the context's table; 2 (the stream family
// only) = a table per stack, in the call's VqParams (dct3d_vq.h).  colour: 1 = the three streams of packed RGB24
// hold the Y, Cb, Cr planes (DCT3D_OPT_COLOUR; px = 3 and the stream family only).
struct Variant {
    int D, px, edge, qt;
    int colour = 0;
};

template <int V>
using Const = std::integral_constant<int, V>;

// The picks: f(Const<value>) for a value of the axis; any other value calls nothing and returns false.
template <class F>
bool with_depth(int D, F&& f) {
    if (D == 8) f(Const<8>{});
    else if (D == 4) f(Const<4>{});
    else return false;
    return true;
}
template <class F>
bool with_px(int px, F&& f) {
    if (px == 1) f(Const<1>{});
    else if (px == 3) f(Const<3>{});
    else return false;
    return true;
}
template <class F>
bool with_flag(int v, F&& f) {
    if (v == 0) f(Const<0>{});
    else if (v == 1) f(Const<1>{});
    else return false;
    return true;
}
// the stream family's table axis
template <class F>
bool with_table(int qt, F&& f) {
    if (qt == 2) f(Const<2>{});
    else return with_flag(qt, f);
    return true;
}
// f(d, p, e) (the probes: every table in one pass) and f(d, p, e, q), q in {0, 1} (the raster ladders: a table
// per stack is outside their axis); true once the innermost pick has called
template <class F>
bool with_variant(int D, int px, int edge, F&& f) {
    bool called = false;
    with_depth(D, [&](auto d) { with_px(px, [&](auto p) { called = with_flag(edge, [&](auto e) { f(d, p, e); }); }); });
    return called;
}
template <class F>
bool with_variant(const Variant& v, F&& f) {
    bool called = false;
    with_variant(v.D, v.px, v.edge, [&](auto d, auto p, auto e) { called = with_flag(v.qt, [&](auto q) { f(d, p, e, q); }); });
    return called;
}
// f(d, p, e, q, ct): the stream ladders' pick, q in {0, 1, 2} and the colour axis as well
template <class F>
bool with_stream_variant(const Variant& v, F&& f) {
    bool called = false;
    with_variant(v.D, v.px, v.edge, [&](auto d, auto p, auto e) {
        with_table(v.qt, [&](auto q) { called = with_flag(v.colour, [&](auto ct) { f(d, p, e, q, ct); }); });
    });
    return called;
}

// ---- which unit holds which variant.  Raster: the int32 encode and decode kernels.  Stream: the fused
//      Exp-Golomb encode and the two stream decodes (grey: px = 1, RGB: px = 3).  A variant with the colour
//      transform belongs to StreamYcc whatever its edge and table, and to no raster unit; one with a table per
//      stack and no transform to StreamVq, and to no raster unit either. ----
struct RasterPlain {  // dct3d_kernels.hip
    static constexpr bool holds(int, int px, int edge, int qt, int colour = 0) { return px == 1 && !edge && !qt && !colour; }
};
struct RasterRgb {  // dct3d_rgb.hip
    static constexpr bool holds(int, int px, int edge, int qt, int colour = 0) { return px == 3 && !edge && !qt && !colour; }
};
struct RasterEdge {  // dct3d_edge.hip
    static constexpr bool holds(int, int, int edge, int qt, int colour = 0) { return edge && !qt && !colour; }
};
struct RasterQuant {  // dct3d_quant.hip
    static constexpr bool holds(int, int, int, int qt, int colour = 0) { return qt == 1 && !colour; }
};
// all_groups: the grey stream decode at 1 | 2 | 4 | 8 groups of cubes per wave (else: 8 alone, the default)
struct StreamPlain {  // dct3d_kernels.hip
    static constexpr bool all_groups = true;
    static constexpr bool holds(int, int px, int edge, int qt, int colour = 0) { return px == 1 && !edge && !qt && !colour; }
};
struct StreamFrames {  // dct3d_eg_frames.hip
    static constexpr bool all_groups = false;
    static constexpr bool holds(int D, int px, int edge, int qt, int colour = 0) {
        return !qt && !colour && !StreamPlain::holds(D, px, edge, qt);
    }
};
struct StreamQuant {  // dct3d_quant_eg.hip
    static constexpr bool all_groups = false;
    static constexpr bool holds(int, int, int, int qt, int colour = 0) { return qt == 1 && !colour; }
};
struct StreamVq {  // dct3d_vq_enc.hip (the encode ladder), dct3d_vq_dec.hip (the two decode ladders)
    static constexpr bool all_groups = false;
    static constexpr bool holds(int, int, int, int qt, int colour = 0) { return qt == 2 && !colour; }
};
struct StreamYcc {  // dct3d_ycc.hip
    static constexpr bool all_groups = false;
    static constexpr bool holds(int, int px, int, int, int colour = 0) { return px == 3 && colour == 1; }
};

// f(Const<groups>): the grey stream decode's groups per wave in unit U (a count U does not build: 8)
template <class U, class F>
void with_groups(int groups_per_wave, F&& f) {
    if constexpr (U::all_groups) {
        switch (groups_per_wave) {
            case 1: return f(Const<1>{});
            case 2: return f(Const<2>{});
            case 4: return f(Const<4>{});
        }
    }
    f(Const<8>{});
}

// A family's units.  index: the unit that holds v (-1: none); route: f(U{}) for that unit, or -1.
template <class... U>
struct Units {
    static constexpr int count(const Variant& v) { return (int(U::holds(v.D, v.px, v.edge, v.qt, v.colour)) + ...); }
    static constexpr int index(const Variant& v) {
        int i = 0, at = -1;
        ((U::holds(v.D, v.px, v.edge, v.qt, v.colour) ? (at = i++) : i++), ...);
        return at;
    }
    template <class F>
    static int route(const Variant& v, F&& f) {
        int rc = -1;
        (void)((U::holds(v.D, v.px, v.edge, v.qt, v.colour) && (rc = f(U{}), true)) || ...);
        return rc;
    }
    // every variant in exactly one unit; a table per stack (qt = 2) and the colour transform: in a family that
    // has them (stream), the transform on packed RGB24 alone; in one that has not, in no unit
    static constexpr bool partition(bool stream) {
        for (int i = 0; i < 16; i++)
            for (int qt = 0; qt < 3; qt++) {
                const Variant v{i & 8 ? 8 : 4, i & 4 ? 3 : 1, (i >> 1) & 1, qt, i & 1};
                if (count(v) != int(stream ? !v.colour || v.px == 3 : qt < 2 && !v.colour)) return false;
            }
        return true;
    }
};
using RasterUnits = Units<RasterPlain, RasterRgb, RasterEdge, RasterQuant>;
using StreamUnits = Units<StreamPlain, StreamFrames, StreamQuant, StreamVq, StreamYcc>;
static_assert(RasterUnits::partition(false) && StreamUnits::partition(true), "each variant belongs to one unit of its family");

}  // namespace dct3d
