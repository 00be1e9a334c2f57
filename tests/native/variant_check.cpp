// variant_check.cpp -- the kernels' variant header (csrc/dct3d_variant.h) on the CPU, for tests/test_variant.py:
// the real predicates, unit lists, picks and group pick.
#include "dct3d_variant.h"

using namespace dct3d;

namespace {
// bit i: unit i of the list holds v
template <class... U>
int held_by(Units<U...>, const Variant& v) {
    int i = 0, mask = 0;
    ((mask |= (U::holds(v.D, v.px, v.edge, v.qt, v.colour) ? 1 : 0) << i++), ...);
    return mask;
}
// the place in the list of the unit that route hands to its functor (-1: it called nothing)
template <class... U>
int routed_to(Units<U...>, const Variant& v) {
    int calls = 0;
    const int at = Units<U...>::route(v, [&](auto u) {
        calls++;
        int i = 0, mine = -1;
        ((std::is_same<decltype(u), U>::value ? (mine = i++) : i++), ...);
        return mine;
    });
    return calls == 1 ? at : calls == 0 && at == -1 ? -1 : -2;
}
}  // namespace

extern "C" {

// family 0: raster {kernels, rgb, edge, quant}; 1: stream {kernels, eg_frames, quant_eg, vq, ycc}
int variant_held_by(int family, int D, int px, int edge, int qt, int colour) {
    const Variant v{D, px, edge, qt, colour};
    return family == 0 ? held_by(RasterUnits{}, v) : held_by(StreamUnits{}, v);
}
int variant_index(int family, int D, int px, int edge, int qt, int colour) {
    const Variant v{D, px, edge, qt, colour};
    return family == 0 ? RasterUnits::index(v) : StreamUnits::index(v);
}
int variant_routed_to(int family, int D, int px, int edge, int qt, int colour) {
    const Variant v{D, px, edge, qt, colour};
    return family == 0 ? routed_to(RasterUnits{}, v) : routed_to(StreamUnits{}, v);
}

// with_variant: the functor's calls; out: the constants of its last call; *said: what the helper returned
int variant_pick4(int D, int px, int edge, int qt, int* out, int* said) {
    int calls = 0;
    *said = with_variant(Variant{D, px, edge, qt}, [&](auto d, auto p, auto e, auto q) {
        calls++;
        out[0] = decltype(d)::value;
        out[1] = decltype(p)::value;
        out[2] = decltype(e)::value;
        out[3] = decltype(q)::value;
    });
    return calls;
}
int variant_pick3(int D, int px, int edge, int* out, int* said) {
    int calls = 0;
    *said = with_variant(D, px, edge, [&](auto d, auto p, auto e) {
        calls++;
        out[0] = decltype(d)::value;
        out[1] = decltype(p)::value;
        out[2] = decltype(e)::value;
    });
    return calls;
}
// with_stream_variant, likewise: the table axis to 2 and the colour axis
int variant_pick5(int D, int px, int edge, int qt, int colour, int* out, int* said) {
    int calls = 0;
    *said = with_stream_variant(Variant{D, px, edge, qt, colour}, [&](auto d, auto p, auto e, auto q, auto ct) {
        calls++;
        out[0] = decltype(d)::value;
        out[1] = decltype(p)::value;
        out[2] = decltype(e)::value;
        out[3] = decltype(q)::value;
        out[4] = decltype(ct)::value;
    });
    return calls;
}

// the grey stream decode's groups per wave in stream unit `unit` for the runtime's value; -1: not called once
int variant_groups(int unit, int groups_per_wave) {
    int calls = 0, got = -1;
    const auto f = [&](auto ng) {
        calls++;
        got = decltype(ng)::value;
    };
    if (unit == 0) with_groups<StreamPlain>(groups_per_wave, f);
    else if (unit == 1) with_groups<StreamFrames>(groups_per_wave, f);
    else if (unit == 2) with_groups<StreamQuant>(groups_per_wave, f);
    else if (unit == 3) with_groups<StreamVq>(groups_per_wave, f);
    else with_groups<StreamYcc>(groups_per_wave, f);
    return calls == 1 ? got : -1;
}

}  // extern "C"
