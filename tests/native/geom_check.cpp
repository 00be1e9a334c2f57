// geom_check.cpp -- the runtime's geometry header (csrc/dct3d_geom.h) on the CPU, for tests/test_geom.py and
// tests/test_fastdiv.py: the real make_geom / set_address_fields / blk_store / fast_div on a struct with the
// kernel parameter blocks' member names.
#include "dct3d_geom.h"

using namespace dct3d;

namespace {
struct Params {  // the address fields of EncodeParams / DecodeParams (dct3d_kernels.h)
    uint32_t n_cubes, cubes_per_stack, nbx, width, height;
    FastDiv div_cps, div_nbx;
    uint64_t plane, stack_stride;
};
}  // namespace

extern "C" {

// 0: the geometry is rejected.  1: out = {n_cubes of the call, wp, hp, edge, cps, plane, then the fields for
// stacks `depth` deep: n_cubes, cubes_per_stack, nbx, width, height, plane, stack_stride, div_cps.m, div_cps.s,
// div_nbx.m, div_nbx.s, blk_store}
int geom_fields(int w, int h, int px, int n_stacks, int any_size, int depth, uint64_t* out) {
    Geom g;
    uint64_t n_cubes;
    if (!make_geom(w, h, px, n_stacks, any_size != 0, &g, &n_cubes)) return 0;
    Params P;
    set_address_fields(P, g, depth, n_cubes);
    const uint64_t v[18] = {n_cubes, (uint64_t)g.wp, (uint64_t)g.hp, g.edge() ? 1u : 0u, g.cps(), g.plane(),
                            P.n_cubes, P.cubes_per_stack, P.nbx, P.width, P.height, P.plane, P.stack_stride,
                            P.div_cps.m, P.div_cps.s, P.div_nbx.m, P.div_nbx.s, blk_store(g, depth)};
    for (int i = 0; i < 18; i++) out[i] = v[i];
    return 1;
}

void fast_div_table(const uint32_t* d, int n, uint32_t* m, uint32_t* s) {
    for (int i = 0; i < n; i++) {
        const FastDiv f = fast_div(d[i]);
        m[i] = f.m;
        s[i] = f.s;
    }
}

}  // extern "C"
