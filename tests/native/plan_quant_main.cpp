// tests/native/plan_quant_main.cpp -- TEST ONLY: a stand-alone program that builds the plan for quantiser tables
// given on the command line, for a host sanitizer build (tests/test_quant_plan.py compiles it with
// dct3d_plan.cpp under -fsanitize=address,undefined).  Arguments: one table per argument, comma-separated steps
// (22 steps: 8x8x8, 18: 8x8x4).  Exit status 0 when every plan builds and its tables are sane.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "dct3d_plan.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        std::vector<int32_t> steps;
        for (const char* p = argv[a]; *p;) {
            char* end;
            steps.push_back((int32_t)strtol(p, &end, 10));
            p = *end == ',' ? end + 1 : end;
        }
        const int cd = (int)steps.size() - 14;
        dct3d::Plan plan;
        if (!dct3d::build_plan(8, 8, cd, steps.data(), plan)) {
            fprintf(stderr, "build_plan failed for table %d\n", a);
            return 1;
        }
        if (plan.steps != steps) return 2;
        for (size_t s = 0; s < steps.size(); s++) {
            if (plan.enc_rstep[s] != (float)(1.0 / steps[s])) return 3;
            if (s && !(plan.enc_G[s] > 0.0f && std::isfinite(plan.enc_E[s]))) return 4;
        }
        if (!(plan.enc_G[0] == 0.0f && plan.enc_E[0] == -INFINITY)) return 5;
        // a table with a step outside [1, 255] is refused and leaves no partial plan behind
        std::vector<int32_t> bad = steps;
        bad.back() = 256;
        dct3d::Plan p2;
        if (dct3d::build_plan(8, 8, cd, bad.data(), p2)) return 6;
        printf("table %d: depth %d ok\n", a, cd);
    }
    return 0;
}
