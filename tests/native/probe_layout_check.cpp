// probe_layout_check.cpp -- the probes' layout header (csrc/dct3d_probe_layout.h) on the CPU, for
// tests/test_probe_layout.py: a stand-alone program (built with the address and undefined-behaviour sanitizers) that
// reads one query per line from its standard input and prints the header's answer, numbers separated by blanks.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "dct3d_probe_layout.h"

using namespace dct3d;

static void put(const Section& s) { printf("%zu %zu ", s.off, s.n); }
static void put(const Place& p) { printf("%zu %zu %zu ", p.off, p.step_t, p.step_s); }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        std::vector<long long> a;
        in >> cmd;
        for (long long v; in >> v;) a.push_back(v);
        if (cmd == "geom" && a.size() == 3) {  // w h D
            const SsimGeom s = ssim_geom((int)a[0], (int)a[1], (int)a[2], 1024, 1024);
            printf("%u %u %u %u %u %llu %llu %d", s.nbx, s.nby, s.nwx, s.nwy, s.bpr, (unsigned long long)s.blk_per_stack,
                   (unsigned long long)s.win_per_stack, s.fits() ? 1 : 0);
        } else if (cmd == "range" && a.size() == 4) {  // budget per_stack n_stacks cap (0: none)
            printf("%d", a[3] ? stacks_per_range(a[0], a[1], (int)a[2], a[3]) : stacks_per_range(a[0], a[1], (int)a[2]));
        } else if (cmd == "ssimrange" && a.size() == 7) {  // budget w h D n planes n_stacks
            const SsimGeom s = ssim_geom((int)a[1], (int)a[2], (int)a[3], 1024, 1024);
            printf("%llu %d", (unsigned long long)s.record_bytes((int)a[4], (int)a[5]), ssim_range_stacks(a[0], s, (int)a[4], (int)a[5], (int)a[6]));
        } else if (cmd == "compact" && a.size() >= 4 && a.size() == 4 + (size_t)(a[3] * a[0])) {  // stride n_tables all n_idx idx..
            std::vector<uint8_t> idx(a.begin() + 4, a.end());
            const TableSlots t = compact_tables(idx.data(), (int)a[3], (int)a[0], (int)a[1], a[2] != 0);
            printf("%d ", t.n);
            for (int i = 0; i < t.n; i++) printf("%d ", t.used[i]);
            for (int i = 0; i < (int)a[1]; i++) printf("%d ", t.slot[i]);
        } else if (cmd == "sums" && a.size() == 4) {  // n_runs ssim sse bits
            const ProbeSums L = probe_sums((size_t)a[0], a[1] != 0, a[2] != 0, a[3] != 0);
            put(L.ssim), put(L.sse), put(L.bits), printf("%zu", L.total);
        } else if (cmd == "c420" && a.size() == 1) {  // ts: the sections, the total, then the source of every (run, channel)
            const C420Sums L = c420_sums((size_t)a[0]);
            put(L.plane[0]), put(L.plane[1]), put(L.plane[2]), printf("%zu ", L.total);
            for (size_t i = 0; i < (size_t)a[0]; i++)
                for (int ch = 0; ch < 3; ch++) printf("%zu ", c420_src(L, i, ch));
        } else if (cmd == "rgb" && a.size() == 8) {  // nk0 nk1 nk2 n_stacks n_cand bits n_sp per
            const int nk[3] = {(int)a[0], (int)a[1], (int)a[2]}, n_stacks = (int)a[3], per = (int)a[7];
            const RgbSums L = rgb_sums(nk, n_stacks, (int)a[4], a[5] != 0, (int)a[6]);
            put(L.plane_sse), put(L.plane_bits), put(L.rgb_sse), put(L.ssim), put(L.ssim_y);
            printf("%zu %zu %zu %zu %zu ", L.total, L.nt, L.toff[0], L.toff[1], L.toff[2]);
            // every plane sum in the order (plane, slot, stack): where it lies in a plane section
            for (int k = 0; k < 3; k++)
                for (int t = 0; t < nk[k]; t++)
                    for (int s = 0; s < n_stacks; s++) {
                        const int s0 = s / per * per, ns = n_stacks - s0 < per ? n_stacks - s0 : per;
                        printf("%zu ", rgb_plane_src(L, s0, ns, k, t, s - s0));
                    }
        } else if (cmd == "place" && a.size() == 6) {  // planar? n_stacks channels s0 ch unit
            put(a[0] ? planar((size_t)a[1], (size_t)a[2], (size_t)a[3], (size_t)a[4], (size_t)a[5])
                     : interleaved((size_t)a[1], (size_t)a[2], (size_t)a[3], (size_t)a[4], (size_t)a[5]));
        } else if (cmd == "chunk" && a.size() == 5) {  // o n_stacks s0 ns inner
            printf("%zu %zu %zu", chunk_src((size_t)a[0], (size_t)a[3], (size_t)a[4]), chunk_dst((size_t)a[0], (size_t)a[1], (size_t)a[2], (size_t)a[4]),
                   triple_at((size_t)a[1], (size_t)a[0], (size_t)a[2], 2));
        } else {
            fprintf(stderr, "bad query: %s\n", line.c_str());
            return 2;
        }
        printf("\n");
    }
    return 0;
}
