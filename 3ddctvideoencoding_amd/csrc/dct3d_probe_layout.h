// dct3d_probe_layout.h -- the probes' host arithmetic (dct3d_probes.cpp): the SSIM geometry of a frame
// size, the stacks a range or a staging chunk takes, the tables a call codes and their slots, and where each
// section of the sums block lies.  Plain integers and no HIP: tests/native/probe_layout_check.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace dct3d {

constexpr int kProbeMaxTables = 32;  // == DCT3D_RATE_MAX_TABLES (tables and candidates of one call)

// The 4 x 4 blocks and the 8 x 8 / stride 4 windows of a w x h plane (dct3d.h), per stack of D frames; bpr: the
// window kernel's blocks per (table, stack) at win_per_block windows each, max_bpr at most.
struct SsimGeom {
    uint32_t nbx, nby, nwx, nwy, bpr;
    uint64_t blk_per_stack, win_per_stack;
    bool fits() const { return win_per_stack < (1ull << 32); }  // (32-bit window indices in the kernels)
    // bytes of one stack's block records: per plane 8 per table (or candidate) and 4 for the source
    uint64_t record_bytes(int n, int planes = 1) const { return blk_per_stack * (8ull * n + 4) * planes; }
};
inline SsimGeom ssim_geom(int w, int h, int D, uint32_t win_per_block, uint32_t max_bpr) {
    SsimGeom s;
    s.nbx = ((uint32_t)w + 3) / 4;
    s.nby = ((uint32_t)h + 3) / 4;
    s.nwx = s.nbx > 1 ? s.nbx - 1 : 1;
    s.nwy = s.nby > 1 ? s.nby - 1 : 1;
    s.blk_per_stack = (uint64_t)D * s.nbx * s.nby;
    s.win_per_stack = (uint64_t)D * s.nwx * s.nwy;
    s.bpr = (uint32_t)std::min<uint64_t>((s.win_per_stack + win_per_block - 1) / win_per_block, max_bpr);
    return s;
}

// The stacks one range takes: as many as fit `budget` bytes at per_stack bytes each, at least 1, n_stacks and cap
// at most (per_stack == 0: 1).
inline int stacks_per_range(uint64_t budget, uint64_t per_stack, int n_stacks, uint64_t cap = UINT64_MAX) {
    if (!per_stack) return 1;
    return (int)std::max<uint64_t>(1, std::min({budget / per_stack, (uint64_t)std::max(n_stacks, 1), cap}));
}
// under the SSIM record budget (the window kernels' grid: 65,535 stacks at most)
inline int ssim_range_stacks(uint64_t budget, const SsimGeom& s, int n, int planes, int n_stacks) {
    return stacks_per_range(budget, s.record_bytes(n, planes), n_stacks, 65535);
}

// The tables a call codes and where a candidate finds them: the tables idx[0], idx[stride], .. (n_idx of them) name,
// in first-use order -- or all n_tables in order.  slot[t]: table t's place among `used`, or -1.
struct TableSlots {
    int n = 0;
    int used[kProbeMaxTables], slot[kProbeMaxTables];
};
inline TableSlots compact_tables(const uint8_t* idx, int n_idx, int stride, int n_tables, bool all) {
    TableSlots c;
    for (int t = 0; t < kProbeMaxTables; t++) c.used[t] = c.slot[t] = -1;
    for (int i = 0; i < (all ? n_tables : n_idx); i++) {
        const int t = all ? i : idx[(size_t)i * stride];
        if (c.slot[t] < 0) {
            c.slot[t] = c.n;
            c.used[c.n++] = t;
        }
    }
    return c;
}

// ---- the sums block (d_rate_sums, and its pinned copy): 8-byte words; a section with n == 0 is not in the call ----
struct Section { size_t off, n; };
struct SectionCursor {
    size_t at = 0;
    Section take(bool on, size_t n) {
        const Section s = {at, on ? n : 0};
        at += s.n;
        return s;
    }
};
// rate, distortion and SSIM probe: [ssim][sse][bits], each [table][stack][channel] (n_runs words)
struct ProbeSums { Section ssim, sse, bits; size_t total; };
inline ProbeSums probe_sums(size_t n_runs, bool ssim, bool sse, bool bits) {
    SectionCursor c;
    return {c.take(ssim, n_runs), c.take(sse, n_runs), c.take(bits, n_runs), c.at};  // (a braced list: left to right)
}
// a result [table][stack][3]: (t, s, k)
inline size_t triple_at(size_t n_stacks, size_t t, size_t s, size_t k) { return (t * n_stacks + s) * 3 + k; }

// The rate probe under 4:2:0: the Y launch's [table][stack][3] block (channel 0 filled), then Cb's and Cr's
// [table][stack]; c420_src: where run i = t * n_stacks + s of channel ch lies (it goes to 3 i + ch).
struct C420Sums { Section plane[3]; size_t total; };
inline C420Sums c420_sums(size_t ts) {
    SectionCursor c;
    return {{c.take(true, 3 * ts), c.take(true, ts), c.take(true, ts)}, c.at};
}
inline size_t c420_src(const C420Sums& L, size_t i, int ch) { return ch ? L.plane[ch].off + i : 3 * i; }

// The RGB-domain probes (YCbCr modes): [plane sse][plane bits][rgb sse][ssim rgb][ssim y].  The plane sections are
// ragged: per range of stacks [s0, s0 + ns), per plane k, [slot of the plane's nk[k] tables][stack of the range].
// n_sp: the SSIM records' planes (0 none, 3 R G B, 4 and the luma).
struct RgbSums {
    Section plane_sse, plane_bits, rgb_sse, ssim, ssim_y;
    size_t total, nt, toff[3];  // the planes' tables together, plane k's first
};
inline RgbSums rgb_sums(const int nk[3], int n_stacks, int n_cand, bool bits, int n_sp) {
    SectionCursor c;
    const size_t nt = (size_t)nk[0] + nk[1] + nk[2], n_rgb = (size_t)n_cand * n_stacks;
    return {c.take(true, nt * n_stacks), c.take(bits, nt * n_stacks), c.take(true, n_rgb), c.take(n_sp >= 3, 3 * n_rgb),
            c.take(n_sp == 4, n_rgb), c.at, nt, {0, (size_t)nk[0], (size_t)nk[0] + nk[1]}};
}
// within a plane section: plane k's sums of the range, and (slot, stack s of the range) among them
inline size_t rgb_range_off(const RgbSums& L, int s0, int ns, int k) { return (size_t)s0 * L.nt + L.toff[k] * ns; }
inline size_t rgb_plane_src(const RgbSums& L, int s0, int ns, int k, int slot, int s) {
    return rgb_range_off(L, s0, ns, k) + (size_t)slot * ns + s;
}

// Where a range's launch puts element (table t, stack s of the range): off + t * step_t + s * step_s, in units
struct Place { size_t off, step_t, step_s; };
// [table][stack][channel][unit] (the sums and the windows of the SSIM probe; the RGB probe's sums with 3 planes)
inline Place interleaved(size_t n_stacks, size_t channels, size_t s0, size_t ch, size_t unit = 1) {
    return {(s0 * channels + ch) * unit, n_stacks * channels * unit, channels * unit};
}
// [candidate][plane][stack][unit] (the RGB probe's windows)
inline Place planar(size_t n_stacks, size_t planes, size_t s0, size_t k, size_t unit) {
    return {(k * n_stacks + s0) * unit, planes * n_stacks * unit, unit};
}

// A host-pointer call's chunk [s0, s0 + ns) of n_stacks: its block [outer][ns][inner] goes into [outer][n_stacks][inner]
inline size_t chunk_src(size_t o, size_t ns, size_t inner) { return o * ns * inner; }
inline size_t chunk_dst(size_t o, size_t n_stacks, size_t s0, size_t inner) { return (o * n_stacks + s0) * inner; }

}  // namespace dct3d
