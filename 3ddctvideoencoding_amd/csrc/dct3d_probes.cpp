// dct3d_probes.cpp -- the probes' host side (include/dct3d.h: dct3d_rate_frames*, dct3d_distortion_frames*,
// dct3d_ssim_frames*, dct3d_distortion_rgb_frames*, dct3d_ssim_rgb_frames*).  One call
// frame (Frame), one table-batch iterator, one window step and one host-pointer chunk walk serve all of them; the
// sizes, slots and offsets come from dct3d_probe_layout.h.
#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "dct3d_c420.h"
#include "dct3d_ctx.h"
#include "dct3d_distortion_rgb.h"
#include "dct3d_probe_layout.h"

using namespace dct3d;
using namespace dct3d::rt;

// Each table's {1 / step, G, 0.5 - E, step} rows from the context's one plan (encoder_tables: the rows
// dct3d_plan_query_quant reports for that table), as the encode kernels' LDS copy holds them (enc_tables); with
// want_steps its steps in fp64 too (as the decode kernels' table)
void rt::probe_tables(dct3d_ctx* c, const int32_t* tables, int n_tables, bool want_steps) {
    static_assert(kRateTabN <= kMaxS && kDistStepN == kMaxS, "a table's rows and steps");
    const int n_steps = (int)c->plan.steps.size();
    c->rate_tabs_host.resize((size_t)n_tables * kRateTabN * 4);
    c->dist_steps_host.resize(want_steps ? (size_t)n_tables * kDistStepN : 0);
    for (int t = 0; t < n_tables; t++) {
        int32_t st[kMaxS];
        float rstep[kMaxS], G[kMaxS], E[kMaxS];
        for (int s = 0; s < kMaxS; s++) {
            st[s] = s < n_steps ? (tables ? tables[(size_t)t * n_steps + s] : c->plan.steps[s]) : reference_step(s);
            if (want_steps) c->dist_steps_host[(size_t)t * kDistStepN + s] = (double)st[s];
        }
        encoder_tables(c->plan, st, rstep, G, E);
        float* row = c->rate_tabs_host.data() + (size_t)t * kRateTabN * 4;
        for (int s = 0; s < kRateTabN; s++, row += 4) {
            row[0] = rstep[s];
            row[1] = G[s];
            row[2] = 0.5f - E[s];
            row[3] = (float)st[s];
        }
    }
}

namespace {

static_assert(kProbeMaxTables == DCT3D_RATE_MAX_TABLES, "the layout header's table limit");
constexpr size_t kSsimBlockBudget = DCT3D_SSIM_BLOCK_BUDGET, kRgbPlaneBudget = DCT3D_RGB_PLANE_BUDGET;
constexpr size_t kChunkBytes = (size_t)64 << 20;  // the host-pointer calls' staging buffer (as the pipeline's chunks)

// the arguments of every probe call (nothing is enqueued before they hold); result: the output the call must give
bool rate_args_ok(const dct3d_ctx* c, const uint8_t* frames, int w, int h, int channels, int n_stacks, const int32_t* tables,
                  int n_tables, const void* result, Geom* g) {
    uint64_t n_cubes;
    if (!c || !make_geom(w, h, channels, n_stacks, true, g, &n_cubes)) return false;
    if (n_tables < 1 || n_tables > DCT3D_RATE_MAX_TABLES || (!tables && n_tables != 1) || !result) return false;
    if (!frames && n_stacks) return false;
    const int n_steps = (int)c->plan.steps.size();
    if (tables)
        for (int i = 0; i < n_tables * n_steps; i++)
            if (tables[i] < kMinStep || tables[i] > kMaxStep) return false;
    return true;
}
// the pinned buffer the probes' sums come back in
int probe_grow_pinned(dct3d_ctx* c, size_t bytes) {
    if (c->h_rate_bytes >= bytes) return DCT3D_OK;
    if (c->h_rate) (void)hipHostFree(c->h_rate);
    c->h_rate_bytes = 0;
    if (hipHostMalloc((void**)&c->h_rate, bytes, hipHostMallocDefault) != hipSuccess) {
        c->h_rate = nullptr;
        return DCT3D_ENOMEM;
    }
    c->h_rate_bytes = bytes;
    return DCT3D_OK;
}

// ---- the call frame of the device bodies: enter, (an empty call returns), begin, the body's launches, end ----
struct Grow {
    DevBuf* buf;
    size_t bytes;     // 0: the call does not use it
    size_t zero = 0;  // its first bytes are cleared behind the uploads
};
struct Frame {
    dct3d_ctx* c;
    size_t sum_bytes = 0;
    hipEvent_t* ev = nullptr;
    int enter() {
        if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
        call_begin(c);
        if (!c->batch) c->last_units = 0;
        return DCT3D_OK;
    }
    // the tables' rows (and steps) and the candidates' slots built and uploaded, the sums block of sum_words words, its
    // pinned copy and the body's buffers grown; the timed region opens
    int begin(const int32_t* tables, int n_tables, bool steps, size_t sum_words, std::initializer_list<Grow> bufs,
              const uint8_t* slots = nullptr, size_t n_slots = 0) {
        probe_tables(c, tables, n_tables, steps);
        sum_bytes = sum_words * sizeof(uint64_t);
        const size_t tab_bytes = c->rate_tabs_host.size() * sizeof(float), step_bytes = c->dist_steps_host.size() * sizeof(double);
        int rc;
        if ((rc = c->d_rate_tabs.grow(tab_bytes)) || (rc = c->d_dist_steps.grow(step_bytes)) || (rc = c->d_rate_sums.grow(sum_bytes)) ||
            (rc = c->d_rgb_slots.grow(n_slots)) || (rc = probe_grow_pinned(c, sum_bytes)))
            return rc;
        for (const Grow& b : bufs)
            if ((rc = b.buf->grow(b.bytes))) return rc;
        const hipStream_t st = c->stream;
        if (hipMemcpyAsync(c->d_rate_tabs.p, c->rate_tabs_host.data(), tab_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
            (step_bytes && hipMemcpyAsync(c->d_dist_steps.p, c->dist_steps_host.data(), step_bytes, hipMemcpyHostToDevice, st) != hipSuccess) ||
            (n_slots && hipMemcpyAsync(c->d_rgb_slots.p, slots, n_slots, hipMemcpyHostToDevice, st) != hipSuccess))
            return DCT3D_EDEVICE;
        for (const Grow& b : bufs)
            if (b.zero && hipMemsetAsync(b.buf->p, 0, b.zero, st) != hipSuccess) return DCT3D_EDEVICE;
        ev = timer_begin(c);
        return DCT3D_OK;
    }
    // the timed region closes, the sums come back in one copy; synchronous on return (the sums are a host result; the
    // tables' host copies and the buffers are free again).  units: the call's work for the statistics
    int end(int rc, uint64_t units) {
        timer_end(c, ev);
        if (!rc && hipMemcpyAsync(c->h_rate, c->d_rate_sums.p, sum_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = DCT3D_EDEVICE;
        if (stream_wait(c) && !rc) rc = DCT3D_EDEVICE;
        if (c->slot_used) count_slot_used(c, units * (uint64_t)c->plan.cs);
        return rc;
    }
    uint64_t* sums(const Section& s) const { return (uint64_t*)c->d_rate_sums.p + s.off; }
    void read_back(const Section& s, void* out) const {
        if (out && s.n) memcpy(out, c->h_rate + s.off, s.n * sizeof(uint64_t));
    }
};

// The one loop over a call's tables, kRateTables per launch: R's tables of the batch at t0 (the rows and steps of
// table first + t0 on), then launch(t0)
template <class Launch>
int each_batch(dct3d_ctx* c, DistParams& R, size_t first, int n_tables, Launch&& launch) {
    int rc = DCT3D_OK;
    for (int t0 = 0; t0 < n_tables && !rc; t0 += kRateTables) {
        R.n_tables = std::min(kRateTables, n_tables - t0);
        R.tabs = (const float4*)c->d_rate_tabs.p + (first + t0) * kRateTabN;
        R.steps = c->dist_steps_host.empty() ? nullptr : (const double*)c->d_dist_steps.p + (first + t0) * kDistStepN;
        rc = launch(t0);
    }
    return rc;
}
// a launch of a kernel that counts into the call's slot
int counted(dct3d_ctx* c, int failed) {
    if (failed) return DCT3D_EKERNEL;
    c->slot_used = true;
    return DCT3D_OK;
}
// the decode's certificate constants and the replay's table, the test margin included
void set_decode_constants(dct3d_ctx* c, DistParams& R, const Geom& g) {
    DecodeParams DP;
    fill_decode_params(c, DP, nullptr, nullptr, g, 0);
    R.inv_coef_t = DP.inv_coef_t;
    R.dec_G = DP.dec_G;
    R.dec_E = DP.dec_E;
    R.dec_l1_max = DP.dec_l1_max;
}
// The windows of one plane of ns stacks under n tables (or candidates) from its block records, and their sums per
// (table, stack): the windows at win + wp (win nullptr: not kept), the sums at sums + sp
int ssim_windows(dct3d_ctx* c, const Geom& g, const SsimGeom& sg, const uint64_t* blk_y, const uint32_t* blk_x, uint64_t blk_stride,
                 int ns, int n, int32_t* win, const Place& wp, uint64_t* sums, const Place& sp) {
    const SsimWinParams W = {blk_y, blk_x, blk_stride, win ? win + wp.off : nullptr, wp.step_t, wp.step_s, (int64_t*)c->d_ssim_part.p,
                             (uint32_t)g.w, (uint32_t)g.h, sg.nbx, sg.nby, sg.nwx, sg.nwy, (uint32_t)c->bd,  // w h nbx nby nwx nwy depth
                             (uint32_t)ns, (uint32_t)n, sg.bpr};                                            // ns n_tables bpr
    return launch_ssim_window(W, c->stream) || launch_ssim_sum(W.part, W.bpr, W.ns, W.n_tables, (int64_t*)sums + sp.off, sp.step_t, sp.step_s, c->stream)
               ? DCT3D_EKERNEL
               : DCT3D_OK;
}

// The rate probe under 4:2:0 on frames in device memory: channel 0 as the colour transform's launch at
// the frames' geometry, channels 1 and 2 as the chroma launches over the subsampled planes' cubes (gc), each plane's
// cube bits in a block of its own ([table][stack][cube]: the layout is ragged, no caller's buffer is offered; the Y
// launch fills channel 0's third of its [stack][channel][cube] block, cleared first, and the sums of the rest are
// dropped).  bits: [n_tables][n_stacks][3].
int probe_c420_dev(dct3d_ctx* c, const uint8_t* d_frames, const Geom& g, int n_stacks, const int32_t* tables, int n_tables, uint64_t* bits) {
    Geom gc;
    uint64_t nc;
    if (!c420_geom(g, n_stacks, &gc, &nc)) return DCT3D_EINVAL;
    const uint64_t ny = g.cps() * (uint64_t)n_stacks, ts = (uint64_t)n_tables * n_stacks;
    Frame F{c};
    int rc;
    if ((rc = F.enter()) || ny == 0) return rc;
    const C420Sums L = c420_sums(ts);
    const size_t y_cubes = (size_t)n_tables * 3 * ny, c_cubes = (size_t)n_tables * nc;
    if ((rc = F.begin(tables, n_tables, false, L.total, {{&c->d_rate_bits, (y_cubes + 2 * c_cubes) * sizeof(uint16_t), y_cubes * sizeof(uint16_t)}})))
        return rc;
    uint16_t* const cb[3] = {(uint16_t*)c->d_rate_bits.p, (uint16_t*)c->d_rate_bits.p + y_cubes, (uint16_t*)c->d_rate_bits.p + y_cubes + c_cubes};
    EncodeParams P, Pc;
    fill_encode_params(c, P, d_frames, nullptr, g, ny);
    fill_encode_params(c, Pc, d_frames, nullptr, g, nc);
    c420_cube_fields(Pc, g, gc);
    const Variant v = stream_variant_of(c, g);
    DistParams R = {};
    rc = each_batch(c, R, 0, n_tables, [&](int t0) {
        int r = DCT3D_OK;
        for (int ch = 0; ch < 3 && !r; ch++) {
            R.ch = ch;
            R.table_stride = ch ? nc : 3 * ny;
            R.cube_bits = cb[ch] + (size_t)t0 * R.table_stride;
            r = counted(c, ch ? launch_rate_c420(v.D, c420_edge(g), Pc, R, c->stream) : launch_rate_ycc(v.D, v.edge, P, R, c->stream));
        }
        return r;
    });
    for (int k = 0; k < 3 && !rc; k++)
        if (launch_rate_sum(cb[k], (uint32_t)(k ? gc.cps() : g.cps()), L.plane[k].n, F.sums(L.plane[k]), c->stream)) rc = DCT3D_EKERNEL;
    if ((rc = F.end(rc, (uint64_t)n_tables * (ny + 2 * nc)))) return rc;
    for (uint64_t i = 0; i < ts; i++)
        for (int ch = 0; ch < 3; ch++) bits[3 * i + ch] = c->h_rate[c420_src(L, i, ch)];
    return DCT3D_OK;
}

// Both probes on frames in device memory (the arguments hold: rate_args_ok).  sse: the distortion probe (bits
// optional; d_cube_sse the caller's per-cube buffer or nullptr); no sse: the rate probe (d_cube_bits likewise).
int probe_dev(dct3d_ctx* c, const uint8_t* d_frames, const Geom& g, int n_stacks, const int32_t* tables, int n_tables, uint64_t* sse,
              uint64_t* bits, uint32_t* d_cube_sse, uint16_t* d_cube_bits) {
    const bool dist = sse != nullptr;
    if (!dist && c420_on(c, g.px)) return probe_c420_dev(c, d_frames, g, n_stacks, tables, n_tables, bits);
    const int channels = g.px;
    const uint64_t n_cubes = g.cps() * (uint64_t)n_stacks, stride = (uint64_t)channels * n_cubes;  // per channel, of one table
    Frame F{c};
    int rc;
    if ((rc = F.enter()) || n_cubes == 0) return rc;
    const ProbeSums L = probe_sums((size_t)n_tables * n_stacks * channels, false, dist, bits != nullptr);
    if ((rc = F.begin(tables, n_tables, dist, L.total,
                      {{&c->d_dist_sse, dist && !d_cube_sse ? (size_t)n_tables * stride * sizeof(uint32_t) : 0},
                       {&c->d_rate_bits, bits && !d_cube_bits ? (size_t)n_tables * stride * sizeof(uint16_t) : 0}})))
        return rc;
    uint32_t* const cube_sse = d_cube_sse ? d_cube_sse : (uint32_t*)c->d_dist_sse.p;
    uint16_t* const cube_bits = d_cube_bits ? d_cube_bits : bits ? (uint16_t*)c->d_rate_bits.p : nullptr;
    EncodeParams P;
    fill_encode_params(c, P, d_frames, nullptr, g, n_cubes);
    DistParams R = {};
    R.table_stride = stride;
    if (dist) set_decode_constants(c, R, g);
    const Variant v = stream_variant_of(c, g);  // (the probes read tables of their own: no qt; colour: the rate probe)
    // one launch per batch and channel (as the stream encode's chains)
    rc = each_batch(c, R, 0, n_tables, [&](int t0) {
        R.cube_bits = cube_bits ? cube_bits + (size_t)t0 * stride : nullptr;
        R.cube_sse = dist ? cube_sse + (size_t)t0 * stride : nullptr;
        int r = DCT3D_OK;
        for (R.ch = 0; R.ch < channels && !r; R.ch++)
            r = counted(c, dist       ? launch_distortion(v.D, v.px, v.edge, P, R, c->stream)
                           : v.colour ? launch_rate_ycc(v.D, v.edge, P, R, c->stream)
                                      : launch_rate(v.D, v.px, v.edge, P, R, c->stream));
        return r;
    });
    if (!rc && dist && launch_distortion_sum(cube_sse, (uint32_t)g.cps(), L.sse.n, F.sums(L.sse), c->stream)) rc = DCT3D_EKERNEL;
    if (!rc && bits && launch_rate_sum(cube_bits, (uint32_t)g.cps(), L.bits.n, F.sums(L.bits), c->stream)) rc = DCT3D_EKERNEL;
    if ((rc = F.end(rc, (uint64_t)n_tables * stride))) return rc;
    F.read_back(L.sse, sse);
    F.read_back(L.bits, bits);
    return DCT3D_OK;
}

// The SSIM probe on frames in device memory (the arguments hold: rate_args_ok).  The distortion probe's
// launches with the block-moment arm, over ranges of stacks whose block records fit kSsimBlockBudget (or one stack
// at a time); per range and channel the records (every launch writes the source's: the same), then the windows of
// all tables and their sums.  sse and bits (optional) as probe_dev leaves them.
int ssim_dev(dct3d_ctx* c, const uint8_t* d_frames, const Geom& g, int n_stacks, const int32_t* tables, int n_tables, int64_t* ssim,
             uint64_t* sse, uint64_t* bits, int32_t* d_win) {
    const int channels = g.px, D = c->bd;
    const uint64_t cps = g.cps(), stride = (uint64_t)channels * cps * n_stacks;  // cubes of one table
    Frame F{c};
    int rc;
    if ((rc = F.enter()) || stride == 0) return rc;
    const SsimGeom sg = ssim_geom(g.w, g.h, D, kSsimWinPerBlock, kSsimMaxBpr);
    if (!sg.fits()) return DCT3D_EINVAL;
    const int rs = ssim_range_stacks(kSsimBlockBudget, sg, n_tables, 1, n_stacks);
    const uint64_t blk_stride = sg.blk_per_stack * rs;
    const ProbeSums L = probe_sums((size_t)n_tables * n_stacks * channels, true, sse != nullptr, bits != nullptr);
    if ((rc = F.begin(tables, n_tables, true, L.total,
                      {{&c->d_dist_sse, sse ? (size_t)n_tables * stride * sizeof(uint32_t) : 0},
                       {&c->d_rate_bits, bits ? (size_t)n_tables * stride * sizeof(uint16_t) : 0},
                       {&c->d_ssim_blk, (size_t)sg.record_bytes(n_tables) * rs},
                       {&c->d_ssim_part, (size_t)n_tables * rs * sg.bpr * sizeof(int64_t)}})))
        return rc;
    uint32_t* const cube_sse = sse ? (uint32_t*)c->d_dist_sse.p : nullptr;
    uint16_t* const cube_bits = bits ? (uint16_t*)c->d_rate_bits.p : nullptr;
    uint64_t* const blk_y = (uint64_t*)c->d_ssim_blk.p;
    const Variant v = stream_variant_of(c, g);
    SsimParams R = {};
    R.table_stride = stride;
    set_decode_constants(c, R, g);
    R.blk_x = (uint32_t*)(blk_y + (size_t)n_tables * blk_stride);
    R.blk_stride = blk_stride;
    R.nbx = sg.nbx;
    R.nby = sg.nby;
    for (int s0 = 0; s0 < n_stacks && !rc; s0 += rs) {
        const int ns = std::min(rs, n_stacks - s0);
        EncodeParams P;
        fill_encode_params(c, P, d_frames + (size_t)s0 * g.plane() * D, nullptr, g, cps * ns);
        const size_t cube_off = (size_t)s0 * channels * cps;  // the range's first cube in a table's block
        for (int ch = 0; ch < channels && !rc; ch++) {
            R.ch = ch;
            rc = each_batch(c, R, 0, n_tables, [&](int t0) {
                R.cube_bits = cube_bits ? cube_bits + (size_t)t0 * stride + cube_off : nullptr;
                R.cube_sse = cube_sse ? cube_sse + (size_t)t0 * stride + cube_off : nullptr;
                R.blk_y = blk_y + (size_t)t0 * blk_stride;
                return counted(c, launch_distortion_ssim(v.D, v.px, v.edge, P, R, c->stream));
            });
            if (!rc)
                rc = ssim_windows(c, g, sg, blk_y, R.blk_x, blk_stride, ns, n_tables, d_win, interleaved(n_stacks, channels, s0, ch, sg.win_per_stack),
                                  F.sums(L.ssim), interleaved(n_stacks, channels, s0, ch));
        }
    }
    if (!rc && sse && launch_distortion_sum(cube_sse, (uint32_t)cps, L.sse.n, F.sums(L.sse), c->stream)) rc = DCT3D_EKERNEL;
    if (!rc && bits && launch_rate_sum(cube_bits, (uint32_t)cps, L.bits.n, F.sums(L.bits), c->stream)) rc = DCT3D_EKERNEL;
    if ((rc = F.end(rc, (uint64_t)n_tables * stride))) return rc;
    F.read_back(L.ssim, ssim);
    F.read_back(L.sse, sse);
    F.read_back(L.bits, bits);
    return DCT3D_OK;
}

// ---- frames in host memory: the frames go up in chunks of whole stacks (one staging buffer of kChunkBytes at most,
//      or one stack), each chunk's results land at its stacks' places; the chunks' statistics add up (batch) ----
struct Scatter {           // a result of 8-byte words, [outer][n_stacks][inner]
    void* dst;             // nullptr: not asked for
    size_t outer, inner;
    uint64_t* part = nullptr;  // a chunk's [outer][ns][inner]
    template <class T = uint64_t>
    T* want() const { return dst ? (T*)part : nullptr; }
};
// body(d_frames, ns, outs): the device body on a chunk of ns stacks, its results into outs[i].want()
template <class Body>
int host_chunks(dct3d_ctx* c, const uint8_t* frames, const Geom& g, int n_stacks, std::vector<Scatter> outs, Body&& body) {
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    const size_t stack_bytes = (size_t)g.plane() * c->bd;  // the unpadded frames of one stack
    const int per = stacks_per_range(kChunkBytes, stack_bytes, n_stacks);
    int rc;
    if ((rc = c->h_in.grow(stack_bytes * per ? stack_bytes * per : 1))) return rc;
    size_t words = 0;
    for (const Scatter& o : outs) words += o.outer * per * o.inner;
    std::vector<uint64_t> part(words);
    words = 0;
    for (Scatter& o : outs) {
        o.part = part.data() + words;
        words += o.outer * per * o.inner;
    }
    c->last_units = 0;  // (no stack: no chunk)
    batch_begin(c);
    rc = DCT3D_OK;
    for (int s0 = 0; s0 < n_stacks && !rc; s0 += per) {
        const int ns = std::min(per, n_stacks - s0);
        if (hipMemcpyAsync(c->h_in.p, frames + (size_t)s0 * stack_bytes, (size_t)ns * stack_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            rc = DCT3D_EDEVICE;
        if (rc || (rc = body((const uint8_t*)c->h_in.p, ns, outs.data()))) break;
        for (const Scatter& o : outs)
            for (size_t i = 0; o.dst && i < o.outer; i++)
                memcpy((uint64_t*)o.dst + chunk_dst(i, n_stacks, s0, o.inner), o.part + chunk_src(i, ns, o.inner), ns * o.inner * sizeof(uint64_t));
    }
    batch_end(c);
    return rc;
}
// ssim: the SSIM probe (sse and bits optional); else as probe_dev
int probe_host(dct3d_ctx* c, const uint8_t* frames, const Geom& g, int n_stacks, const int32_t* tables, int n_tables, uint64_t* sse,
               uint64_t* bits, int64_t* ssim = nullptr) {
    const size_t n = (size_t)n_tables, px = (size_t)g.px;
    return host_chunks(c, frames, g, n_stacks, {{sse, n, px}, {bits, n, px}, {ssim, n, px}}, [&](const uint8_t* d, int ns, const Scatter* o) {
        return ssim ? ssim_dev(c, d, g, ns, tables, n_tables, o[2].want<int64_t>(), o[0].want(), o[1].want(), nullptr)
                    : probe_dev(c, d, g, ns, tables, n_tables, o[0].want(), o[1].want(), nullptr, nullptr);
    });
}

// ---- the RGB-domain probes: (Y, Cb, Cr) table triples on packed RGB24, in all three colour modes ----
struct RgbArgs {
    const int32_t* tables;
    int n_tables;
    const uint8_t* cand;  // [n_cand][3], never nullptr here (rgb_call)
    int n_cand;
};
struct RgbOut {              // ssim != nullptr: the RGB and luma SSIM probe (sse optional, no plane_sse, no d_cube_sse)
    uint64_t *sse, *plane_sse, *bits;  // [n_cand][n_stacks], [n_tables][n_stacks][3] twice
    uint32_t* d_cube_sse;    // device, or nullptr
    int64_t *ssim, *ssim_y;  // [n_cand][n_stacks][3], [n_cand][n_stacks] or nullptr
    int32_t* d_win;          // device [n_cand][3][n_stacks][D][nwy][nwx] or nullptr
};
// the arguments (nothing is enqueued before they hold); packed RGB24 frames
bool rgb_args_ok(const dct3d_ctx* c, const uint8_t* frames, int w, int h, int n_stacks, const int32_t* tables, int n_tables,
                 const uint8_t* cand, int n_cand, const void* result, Geom* g) {
    if (!rate_args_ok(c, frames, w, h, 3, n_stacks, tables, n_tables, result, g)) return false;
    if (n_cand < 1 || n_cand > DCT3D_RATE_MAX_TABLES || (!cand && n_cand != n_tables)) return false;
    if (cand)
        for (int i = 0; i < 3 * n_cand; i++)
            if (cand[i] >= n_tables) return false;
    return !c420_refused(c, 3);
}

// Planes mode: the distortion probe (or, ssim, the SSIM probe: ssim_dev) itself on the three planes -- the SSIM probe on
// the tables some candidate uses, all of them when bits is asked for.  A candidate's numbers are its three planes'
// under their tables, put together on the host; its cubes a gather over the probe's per-cube buffer, its windows
// strided copies out of the plane probe's.
int rgb_planes_dev(dct3d_ctx* c, const uint8_t* d_frames, const Geom& g, int n_stacks, const RgbArgs& A, const RgbOut& O) {
    const bool ss = O.ssim != nullptr, compact = ss && !O.bits;
    const TableSlots T = compact_tables(A.cand, 3 * A.n_cand, 1, A.n_tables, !compact);
    const int n_steps = (int)c->plan.steps.size();
    const int32_t* tb = A.tables;
    if (A.tables && compact) {
        c->rgb_tables.resize((size_t)T.n * n_steps);
        for (int i = 0; i < T.n; i++) memcpy(&c->rgb_tables[(size_t)i * n_steps], A.tables + (size_t)T.used[i] * n_steps, n_steps * sizeof(int32_t));
        tb = c->rgb_tables.data();
    }
    const size_t wps = (size_t)ssim_geom(g.w, g.h, c->bd, kSsimWinPerBlock, kSsimMaxBpr).win_per_stack, n_runs = (size_t)T.n * n_stacks * 3;
    int rc;
    if (O.d_win && (rc = c->d_ssim_win.grow(n_runs * wps * sizeof(int32_t) + 4))) return rc;
    std::vector<int64_t> pm(ss ? n_runs : 0);
    std::vector<uint64_t> ps(O.sse ? n_runs : 0);
    uint64_t* const pe = O.sse ? ps.data() : nullptr;
    rc = ss ? ssim_dev(c, d_frames, g, n_stacks, tb, T.n, pm.data(), pe, O.bits, O.d_win ? (int32_t*)c->d_ssim_win.p : nullptr)
            : probe_dev(c, d_frames, g, n_stacks, tb, T.n, pe, O.bits, nullptr, nullptr);
    if (rc || n_stacks == 0) return rc;
    for (int i = 0; i < A.n_cand; i++)
        for (int s = 0; s < n_stacks; s++) {
            uint64_t v = 0;
            for (int k = 0; k < 3; k++) {
                const size_t at = triple_at(n_stacks, T.slot[A.cand[3 * i + k]], s, k);
                if (ss) O.ssim[triple_at(n_stacks, i, s, k)] = pm[at];
                if (O.sse) v += ps[at];
            }
            if (O.sse) O.sse[(size_t)i * n_stacks + s] = v;
        }
    if (O.plane_sse) memcpy(O.plane_sse, ps.data(), n_runs * sizeof(uint64_t));
    if (!O.d_cube_sse && !O.d_win) return DCT3D_OK;
    if (O.d_cube_sse) {
        const uint64_t n_cubes = g.cps() * (uint64_t)n_stacks;
        if ((rc = c->d_rgb_slots.grow((size_t)3 * A.n_cand))) return rc;
        if (hipMemcpyAsync(c->d_rgb_slots.p, A.cand, (size_t)3 * A.n_cand, hipMemcpyHostToDevice, c->stream) != hipSuccess) return DCT3D_EDEVICE;
        if (launch_distortion_rgb_gather((const uint32_t*)c->d_dist_sse.p, 3 * n_cubes, (const uint8_t*)c->d_rgb_slots.p, (uint32_t)A.n_cand,
                                         (uint32_t)g.cps(), (uint32_t)n_stacks, O.d_cube_sse, n_cubes, c->stream))
            rc = DCT3D_EKERNEL;
    }
    // [table][stack][plane][windows] -> [candidate][plane][stack][windows]: one strided copy per (candidate, plane)
    for (int i = 0; i < 3 * A.n_cand && O.d_win && !rc; i++) {
        const int32_t* const from = (const int32_t*)c->d_ssim_win.p + triple_at(n_stacks, T.slot[A.cand[i]], 0, i % 3) * wps;
        if (hipMemcpy2DAsync(O.d_win + (size_t)i * n_stacks * wps, wps * sizeof(int32_t), from, 3 * wps * sizeof(int32_t), wps * sizeof(int32_t),
                             (size_t)n_stacks, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
            rc = DCT3D_EDEVICE;
    }
    if (stream_wait(c) && !rc) rc = DCT3D_EDEVICE;  // (the candidates' host copy is free again)
    return rc;
}

// YCbCr and YCbCr + 4:2:0 on frames in device memory.  The stacks go in ranges whose decoded planes fit the budget;
// per range, pass 1 per plane and kRateTables tables (launch_distortion_plane) with the planes' sums, then pass 2 over
// the candidates.  A plane is coded under the tables some candidate uses for it, or under all of them when plane_sse
// or bits is asked for.  The SSIM probe's ranges fit kSsimBlockBudget too.
struct RgbPlan {
    bool c420;
    Geom gp[3];                   // the planes' geometries (grey)
    TableSlots T[3];              // each plane's tables, and where a candidate finds its plane
    size_t cps[3], pframes[3];    // cubes per stack, bytes of one stack's frames of the plane
    size_t stack_planes, stack_cubes;  // of one stack, all planes and their tables
    const uint8_t* slots;         // host [n_cand][3]
    SsimGeom sg;
    int n_sp, per;                // the planes of the SSIM records; stacks per range
    RgbSums L;
};
struct RgbRange {
    int s0, ns;
    const uint8_t* fr;
    uint8_t* planes[3];  // [table of the plane][stack of the range]: the decoded planes, their cubes' errors and bits
    uint32_t* psse[3];
    uint16_t* pbits[3];
};
// the planes' tables (c->rgb_tables; its tail: the candidates' slots, bytes), the sizes and the sums' layout
int rgb_setup(dct3d_ctx* c, const Geom& g, int n_stacks, const RgbArgs& A, const RgbOut& O, RgbPlan& S) {
    const int n_steps = (int)c->plan.steps.size();
    int nk[3];
    for (int k = 0; k < 3; k++) {
        S.T[k] = compact_tables(A.cand + k, A.n_cand, 3, A.n_tables, O.plane_sse || O.bits);
        nk[k] = S.T[k].n;
    }
    S.n_sp = O.ssim ? (O.ssim_y ? 4 : 3) : 0;
    S.L = rgb_sums(nk, n_stacks, A.n_cand, O.bits != nullptr, S.n_sp);
    c->rgb_tables.resize(S.L.nt * n_steps + 3 * DCT3D_RATE_MAX_TABLES);
    uint8_t* const slots = (uint8_t*)(c->rgb_tables.data() + S.L.nt * n_steps);
    S.slots = slots;
    S.stack_planes = S.stack_cubes = 0;
    for (int k = 0; k < 3; k++) {
        for (int i = 0; i < nk[k]; i++)
            for (int s = 0; s < n_steps; s++)
                c->rgb_tables[(S.L.toff[k] + i) * n_steps + s] = A.tables ? A.tables[(size_t)S.T[k].used[i] * n_steps + s] : c->plan.steps[s];
        for (int i = 0; i < A.n_cand; i++) slots[3 * i + k] = (uint8_t)S.T[k].slot[A.cand[3 * i + k]];
        S.cps[k] = (size_t)S.gp[k].cps();
        S.pframes[k] = (size_t)S.gp[k].w * S.gp[k].h * c->bd;
        S.stack_planes += nk[k] * S.pframes[k];
        S.stack_cubes += nk[k] * S.cps[k];
    }
    S.sg = ssim_geom(g.w, g.h, c->bd, kSsimWinPerBlock, kSsimMaxBpr);
    S.per = stacks_per_range(kRgbPlaneBudget, S.stack_planes, n_stacks);
    if (!O.ssim) return DCT3D_OK;
    if (!S.sg.fits()) return DCT3D_EINVAL;
    S.per = std::min(S.per, ssim_range_stacks(kSsimBlockBudget, S.sg, A.n_cand, S.n_sp, n_stacks));
    return DCT3D_OK;
}
// pass 1 of plane k of a range, and the range's sums of the plane: [table of the plane][stack of the range]
int rgb_pass1(dct3d_ctx* c, const Frame& F, const Geom& g, const RgbPlan& S, const RgbRange& Rg, int k) {
    const bool sub = S.c420 && k > 0;
    const int nk = S.T[k].n;
    const uint64_t ncu = S.cps[k] * (uint64_t)Rg.ns;
    EncodeParams P;
    fill_encode_params(c, P, Rg.fr, nullptr, g, ncu);
    if (sub) c420_cube_fields(P, g, S.gp[k]);
    DistPlaneParams R = {};
    R.table_stride = ncu;
    R.ch = k;
    set_decode_constants(c, R, g);
    R.plane_stride = S.pframes[k] * Rg.ns;
    R.pw = (uint32_t)S.gp[k].w;
    R.ph = (uint32_t)S.gp[k].h;
    int rc = each_batch(c, R, S.L.toff[k], nk, [&](int t0) {
        R.cube_sse = Rg.psse[k] + (size_t)t0 * ncu;
        R.cube_bits = Rg.pbits[k] ? Rg.pbits[k] + (size_t)t0 * ncu : nullptr;
        R.planes = Rg.planes[k] + (size_t)t0 * R.plane_stride;
        return counted(c, launch_distortion_plane(c->bd, sub ? c420_edge(g) : (g.edge() ? 1 : 0), sub ? 2 : 1, P, R, c->stream));
    });
    const size_t at = rgb_range_off(S.L, Rg.s0, Rg.ns, k);
    if (!rc && launch_distortion_sum(Rg.psse[k], (uint32_t)S.cps[k], (uint64_t)nk * Rg.ns, F.sums(S.L.plane_sse) + at, c->stream)) rc = DCT3D_EKERNEL;
    if (!rc && Rg.pbits[k] && launch_rate_sum(Rg.pbits[k], (uint32_t)S.cps[k], (uint64_t)nk * Rg.ns, F.sums(S.L.plane_bits) + at, c->stream))
        rc = DCT3D_EKERNEL;
    return rc;
}
// Pass 2 of a range: the candidates' cube errors (launch_distortion_rgb_combine, where sse is asked for) and / or
// the SSIM probe's block records of R, G, B (and luma) per candidate in d_ssim_blk (launch_ssim_rgb_block), then per
// plane the windows of all candidates and their sums per (candidate, stack)
int rgb_pass2(dct3d_ctx* c, const Frame& F, const Geom& g, int n_stacks, const RgbPlan& S, const RgbRange& Rg, int n_cand, const RgbOut& O,
              uint32_t* cube_out) {
    const int D = c->bd, ns = Rg.ns;
    const uint32_t cps = (uint32_t)S.cps[0], nbx = (uint32_t)(g.wp / 8);
    const RgbCombineParams C = {Rg.fr, Rg.planes[0], Rg.planes[1], Rg.planes[2], S.pframes[0] * ns, S.pframes[1] * ns,  // frames y cb cr, strides
                                (uint32_t)g.w, (uint32_t)g.h, (uint32_t)S.gp[1].w, (uint32_t)S.gp[1].h, S.c420 ? 1u : 0u,  // w h cw chh shift
                                nbx, cps, cps * (uint32_t)ns, fast_div(cps), fast_div(nbx),  // the frames' grid: nbx cubes_per_stack n_cubes
                                (const uint8_t*)c->d_rgb_slots.p, (uint32_t)n_cand, cube_out + (size_t)Rg.s0 * cps, cps * (uint64_t)n_stacks};
    if (O.sse && launch_distortion_rgb_combine(D, C, c->stream)) return DCT3D_EKERNEL;
    if (!O.ssim) return DCT3D_OK;
    uint64_t* const blk_y = (uint64_t*)c->d_ssim_blk.p;
    SsimRgbParams B = {C, blk_y, nullptr, S.sg.blk_per_stack * ns, S.sg.nbx, S.sg.nby};
    B.C.cube_sse = nullptr;
    B.blk_x = (uint32_t*)(blk_y + (size_t)S.n_sp * n_cand * B.blk_stride);
    int rc = launch_ssim_rgb_block(D, S.n_sp == 4, B, c->stream) ? DCT3D_EKERNEL : DCT3D_OK;
    for (int k = 0; k < S.n_sp && !rc; k++)  // ssim[c][s][k]; ssim_y[c][s], no windows of the luma
        rc = ssim_windows(c, g, S.sg, B.blk_y + (size_t)k * n_cand * B.blk_stride, B.blk_x + (size_t)k * B.blk_stride, B.blk_stride, ns, n_cand,
                          k < 3 ? O.d_win : nullptr, planar(n_stacks, 3, Rg.s0, k, S.sg.win_per_stack), F.sums(k < 3 ? S.L.ssim : S.L.ssim_y),
                          k < 3 ? interleaved(n_stacks, 3, Rg.s0, k) : interleaved(n_stacks, 1, Rg.s0, 0));
    return rc;
}
int rgb_ycc_dev(dct3d_ctx* c, const uint8_t* d_frames, const Geom& g, int n_stacks, const RgbArgs& A, const RgbOut& O) {
    RgbPlan S;
    uint64_t nc;
    S.c420 = c420_on(c, 3);
    if (!make_geom(g.w, g.h, 1, n_stacks, true, &S.gp[0], &nc)) return DCT3D_EINVAL;
    S.gp[1] = S.gp[0];
    if (S.c420 && !c420_geom(g, n_stacks, &S.gp[1], &nc)) return DCT3D_EINVAL;
    S.gp[2] = S.gp[1];
    Frame F{c};
    int rc;
    if ((rc = F.enter()) || n_stacks == 0 || (rc = rgb_setup(c, g, n_stacks, A, O, S))) return rc;
    const size_t per = (size_t)S.per, n_cand = (size_t)A.n_cand, n_out = n_cand * S.cps[0] * n_stacks;
    if ((rc = F.begin(c->rgb_tables.data(), (int)S.L.nt, true, S.L.total,
                      {{&c->d_rgb_planes, S.stack_planes * per},
                       {&c->d_rgb_psse, S.stack_cubes * per * sizeof(uint32_t)},
                       {&c->d_rgb_pbits, O.bits ? S.stack_cubes * per * sizeof(uint16_t) : 0},
                       {&c->d_rgb_cube, O.sse && !O.d_cube_sse ? n_out * sizeof(uint32_t) : 0},
                       {&c->d_ssim_blk, O.ssim ? (size_t)S.sg.record_bytes(A.n_cand, S.n_sp) * per : 0},
                       {&c->d_ssim_part, O.ssim ? n_cand * per * S.sg.bpr * sizeof(int64_t) : 0}},
                      S.slots, 3 * n_cand)))
        return rc;
    uint32_t* const cube_out = O.d_cube_sse ? O.d_cube_sse : (uint32_t*)c->d_rgb_cube.p;
    for (int s0 = 0; s0 < n_stacks && !rc; s0 += S.per) {
        const int ns = std::min(S.per, n_stacks - s0);
        RgbRange Rg = {s0, ns, d_frames + (size_t)s0 * g.plane() * c->bd, {(uint8_t*)c->d_rgb_planes.p}, {(uint32_t*)c->d_rgb_psse.p},
                       {O.bits ? (uint16_t*)c->d_rgb_pbits.p : nullptr}};
        for (int k = 1; k < 3; k++) {
            Rg.planes[k] = Rg.planes[k - 1] + S.T[k - 1].n * S.pframes[k - 1] * ns;
            Rg.psse[k] = Rg.psse[k - 1] + S.T[k - 1].n * S.cps[k - 1] * ns;
            Rg.pbits[k] = O.bits ? Rg.pbits[k - 1] + S.T[k - 1].n * S.cps[k - 1] * ns : nullptr;
        }
        for (int k = 0; k < 3 && !rc; k++) rc = rgb_pass1(c, F, g, S, Rg, k);
        if (!rc) rc = rgb_pass2(c, F, g, n_stacks, S, Rg, A.n_cand, O, cube_out);
    }
    if (!rc && O.sse && launch_distortion_sum(cube_out, (uint32_t)S.cps[0], S.L.rgb_sse.n, F.sums(S.L.rgb_sse), c->stream)) rc = DCT3D_EKERNEL;
    if ((rc = F.end(rc, (uint64_t)S.stack_cubes * n_stacks))) return rc;
    F.read_back(S.L.rgb_sse, O.sse);
    F.read_back(S.L.ssim, O.ssim);
    F.read_back(S.L.ssim_y, O.ssim_y);
    // plane_sse or bits: every (table, plane) pair was coded, slot t of plane k is table t
    for (int s0 = 0; s0 < n_stacks && (O.plane_sse || O.bits); s0 += S.per) {
        const int ns = std::min(S.per, n_stacks - s0);
        for (int k = 0; k < 3; k++)
            for (int t = 0; t < A.n_tables; t++)
                for (int s = 0; s < ns; s++) {
                    const size_t src = rgb_plane_src(S.L, s0, ns, k, t, s), dst = triple_at(n_stacks, t, s0 + s, k);
                    if (O.plane_sse) O.plane_sse[dst] = c->h_rate[S.L.plane_sse.off + src];
                    if (O.bits) O.bits[dst] = c->h_rate[S.L.plane_bits.off + src];
                }
    }
    return DCT3D_OK;
}

int rgb_dev(dct3d_ctx* c, const uint8_t* d_frames, const Geom& g, int n_stacks, const RgbArgs& A, const RgbOut& O) {
    return c->opt_colour ? rgb_ycc_dev(c, d_frames, g, n_stacks, A, O)
                         : rgb_planes_dev(c, d_frames, g, n_stacks, A, O);
}
// the four entry points' body: the argument check (result: the output the call must give), candidate i = (i, i, i)
// where the caller gives no list, frames in host or device memory
int rgb_call(dct3d_ctx* c, const uint8_t* frames, bool host, int w, int h, int n_stacks, const int32_t* tables, int n_tables,
             const uint8_t* cand, int n_cand, const void* result, const RgbOut& O) {
    Geom g;
    if (!rgb_args_ok(c, frames, w, h, n_stacks, tables, n_tables, cand, n_cand, result, &g)) return DCT3D_EINVAL;
    if (O.ssim_y && !c->opt_colour) return DCT3D_EINVAL;  // planes mode has no luma plane
    uint8_t own[3 * DCT3D_RATE_MAX_TABLES];
    for (int i = 0; i < 3 * n_cand && !cand; i++) own[i] = (uint8_t)(i / 3);
    const RgbArgs A = {tables, n_tables, cand ? cand : own, n_cand};
    if (!host) return rgb_dev(c, frames, g, n_stacks, A, O);
    const size_t nc = (size_t)n_cand, nt = (size_t)n_tables;
    return host_chunks(c, frames, g, n_stacks, {{O.sse, nc, 1}, {O.plane_sse, nt, 3}, {O.bits, nt, 3}, {O.ssim, nc, 3}, {O.ssim_y, nc, 1}},
                       [&](const uint8_t* d, int ns, const Scatter* o) {
                           return rgb_dev(c, d, g, ns, A, RgbOut{o[0].want(), o[1].want(), o[2].want(), nullptr, o[3].want<int64_t>(), o[4].want<int64_t>(), nullptr});
                       });
}

}  // namespace

extern "C" {

// ---- rate probe: the streams' exact sizes under several tables, one transform per cube (dct3d.h) ----
int dct3d_rate_frames_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int channels, int n_stacks,
                          const int32_t* tables, int n_tables, uint64_t* bits, uint16_t* d_cube_bits) {
    Geom g;
    if (!rate_args_ok(c, d_frames, w, h, channels, n_stacks, tables, n_tables, bits, &g)) return DCT3D_EINVAL;
    // 4:2:0: the cube layout is ragged (the chroma planes have fewer cubes): only the totals are offered
    if (c420_refused(c, channels) || (c420_on(c, channels) && d_cube_bits)) return DCT3D_EINVAL;
    return probe_dev(c, d_frames, g, n_stacks, tables, n_tables, nullptr, bits, nullptr, d_cube_bits);
}

int dct3d_rate_frames(dct3d_ctx* c, const uint8_t* frames, int w, int h, int channels, int n_stacks,
                      const int32_t* tables, int n_tables, uint64_t* bits) {
    Geom g;
    if (!rate_args_ok(c, frames, w, h, channels, n_stacks, tables, n_tables, bits, &g) || c420_refused(c, channels)) return DCT3D_EINVAL;
    return probe_host(c, frames, g, n_stacks, tables, n_tables, nullptr, bits);
}

// ---- distortion probe: the exact squared error of encode + decode under several tables, one transform per
//      cube and one certified decode tile per cube and table (dct3d.h) ----
int dct3d_distortion_frames_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int channels, int n_stacks,
                                const int32_t* tables, int n_tables, uint64_t* sse, uint64_t* bits, uint32_t* d_cube_sse) {
    Geom g;
    if (!rate_args_ok(c, d_frames, w, h, channels, n_stacks, tables, n_tables, sse, &g) || colour_refused(c, channels)) return DCT3D_EINVAL;
    return probe_dev(c, d_frames, g, n_stacks, tables, n_tables, sse, bits, d_cube_sse, nullptr);
}

int dct3d_distortion_frames(dct3d_ctx* c, const uint8_t* frames, int w, int h, int channels, int n_stacks,
                            const int32_t* tables, int n_tables, uint64_t* sse, uint64_t* bits) {
    Geom g;
    if (!rate_args_ok(c, frames, w, h, channels, n_stacks, tables, n_tables, sse, &g) || colour_refused(c, channels)) return DCT3D_EINVAL;
    return probe_host(c, frames, g, n_stacks, tables, n_tables, sse, bits);
}

// ---- SSIM probe: the exact 8 x 8 / stride 4 windowed SSIM of encode + decode under several tables, from the
//      distortion probe's transform and decode tile per cube (dct3d.h states the definition) ----
int dct3d_ssim_windows(int w, int h, int* nwx, int* nwy) {
    if (w < 1 || h < 1 || !nwx || !nwy) return DCT3D_EINVAL;
    const SsimGeom sg = ssim_geom(w, h, 1, kSsimWinPerBlock, kSsimMaxBpr);
    *nwx = (int)sg.nwx;
    *nwy = (int)sg.nwy;
    return DCT3D_OK;
}

int dct3d_ssim_frames_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int channels, int n_stacks,
                          const int32_t* tables, int n_tables, int64_t* ssim, uint64_t* sse, uint64_t* bits, int32_t* d_window_ssim) {
    Geom g;
    if (!rate_args_ok(c, d_frames, w, h, channels, n_stacks, tables, n_tables, ssim, &g) || colour_refused(c, channels) || c420_refused(c, channels))
        return DCT3D_EINVAL;
    return ssim_dev(c, d_frames, g, n_stacks, tables, n_tables, ssim, sse, bits, d_window_ssim);
}

int dct3d_ssim_frames(dct3d_ctx* c, const uint8_t* frames, int w, int h, int channels, int n_stacks,
                      const int32_t* tables, int n_tables, int64_t* ssim, uint64_t* sse, uint64_t* bits) {
    Geom g;
    if (!rate_args_ok(c, frames, w, h, channels, n_stacks, tables, n_tables, ssim, &g) || colour_refused(c, channels) || c420_refused(c, channels))
        return DCT3D_EINVAL;
    return probe_host(c, frames, g, n_stacks, tables, n_tables, sse, bits, ssim);
}

// ---- RGB-domain distortion probe: the exact squared error, in the RGB pixels, of the stream encode + decode
//      under (Y, Cb, Cr) table triples, in all three colour modes (dct3d.h) ----
int dct3d_distortion_rgb_frames_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int n_stacks, const int32_t* tables,
                                    int n_tables, const uint8_t* cand, int n_cand, uint64_t* sse, uint64_t* plane_sse,
                                    uint64_t* bits, uint32_t* d_cube_sse) {
    return rgb_call(c, d_frames, false, w, h, n_stacks, tables, n_tables, cand, n_cand, sse, RgbOut{sse, plane_sse, bits, d_cube_sse, nullptr, nullptr, nullptr});
}

int dct3d_distortion_rgb_frames(dct3d_ctx* c, const uint8_t* frames, int w, int h, int n_stacks, const int32_t* tables,
                                int n_tables, const uint8_t* cand, int n_cand, uint64_t* sse, uint64_t* plane_sse, uint64_t* bits) {
    return rgb_call(c, frames, true, w, h, n_stacks, tables, n_tables, cand, n_cand, sse, RgbOut{sse, plane_sse, bits, nullptr, nullptr, nullptr, nullptr});
}

// ---- RGB and luma SSIM probe: the SSIM probe's numbers on the RGB bytes (and the luma plane) of the stream encode
//      + decode under (Y, Cb, Cr) table triples, in all three colour modes (dct3d.h) ----
int dct3d_ssim_rgb_frames_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int n_stacks, const int32_t* tables,
                              int n_tables, const uint8_t* cand, int n_cand, int64_t* ssim, int64_t* ssim_y, uint64_t* sse,
                              uint64_t* bits, int32_t* d_window_ssim) {
    return rgb_call(c, d_frames, false, w, h, n_stacks, tables, n_tables, cand, n_cand, ssim, RgbOut{sse, nullptr, bits, nullptr, ssim, ssim_y, d_window_ssim});
}

int dct3d_ssim_rgb_frames(dct3d_ctx* c, const uint8_t* frames, int w, int h, int n_stacks, const int32_t* tables, int n_tables,
                          const uint8_t* cand, int n_cand, int64_t* ssim, int64_t* ssim_y, uint64_t* sse, uint64_t* bits) {
    return rgb_call(c, frames, true, w, h, n_stacks, tables, n_tables, cand, n_cand, ssim, RgbOut{sse, nullptr, bits, nullptr, ssim, ssim_y, nullptr});
}

}  // extern "C"
