// dct3d_runtime.cpp -- the C-ABI (include/dct3d.h): context, buffers, launches.
//
// Replaces the reference's per-call OpenCL setup (encoder.c:147-197, decoder.c:153-202,
// OpenCLUtils.c:49-165) with a persistent context: the transform plan (DCT.initialize equivalent,
// dct3d_plan.cpp) is built once and its fold tables uploaded once; device work buffers are grown on
// demand and reused; everything runs on one HIP stream.  Errors are returned, never printed, never
// exit()ed (the reference exit(1)s inside OpenCLUtils.c:40-162).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <vector>
#include <cstring>
#include <mutex>
#include <condition_variable>
#include <deque>
#include <thread>
#include <new>

#include "dct3d_ctx.h"
#include "dct3d_c420.h"
#include "dct3d_distortion.h"

using namespace dct3d;
using namespace dct3d::rt;

namespace {

// the stream decode's status words (d_egd_status): [0, 4) the sync / mark passes' (EgDecParams::status),
// [4, 6) the chunk scan's (EgParams::status)
constexpr size_t kEgdStatusBytes = 6 * sizeof(uint64_t);
// the pinned host words (h_status): [0, 6) a call's status words, [6] and [7] the decode's and the encode's
// hand-off tags, [8, 26) the three fronts' words of a packed RGB24 stream decode
constexpr size_t kHostStatusBytes = (8 + 18) * sizeof(uint64_t);

}  // namespace

// diagonal-slice order (CubeUtils.c:5-46): x + y + z ascending; y outer, z middle, x inner
static int diagonal_order(int bw, int bh, int bd, uint16_t* out) {
    int n = 0;
    for (int t = 0; t <= (bw - 1) + (bh - 1) + (bd - 1); t++)
        for (int y = 0; y <= (bh - 1 < t ? bh - 1 : t); y++)
            for (int z = 0; z <= (bd - 1 < t ? bd - 1 : t); z++) {
                const int x = t - y - z;
                if (x < 0 || x > bw - 1) continue;
                out[n++] = (uint16_t)(x + bw * y + bw * bh * z);
            }
    return n;
}

extern "C" {

int dct3d_abi_version(void) { return DCT3D_ABI_VERSION; }

const char* dct3d_strerror(int code) {
    switch (code) {
        case DCT3D_OK: return "ok";
        case DCT3D_EINVAL: return "invalid argument";
        case DCT3D_EDEVICE: return "HIP device error";
        case DCT3D_ENOMEM: return "out of memory";
        case DCT3D_EKERNEL: return "kernel launch failed";
        case DCT3D_ENOSPC: return "output buffer too small";
        case DCT3D_ENODATA: return "input stream ends early";
        default: return "unknown error";
    }
}

// the status words of an entropy stage (device, written by its kernels on the context stream): one
// asynchronous copy into the pinned words, then the stream's completion
// The end of a synchronous call: the stream polled for a while before blocking (a blocking wait took
// ~15-40 us to return after the stream's last kernel, profiles/r06/gaps/), so that the caller's next
// call reaches the device sooner.
extern "C++" int rt::stream_wait(dct3d_ctx* c) {
    for (int i = 0; i < 20000; i++) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) return DCT3D_OK;
        if (e != hipErrorNotReady) return DCT3D_EDEVICE;
    }
    return hipStreamSynchronize(c->stream) == hipSuccess ? DCT3D_OK : DCT3D_EDEVICE;
}
static int read_status(dct3d_ctx* c, const void* d_status, size_t bytes, uint64_t* out) {
    if (hipMemcpyAsync(c->h_status, d_status, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        stream_wait(c))
        return DCT3D_EDEVICE;
    memcpy(out, c->h_status, bytes);
    return DCT3D_OK;
}

// The encode stream's status words for this call (zeroed: by a memset unless the last call's stitch kernel
// cleared this slot), and the kernel-side hand-off (EgParams::status_host / status_clear).
static uint64_t* eg_status_begin(dct3d_ctx* c, int* rc) {
    uint64_t* st = (uint64_t*)c->d_eg_status.p + 2 * c->eg_slot;
    const bool clean = c->eg_clean[c->eg_slot];
    c->eg_clean[c->eg_slot] = false;
    *rc = !clean && hipMemsetAsync(st, 0, 16, c->stream) != hipSuccess ? DCT3D_EDEVICE : DCT3D_OK;
    return st;
}
static void eg_status_handoff(dct3d_ctx* c, EgParams& P) {
    P.status_host = c->h_status_dev;
    P.status_clear = (uint64_t*)c->d_eg_status.p + 2 * (c->eg_slot ^ 1);
    P.seq = ++c->eg_seq;
}
static int wait_tag(dct3d_ctx* c, int word, uint64_t seq, uint64_t* value, uint32_t* flags);
// after the stitch kernel was enqueued with the hand-off: the call returns when the stitch's block 0 has
// handed the verdict over (the tag), the stitch's last words completing on the stream (a wait for the
// stream's end instead took ~30 us longer to return, profiles/r06/gaps/timed)
static int eg_status_end(dct3d_ctx* c, bool handoff, const uint64_t* st, uint64_t* out, uint64_t seq = 0) {
    int rc;
    if (handoff) {
        c->eg_clean[c->eg_slot ^ 1] = true;
        uint64_t v = 0;
        uint32_t fl = 0;
        rc = wait_tag(c, 7, seq, &v, &fl);
        if (!rc && (fl & kTagOverflow)) {  // the total did not fit the tag: the words, after the stream
            rc = stream_wait(c);
            if (!rc) memcpy(out, c->h_status, 16);
        } else if (!rc) {
            out[0] = v;
            out[1] = fl & 3u;
        }
    } else {
        rc = read_status(c, st, 16, out);
    }
    c->eg_slot ^= 1;
    return rc;
}

static int upload(DevBuf& b, const void* src, size_t bytes) {
    int rc = b.grow(bytes);
    if (rc) return rc;
    return hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? DCT3D_OK : DCT3D_EDEVICE;
}

// a caller's quantiser table for block dims (bw, bh, bd): its length (the steps' range: build_plan)
static bool quant_len_ok(int bw, int bh, int bd, const int32_t* steps, int n) {
    return !steps || (bw > 0 && bh > 0 && bd > 0 && n == bw + bh + bd - 2);
}

int dct3d_plan_query(int bw, int bh, int bd, dct3d_plan_info* info, int32_t* ngroups, double* coef,
                     uint8_t* group_of, double* enc_K) {
    return dct3d_plan_query_quant(bw, bh, bd, nullptr, 0, info, ngroups, coef, group_of, enc_K);
}

int dct3d_plan_query_quant(int bw, int bh, int bd, const int32_t* steps, int n, dct3d_plan_info* info, int32_t* ngroups,
                           double* coef, uint8_t* group_of, double* enc_K) {
    Plan p;
    if (!quant_len_ok(bw, bh, bd, steps, n) || !build_plan(bw, bh, bd, steps, p)) return DCT3D_EINVAL;
    if (info) {
        memset(info, 0, sizeof(*info));
        info->cube_size = p.cs;
        info->n_mults = p.n_mults;
        info->treeified = p.treeified ? 1 : 0;
        info->coef_dc = p.coef_dc;
        info->dec_G = p.dec_G;
        info->dec_E = p.dec_E;
        info->dec_l1_max = p.dec_l1_max;
        memcpy(info->enc_rstep, p.enc_rstep, sizeof(info->enc_rstep));
        memcpy(info->enc_G, p.enc_G, sizeof(info->enc_G));
        memcpy(info->enc_E, p.enc_E, sizeof(info->enc_E));
        memcpy(info->enc_thr64, p.enc_thr64, sizeof(info->enc_thr64));
    }
    if (ngroups) memcpy(ngroups, p.fwd_ngroups.data(), sizeof(int32_t) * p.cs);
    if (coef) memcpy(coef, p.fwd_coef.data(), sizeof(double) * p.fwd_coef.size());
    if (group_of) memcpy(group_of, p.fwd_group_of.data(), p.fwd_group_of.size());
    if (enc_K) memcpy(enc_K, p.enc_K.data(), sizeof(double) * p.cs);
    return DCT3D_OK;
}

// The plan's tables that depend on the quantiser, to the device (context creation, dct3d_ctx_set_quant):
// the encode's {1 / step, G, E} per s, and the fp64 table [64] basis, [32] second-certificate thresholds,
// [32] steps (kQtStepOff; entries past the cube's largest s: the reference's, never read)
static int upload_quant_tables(dct3d_ctx* c) {
    const Plan& p = c->plan;
    float tabs[3 * kMaxS];
    memcpy(tabs, p.enc_rstep, sizeof(float) * kMaxS);
    memcpy(tabs + kMaxS, p.enc_G, sizeof(float) * kMaxS);
    memcpy(tabs + 2 * kMaxS, p.enc_E, sizeof(float) * kMaxS);
    int rc = upload(c->d_tabs, tabs, sizeof(tabs));
    if (rc) return rc;
    static_assert(kQtStepOff == 64 + kMaxS, "the steps follow the thresholds");
    double t64[kQtStepOff + kMaxS];
    memcpy(t64, p.basis64, sizeof(p.basis64));
    memcpy(t64 + 64, p.enc_thr64, sizeof(p.enc_thr64));
    for (int s = 0; s < kMaxS; s++) t64[kQtStepOff + s] = s < (int)p.steps.size() ? p.steps[s] : reference_step(s);
    return upload(c->d_tabs64, t64, sizeof(t64));
}
// The kernels' variant for geometry g.  qt: the context's calls run the table kernels (else: the product
// kernels, the reference steps in their text)
static Variant variant_of(const dct3d_ctx* c, const Geom& g) {
    return Variant{c->bd, g.px, g.edge(), !c->plan.reference_quant || c->opt_quant_force};
}
// the stream kernels' and the rate probe's: the colour transform acts on packed RGB24 alone; qt = 2 while a vq
// call is open (vq_begin .. vq_end: a table per stack, c->vq; the one place that turns it into a variant.  No
// probe runs inside one, and probe_dev reads no qt)
extern "C++" Variant rt::stream_variant_of(const dct3d_ctx* c, const Geom& g) {
    Variant v = variant_of(c, g);
    if (c->vq) v.qt = 2;
    v.colour = (c->opt_colour && g.px == 3) ? 1 : 0;
    return v;
}
// a call on packed frames that has no colour stage refuses the option (dct3d.h)
extern "C++" bool rt::colour_refused(const dct3d_ctx* c, int px) { return c && c->opt_colour && px == 3; }
// 4:2:0 acts on packed frames alone, on top of the colour transform: a packed call with the mode on and
// the transform off is refused (c420_refused) before anything is queued.  c420_geom: the chroma plane's geometry
// (grey, ceil(w / 2) x ceil(h / 2)) and its cubes per channel
extern "C++" bool rt::c420_on(const dct3d_ctx* c, int px) { return c && c->chroma == DCT3D_CHROMA_420 && px == 3; }
extern "C++" bool rt::c420_refused(const dct3d_ctx* c, int px) { return c420_on(c, px) && !c->opt_colour; }
extern "C++" bool rt::c420_geom(const Geom& g, int n_stacks, Geom* gc, uint64_t* n_cubes) {
    return make_geom(g.w / 2 + g.w % 2, g.h / 2 + g.h % 2, 1, n_stacks, true, gc, n_cubes);
}
static const double* qt_steps(const dct3d_ctx* c) { return (const double*)c->d_tabs64.p + kQtStepOff; }

int dct3d_ctx_set_quant(dct3d_ctx* c, const int32_t* steps, int n) {
    if (!c || !quant_len_ok(c->bw, c->bh, c->bd, steps, n)) return DCT3D_EINVAL;
    Plan p;
    if (!build_plan(c->bw, c->bh, c->bd, steps, p)) return DCT3D_EINVAL;  // (a step outside [1, 255])
    if (p.steps == c->plan.steps) return DCT3D_OK;
    // a call enqueued earlier still reads the tables that are rewritten below
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return DCT3D_EDEVICE;
    c->plan = std::move(p);
    return upload_quant_tables(c);
}

int dct3d_ctx_get_quant(const dct3d_ctx* c, int32_t* steps, int n) {
    if (!c || !steps || n != (int)c->plan.steps.size()) return DCT3D_EINVAL;
    memcpy(steps, c->plan.steps.data(), sizeof(int32_t) * n);
    return DCT3D_OK;
}

int dct3d_ctx_create(int device, int block_w, int block_h, int block_d, dct3d_ctx** out) {
    if (!out) return DCT3D_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return DCT3D_EDEVICE;
    dct3d_ctx* c = new (std::nothrow) dct3d_ctx();
    if (!c) return DCT3D_ENOMEM;
    c->device = device;
    c->bw = block_w;
    c->bh = block_h;
    c->bd = block_d;
    if (!build_plan(block_w, block_h, block_d, c->plan)) {
        delete c;
        return DCT3D_EINVAL;
    }
    // the context's own stream is a blocking stream: ordered with the legacy default stream, so device
    // buffers a caller fills or reads there (e.g. a framework's default stream) need no extra sync
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamDefault) != hipSuccess) {
        delete c;
        return DCT3D_EDEVICE;
    }
    c->stream = c->own_stream;
    for (auto& q : c->ev)
        for (auto& e : q)
            if (hipEventCreate(&e) != hipSuccess) {
                dct3d_ctx_destroy(c);
                return DCT3D_EDEVICE;
            }
    const Plan& p = c->plan;
    int rc = upload(c->d_ngroups, p.fwd_ngroups.data(), p.fwd_ngroups.size() * sizeof(int32_t));
    if (!rc) rc = upload(c->d_coef, p.fwd_coef.data(), p.fwd_coef.size() * sizeof(double));
    if (!rc) rc = upload(c->d_group_of, p.fwd_group_of.data(), p.fwd_group_of.size());
    if (!rc) {  // transposed, [k][n]: the replay kernel's threads (one per pixel n) read it coalesced
        std::vector<double> t(p.inv_coef.size());
        for (int n = 0; n < p.cs; n++)
            for (int k = 0; k < p.cs; k++) t[(size_t)k * p.cs + n] = p.inv_coef[(size_t)n * p.cs + k];
        rc = upload(c->d_inv_coef, t.data(), t.size() * sizeof(double));
    }
    if (!rc) rc = upload_quant_tables(c);
    if (!rc) rc = c->d_enc_counts.grow(4 * kCountSpread * sizeof(uint32_t));
    if (!rc && hipMemset(c->d_enc_counts.p, 0, 4 * kCountSpread * sizeof(uint32_t)) != hipSuccess) rc = DCT3D_EDEVICE;
    if (!rc) {
        std::vector<uint16_t> diag(p.cs);
        diagonal_order(block_w, block_h, block_d, diag.data());
        rc = upload(c->d_diag, diag.data(), diag.size() * sizeof(uint16_t));
    }
    if (!rc) rc = c->d_eg_status.grow(32);
    if (!rc && hipMemset(c->d_eg_status.p, 0, 32) != hipSuccess) rc = DCT3D_EDEVICE;
    if (!rc) rc = c->d_egd_status.grow(2 * kEgdStatusBytes);
    if (!rc && hipMemset(c->d_egd_status.p, 0, 2 * kEgdStatusBytes) != hipSuccess) rc = DCT3D_EDEVICE;
    if (!rc && hipHostMalloc((void**)&c->h_status, kHostStatusBytes, hipHostMallocDefault) != hipSuccess) {
        c->h_status = nullptr;
        rc = DCT3D_ENOMEM;
    }
    if (!rc) memset(c->h_status, 0, kHostStatusBytes);
    if (!rc) rc = c->d_egd_status3.grow(3 * kEgdStatusBytes);
    if (!rc && hipHostGetDevicePointer((void**)&c->h_status_dev, c->h_status, 0) != hipSuccess) c->h_status_dev = nullptr;
    if (rc) {
        dct3d_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return DCT3D_OK;
}

void dct3d_ctx_destroy(dct3d_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // work may still be queued on the context's stream -- its own or a caller's (dct3d_ctx_set_stream) -- that
    // reads the buffers released below
    if (c->stream && c->stream != c->own_stream) (void)hipStreamSynchronize(c->stream);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    for (DevBuf* b : {&c->d_ngroups, &c->d_coef, &c->d_group_of, &c->d_inv_coef, &c->d_tabs, &c->d_tabs64,
                      &c->d_enc_counts, &c->h_in, &c->h_out, &c->h_aux, &c->d_diag, &c->d_eg_bits,
                      &c->d_eg_off, &c->d_eg_bsum, &c->d_eg_status, &c->d_eg_out, &c->d_eg_q, &c->d_eg_ht,
                      &c->d_egd_exit, &c->d_egd_status, &c->d_egd_in, &c->d_egd_raster, &c->d_egd_mark, &c->d_egd_desc,
                      &c->d_egf_slot, &c->d_eg_out_x[0], &c->d_eg_out_x[1], &c->d_egd_in_x[0], &c->d_egd_in_x[1],
                      &c->d_eg_q_ch, &c->d_egd_status3, &c->d_rate_tabs, &c->d_rate_bits, &c->d_rate_sums,
                      &c->d_dist_steps, &c->d_dist_sse, &c->d_vq, &c->d_c420, &c->d_rgb_planes, &c->d_rgb_psse,
                      &c->d_rgb_pbits, &c->d_rgb_slots, &c->d_rgb_cube, &c->d_ssim_blk, &c->d_ssim_part, &c->d_ssim_win})
        b->release();
    if (c->h_rate) (void)hipHostFree(c->h_rate);
    if (c->vq_host) (void)hipHostFree(c->vq_host);
    if (c->h_status) (void)hipHostFree(c->h_status);
    for (auto& q : c->ev)
        for (auto& e : q)
            if (e) (void)hipEventDestroy(e);
    if (c->s_up) (void)hipStreamDestroy(c->s_up);
    if (c->s_down) (void)hipStreamDestroy(c->s_down);
    for (int i = 0; i < 2; i++) {
        if (c->pe_in[i]) (void)hipEventDestroy(c->pe_in[i]);
        if (c->pe_done[i]) (void)hipEventDestroy(c->pe_done[i]);
    }
    if (c->ev_switch) (void)hipEventDestroy(c->ev_switch);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int dct3d_ctx_set_stream(dct3d_ctx* c, void* s) {
    if (!c) return DCT3D_EINVAL;
    const hipStream_t ns = s ? (hipStream_t)s : c->own_stream;
    if (ns != c->stream) {
        // work enqueued on the new stream runs after the old stream's: a later launch would otherwise
        // overlap an earlier one whose block 0 clears the counter slot the later one counts into
        if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
        if (!c->ev_switch && hipEventCreateWithFlags(&c->ev_switch, hipEventDisableTiming) != hipSuccess)
            return DCT3D_EDEVICE;
        if (hipEventRecord(c->ev_switch, c->stream) == hipSuccess) {
            if (hipStreamWaitEvent(ns, c->ev_switch, 0) != hipSuccess) return DCT3D_EDEVICE;
        } else {
            // HIP rejected the old handle (a caller's stream destroyed before the switch, against the
            // contract in dct3d.h): order by a device-wide synchronisation.  A destroyed handle that HIP
            // has reused for a new stream is not detectable here -- hence the contract.
            (void)hipGetLastError();
            if (hipDeviceSynchronize() != hipSuccess) return DCT3D_EDEVICE;
        }
    }
    c->stream = ns;
    return DCT3D_OK;
}

int dct3d_ctx_info(const dct3d_ctx* c, int* device, int* block_d, void** hip_stream) {
    if (!c) return DCT3D_EINVAL;
    if (device) *device = c->device;
    if (block_d) *block_d = c->bd;
    if (hip_stream) *hip_stream = (void*)c->stream;
    return DCT3D_OK;
}

int dct3d_ctx_set_option(dct3d_ctx* c, int option, double value) {
    if (!c || !(value >= 0.0)) return DCT3D_EINVAL;
    switch (option) {
        case DCT3D_OPT_DEC_MARGIN: c->opt_dec_margin = value; return DCT3D_OK;
        case DCT3D_OPT_ENC_NO_RECHECK: c->opt_enc_no_recheck = value != 0.0; return DCT3D_OK;
        case DCT3D_OPT_EG_TWO_STEP: c->opt_eg_two_step = value != 0.0; return DCT3D_OK;
        case DCT3D_OPT_EG_NO_RESOLVE: c->opt_eg_no_resolve = value != 0.0; return DCT3D_OK;
        case DCT3D_OPT_EG_FORCE_RETRY: c->opt_eg_force_retry = value != 0.0; return DCT3D_OK;
        case DCT3D_OPT_EG_FUSED_FRONT: c->opt_eg_fused_front = value != 0.0; return DCT3D_OK;
        case DCT3D_OPT_QUANT_FORCE_TABLE: c->opt_quant_force = value != 0.0; return DCT3D_OK;
        case DCT3D_OPT_COLOUR:
            if (value != (double)DCT3D_COLOUR_PLANES && value != (double)DCT3D_COLOUR_YCBCR) return DCT3D_EINVAL;
            c->opt_colour = (int)value;
            return DCT3D_OK;
        case DCT3D_OPT_EG_DEC_GROUPS:
            if (value != 0.0 && value != 1.0 && value != 2.0 && value != 4.0 && value != 8.0) return DCT3D_EINVAL;
            c->opt_eg_dec_groups = (int)value;
            return DCT3D_OK;
        default: return DCT3D_EINVAL;
    }
}

int dct3d_ctx_set_chroma(dct3d_ctx* c, int mode) {
    if (!c || (mode != DCT3D_CHROMA_444 && mode != DCT3D_CHROMA_420)) return DCT3D_EINVAL;
    c->chroma = mode;
    return DCT3D_OK;
}

int dct3d_ctx_get_chroma(const dct3d_ctx* c, int* mode) {
    if (!c || !mode) return DCT3D_EINVAL;
    *mode = c->chroma;
    return DCT3D_OK;
}

int dct3d_chroma_size(int w, int h, int* cw, int* ch) {
    if (w <= 0 || h <= 0 || !cw || !ch) return DCT3D_EINVAL;
    *cw = w / 2 + w % 2;
    *ch = h / 2 + h % 2;
    return DCT3D_OK;
}

int dct3d_eg_sync_launches(const dct3d_ctx* c, uint64_t* max_per_front, uint64_t* sum) {
    if (!c || !max_per_front || !sum) return DCT3D_EINVAL;
    *max_per_front = *sum = 0;
    for (uint64_t n : c->egd_launches) {
        *max_per_front = n > *max_per_front ? n : *max_per_front;
        *sum += n;
    }
    return DCT3D_OK;
}

int dct3d_ctx_set_profiling(dct3d_ctx* c, int on) {
    if (!c) return DCT3D_EINVAL;
    c->profiling = on != 0;
    return DCT3D_OK;
}

int dct3d_synchronize(dct3d_ctx* c) {
    if (!c) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    return hipStreamSynchronize(c->stream) == hipSuccess ? DCT3D_OK : DCT3D_EDEVICE;
}

// Resolves the oldest `n` pending timing slots (their events have been recorded on the stream).
static int resolve_timers(dct3d_ctx* c, int n) {
    for (; n > 0 && c->ring_pending > 0; n--) {
        const int slot = (c->ring_head - c->ring_pending + dct3d_ctx::kRing) % dct3d_ctx::kRing;
        hipEvent_t* e = c->ev[slot];
        if (hipEventSynchronize(e[3]) != hipSuccess) return DCT3D_EDEVICE;
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, e[0], e[1]) != hipSuccess || hipEventElapsedTime(&b, e[2], e[3]) != hipSuccess)
            return DCT3D_EDEVICE;
        c->kernel_ms += a;
        c->aux_ms += b;
        c->n_timed++;
        c->ring_pending--;
    }
    return DCT3D_OK;
}

// Returns the event quadruple for this call (or nullptr when profiling is off).
static hipEvent_t* timing_slot(dct3d_ctx* c) {
    if (!c->profiling) return nullptr;
    if (c->ring_pending == dct3d_ctx::kRing && resolve_timers(c, 1)) return nullptr;
    hipEvent_t* e = c->ev[c->ring_head];
    c->ring_head = (c->ring_head + 1) % dct3d_ctx::kRing;
    c->ring_pending++;
    return e;
}
// A call of one launch: events 0-1 bracket it, the second pair brackets nothing.
extern "C++" hipEvent_t* rt::timer_begin(dct3d_ctx* c) {
    hipEvent_t* ev = timing_slot(c);
    if (ev) (void)hipEventRecord(ev[0], c->stream);
    return ev;
}
extern "C++" void rt::timer_end(dct3d_ctx* c, hipEvent_t* ev) {
    if (!ev) return;
    for (int i = 1; i < 4; i++) (void)hipEventRecord(ev[i], c->stream);
}

int dct3d_reset_timers(dct3d_ctx* c) {
    if (!c) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    int rc = resolve_timers(c, dct3d_ctx::kRing);
    c->n_timed = 0;
    c->kernel_ms = c->aux_ms = 0.0;
    return rc;
}

int dct3d_get_stats(dct3d_ctx* c, dct3d_stats* st) {
    if (!c || !st) return DCT3D_EINVAL;
    memset(st, 0, sizeof(*st));
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (resolve_timers(c, dct3d_ctx::kRing)) return DCT3D_EDEVICE;
    st->n_timed = c->n_timed;
    st->kernel_ms_total = c->kernel_ms;
    st->aux_ms_total = c->aux_ms;
    st->n_units = c->last_units;
    if (!c->last_valid || c->last_count_slot < 0) return DCT3D_OK;
    // the call's counter slot (in-wave replays: every replaying path has one)
    std::vector<uint32_t> w(2 * kCountSpread);
    if (hipMemcpyAsync(w.data(), (uint32_t*)c->d_enc_counts.p + c->last_count_slot * 2 * kCountSpread,
                       w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return DCT3D_EDEVICE;
    for (int i = 0; i < kCountSpread; i++) {
        st->n_flagged += w[i];
        st->n_rechecked += w[kCountSpread + i];
    }
    return DCT3D_OK;
}

// ---------------------------------------------------------------------------------------------
// Decode: uncertified cubes are replayed inside the wave; the replay count goes to the ctx's current
// counter slot, and the launch zeroes the other one for the next call (see d_enc_counts).
static void set_count_slot(dct3d_ctx* c, unsigned int*& count, unsigned int*& clear) {
    count = (unsigned int*)c->d_enc_counts.p + c->enc_slot * 2 * kCountSpread;
    clear = (unsigned int*)c->d_enc_counts.p + (c->enc_slot ^ 1) * 2 * kCountSpread;
}
static void set_dec_replay(dct3d_ctx* c, DecodeParams& P) {
    P.inv_coef_t = (const double*)c->d_inv_coef.p;
    set_count_slot(c, P.replay_count, P.replay_clear);
}
// A call's counting kernels are enqueued: its statistics are in enc_slot (units of work: `units`).  The
// slot flips at the end of the call -- of every chunk together inside a host entry point's pipeline
// (batch), and whenever a counting kernel was enqueued, even if a later step of the call failed (the
// next call must start on the slot this one's launches zeroed).
extern "C++" void rt::count_slot_used(dct3d_ctx* c, uint64_t units) {
    c->slot_used = true;
    if (c->batch) {
        c->batch_units += units;
        return;
    }
    c->last_count_slot = c->enc_slot;
    c->enc_slot ^= 1;
    c->slot_used = false;
    c->last_units = units;
    c->last_valid = true;
}
// The start of a call on the device: the last call's statistics no longer stand (inside a host entry point's
// pipeline the call is one chunk of many: batch_begin did it).
extern "C++" void rt::call_begin(dct3d_ctx* c) {
    if (c->batch) return;
    c->last_valid = false;
    c->last_count_slot = -1;
    c->slot_used = false;
}
extern "C++" void rt::batch_begin(dct3d_ctx* c) {
    c->batch = true;
    c->batch_units = 0;
    c->slot_used = false;
    c->last_valid = false;
    c->last_count_slot = -1;
}
extern "C++" void rt::batch_end(dct3d_ctx* c) {
    c->batch = false;
    if (!c->slot_used) return;
    c->last_count_slot = c->enc_slot;
    c->enc_slot ^= 1;
    c->slot_used = false;
    c->last_units = c->batch_units;
    c->last_valid = true;
}

static int forward_f64_raster(dct3d_ctx* c, const uint8_t* d_raster, int w, int h, uint64_t n_cubes, double* d_out) {
    Fwd64Params P;
    P.raster = d_raster;
    P.out = d_out;
    P.n_cubes = (uint32_t)n_cubes;
    P.cubes_per_stack = (uint32_t)((w / 8) * (h / 8));
    P.nbx = (uint32_t)(w / 8);
    P.width = (uint32_t)w;
    P.plane = (uint64_t)w * h;
    P.stack_stride = P.plane * c->bd;
    return launch_fwd64_raster(c->bd, P, c->stream) ? DCT3D_EKERNEL : DCT3D_OK;
}

// The encode and decode kernels' parameters for the cubes [0, n_cubes) of geometry g (packed RGB24: n_cubes
// counts RGB cubes); the address fields: set_address_fields (dct3d_geom.h).
extern "C++" void rt::fill_encode_params(dct3d_ctx* c, EncodeParams& P, const uint8_t* d_raster, int32_t* d_q, const Geom& g,
                               uint64_t n_cubes) {
    memset(&P, 0, sizeof(P));
    P.raster = d_raster;
    P.out = d_q;
    set_address_fields(P, g, c->bd, n_cubes);
    P.coef_dc = c->plan.coef_dc;
    const float* tabs = (const float*)c->d_tabs.p;
    P.tab_rstep = tabs;
    P.tab_G = tabs + kMaxS;
    P.tab_E = tabs + 2 * kMaxS;
    P.ngroups = (const int32_t*)c->d_ngroups.p;
    P.coef = (const double*)c->d_coef.p;
    P.group_of = (const uint8_t*)c->d_group_of.p;
    set_count_slot(c, P.replay_count, P.replay_clear);
    P.tab64 = (const double*)c->d_tabs64.p;
    P.recheck = c->opt_enc_no_recheck ? 0u : 1u;
}
extern "C++" void rt::fill_decode_params(dct3d_ctx* c, DecodeParams& P, const int32_t* d_q, uint8_t* d_raster, const Geom& g,
                               uint64_t n_cubes) {
    P.in = d_q;
    P.out = d_raster;
    set_address_fields(P, g, c->bd, n_cubes);
    P.cube_base = 0;
    P.dec_G = c->plan.dec_G;
    P.dec_E = c->plan.dec_E;
    P.dec_l1_max = c->plan.dec_l1_max;
    P.blk_store = blk_store(g, c->bd);
    // test option: widen the certification margin so that most pixels are uncertified and their cubes
    // take the whole-cube replay path (tests/test_gpu_parity.py); a wider margin is never unsafe
    P.dec_E += c->opt_dec_margin;
    set_dec_replay(c, P);
}

// ---- int32 cubes <-> raster on the device: grey or packed RGB24 (dct3d.h, ABI 9: over the RGB cubes, each
//      three cubes of the int32 side [stack][channel][cube]), multiples of 8 or frames of any size (Geom) ----
// the arguments every raster call shares, and its geometry
static int check_args(const dct3d_ctx* c, const void* a, const void* b, int w, int h, int px, int n_stacks, bool any_size,
                      Geom* g, uint64_t* n_cubes) {
    if (!c || ((!a || !b) && n_stacks) || colour_refused(c, px)) return DCT3D_EINVAL;
    return make_geom(w, h, px, n_stacks, any_size, g, n_cubes) ? DCT3D_OK : DCT3D_EINVAL;
}

// One launch; uncertified coefficients are replayed inside the wave (exact Java fold).
static int encode_dev(dct3d_ctx* c, const uint8_t* d_raster, const Geom& g, uint64_t n_cubes, int32_t* d_q, double* d_dct) {
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    call_begin(c);
    if (n_cubes == 0) return DCT3D_OK;
    EncodeParams P;
    fill_encode_params(c, P, d_raster, d_q, g, n_cubes);
    hipEvent_t* ev = timer_begin(c);
    if (launch_encode(variant_of(c, g), P, c->stream)) return DCT3D_EKERNEL;
    timer_end(c, ev);
    count_slot_used(c, (uint64_t)g.px * n_cubes * (uint64_t)c->plan.cs);
    if (d_dct) return forward_f64_raster(c, d_raster, g.w, g.h, n_cubes, d_dct);
    return DCT3D_OK;
}

static int decode_dev(dct3d_ctx* c, const int32_t* d_q, const Geom& g, uint64_t n_cubes, uint8_t* d_raster) {
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    call_begin(c);
    if (n_cubes == 0) return DCT3D_OK;
    DecodeParamsQ P;  // (the product kernels take its DecodeParams part)
    fill_decode_params(c, P, d_q, d_raster, g, n_cubes);
    P.steps = qt_steps(c);
    hipEvent_t* ev = timer_begin(c);
    if (launch_decode(variant_of(c, g), P, c->stream)) return DCT3D_EKERNEL;
    timer_end(c, ev);
    count_slot_used(c, (uint64_t)g.px * n_cubes * (uint64_t)c->plan.cs);
    return DCT3D_OK;
}

int dct3d_encode_stacks_dev(dct3d_ctx* c, const uint8_t* d_raster, int w, int h, int n_stacks, int32_t* d_q,
                            double* d_dct) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, d_raster, d_q, w, h, 1, n_stacks, false, &g, &n_cubes);
    return rc ? rc : encode_dev(c, d_raster, g, n_cubes, d_q, d_dct);
}

int dct3d_decode_stacks_dev(dct3d_ctx* c, const int32_t* d_q, int w, int h, int n_stacks, uint8_t* d_raster) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, d_q, d_raster, w, h, 1, n_stacks, false, &g, &n_cubes);
    return rc ? rc : decode_dev(c, d_q, g, n_cubes, d_raster);
}

int dct3d_encode_stacks_rgb_dev(dct3d_ctx* c, const uint8_t* d_rgb, int w, int h, int n_stacks, int32_t* d_q) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, d_rgb, d_q, w, h, 3, n_stacks, false, &g, &n_cubes);
    return rc ? rc : encode_dev(c, d_rgb, g, n_cubes, d_q, nullptr);
}

int dct3d_decode_stacks_rgb_dev(dct3d_ctx* c, const int32_t* d_q, int w, int h, int n_stacks, uint8_t* d_rgb) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, d_q, d_rgb, w, h, 3, n_stacks, false, &g, &n_cubes);
    return rc ? rc : decode_dev(c, d_q, g, n_cubes, d_rgb);
}

// frames of any size: a geometry that is a multiple of 8 both ways is the *_stacks* call's, the very same kernels
int dct3d_encode_frames_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int channels, int n_stacks,
                            int32_t* d_q) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, d_frames, d_q, w, h, channels, n_stacks, true, &g, &n_cubes);
    return rc ? rc : encode_dev(c, d_frames, g, n_cubes, d_q, nullptr);
}

int dct3d_decode_frames_dev(dct3d_ctx* c, const int32_t* d_q, int w, int h, int channels, int n_stacks,
                            uint8_t* d_frames) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, d_q, d_frames, w, h, channels, n_stacks, true, &g, &n_cubes);
    return rc ? rc : decode_dev(c, d_q, g, n_cubes, d_frames);
}

// ---- host-pointer pipeline ------------------------------------------------------
// The host entry points move whole stacks in chunks: chunk i's upload (copy stream s_up, issued here),
// its kernels (the context stream, after the upload's event) and its download (copy stream s_down,
// issued by a helper thread: a D2H copy into pageable memory blocks the thread that issues it) overlap
// with chunk i+1's upload and chunk i-1's download.  PCIe is full duplex (~57 GB/s each way measured,
// pinned or pageable), so a call approaches max(in, out) / link rate instead of (in + out) / rate.
// Two device slots per direction; chunk i reuses slot i & 1 after chunk i-2's kernels (event) and
// download (the helper has returned from it) are done.  Synchronous on return, like the reference.
}  // extern "C" (the pipeline helpers are C++ templates)
static int ensure_pipe(dct3d_ctx* c) {
    if (c->s_up) return DCT3D_OK;
    if (hipStreamCreateWithFlags(&c->s_up, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->s_down, hipStreamNonBlocking) != hipSuccess)
        return DCT3D_EDEVICE;
    for (int i = 0; i < 2; i++)
        if (hipEventCreateWithFlags(&c->pe_in[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->pe_done[i], hipEventDisableTiming) != hipSuccess)
            return DCT3D_EDEVICE;
    return DCT3D_OK;
}

static int chunk_stacks_for(size_t bytes_per_stack, int n_stacks) {
    // ~64 MB per chunk on the heavier side, at least 1 stack, at most n_stacks / 2 (some overlap)
    size_t k = (64u << 20) / (bytes_per_stack ? bytes_per_stack : 1);
    if (k < 1) k = 1;
    const int half = n_stacks > 1 ? (n_stacks + 1) / 2 : 1;
    return (int)(k < (size_t)half ? k : (size_t)half);
}

// compute(d_in, d_out, first_stack, stacks) enqueues one chunk's kernels on c->stream; align: chunks of a
// multiple of this many stacks (the last one ragged)
template <class Compute>
static int run_pipeline(dct3d_ctx* c, int n_stacks, size_t in_per_stack, size_t out_per_stack, const void* host_in,
                        void* host_out, Compute&& compute, int align = 1) {
    int rc = ensure_pipe(c);
    if (rc) return rc;
    int cst = chunk_stacks_for(in_per_stack > out_per_stack ? in_per_stack : out_per_stack, n_stacks);
    cst = (cst + align - 1) / align * align;
    const int n_chunks = (n_stacks + cst - 1) / cst;
    for (int s = 0; s < 2; s++)
        if ((in_per_stack && (rc = c->p_in[s].grow(cst * in_per_stack))) || (rc = c->p_out[s].grow(cst * out_per_stack)))
            return rc;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<int> todo;
    int downloaded = 0;  // chunks whose download has completed
    bool closing = false, failed = false;
    std::thread helper([&] {
        if (hipSetDevice(c->device) != hipSuccess) {
            std::lock_guard<std::mutex> lk(mu);
            failed = true;
        }
        for (;;) {
            int i;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !todo.empty() || closing; });
                if (todo.empty()) return;
                i = todo.front();
                todo.pop_front();
            }
            const int s = i & 1, st0 = i * cst, ns = (st0 + cst <= n_stacks) ? cst : n_stacks - st0;
            bool ok = !failed && hipStreamWaitEvent(c->s_down, c->pe_done[s], 0) == hipSuccess &&
                      hipMemcpyAsync((char*)host_out + (size_t)st0 * out_per_stack, c->p_out[s].p, ns * out_per_stack,
                                     hipMemcpyDeviceToHost, c->s_down) == hipSuccess &&
                      hipStreamSynchronize(c->s_down) == hipSuccess;
            {
                std::lock_guard<std::mutex> lk(mu);
                if (!ok) failed = true;
                downloaded++;
            }
            cv.notify_all();
        }
    });
    for (int i = 0; i < n_chunks && rc == DCT3D_OK; i++) {
        const int s = i & 1, st0 = i * cst, ns = (st0 + cst <= n_stacks) ? cst : n_stacks - st0;
        if (host_in) {  // (no upload when the input is already on the device)
            if (i >= 2 && hipStreamWaitEvent(c->s_up, c->pe_done[s], 0) != hipSuccess) rc = DCT3D_EDEVICE;
            if (!rc && (hipMemcpyAsync(c->p_in[s].p, (const char*)host_in + (size_t)st0 * in_per_stack,
                                       ns * in_per_stack, hipMemcpyHostToDevice, c->s_up) != hipSuccess ||
                        hipEventRecord(c->pe_in[s], c->s_up) != hipSuccess ||
                        hipStreamWaitEvent(c->stream, c->pe_in[s], 0) != hipSuccess))
                rc = DCT3D_EDEVICE;
        }
        {  // slot s's previous download (chunk i - 2) must be finished before its kernels overwrite it
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return downloaded >= i - 1 || failed; });
            if (failed) rc = DCT3D_EDEVICE;
        }
        if (!rc) rc = compute(c->p_in[s].p, c->p_out[s].p, st0, ns);
        if (!rc && hipEventRecord(c->pe_done[s], c->stream) != hipSuccess) rc = DCT3D_EDEVICE;
        if (!rc) {
            std::lock_guard<std::mutex> lk(mu);
            todo.push_back(i);
        }
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        closing = true;
    }
    cv.notify_all();
    helper.join();
    if (failed && !rc) rc = DCT3D_EDEVICE;
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = DCT3D_EDEVICE;
    return rc;
}

extern "C" {
// ---- host-pointer entry points (synchronous; the reference's blocking transfers) ----------------
// Chunks of whole stacks (contiguous on both sides) through the pipeline; the copies of the raster side move
// the unpadded frames' bytes only.  Every chunk counts into one slot: dct3d_get_stats reports the whole call.
static int host_stacks(dct3d_ctx* c, bool encode, const void* in, void* out, const Geom& g, int n_stacks, uint64_t n_cubes) {
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (n_cubes == 0) return DCT3D_OK;
    const size_t raster_ps = (size_t)g.plane() * c->bd;                                     // bytes per stack
    const size_t q_ps = (size_t)g.px * g.cps() * c->plan.cs * sizeof(int32_t);
    batch_begin(c);
    const int rc = run_pipeline(c, n_stacks, encode ? raster_ps : q_ps, encode ? q_ps : raster_ps, in, out,
                                [&](const void* din, void* dout, int, int ns) {
                                    const uint64_t n = g.cps() * (uint64_t)ns;
                                    return encode ? encode_dev(c, (const uint8_t*)din, g, n, (int32_t*)dout, nullptr)
                                                  : decode_dev(c, (const int32_t*)din, g, n, (uint8_t*)dout);
                                });
    batch_end(c);
    return rc;
}

int dct3d_encode_stacks(dct3d_ctx* c, const uint8_t* raster, int w, int h, int n_stacks, int32_t* q, double* dct) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, raster, q, w, h, 1, n_stacks, false, &g, &n_cubes);
    if (rc) return rc;
    if (!dct) return host_stacks(c, true, raster, q, g, n_stacks, n_cubes);
    // with the fp64 coefficients: unpipelined, whole buffers
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (n_cubes == 0) return DCT3D_OK;
    const size_t in_bytes = n_cubes * c->plan.cs, out_bytes = in_bytes * sizeof(int32_t);
    if ((rc = c->h_in.grow(in_bytes)) || (rc = c->h_out.grow(out_bytes))) return rc;
    if (hipMemcpyAsync(c->h_in.p, raster, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return DCT3D_EDEVICE;
    if ((rc = c->h_aux.grow(in_bytes * sizeof(double)))) return rc;
    if ((rc = encode_dev(c, (const uint8_t*)c->h_in.p, g, n_cubes, (int32_t*)c->h_out.p, (double*)c->h_aux.p))) return rc;
    if (hipMemcpyAsync(dct, c->h_aux.p, in_bytes * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        return DCT3D_EDEVICE;
    if (hipMemcpyAsync(q, c->h_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return DCT3D_EDEVICE;
    return hipStreamSynchronize(c->stream) == hipSuccess ? DCT3D_OK : DCT3D_EDEVICE;
}

int dct3d_decode_stacks(dct3d_ctx* c, const int32_t* q, int w, int h, int n_stacks, uint8_t* raster) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, q, raster, w, h, 1, n_stacks, false, &g, &n_cubes);
    return rc ? rc : host_stacks(c, false, q, raster, g, n_stacks, n_cubes);
}

int dct3d_encode_stacks_rgb(dct3d_ctx* c, const uint8_t* rgb, int w, int h, int n_stacks, int32_t* q) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, rgb, q, w, h, 3, n_stacks, false, &g, &n_cubes);
    return rc ? rc : host_stacks(c, true, rgb, q, g, n_stacks, n_cubes);
}

int dct3d_decode_stacks_rgb(dct3d_ctx* c, const int32_t* q, int w, int h, int n_stacks, uint8_t* rgb) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, q, rgb, w, h, 3, n_stacks, false, &g, &n_cubes);
    return rc ? rc : host_stacks(c, false, q, rgb, g, n_stacks, n_cubes);
}

int dct3d_encode_frames(dct3d_ctx* c, const uint8_t* frames, int w, int h, int channels, int n_stacks, int32_t* q) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, frames, q, w, h, channels, n_stacks, true, &g, &n_cubes);
    return rc ? rc : host_stacks(c, true, frames, q, g, n_stacks, n_cubes);
}

int dct3d_decode_frames(dct3d_ctx* c, const int32_t* q, int w, int h, int channels, int n_stacks, uint8_t* frames) {
    Geom g;
    uint64_t n_cubes;
    int rc = check_args(c, q, frames, w, h, channels, n_stacks, true, &g, &n_cubes);
    return rc ? rc : host_stacks(c, false, q, frames, g, n_stacks, n_cubes);
}

// ---- drop-in (A): float cube-major <-> float cube-major --------------------------------------
// one launch of the float kernel, timed like the fused kernels when profiling is on (no auxiliary launch:
// the second event pair brackets nothing)
static int cube_f32_dev(dct3d_ctx* c, const float* d_in, size_t n_cubes, float* d_out, bool inverse) {
    if (!c || (n_cubes && (!d_in || !d_out)) || n_cubes >= (1ull << 31) / 8) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (!n_cubes) return DCT3D_OK;
    hipEvent_t* ev = timer_begin(c);
    if (launch_cube_f32(c->bd, inverse, d_in, d_out, (uint32_t)n_cubes, c->stream)) return DCT3D_EKERNEL;
    timer_end(c, ev);
    c->last_units = n_cubes * (uint64_t)c->plan.cs;
    c->last_valid = false;  // no flag counters for the float path
    c->last_count_slot = -1;
    return DCT3D_OK;
}

int dct3d_forward_f32_dev(dct3d_ctx* c, const float* d_in, size_t n_cubes, float* d_out) {
    return cube_f32_dev(c, d_in, n_cubes, d_out, false);
}

int dct3d_inverse_f32_dev(dct3d_ctx* c, const float* d_in, size_t n_cubes, float* d_out) {
    return cube_f32_dev(c, d_in, n_cubes, d_out, true);
}

static int cube_f32_host(dct3d_ctx* c, const float* in, size_t n_cubes, float* out, bool inverse) {
    if (!c || (n_cubes && (!in || !out)) || n_cubes >= (1ull << 31) / 8) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (!n_cubes) return DCT3D_OK;
    const size_t bytes = n_cubes * c->plan.cs * sizeof(float);
    int rc;
    if ((rc = c->h_in.grow(bytes)) || (rc = c->h_out.grow(bytes))) return rc;
    if (hipMemcpyAsync(c->h_in.p, in, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return DCT3D_EDEVICE;
    if (launch_cube_f32(c->bd, inverse, (const float*)c->h_in.p, (float*)c->h_out.p, (uint32_t)n_cubes, c->stream))
        return DCT3D_EKERNEL;
    if (hipMemcpyAsync(out, c->h_out.p, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return DCT3D_EDEVICE;
    return hipStreamSynchronize(c->stream) == hipSuccess ? DCT3D_OK : DCT3D_EDEVICE;
}

int dct3d_forward_f32(dct3d_ctx* c, const float* in, size_t n_cubes, float* out) {
    return cube_f32_host(c, in, n_cubes, out, false);
}

int dct3d_inverse_f32(dct3d_ctx* c, const float* in, size_t n_cubes, float* out) {
    return cube_f32_host(c, in, n_cubes, out, true);
}

// ---- Exp-Golomb stage ----------------------------------------------------------------------------
int dct3d_diagonal_order(int bw, int bh, int bd, uint16_t* out) {
    if (!out || bw != 8 || bh != 8 || (bd != 8 && bd != 4)) return DCT3D_EINVAL;
    diagonal_order(bw, bh, bd, out);
    return DCT3D_OK;
}

static int eg_run(dct3d_ctx* c, const int32_t* d_q, uint64_t n_cubes, uint8_t carry_byte, int carry_bits,
                  uint32_t* d_out, uint64_t out_cap, uint64_t* total_bits) {
    const uint64_t n_chunks = (n_cubes + 4095) / 4096;
    int rc = c->d_eg_bits.grow(n_cubes * sizeof(uint32_t));
    if (!rc) rc = c->d_eg_off.grow(n_cubes * sizeof(uint64_t));
    if (!rc) rc = c->d_eg_bsum.grow((n_chunks + 1) * sizeof(uint64_t));
    if (!rc) rc = c->d_eg_ht.grow(2 * n_cubes * sizeof(uint32_t));
    if (rc) return rc;
    uint64_t* const sw = eg_status_begin(c, &rc);
    if (rc) return rc;
    EgParams P{};
    P.q = d_q;
    P.n_cubes = n_cubes;
    P.diag = (const uint16_t*)c->d_diag.p;
    P.bits = (uint32_t*)c->d_eg_bits.p;
    P.off = (uint64_t*)c->d_eg_off.p;
    P.bsum = (uint64_t*)c->d_eg_bsum.p;
    P.status = sw;
    eg_status_handoff(c, P);  // the stitch kernel (the last of launch_eg_encode) hands the words over
    P.head = (uint32_t*)c->d_eg_ht.p;
    P.tail = (uint32_t*)c->d_eg_ht.p + n_cubes;
    P.out = d_out;
    P.out_cap_words = out_cap / 4;
    P.carry_bits = (uint32_t)carry_bits;
    P.carry_byte = carry_byte;
    if (launch_eg_encode(c->bd, P, c->stream)) return DCT3D_EKERNEL;
    uint64_t st[2] = {0, 0};
    if (eg_status_end(c, true, sw, st, P.seq)) return DCT3D_EDEVICE;
    if (total_bits) *total_bits = st[0];
    if (st[1] & 2) return DCT3D_EINVAL;
    if (st[1] & 1) return DCT3D_ENOSPC;
    return DCT3D_OK;
}

int dct3d_eg_encode_dev(dct3d_ctx* c, const int32_t* d_q, uint64_t n_cubes, uint8_t carry_byte, int carry_bits,
                        uint8_t* d_out, uint64_t out_cap, uint64_t* total_bits) {
    if (!c || carry_bits < 0 || carry_bits > 7 || (n_cubes && (!d_q || !d_out)) || ((uintptr_t)d_out & 3))
        return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (n_cubes == 0) {
        if (total_bits) *total_bits = (uint64_t)carry_bits;
        if (carry_bits == 0) return DCT3D_OK;
        if (out_cap < 4) return DCT3D_ENOSPC;
        const uint32_t w = carry_byte & (0xFF00u >> carry_bits);
        return hipMemcpy(d_out, &w, 4, hipMemcpyHostToDevice) == hipSuccess ? DCT3D_OK : DCT3D_EDEVICE;
    }
    return eg_run(c, d_q, n_cubes, carry_byte, carry_bits, (uint32_t*)d_out, out_cap, total_bits);
}

// 4:2:0: the encode kernels' cube fields from the chroma plane gc, their address fields (set_address_fields did
// them) from the frames g, the height set whatever the edge (c420_row8 clamps by it)
extern "C++" void rt::c420_cube_fields(EncodeParams& P, const Geom& g, const Geom& gc) {
    P.cubes_per_stack = (uint32_t)gc.cps();
    P.nbx = (uint32_t)(gc.wp / 8);
    P.div_cps = fast_div(P.cubes_per_stack);
    P.div_nbx = fast_div(P.nbx);
    P.height = (uint32_t)g.h;
}
// the chroma loader's edge: a width or a height that is no multiple of 16
extern "C++" int rt::c420_edge(const Geom& g) { return g.w % 16 || g.h % 16 ? 1 : 0; }

// One fused launch chain on the context stream: encode_eg_kernel (transform, quantise, in-wave exact replay,
// lane-level Exp-Golomb into slots) -> scan over segments -> eg_compact_kernel -> eg_stitch_kernel, for
// channel ch of the n_cubes cubes of d_raster.  Returns once *total_bits is known.  A packed RGB24 call runs
// one chain per channel back to back, reusing the slot, bits, offset and head / tail buffers.
// gc (4:2:0, ch = 1 | 2): the chroma plane's geometry, n_cubes its cubes; the kernel reads the frames of g.
static int encode_eg_chain(dct3d_ctx* c, const uint8_t* d_raster, const Geom& g, int ch, uint64_t n_cubes,
                           uint8_t carry_byte, int carry_bits, uint8_t* d_out, uint64_t out_cap, uint64_t* total_bits,
                           const Geom* gc = nullptr) {
    const bool plain = g.px == 1 && !g.edge();  // dct3d_encode_eg_dev's geometry: its kernel
    int rc;
    const uint64_t n_seg = (n_cubes + 7) / 8, n_chunks = (n_seg + 4095) / 4096;
    // worst case per lane: cs/8 values x 27 bits (|q| <= 255 sqrt(cs) -> codes <= 27 bits)
    const uint32_t seg_cap = (uint32_t)(64 * (((c->plan.cs / 8) * 27 + 31) / 32));
    // two passes: K1 codes into per-segment slots, then scan + compaction (a single pass by decoupled
    // look-back wrote the same stream but measured slower: DESIGN.md §4b)
    if ((rc = c->d_egf_slot.grow(n_seg * seg_cap * sizeof(uint32_t))) ||
        (rc = c->d_eg_bits.grow(n_seg * sizeof(uint32_t))) ||
        (rc = c->d_eg_off.grow(n_seg * sizeof(uint64_t))) || (rc = c->d_eg_bsum.grow((n_chunks + 1) * sizeof(uint64_t))) ||
        (rc = c->d_eg_ht.grow(2 * n_seg * sizeof(uint32_t))))
        return rc;
    uint64_t* const sw = eg_status_begin(c, &rc);
    if (rc) return rc;
    EncodeParams P;  // no int32 output; the replay tables travel in E
    fill_encode_params(c, P, d_raster, nullptr, g, n_cubes);
    if (gc) c420_cube_fields(P, g, *gc);
    // (the new geometries' kernels count their exact replays; dct3d_encode_eg_dev's reports none)
    if (plain) P.replay_count = P.replay_clear = nullptr;
    EgFusedParams E;
    E.ch = ch;
    E.ngroups = (const int32_t*)c->d_ngroups.p;
    E.coef = (const double*)c->d_coef.p;
    E.group_of = (const uint8_t*)c->d_group_of.p;
    E.diag = (const uint16_t*)c->d_diag.p;
    E.slot = (uint32_t*)c->d_egf_slot.p;
    E.seg_cap = seg_cap;
    E.seg_bits = (uint32_t*)c->d_eg_bits.p;
    EgParams G{};
    G.q = nullptr;
    G.n_cubes = n_seg;  // segments
    G.diag = E.diag;
    G.bits = E.seg_bits;
    G.off = (uint64_t*)c->d_eg_off.p;
    G.bsum = (uint64_t*)c->d_eg_bsum.p;
    G.status = sw;
    eg_status_handoff(c, G);  // the stitch kernel (the last of launch_eg_compact) hands the words over
    // (Round 6: handed over by the compaction's block 0 instead, the call returning while the compaction and
    // the stitch ran, the compaction slowed 151 -> 205 us beside the next call's launches: c7 +15-25 us per
    // call, profiles/r06/gaps/async7.  The stream decode's consumer, compute-bound, does not slow.)
    G.head = (uint32_t*)c->d_eg_ht.p;
    G.tail = (uint32_t*)c->d_eg_ht.p + n_seg;
    G.out = (uint32_t*)d_out;
    G.out_cap_words = out_cap / 4;
    G.carry_bits = (uint32_t)carry_bits;
    G.carry_byte = carry_byte;
    uint64_t st[2] = {0, 0};
    hipEvent_t* ev = timer_begin(c);  // events 0-1 bracket K1, 2-3 the compaction
    const Variant v = stream_variant_of(c, g);
    const VqParams* const vq = c->vq ? &c->vq_ch[ch] : nullptr;  // channel ch's map column
    if (gc ? launch_encode_eg_c420(v.D, c420_edge(g), v.qt, P, E, vq, c->stream) : launch_encode_eg(v, P, E, vq, c->stream))
        return DCT3D_EKERNEL;
    if (!plain) c->slot_used = true;  // (the call flips the counter slot: count_slot_used)
    if (ev) (void)hipEventRecord(ev[1], c->stream);
    if (ev) (void)hipEventRecord(ev[2], c->stream);
    if (launch_eg_compact(G, E.slot, seg_cap, c->stream)) return DCT3D_EKERNEL;
    if (ev) (void)hipEventRecord(ev[3], c->stream);
    if (eg_status_end(c, true, sw, st, G.seq)) return DCT3D_EDEVICE;
    if (total_bits) *total_bits = st[0];
    c->last_units = n_cubes * (uint64_t)c->plan.cs;
    if (st[1] & 1) return DCT3D_ENOSPC;
    return DCT3D_OK;
}

// Fused device path, grey frames whose width and height are multiples of 8.
int dct3d_encode_eg_dev(dct3d_ctx* c, const uint8_t* d_raster, int w, int h, int n_stacks, uint8_t carry_byte,
                        int carry_bits, uint8_t* d_out, uint64_t out_cap, uint64_t* total_bits) {
    if (!c || (!d_raster && n_stacks) || carry_bits < 0 || carry_bits > 7 || ((uintptr_t)d_out & 3)) return DCT3D_EINVAL;
    Geom g;
    uint64_t n_cubes;
    if (!make_geom(w, h, 1, n_stacks, false, &g, &n_cubes)) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    call_begin(c);
    if (n_cubes == 0) return dct3d_eg_encode_dev(c, nullptr, 0, carry_byte, carry_bits, d_out, out_cap, total_bits);
    if (!d_out) return DCT3D_EINVAL;
    return encode_eg_chain(c, d_raster, g, 0, n_cubes, carry_byte, carry_bits, d_out, out_cap, total_bits);
}

// channel ch's host-call stream buffer on the device, and the bytes the last call left there
static DevBuf& eg_out_buf(dct3d_ctx* c, int ch) { return ch == 0 ? c->d_eg_out : c->d_eg_out_x[ch - 1]; }
static uint64_t& eg_last_bytes(dct3d_ctx* c, int ch) { return ch == 0 ? c->eg_last_bytes : c->eg_last_bytes_x[ch - 1]; }
}  // extern "C"
// run(outs, caps) codes n_ch streams into the buffers of channels ch0 .. ch0 + n_ch - 1 and sets their tb[]: first
// with room for 8 bits per value (cap; typical content needs 1.5-4), on DCT3D_ENOSPC grown to fit and run again
template <class Run>
static int eg_run_to_fit(dct3d_ctx* c, int ch0, int n_ch, uint64_t first_cap, const uint64_t* tb, Run&& run) {
    uint64_t cap[3] = {first_cap, first_cap, first_cap};
    uint8_t* outs[3] = {nullptr, nullptr, nullptr};
    int rc = DCT3D_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
        for (int i = 0; i < n_ch; i++) {
            DevBuf& b = eg_out_buf(c, ch0 + i);
            if ((rc = b.grow(cap[i]))) return rc;
            outs[i] = (uint8_t*)b.p;
            cap[i] = b.bytes;
        }
        rc = run(outs, cap);
        if (rc != DCT3D_ENOSPC) break;
        for (int i = 0; i < n_ch; i++) cap[i] = (tb[i] + 31) / 32 * 4 + 64;
    }
    return rc;
}
extern "C" {

int dct3d_encode_eg(dct3d_ctx* c, const uint8_t* raster, int w, int h, int n_stacks, uint8_t carry_byte,
                    int carry_bits, uint64_t* total_bits) {
    if (!c || (!raster && n_stacks) || carry_bits < 0 || carry_bits > 7) return DCT3D_EINVAL;
    Geom g;
    uint64_t n_cubes;
    if (!make_geom(w, h, 1, n_stacks, false, &g, &n_cubes)) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    c->eg_last_bytes = c->eg_last_bytes_x[0] = c->eg_last_bytes_x[1] = 0;
    const size_t in_bytes = n_cubes * c->plan.cs;
    int rc;
    if ((rc = c->h_in.grow(in_bytes ? in_bytes : 1)) || (rc = c->d_eg_q.grow((in_bytes ? in_bytes : 1) * sizeof(int32_t))))
        return rc;
    if (n_cubes && hipMemcpyAsync(c->h_in.p, raster, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return DCT3D_EDEVICE;
    // A/B option: int32 cube-major, then the stand-alone EG stage
    const bool two_step = c->opt_eg_two_step && n_cubes;
    if (two_step && (rc = encode_dev(c, (const uint8_t*)c->h_in.p, g, n_cubes, (int32_t*)c->d_eg_q.p, nullptr))) return rc;
    uint64_t tb = 0;
    rc = eg_run_to_fit(c, 0, 1, in_bytes + 64, &tb, [&](uint8_t* const* outs, const uint64_t* caps) {
        return two_step ? eg_run(c, (const int32_t*)c->d_eg_q.p, n_cubes, carry_byte, carry_bits, (uint32_t*)outs[0], caps[0], &tb)
                        : dct3d_encode_eg_dev(c, (const uint8_t*)c->h_in.p, w, h, n_stacks, carry_byte, carry_bits, outs[0],
                                              caps[0], &tb);
    });
    if (rc) return rc;
    if (total_bits) *total_bits = tb;
    c->eg_last_bytes = (tb + 7) / 8;
    return DCT3D_OK;
}

// the bytes of channel `channel`'s stream that the last host stream encode left on the device
int dct3d_eg_fetch_channel(dct3d_ctx* c, int channel, uint8_t* out, uint64_t nbytes) {
    if (!c || channel < 0 || channel > 2) return DCT3D_EINVAL;
    if ((nbytes && !out) || nbytes > eg_last_bytes(c, channel)) return DCT3D_EINVAL;
    if (nbytes == 0) return DCT3D_OK;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (hipMemcpyAsync(out, eg_out_buf(c, channel).p, nbytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return DCT3D_EDEVICE;
    return DCT3D_OK;
}

int dct3d_eg_fetch(dct3d_ctx* c, uint8_t* out, uint64_t nbytes) { return dct3d_eg_fetch_channel(c, 0, out, nbytes); }

// ---- frames of any size and packed RGB24 -> one Exp-Golomb stream per channel (dct3d.h) ----
// (grey at multiples of 8: the call hands over to the grey one)
static bool eg_aligned(const Geom& g) { return g.px == 1 && !g.edge(); }

int dct3d_encode_eg_frames_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int channels, int n_stacks,
                               const uint8_t carry_byte[], const int carry_bits[], uint8_t* const d_out[],
                               const uint64_t out_cap[], uint64_t total_bits[]) {
    Geom g;
    uint64_t n_cubes;
    if (!c || !make_geom(w, h, channels, n_stacks, true, &g, &n_cubes)) return DCT3D_EINVAL;
    if (!carry_byte || !carry_bits || !d_out || !out_cap || !total_bits) return DCT3D_EINVAL;
    if (c->opt_eg_two_step && colour_refused(c, channels)) return DCT3D_EINVAL;  // the int32 intermediate has no colour stage
    Geom gc = g;
    uint64_t nc[3] = {n_cubes, n_cubes, n_cubes};  // cubes per channel (4:2:0: the chroma planes')
    const bool c420 = c420_on(c, channels);
    if (c420_refused(c, channels) || (c420 && !c420_geom(g, n_stacks, &gc, &nc[1]))) return DCT3D_EINVAL;
    nc[2] = nc[1];
    if (eg_aligned(g))
        return dct3d_encode_eg_dev(c, d_frames, w, h, n_stacks, carry_byte[0], carry_bits[0], d_out[0], out_cap[0], total_bits);
    if (!d_frames && n_stacks) return DCT3D_EINVAL;
    for (int ch = 0; ch < channels; ch++)
        if (carry_bits[ch] < 0 || carry_bits[ch] > 7 || ((uintptr_t)d_out[ch] & 3) || (n_cubes && !d_out[ch])) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    call_begin(c);
    int rc, first = DCT3D_OK;  // every channel runs (each total_bits[ch] is set); the first error is returned
    for (int ch = 0; ch < channels; ch++) {
        total_bits[ch] = 0;
        rc = n_cubes ? encode_eg_chain(c, d_frames, g, ch, nc[ch], carry_byte[ch], carry_bits[ch], d_out[ch], out_cap[ch], &total_bits[ch],
                                       c420 && ch ? &gc : nullptr)
                     : dct3d_eg_encode_dev(c, nullptr, 0, carry_byte[ch], carry_bits[ch], d_out[ch], out_cap[ch], &total_bits[ch]);
        if (rc && !first) first = rc;
        if (rc && rc != DCT3D_ENOSPC) break;
    }
    if (c->slot_used) count_slot_used(c, (channels == 3 ? nc[0] + nc[1] + nc[2] : n_cubes) * (uint64_t)c->plan.cs);
    return first;
}

int dct3d_encode_eg_frames(dct3d_ctx* c, const uint8_t* frames, int w, int h, int channels, int n_stacks,
                           const uint8_t carry_byte[], const int carry_bits[], uint64_t total_bits[]) {
    Geom g;
    uint64_t n_cubes;
    if (!c || !make_geom(w, h, channels, n_stacks, true, &g, &n_cubes)) return DCT3D_EINVAL;
    if (!carry_byte || !carry_bits || !total_bits) return DCT3D_EINVAL;
    if (c->opt_eg_two_step && colour_refused(c, channels)) return DCT3D_EINVAL;
    if (c420_refused(c, channels)) return DCT3D_EINVAL;
    if (eg_aligned(g)) return dct3d_encode_eg(c, frames, w, h, n_stacks, carry_byte[0], carry_bits[0], total_bits);
    if (!frames && n_stacks) return DCT3D_EINVAL;
    for (int ch = 0; ch < channels; ch++)
        if (carry_bits[ch] < 0 || carry_bits[ch] > 7) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    c->eg_last_bytes = c->eg_last_bytes_x[0] = c->eg_last_bytes_x[1] = 0;
    const size_t in_bytes = (size_t)g.plane() * c->bd * n_stacks;  // the unpadded frames: one copy
    const size_t ch_vals = n_cubes * c->plan.cs;                   // values of one channel
    int rc;
    if ((rc = c->h_in.grow(in_bytes ? in_bytes : 1))) return rc;
    if (in_bytes && hipMemcpyAsync(c->h_in.p, frames, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return DCT3D_EDEVICE;
    uint64_t tb[3] = {0, 0, 0};
    if (!c->opt_eg_two_step || n_cubes == 0) {
        rc = eg_run_to_fit(c, 0, channels, ch_vals + 64, tb, [&](uint8_t* const* outs, const uint64_t* caps) {
            return dct3d_encode_eg_frames_dev(c, (const uint8_t*)c->h_in.p, w, h, channels, n_stacks, carry_byte, carry_bits,
                                              outs, caps, tb);
        });
        if (rc) return rc;
    } else {
        // A/B option: the int32 cubes ([stack][channel][cube]), then the stand-alone Exp-Golomb stage over each
        // channel's blocks (gathered: they lie 3 blocks apart)
        const size_t blk = (size_t)g.cps() * c->plan.cs * sizeof(int32_t);  // one (stack, channel) block
        if ((rc = c->d_eg_q.grow(channels * ch_vals * sizeof(int32_t))) ||
            (channels == 3 && (rc = c->d_eg_q_ch.grow(ch_vals * sizeof(int32_t)))))
            return rc;
        if ((rc = encode_dev(c, (const uint8_t*)c->h_in.p, g, n_cubes, (int32_t*)c->d_eg_q.p, nullptr))) return rc;
        for (int ch = 0; ch < channels; ch++) {
            const int32_t* q = (const int32_t*)c->d_eg_q.p;
            if (channels == 3) {
                if (hipMemcpy2DAsync(c->d_eg_q_ch.p, blk, (const char*)c->d_eg_q.p + ch * blk, 3 * blk, blk, (size_t)n_stacks,
                                     hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                    return DCT3D_EDEVICE;
                q = (const int32_t*)c->d_eg_q_ch.p;
            }
            rc = eg_run_to_fit(c, ch, 1, ch_vals + 64, &tb[ch], [&](uint8_t* const* outs, const uint64_t* caps) {
                return eg_run(c, q, n_cubes, carry_byte[ch], carry_bits[ch], (uint32_t*)outs[0], caps[0], &tb[ch]);
            });
            if (rc) return rc;
        }
    }
    for (int ch = 0; ch < channels; ch++) {
        total_bits[ch] = tb[ch];
        eg_last_bytes(c, ch) = (tb[ch] + 7) / 8;
    }
    return DCT3D_OK;
}

// Stream decode front: sync passes until the chunk exits converge, the scan of per-chunk code counts,
// the mark pass (bit position of every 32nd value).  No host wait after the last pass; the caller's
// consumer kernel (emit / fused decode) skips itself on a corrupt or short stream, and eg_decode_status
// reports it.  spec (with resolve): no host wait after pass 0 either -- the scan, the mark pass and the
// consumer are enqueued behind it at once; the mark pass reads the pass's verdict (status[0]) first and,
// should a chunk not have resolved (never seen on encoder output), writes no marks and flags status[2]
// bit 4, the consumer skips itself, and eg_decode_status asks the caller to rerun without speculation
// (kEgRetry).  This takes the host round trip between pass 0 and the scan off every call.
constexpr int kEgRetry = 1000;
#ifndef DCT3D_EG_PLAIN_CONFIRM  // A/B only: 1 = the rerun's confirming passes as plain eg_sync_kernel passes, one chunk each
#define DCT3D_EG_PLAIN_CONFIRM 0
#endif
constexpr bool kEgPlainConfirm = DCT3D_EG_PLAIN_CONFIRM != 0;
// a stream decode call begins: its fronts' sync launches are counted from here (dct3d_eg_sync_launches)
static void egd_launches_reset(dct3d_ctx* c) { c->egd_launches[0] = c->egd_launches[1] = c->egd_launches[2] = 0; }
// set >= 0 (a packed RGB24 stream decode: one front per channel, all three alive for the consumer): the front
// keeps its marks in region `set` of three in d_egd_mark and its status words in d_egd_status3[set], zeroed
// here; the other work buffers are reused from front to front in stream order.  set < 0: the grey calls' one
// front, whose status words alternate between two slots.  region_cubes: the cubes the mark regions are sized for
// (0: n_cubes; the same for the three fronts of a call, so that the first front's allocation holds all three).
static int eg_decode_front(dct3d_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, uint64_t start_bit, uint64_t n_cubes,
                           EgDecParams& D, bool spec, int set = -1, uint64_t region_cubes = 0) {
    const uint64_t limit = nbytes * 8;
    const uint64_t n_chunks = (limit - start_bit + kEgChunkBits - 1) / kEgChunkBits;
    const uint64_t n_scan = (n_chunks + 4095) / 4096;
    int rc = c->d_egd_exit.grow(2 * n_chunks * sizeof(uint64_t));
    if (!rc) rc = c->d_eg_bits.grow(n_chunks * sizeof(uint32_t));
    if (!rc) rc = c->d_eg_off.grow(16 * n_scan * sizeof(uint32_t));  // the scan's parts (launch_eg_dscan)
    if (!rc) rc = c->d_eg_bsum.grow((n_scan + 1) * sizeof(uint64_t));
    const uint64_t n_marks = n_cubes * (uint64_t)c->plan.cs / 32;
    const uint64_t n_mark_groups = n_marks / kMarkGroup + 1;
    // a region of the three: sized for region_cubes when the fronts' streams differ in length (4:2:0: the Y stream's)
    const uint64_t r_marks = (region_cubes > n_cubes ? region_cubes : n_cubes) * (uint64_t)c->plan.cs / 32;
    const size_t mark_bytes = ((r_marks / kMarkGroup + 1) * sizeof(uint64_t) + (r_marks + 1) * sizeof(uint16_t) + 7) & ~(size_t)7;
    if (!rc) rc = c->d_egd_mark.grow((set < 0 ? 1 : 3) * mark_bytes);
    if (rc) return rc;
    D.words = (const uint32_t*)d_bytes;
    D.n_words = (nbytes + 3) / 4;
    D.start_bit = start_bit;
    D.limit_bit = limit;
    D.n_chunks = n_chunks;
    D.n_values = n_cubes * (uint64_t)c->plan.cs;
    D.cs = c->plan.cs;
    D.diag = (const uint16_t*)c->d_diag.p;
    uint64_t* ex[2] = {(uint64_t*)c->d_egd_exit.p, (uint64_t*)c->d_egd_exit.p + n_chunks};
    D.count = (uint32_t*)c->d_eg_bits.p;
    D.off = nullptr;
    D.part = (uint32_t*)c->d_eg_off.p;
    D.bsum = (uint64_t*)c->d_eg_bsum.p;
    uint64_t* const st = set < 0 ? (uint64_t*)c->d_egd_status.p + 6 * c->egd_slot  // this call's words
                                 : (uint64_t*)c->d_egd_status3.p + 6 * set;
    const bool clean = set < 0 && c->egd_clean[c->egd_slot];
    if (set < 0) c->egd_clean[c->egd_slot] = false;
    D.status = st;
    D.status_clear = nullptr;
    D.mark_base = (uint64_t*)((char*)c->d_egd_mark.p + (set < 0 ? 0 : set) * mark_bytes);
    D.mark = (uint16_t*)(D.mark_base + n_mark_groups);
    D.q = nullptr;
    D.status_host = nullptr;
    if (spec && c->opt_eg_fused_front) {
        // A/B option: the fused front, one launch (eg_front_kernel); the consumer reads its verdict on the device
        const uint64_t nb = front_blocks(n_chunks);
        if ((rc = c->d_egd_desc.grow(nb * sizeof(uint64_t)))) return rc;
        if ((!clean && hipMemsetAsync(st, 0, kEgdStatusBytes, c->stream) != hipSuccess) ||
            hipMemsetAsync(c->d_egd_desc.p, 0, nb * sizeof(uint64_t), c->stream) != hipSuccess)
            return DCT3D_EDEVICE;
        if (launch_eg_front(D, (uint64_t*)c->d_egd_desc.p, c->opt_eg_force_retry ? 1 : 0, c->stream)) return DCT3D_EKERNEL;
        c->egd_launches[set < 0 ? 0 : set]++;
        return DCT3D_OK;
    }
    // sync passes until no chunk exit changes: pass 0 parses from the nominal chunk starts and, resolving,
    // usually proves every chunk in sync by itself; otherwise confirming passes follow, each also handing the
    // exits on inside its blocks of 256 chunks (eg_chain_kernel): after confirming pass j every chunk of blocks
    // 0 .. j - 1 is final by induction from chunk 0, so ceil(n_chunks / 256) of them finish a stream whose wrong
    // parses never meet the true one, and one more sees no change.  DCT3D_OPT_EG_NO_RESOLVE: always confirm (A/B, tests)
    const bool resolve = !c->opt_eg_no_resolve;
    const uint64_t last = kEgPlainConfirm ? n_chunks + 1 : (n_chunks + 255) / 256 + 1;
    uint64_t& launches = c->egd_launches[set < 0 ? 0 : set];
    int cur = 0;
    for (uint64_t it = 0; it <= last; it++) {
        if (!(it == 0 && clean) && hipMemsetAsync(st, 0, kEgdStatusBytes, c->stream) != hipSuccess) return DCT3D_EDEVICE;
        D.exit_in = ex[cur];
        D.exit_out = ex[cur ^ 1];
        if ((it == 0 || kEgPlainConfirm) ? launch_eg_sync(D, it ? 1 : 0, resolve, c->stream) : launch_eg_chain(D, c->stream))
            return DCT3D_EKERNEL;
        launches++;
        cur ^= 1;
        if (it == 0 && !resolve) continue;
        if (it == 0 && spec) {  // speculative front: the verdict is read on the device (eg_mark_kernel)
            if (c->opt_eg_force_retry && hipMemsetAsync(st, 0x01, 1, c->stream) != hipSuccess)
                return DCT3D_EDEVICE;
            break;
        }
        uint64_t changed = 0;
        if (read_status(c, st, 8, &changed)) return DCT3D_EDEVICE;
        if (!changed) break;
        if (it == last) return DCT3D_EINVAL;  // cannot happen: the induction above
    }
    // value index of each chunk's first codeword
    EgParams S;
    memset(&S, 0, sizeof(S));
    S.n_cubes = n_chunks;
    S.bits = D.count;
    S.bsum = D.bsum;
    S.status = D.status + 4;  // zeroed with the decode's words
    S.out_cap_words = ~0ull;
    if (launch_eg_dscan(D, S, c->stream)) return DCT3D_EKERNEL;
    D.exit_in = ex[cur];  // the converged exits
    if (launch_eg_mark(D, c->stream)) return DCT3D_EKERNEL;
    return DCT3D_OK;
}

// waits for the stream; the decode's verdict (corrupt: EINVAL, too short: ENODATA) and end bit (the
// consumer wrote the words to the host itself when D.status_host is set)
// The fused decode's verdict is final once the mark pass has run: the consumer's block 0 hands it over as
// the consumer starts (h_status[6] = the call's sequence number, after the words), and the call returns then,
// while the consumer still runs -- the raster completes on the context stream, as every *_dev output does,
// and the caller's next call is queued behind it (round 6: the synchronous return left ~50 us per call with
// the device idle between the consumer's end and the next call's first kernel, profiles/r06/gaps/).
// polls the pinned word h_status[word] for the call's hand-off tag (hand_off_tag: its sequence number in the
// top 16 bits) and returns the tag's value and flags
static int wait_tag(dct3d_ctx* c, int word, uint64_t seq, uint64_t* value, uint32_t* flags) {
    const volatile uint64_t* h = c->h_status;
    uint64_t t = 0;
    for (uint32_t n = 1;; n++) {
        t = h[word];
        if ((t >> 48) == (seq & 0xFFFFu)) break;
        if ((n & 255u) == 0u) {  // now and then: has the stream ended (or failed) without the hand-off?
            const hipError_t e = hipStreamQuery(c->stream);
            if (e != hipSuccess && e != hipErrorNotReady) return DCT3D_EDEVICE;
            if (e == hipSuccess && (h[word] >> 48) != (seq & 0xFFFFu)) return DCT3D_EDEVICE;
        }
        // a long call (a large stream, a busy device): after ~64 k polls the host thread yields its core
        if (n < 65536u) __builtin_ia32_pause();
        else std::this_thread::yield();
    }
    t = h[word];
    *value = t & kTagValueMask;
    *flags = (uint32_t)(t >> 40) & 0xFFu;
    return DCT3D_OK;
}
// the decode's verdict from the tag: w[1] = end bit, w[2] = flags, w[4] = a total that passes the short
// check (the tag's flag 8 says short); the whole words after the stream when the end bit did not fit
static int egd_wait_verdict(dct3d_ctx* c, const EgDecParams& D, uint64_t* w) {
    uint64_t v = 0;
    uint32_t fl = 0;
    if (wait_tag(c, 6, D.seq, &v, &fl)) return DCT3D_EDEVICE;
    if (fl & kTagOverflow) {
        if (stream_wait(c)) return DCT3D_EDEVICE;
        memcpy(w, c->h_status, kEgdStatusBytes);
        return DCT3D_OK;
    }
    w[1] = v;
    w[2] = fl & 7u;
    w[4] = (fl & 8u) ? 0u : D.n_values;
    return DCT3D_OK;
}
// a front's six status words -> the call's result and end bit
static int egd_verdict(const uint64_t* w, uint64_t n_values, uint64_t* end_bit) {
    const uint64_t* st = w;         // the decode's words
    const uint64_t* total = w + 4;  // the scan's: total bits, flags
    if (st[2] & 4) return kEgRetry;  // a speculative front whose pass 0 did not resolve: rerun
    if (st[2] & 1) return DCT3D_EINVAL;
    if ((st[2] & 2) || total[0] < n_values) return DCT3D_ENODATA;
    if (end_bit) *end_bit = st[1];
    return DCT3D_OK;
}
static int eg_decode_status(dct3d_ctx* c, const EgDecParams& D, uint64_t* end_bit) {
    uint64_t w[6] = {0, 0, 0, 0, 0, 0};
    if (D.status_host) {
        if (egd_wait_verdict(c, D, w)) return DCT3D_EDEVICE;
    } else if (read_status(c, D.status, kEgdStatusBytes, w)) {
        return DCT3D_EDEVICE;
    }
    c->egd_slot ^= 1;  // the next call's words
    return egd_verdict(w, D.n_values, end_bit);
}

int dct3d_eg_decode_dev(dct3d_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, uint64_t start_bit, uint64_t n_cubes,
                        int32_t* d_q, uint64_t* end_bit) {
    if (!c || (n_cubes && (!d_bytes || !d_q)) || ((uintptr_t)d_bytes & 3)) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (end_bit) *end_bit = start_bit;
    if (n_cubes == 0) return DCT3D_OK;
    if (start_bit >= nbytes * 8) return DCT3D_ENODATA;
    egd_launches_reset(c);
    for (int spec = 1;; spec = 0) {
        EgDecParams D{};
        int rc = eg_decode_front(c, d_bytes, nbytes, start_bit, n_cubes, D, spec && !c->opt_eg_no_resolve);
        if (rc) return rc;
        D.q = d_q;
        if (launch_eg_emit(c->bd, D, c->stream)) return DCT3D_EKERNEL;
        rc = eg_decode_status(c, D, end_bit);
        if (rc != kEgRetry || !spec) return rc == kEgRetry ? DCT3D_EDEVICE : rc;
    }
}

// Fused stream -> raster decode of stacks [st0, st0 + ns) after eg_decode_front: the decode kernel parses
// its cubes at the marks (no int32 cube-major intermediate) and replays uncertified cubes in the wave by
// re-parsing them.  out_stack0 = where stack st0 goes (the raster pointer is rebased so that the
// kernels' global cube indices land in it).
}  // extern "C"
// A decode_eg_kernel launch starts on a consumer group (kMarkGroup marks = 2,048 values: the group's first
// whole position is in mark_base, and the group's end is the next group's first): its first stack st0 must
// put st0 * cubes-per-stack * cs on a multiple of 2,048 values.  The smallest stack count that does for a
// w x h frame (1 at 1080p; 8 for a frame of an odd number of 8x8x8 cubes).  (Round 6: the host path's
// chunks of stacks started anywhere, and a chunk starting inside a group parsed past its window.)
static int eg_stack_align(const dct3d_ctx* c, const Geom& g) {
    const uint64_t per = g.cps() * (uint64_t)c->plan.cs;  // (the padded raster's cubes)
    const uint64_t grp = kMarkGroup * 32;
    uint64_t a = per % grp, b = grp;  // gcd(per, grp)
    while (a) {
        const uint64_t t = b % a;
        b = a;
        a = t;
    }
    return (int)(grp / b);
}
// E: the front of each of g.px streams (packed RGB24: one per channel)
static int decode_eg_range(dct3d_ctx* c, const EgDecParams* E, const Geom& g, int st0, int ns, uint8_t* out_stack0) {
    const int D = c->bd;
    const uint64_t cps = g.cps();
    DecodeParamsQ P;  // the cubes [cube_base, n_cubes); rebased: stack st0 at out_stack0
    fill_decode_params(c, P, nullptr, out_stack0 - (size_t)st0 * g.plane() * D, g, (st0 + ns) * cps);
    P.cube_base = (uint32_t)(st0 * cps);
    P.steps = qt_steps(c);
    const Variant v = stream_variant_of(c, g);
    hipEvent_t* ev = timer_begin(c);
    int lrc;
    if (g.px == 3) {
        EgDecRgbParams R;
        for (int ch = 0; ch < 3; ch++)
            R.s[ch] = EgDecStream{E[ch].words, E[ch].n_words, E[ch].n_values, E[ch].mark, E[ch].mark_base, E[ch].status};
        R.diag = E[0].diag;
        lrc = launch_decode_eg_rgb(v, P, R, c->vq, c->vq_ch_stride, c->stream);
    } else {  // (the test option's groups per wave: where the variant's unit builds them.  A vq call's map is
              // indexed by the call's stacks: the chunks' cube indices are the call's)
        lrc = launch_decode_eg(v, P, E[0], c->opt_eg_dec_groups ? c->opt_eg_dec_groups : 8, c->vq, c->stream);
    }
    if (lrc) return DCT3D_EKERNEL;
    timer_end(c, ev);
    count_slot_used(c, (uint64_t)g.px * ns * cps * (uint64_t)c->plan.cs);
    return DCT3D_OK;
}

// The fused stream -> raster decode of n_stacks stacks: the front of each of the g.px device streams, then the
// consumer -- to d_out (host_out == nullptr: asynchronous, the call returning once the verdicts are known), or
// in chunks of stacks through the pipeline to host_out.  end_bit[ch] (start_bit[ch] on entry) is set for
// every stream whose own verdict is good; the first bad verdict is returned.  One grey stream to a device
// raster hands its verdict over from the consumer; the other cases read the status words back.
static int decode_eg_run(dct3d_ctx* c, const uint8_t* const* d_bytes, const uint64_t* nbytes, const uint64_t* start_bit,
                         const Geom& g, int n_stacks, uint64_t n_cubes, uint8_t* d_out, uint8_t* host_out,
                         uint64_t* end_bit) {
    const bool handoff = !host_out && g.px == 1;
    int rc;
    egd_launches_reset(c);
    for (int spec = 1;; spec = 0) {
        EgDecParams E[3] = {};
        for (int ch = 0; ch < g.px; ch++)
            if ((rc = eg_decode_front(c, d_bytes[ch], nbytes[ch], start_bit[ch], n_cubes, E[ch],
                                      spec && !c->opt_eg_no_resolve, g.px == 1 ? -1 : ch)))
                return rc;
        if (handoff) {
            E[0].status_host = c->h_status_dev;  // the consumer hands the verdict to the host (nullptr: a copy)
            E[0].seq = ++c->egd_seq;
            E[0].status_clear = (uint64_t*)c->d_egd_status.p + 6 * (c->egd_slot ^ 1);  // and zeroes the next call's
        }
        if (host_out) {
            // the raster leaves in chunks of stacks while the next chunk decodes (the stream is small: no upload)
            const size_t per_stack = (size_t)g.plane() * c->bd;
            batch_begin(c);
            rc = run_pipeline(c, n_stacks, 0, per_stack, nullptr, host_out, [&](const void*, void* dout, int st0, int ns) {
                return decode_eg_range(c, E, g, st0, ns, (uint8_t*)dout);
            }, eg_stack_align(c, g));  // each chunk's first cube on a consumer group
            batch_end(c);
        } else {
            rc = decode_eg_range(c, E, g, 0, n_stacks, d_out);
        }
        if (rc) return rc;
        if (handoff) c->egd_clean[c->egd_slot ^ 1] = true;
        if (g.px == 1) {
            rc = eg_decode_status(c, E[0], end_bit);
        } else {  // the three fronts' words in one read-back
            uint64_t w[18];
            if (hipMemcpyAsync(c->h_status + 8, c->d_egd_status3.p, sizeof(w), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                stream_wait(c))
                return DCT3D_EDEVICE;
            memcpy(w, c->h_status + 8, sizeof(w));
            int v[3];
            bool retry = false;
            for (int ch = 0; ch < 3; ch++) retry |= (v[ch] = egd_verdict(w + 6 * ch, E[ch].n_values, nullptr)) == kEgRetry;
            rc = retry ? kEgRetry : DCT3D_OK;
            for (int ch = 0; ch < 3 && !retry; ch++) {
                if (!v[ch]) end_bit[ch] = w[6 * ch + 1];
                else if (!rc) rc = v[ch];
            }
        }
        if (rc != kEgRetry || !spec) return rc == kEgRetry ? DCT3D_EDEVICE : rc;
    }
}

// The packed RGB24 stream decode under 4:2:0 of stacks [st0, st0 + ns) after the three fronts E (stream 0
// over the frames' cubes, streams 1 and 2 over the chroma plane's: gc): (a) the grey stream decode of streams 1 and 2
// at the chroma geometry into the context's two planes, sized for this range, and (b) the Y kernel, which reads them
// and stores the frames at out_stack0 -- unless a front's verdict is bad: then nothing is stored (the planes may hold
// anything).  Every pointer is rebased so that the kernels' global cube and stack indices land in the range's buffers.
static int decode_c420_range(dct3d_ctx* c, const EgDecParams* E, const Geom& g, const Geom& gc, int st0, int ns,
                             uint8_t* out_stack0) {
    const int D = c->bd;
    const size_t stack_c = (size_t)gc.plane() * D;  // bytes of a stack of one chroma plane
    int rc;
    if ((rc = c->d_c420.grow(2 * stack_c * ns))) return rc;
    const uint64_t cps = g.cps(), cps_c = gc.cps();
    uint8_t* const planes[2] = {(uint8_t*)c->d_c420.p - (size_t)st0 * stack_c,
                                (uint8_t*)c->d_c420.p + (size_t)ns * stack_c - (size_t)st0 * stack_c};
    const Variant v = stream_variant_of(c, g), vc = stream_variant_of(c, gc);
    hipEvent_t* ev = timer_begin(c);
    for (int ch = 1; ch < 3; ch++) {
        DecodeParamsQ Pc;
        fill_decode_params(c, Pc, nullptr, planes[ch - 1], gc, (st0 + ns) * cps_c);
        Pc.cube_base = (uint32_t)(st0 * cps_c);
        Pc.steps = qt_steps(c);
        if (launch_decode_eg(vc, Pc, E[ch], c->opt_eg_dec_groups ? c->opt_eg_dec_groups : 8, c->vq ? &c->vq_ch[ch] : nullptr, c->stream))
            return DCT3D_EKERNEL;
        count_slot_used(c, ns * cps_c * (uint64_t)c->plan.cs);
    }
    DecodeParamsQ P;
    fill_decode_params(c, P, nullptr, out_stack0 - (size_t)st0 * g.plane() * D, g, (st0 + ns) * cps);
    P.cube_base = (uint32_t)(st0 * cps);
    P.height = (uint32_t)g.h;  // (the chroma fetch clamps by it whatever the edge)
    P.steps = qt_steps(c);
    EgDecRgbParams R;
    for (int ch = 0; ch < 3; ch++)
        R.s[ch] = EgDecStream{E[ch].words, E[ch].n_words, E[ch].n_values, E[ch].mark, E[ch].mark_base, E[ch].status};
    R.diag = E[0].diag;
    if (launch_decode_eg_y420(v.D, v.edge, v.qt, P, R, C420Planes{planes[0], planes[1]}, c->vq, c->stream)) return DCT3D_EKERNEL;
    timer_end(c, ev);
    count_slot_used(c, ns * cps * (uint64_t)c->plan.cs);
    return DCT3D_OK;
}

// The whole call: the three fronts, then the ranges -- to d_out (host_out == nullptr), or in chunks of stacks through
// the pipeline to host_out, each chunk starting on a consumer group in both geometries (the lcm of their
// eg_stack_align).  One counter slot for all launches (batch).  end_bit and the verdicts: as decode_eg_run's packed case.
static int decode_c420_run(dct3d_ctx* c, const uint8_t* const* d_bytes, const uint64_t* nbytes, const uint64_t* start_bit,
                           const Geom& g, const Geom& gc, int n_stacks, uint64_t n_cubes, uint64_t nc, uint8_t* d_out,
                           uint8_t* host_out, uint64_t* end_bit) {
    const uint64_t cubes[3] = {n_cubes, nc, nc};
    int rc;
    egd_launches_reset(c);
    for (int spec = 1;; spec = 0) {
        EgDecParams E[3] = {};
        for (int ch = 0; ch < 3; ch++)
            if ((rc = eg_decode_front(c, d_bytes[ch], nbytes[ch], start_bit[ch], cubes[ch], E[ch], spec && !c->opt_eg_no_resolve, ch, n_cubes)))
                return rc;
        batch_begin(c);
        if (host_out) {
            const int ay = eg_stack_align(c, g), ac = eg_stack_align(c, gc);
            int a = ay, b = ac;  // gcd
            while (b) {
                const int t = a % b;
                a = b;
                b = t;
            }
            rc = run_pipeline(c, n_stacks, 0, (size_t)g.plane() * c->bd, nullptr, host_out, [&](const void*, void* dout, int st0, int ns) {
                return decode_c420_range(c, E, g, gc, st0, ns, (uint8_t*)dout);
            }, ay / a * ac);
        } else {
            rc = decode_c420_range(c, E, g, gc, 0, n_stacks, d_out);
        }
        batch_end(c);
        if (rc) return rc;
        uint64_t w[18];
        if (hipMemcpyAsync(c->h_status + 8, c->d_egd_status3.p, sizeof(w), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            stream_wait(c))
            return DCT3D_EDEVICE;
        memcpy(w, c->h_status + 8, sizeof(w));
        int vd[3];
        bool retry = false;
        for (int ch = 0; ch < 3; ch++) retry |= (vd[ch] = egd_verdict(w + 6 * ch, E[ch].n_values, nullptr)) == kEgRetry;
        rc = retry ? kEgRetry : DCT3D_OK;
        for (int ch = 0; ch < 3 && !retry; ch++) {
            if (!vd[ch]) end_bit[ch] = w[6 * ch + 1];
            else if (!rc) rc = vd[ch];
        }
        if (rc != kEgRetry || !spec) return rc == kEgRetry ? DCT3D_EDEVICE : rc;
    }
}
extern "C" {

// Fused: device stream -> device raster.  On a corrupt stream the decode kernel skips itself; on a short
// one it decodes whatever the marks hold (bounded windows); the error is returned either way.
int dct3d_decode_eg_dev(dct3d_ctx* c, const uint8_t* d_bytes, uint64_t nbytes, uint64_t start_bit, int w, int h,
                        int n_stacks, uint8_t* d_raster, uint64_t* end_bit) {
    if (!c || (n_stacks && (!d_bytes || !d_raster)) || ((uintptr_t)d_bytes & 3)) return DCT3D_EINVAL;
    Geom g;
    uint64_t n_cubes;
    if (!make_geom(w, h, 1, n_stacks, false, &g, &n_cubes)) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    call_begin(c);
    if (end_bit) *end_bit = start_bit;
    if (n_cubes == 0) return DCT3D_OK;
    if (start_bit >= nbytes * 8) return DCT3D_ENODATA;
    return decode_eg_run(c, &d_bytes, &nbytes, &start_bit, g, n_stacks, n_cubes, d_raster, nullptr, end_bit);
}

int dct3d_decode_eg(dct3d_ctx* c, const uint8_t* bytes, uint64_t nbytes, int start_bit, int w, int h, int n_stacks,
                    uint8_t* raster, uint64_t* end_bit) {
    if (!c || (n_stacks && (!bytes || !raster)) || start_bit < 0 || start_bit > 7) return DCT3D_EINVAL;
    Geom g;
    uint64_t n_cubes;
    if (!make_geom(w, h, 1, n_stacks, false, &g, &n_cubes)) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    if (end_bit) *end_bit = (uint64_t)start_bit;
    if (n_cubes == 0) return DCT3D_OK;
    if ((uint64_t)start_bit >= nbytes * 8) return DCT3D_ENODATA;
    int rc;
    if ((rc = c->d_egd_in.grow((nbytes + 8) & ~(uint64_t)3))) return rc;
    if (hipMemcpyAsync(c->d_egd_in.p, bytes, nbytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return DCT3D_EDEVICE;
    const uint8_t* const d_bytes = (const uint8_t*)c->d_egd_in.p;
    const uint64_t sb = (uint64_t)start_bit;
    return decode_eg_run(c, &d_bytes, &nbytes, &sb, g, n_stacks, n_cubes, nullptr, raster, end_bit);
}

// ---- one Exp-Golomb stream per channel -> frames of any size, grey or packed RGB24 (dct3d.h) ----
int dct3d_decode_eg_frames_dev(dct3d_ctx* c, const uint8_t* const d_bytes[], const uint64_t nbytes[],
                               const uint64_t start_bit[], int w, int h, int channels, int n_stacks, uint8_t* d_frames,
                               uint64_t end_bit[]) {
    Geom g;
    uint64_t n_cubes;
    if (!c || !make_geom(w, h, channels, n_stacks, true, &g, &n_cubes)) return DCT3D_EINVAL;
    if (!d_bytes || !nbytes || !start_bit || !end_bit) return DCT3D_EINVAL;
    if (c->opt_eg_two_step && colour_refused(c, channels)) return DCT3D_EINVAL;  // the int32 intermediate has no colour stage
    Geom gc = g;
    uint64_t nc = n_cubes;  // 4:2:0: the chroma planes' cubes
    const bool c420 = c420_on(c, channels);
    if (c420_refused(c, channels) || (c420 && !c420_geom(g, n_stacks, &gc, &nc))) return DCT3D_EINVAL;
    if (eg_aligned(g)) return dct3d_decode_eg_dev(c, d_bytes[0], nbytes[0], start_bit[0], w, h, n_stacks, d_frames, end_bit);
    if (n_stacks && !d_frames) return DCT3D_EINVAL;
    for (int ch = 0; ch < channels; ch++)
        if ((n_stacks && !d_bytes[ch]) || ((uintptr_t)d_bytes[ch] & 3)) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    call_begin(c);
    int rc;
    for (int ch = 0; ch < channels; ch++) end_bit[ch] = start_bit[ch];
    if (n_cubes == 0) return DCT3D_OK;
    for (int ch = 0; ch < channels; ch++)
        if (start_bit[ch] >= nbytes[ch] * 8) return DCT3D_ENODATA;
    if (c->opt_eg_two_step) {
        // A/B option: each stream through the stand-alone stage into its blocks of the int32 cubes
        // ([stack][channel][cube]), then dct3d_decode_frames_dev
        const size_t ch_vals = n_cubes * c->plan.cs, blk = (size_t)g.cps() * c->plan.cs * sizeof(int32_t);
        if ((rc = c->d_eg_q.grow(channels * ch_vals * sizeof(int32_t))) ||
            (channels == 3 && (rc = c->d_eg_q_ch.grow(ch_vals * sizeof(int32_t)))))
            return rc;
        int first = DCT3D_OK;
        for (int ch = 0; ch < channels; ch++) {
            int32_t* q = channels == 3 ? (int32_t*)c->d_eg_q_ch.p : (int32_t*)c->d_eg_q.p;
            rc = dct3d_eg_decode_dev(c, d_bytes[ch], nbytes[ch], start_bit[ch], n_cubes, q, &end_bit[ch]);
            if (rc && !first) first = rc;
            if (rc && rc != DCT3D_ENODATA && rc != DCT3D_EINVAL) return rc;
            if (channels == 3 && hipMemcpy2DAsync((char*)c->d_eg_q.p + ch * blk, 3 * blk, q, blk, blk, (size_t)n_stacks,
                                                  hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                return DCT3D_EDEVICE;
        }
        if (first) return first;
        return decode_dev(c, (const int32_t*)c->d_eg_q.p, g, n_cubes, d_frames);
    }
    if (c420) return decode_c420_run(c, d_bytes, nbytes, start_bit, g, gc, n_stacks, n_cubes, nc, d_frames, nullptr, end_bit);
    return decode_eg_run(c, d_bytes, nbytes, start_bit, g, n_stacks, n_cubes, d_frames, nullptr, end_bit);
}

// channel ch's host-call stream buffer on the device
static DevBuf& egd_in_buf(dct3d_ctx* c, int ch) { return ch == 0 ? c->d_egd_in : c->d_egd_in_x[ch - 1]; }

int dct3d_decode_eg_frames(dct3d_ctx* c, const uint8_t* const bytes[], const uint64_t nbytes[], const int start_bit[],
                           int w, int h, int channels, int n_stacks, uint8_t* frames, uint64_t end_bit[]) {
    Geom g;
    uint64_t n_cubes;
    if (!c || !make_geom(w, h, channels, n_stacks, true, &g, &n_cubes)) return DCT3D_EINVAL;
    if (!bytes || !nbytes || !start_bit || !end_bit) return DCT3D_EINVAL;
    if (c->opt_eg_two_step && colour_refused(c, channels)) return DCT3D_EINVAL;
    if (c420_refused(c, channels)) return DCT3D_EINVAL;
    int rc;
    if (eg_aligned(g)) return dct3d_decode_eg(c, bytes[0], nbytes[0], start_bit[0], w, h, n_stacks, frames, end_bit);
    if (n_stacks && !frames) return DCT3D_EINVAL;
    for (int ch = 0; ch < channels; ch++)
        if ((n_stacks && !bytes[ch]) || start_bit[ch] < 0 || start_bit[ch] > 7) return DCT3D_EINVAL;
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    uint64_t sb[3] = {0, 0, 0};
    for (int ch = 0; ch < channels; ch++) end_bit[ch] = sb[ch] = (uint64_t)start_bit[ch];
    if (n_cubes == 0) return DCT3D_OK;
    for (int ch = 0; ch < channels; ch++)
        if (sb[ch] >= nbytes[ch] * 8) return DCT3D_ENODATA;
    const uint8_t* d_bytes[3] = {nullptr, nullptr, nullptr};
    for (int ch = 0; ch < channels; ch++) {
        if ((rc = egd_in_buf(c, ch).grow((nbytes[ch] + 8) & ~(uint64_t)3))) return rc;
        d_bytes[ch] = (const uint8_t*)egd_in_buf(c, ch).p;
        if (hipMemcpyAsync(egd_in_buf(c, ch).p, bytes[ch], nbytes[ch], hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return DCT3D_EDEVICE;
    }
    if (c->opt_eg_two_step) {  // A/B option: through the int32 cubes, the frames in one copy
        const size_t out_bytes = (size_t)g.plane() * c->bd * n_stacks;
        if ((rc = c->d_egd_raster.grow(out_bytes))) return rc;
        if ((rc = dct3d_decode_eg_frames_dev(c, d_bytes, nbytes, sb, w, h, channels, n_stacks, (uint8_t*)c->d_egd_raster.p, end_bit)))
            return rc;
        if (hipMemcpyAsync(frames, c->d_egd_raster.p, out_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return DCT3D_EDEVICE;
        return hipStreamSynchronize(c->stream) == hipSuccess ? DCT3D_OK : DCT3D_EDEVICE;
    }
    if (c420_on(c, channels)) {
        Geom gc;
        uint64_t nc;
        if (!c420_geom(g, n_stacks, &gc, &nc)) return DCT3D_EINVAL;
        return decode_c420_run(c, d_bytes, nbytes, sb, g, gc, n_stacks, n_cubes, nc, nullptr, frames, end_bit);
    }
    return decode_eg_run(c, d_bytes, nbytes, sb, g, n_stacks, n_cubes, nullptr, frames, end_bit);
}

// ---- per-stack quantiser tables in the fused stream calls (dct3d.h) ----
}  // extern "C"
// The three extra arguments of a vq call: checked, the palette's rows and steps made from the context's one plan
// (probe_tables: encoder_tables per entry, no plan rebuild), and steps, map and rows queued to the device on the
// context stream as one block laid out as VqParams says (launch_vq_upload, from the context's pinned copy).  From here to vq_end the stream calls' host bodies
// launch the vq kernels.
// per_channel (the _vqc calls): stack_table is [n_stacks][channels], else [n_stacks] for every channel.
// The block holds one {steps, FastDiv, map column} per distinct (column, plane geometry) -- one for a _vq call, two
// under 4:2:0 (the frames' and the chroma plane's cubes per stack), one per channel for a _vqc call of three
// channels -- and the palette's rows once behind them; c->vq_ch[ch] is channel ch's view.
static int vq_begin(dct3d_ctx* c, int w, int h, int channels, int n_stacks, const int32_t* tables, int n_tables,
                    const uint8_t* stack_table, bool per_channel = false) {
    if (!c || !tables || !stack_table || n_tables < 1 || n_tables > kVqMaxTables) return DCT3D_EINVAL;
    if (c->opt_eg_two_step) return DCT3D_EINVAL;  // the int32 intermediate has no table per stack (dct3d.h)
    if (c420_refused(c, channels)) return DCT3D_EINVAL;  // (before the upload is queued)
    Geom g;
    uint64_t n_cubes;
    if (!make_geom(w, h, channels, n_stacks, true, &g, &n_cubes)) return DCT3D_EINVAL;
    const int n_steps = (int)c->plan.steps.size();
    for (int i = 0; i < n_tables * n_steps; i++)
        if (tables[i] < kMinStep || tables[i] > kMaxStep) return DCT3D_EINVAL;
    const int map_w = per_channel ? channels : 1;  // entries per stack in stack_table
    for (size_t i = 0; i < (size_t)n_stacks * map_w; i++)
        if (stack_table[i] >= n_tables) return DCT3D_EINVAL;
    if (n_stacks == 0) return DCT3D_OK;  // (nothing to upload; the base call ends before any launch)
    if (hipSetDevice(c->device) != hipSuccess) return DCT3D_EDEVICE;
    static_assert(kVqTabN == kRateTabN && kVqStepN == kDistStepN && kVqMaxTables == DCT3D_RATE_MAX_TABLES, "the probes' layouts");
    const size_t n_ints = (size_t)n_tables * n_steps;
    if (c->vq_tables.size() != n_ints || memcmp(c->vq_tables.data(), tables, n_ints * sizeof(int32_t)) != 0) {
        probe_tables(c, tables, n_tables, true);  // (the probes' host vectors: copied out, a probe call rewrites them)
        c->vq_rows = c->rate_tabs_host;
        c->vq_steps = c->dist_steps_host;
        c->vq_tables.assign(tables, tables + n_ints);
    }
    const size_t tab_bytes = c->vq_rows.size() * sizeof(float), step_bytes = c->vq_steps.size() * sizeof(double);
    const size_t map_off = kVqStepsBytes + sizeof(FastDiv);
    const size_t blk_bytes = (map_off + (size_t)n_stacks + 15) & ~(size_t)15;  // one {steps, FastDiv, map column}
    // 4:2:0: the chroma channels' blocks have the chroma plane's cubes per stack in their FastDiv (the grey decode's
    // exact replay finds its stack through it)
    Geom gc = g;
    uint64_t nc = 0;
    const bool c420 = c420_on(c, channels);
    if (c420 && !c420_geom(g, n_stacks, &gc, &nc)) return DCT3D_EINVAL;
    const bool cols = per_channel && channels == 3;  // a column per channel
    const int n_blk = cols ? 3 : c420 ? 2 : 1;
    const int blk_of[3] = {0, n_blk > 1 ? 1 : 0, cols ? 2 : n_blk > 1 ? 1 : 0};
    const size_t tab_off = (size_t)n_blk * blk_bytes;  // the rows: 16-byte aligned
    const size_t blob_bytes = tab_off + tab_bytes;
    int rc;
    if (c->vq_host_bytes < blob_bytes) {
        // (a call that returned has started its last kernel: the copy out of the old block is over)
        if (c->vq_host) (void)hipHostFree(c->vq_host);
        c->vq_host = nullptr;
        c->vq_host_bytes = 0;
        if (hipHostMalloc((void**)&c->vq_host, blob_bytes + 4096, hipHostMallocDefault) != hipSuccess) {
            c->vq_host = nullptr;
            return DCT3D_ENOMEM;
        }
        if (hipHostGetDevicePointer((void**)&c->vq_host_dev, c->vq_host, 0) != hipSuccess) {
            (void)hipHostFree(c->vq_host);
            c->vq_host = nullptr;
            return DCT3D_EDEVICE;
        }
        c->vq_host_bytes = blob_bytes + 4096;
    }
    uint8_t* const blob = c->vq_host;
    for (int b = 0; b < n_blk; b++) {
        uint8_t* const blk = blob + (size_t)b * blk_bytes;
        memcpy(blk, c->vq_steps.data(), step_bytes);
        const FastDiv div = fast_div((uint32_t)(c420 && b ? gc.cps() : g.cps()));
        memcpy(blk + kVqStepsBytes, &div, sizeof(div));
        if (cols)  // column b of [n_stacks][3]
            for (int s = 0; s < n_stacks; s++) blk[map_off + s] = stack_table[(size_t)s * 3 + b];
        else
            memcpy(blk + map_off, stack_table, (size_t)n_stacks);
    }
    memcpy(blob + tab_off, c->vq_rows.data(), tab_bytes);
    const size_t n16 = (blob_bytes + 15) / 16;  // (the pinned block has 4 KiB to spare behind blob_bytes)
    if ((rc = c->d_vq.grow(n16 * 16))) return rc;
    char* const d = (char*)c->d_vq.p;
    if (launch_vq_upload(c->vq_host_dev, d, (uint32_t)n16, c->stream)) return DCT3D_EKERNEL;
    for (int ch = 0; ch < 3; ch++) {
        const double* const st = (const double*)(d + (size_t)blk_of[ch] * blk_bytes);
        c->vq_ch[ch] = VqParams{(const float4*)(d + tab_off), st, vq_map_behind(st)};
    }
    // (decode_eg_rgb_kernel, the 4:4:4 decode of three channels, walks the blocks from channel 0's: VqcParams)
    c->vq_ch_stride = cols && !c420 ? (uint32_t)blk_bytes : 0u;
    c->vq = c->vq_ch;
    return DCT3D_OK;
}
// the call is over.  A call that ended before its kernels ran (an argument the base call refuses, a stream with
// no data, a failed launch) may leave the upload queued: it reads the context's pinned copy, which the next call
// rewrites, so the stream is waited for
static int vq_end(dct3d_ctx* c, int rc) {
    if (c->vq && rc != DCT3D_OK) (void)stream_wait(c);
    c->vq = nullptr;
    c->vq_ch_stride = 0;
    return rc;
}
extern "C" {

int dct3d_encode_eg_frames_vq_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int channels, int n_stacks,
                                  const int32_t* tables, int n_tables, const uint8_t* stack_table,
                                  const uint8_t carry_byte[], const int carry_bits[], uint8_t* const d_out[],
                                  const uint64_t out_cap[], uint64_t total_bits[]) {
    const int rc = vq_begin(c, w, h, channels, n_stacks, tables, n_tables, stack_table);
    if (rc) return rc;
    return vq_end(c, dct3d_encode_eg_frames_dev(c, d_frames, w, h, channels, n_stacks, carry_byte, carry_bits, d_out, out_cap, total_bits));
}

int dct3d_encode_eg_frames_vq(dct3d_ctx* c, const uint8_t* frames, int w, int h, int channels, int n_stacks,
                              const int32_t* tables, int n_tables, const uint8_t* stack_table,
                              const uint8_t carry_byte[], const int carry_bits[], uint64_t total_bits[]) {
    const int rc = vq_begin(c, w, h, channels, n_stacks, tables, n_tables, stack_table);
    if (rc) return rc;
    return vq_end(c, dct3d_encode_eg_frames(c, frames, w, h, channels, n_stacks, carry_byte, carry_bits, total_bits));
}

int dct3d_decode_eg_frames_vq_dev(dct3d_ctx* c, const uint8_t* const d_bytes[], const uint64_t nbytes[],
                                  const uint64_t start_bit[], int w, int h, int channels, int n_stacks,
                                  const int32_t* tables, int n_tables, const uint8_t* stack_table, uint8_t* d_frames,
                                  uint64_t end_bit[]) {
    const int rc = vq_begin(c, w, h, channels, n_stacks, tables, n_tables, stack_table);
    if (rc) return rc;
    return vq_end(c, dct3d_decode_eg_frames_dev(c, d_bytes, nbytes, start_bit, w, h, channels, n_stacks, d_frames, end_bit));
}

int dct3d_decode_eg_frames_vq(dct3d_ctx* c, const uint8_t* const bytes[], const uint64_t nbytes[], const int start_bit[],
                              int w, int h, int channels, int n_stacks, const int32_t* tables, int n_tables,
                              const uint8_t* stack_table, uint8_t* frames, uint64_t end_bit[]) {
    const int rc = vq_begin(c, w, h, channels, n_stacks, tables, n_tables, stack_table);
    if (rc) return rc;
    return vq_end(c, dct3d_decode_eg_frames(c, bytes, nbytes, start_bit, w, h, channels, n_stacks, frames, end_bit));
}

// ---- a table per (stack, channel): table_map[n_stacks][channels] (dct3d.h) ----
int dct3d_encode_eg_frames_vqc_dev(dct3d_ctx* c, const uint8_t* d_frames, int w, int h, int channels, int n_stacks,
                                   const int32_t* tables, int n_tables, const uint8_t* table_map,
                                   const uint8_t carry_byte[], const int carry_bits[], uint8_t* const d_out[],
                                   const uint64_t out_cap[], uint64_t total_bits[]) {
    const int rc = vq_begin(c, w, h, channels, n_stacks, tables, n_tables, table_map, true);
    if (rc) return rc;
    return vq_end(c, dct3d_encode_eg_frames_dev(c, d_frames, w, h, channels, n_stacks, carry_byte, carry_bits, d_out, out_cap, total_bits));
}

int dct3d_encode_eg_frames_vqc(dct3d_ctx* c, const uint8_t* frames, int w, int h, int channels, int n_stacks,
                               const int32_t* tables, int n_tables, const uint8_t* table_map,
                               const uint8_t carry_byte[], const int carry_bits[], uint64_t total_bits[]) {
    const int rc = vq_begin(c, w, h, channels, n_stacks, tables, n_tables, table_map, true);
    if (rc) return rc;
    return vq_end(c, dct3d_encode_eg_frames(c, frames, w, h, channels, n_stacks, carry_byte, carry_bits, total_bits));
}

int dct3d_decode_eg_frames_vqc_dev(dct3d_ctx* c, const uint8_t* const d_bytes[], const uint64_t nbytes[],
                                   const uint64_t start_bit[], int w, int h, int channels, int n_stacks,
                                   const int32_t* tables, int n_tables, const uint8_t* table_map, uint8_t* d_frames,
                                   uint64_t end_bit[]) {
    const int rc = vq_begin(c, w, h, channels, n_stacks, tables, n_tables, table_map, true);
    if (rc) return rc;
    return vq_end(c, dct3d_decode_eg_frames_dev(c, d_bytes, nbytes, start_bit, w, h, channels, n_stacks, d_frames, end_bit));
}

int dct3d_decode_eg_frames_vqc(dct3d_ctx* c, const uint8_t* const bytes[], const uint64_t nbytes[], const int start_bit[],
                               int w, int h, int channels, int n_stacks, const int32_t* tables, int n_tables,
                               const uint8_t* table_map, uint8_t* frames, uint64_t end_bit[]) {
    const int rc = vq_begin(c, w, h, channels, n_stacks, tables, n_tables, table_map, true);
    if (rc) return rc;
    return vq_end(c, dct3d_decode_eg_frames(c, bytes, nbytes, start_bit, w, h, channels, n_stacks, frames, end_bit));
}

}  // extern "C"
