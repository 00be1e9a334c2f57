// dct3d_ctx.h -- the C-ABI's context (include/dct3d.h: dct3d_ctx) and the runtime's helpers that more than one
// host unit uses: dct3d_runtime.cpp defines them, dct3d_probes.cpp (the probes' host side) calls them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/dct3d.h"
#include "dct3d_kernels.h"
#include "dct3d_plan.h"
#include "dct3d_vq.h"

namespace dct3d {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int grow(size_t need) {
        if (need <= bytes) return DCT3D_OK;
        release();
        if (hipMalloc(&p, need) != hipSuccess) return DCT3D_ENOMEM;
        bytes = need;
        return DCT3D_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

}  // namespace dct3d

struct dct3d_ctx {
    int device = 0;
    int bw = 8, bh = 8, bd = 8;
    dct3d::Plan plan;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    bool profiling = false;
    // ring of event quadruples (main kernel begin/end, auxiliary launch begin/end); resolved lazily
    static constexpr int kRing = 256;
    hipEvent_t ev[kRing][4] = {};
    int ring_head = 0, ring_pending = 0;
    uint64_t n_timed = 0;
    double kernel_ms = 0.0, aux_ms = 0.0;
    // plan tables on device
    dct3d::DevBuf d_ngroups, d_coef, d_group_of, d_inv_coef, d_tabs, d_tabs64;
    // test / diagnostic options (dct3d_ctx_set_option): how later calls reach their results
    double opt_dec_margin = 0.0;    // added to the decode margin
    bool opt_enc_no_recheck = false, opt_eg_two_step = false,
         opt_eg_no_resolve = false;
    bool opt_eg_force_retry = false;
    bool opt_eg_fused_front = false;
    int opt_eg_dec_groups = 0;  // fused stream decode: groups per wave (0: the default, 8)
    int opt_colour = 0;            // DCT3D_OPT_COLOUR: 1 = the packed RGB24 stream calls and the rate probe code Y, Cb, Cr
    bool opt_quant_force = false;  // the table kernels even for the reference table (DCT3D_OPT_QUANT_FORCE_TABLE)
    // certify-or-replay state
    uint64_t last_units = 0;
    bool last_valid = false;
    // in-wave replay (encode, decode): two counter slots that alternate between calls; each launch zeroes
    // the other slot for the next call, so a call needs no reset copy (zeroed once at creation).
    // Slot j (2 kCountSpread words at j * 2 kCountSpread): Java-fold replays, then second-certificate
    // settlements, each spread over kCountSpread words (dct3d_kernels.h).
    dct3d::DevBuf d_enc_counts;
    int enc_slot = 0;
    int last_count_slot = -1;  // >= 0: the last call's statistics are in d_enc_counts[slot]
    bool slot_used = false;    // a counting kernel of the current call was enqueued into enc_slot
    bool batch = false;        // a host entry point's chunks: one slot for the whole call (batch_end flips it)
    uint64_t batch_units = 0;
    hipEvent_t ev_switch = nullptr;  // orders a dct3d_ctx_set_stream switch after the old stream's work
    // host-pointer entry point staging
    dct3d::DevBuf h_in, h_out, h_aux;
    // Exp-Golomb stage: diagonal order, per-cube bits / offsets, chunk sums, status, device stream
    dct3d::DevBuf d_diag, d_eg_bits, d_eg_off, d_eg_bsum, d_eg_status, d_eg_out, d_eg_q, d_eg_ht;
    // fused encode + Exp-Golomb: per-segment slots and lane bit counts
    dct3d::DevBuf d_egf_slot;
    // Exp-Golomb decode: chunk exits (two passes' worth), decode status, staged stream / raster
    // (d_egd_status: the decode's four status words, then the scan's two -- one read-back per call)
    dct3d::DevBuf d_egd_exit, d_egd_status, d_egd_in, d_egd_raster, d_egd_mark, d_egd_desc;
    // d_egd_status holds two slots of the words; calls alternate between them, and the fused decode's
    // consumer zeroes the other slot for the next call (clean: known zero, no memset needed)
    int egd_slot = 0;
    bool egd_clean[2] = {true, true};
    // the sync launches (eg_sync_kernel, eg_chain_kernel, eg_front_kernel) of the last stream decode call's
    // fronts, per channel, the speculative attempt and its rerun together (dct3d_eg_sync_launches)
    uint64_t egd_launches[3] = {0, 0, 0};
    // the same for the encode stream's two status words (d_eg_status: two slots of 16 bytes)
    int eg_slot = 0;
    bool eg_clean[2] = {true, true};
    // pinned host words the entropy stages' status lands in (one DMA read-back, not a pageable copy)
    uint64_t* h_status = nullptr;
    uint64_t* h_status_dev = nullptr;  // its device-side address (decode_eg_kernel writes the words there)
    uint64_t egd_seq = 0;              // stream-decode calls so far: decode_eg_kernel's hand-off tag (h_status[6])
    uint64_t eg_seq = 0;               // stream-encode calls so far: eg_stitch_kernel's hand-off tag (h_status[7])
    // host-pointer pipeline: copy streams, slot events, double-buffered slots
    hipStream_t s_up = nullptr, s_down = nullptr;
    hipEvent_t pe_in[2] = {}, pe_done[2] = {};
    dct3d::DevBuf p_in[2], p_out[2];
    uint64_t eg_last_bytes = 0;
    // frames of any size / packed RGB24 through the fused Exp-Golomb calls (dct3d_*_eg_frames*): channels 1
    // and 2 of the host calls' device streams (channel 0: d_eg_out / d_egd_in), a gathered channel for the
    // two-step option, and the three fronts' status words (3 x 6; their marks share d_egd_mark)
    dct3d::DevBuf d_eg_out_x[2], d_egd_in_x[2], d_eg_q_ch, d_egd_status3;
    uint64_t eg_last_bytes_x[2] = {0, 0};
    // rate probe (dct3d_rate_frames*): the candidate tables' rows (host copy, device), the per-cube bits when
    // the caller keeps none, the per-(table, stack, channel) sums and their pinned host copy
    std::vector<float> rate_tabs_host;
    dct3d::DevBuf d_rate_tabs, d_rate_bits, d_rate_sums;
    uint64_t* h_rate = nullptr;
    size_t h_rate_bytes = 0;
    // distortion probe (dct3d_distortion_frames*): the tables' fp64 steps (host copy, device) and the per-cube
    // squared errors when the caller keeps none; the rows, bits, sums and pinned copy are the rate probe's
    std::vector<double> dist_steps_host;
    dct3d::DevBuf d_dist_steps, d_dist_sse;
    // per-stack quantiser tables (dct3d_*_eg_frames_vq*): the call's fp64 steps, map and palette rows in one
    // device buffer and its host copy (VqParams' layout), and -- while such a call runs the stream calls' host
    // bodies -- the kernels' view of them (else nullptr)
    // (the host copy is pinned: the upload is one asynchronous DMA, no staging and no wait; the palette's rows
    // and steps are kept from call to call and rebuilt only when the tables change)
    dct3d::DevBuf d_vq;
    uint8_t* vq_host = nullptr;
    uint8_t* vq_host_dev = nullptr;  // its device-side address (launch_vq_upload reads it)
    size_t vq_host_bytes = 0;
    std::vector<int32_t> vq_tables;
    std::vector<float> vq_rows;
    std::vector<double> vq_steps;
    // (one view per channel: vq_ch[ch] is channel ch's block {steps, FastDiv, map column}, with the cubes per
    // stack of that channel's plane in the FastDiv -- the chroma plane's under 4:2:0.  A _vq call's channels share
    // a block where their planes' geometry is the same.  vq == vq_ch.)
    dct3d::VqParams vq_ch[3] = {};
    const dct3d::VqParams* vq = nullptr;
    uint32_t vq_ch_stride = 0;  // != 0: a _vqc call's 4:4:4 RGB decode, the bytes from one channel's block to the next
    // 4:2:0 chroma subsampling (dct3d_ctx_set_chroma): the mode, the stream decode's two chroma planes
    // (S(Cb) then S(Cr), each [n_stacks * bd][ceil(h / 2)][ceil(w / 2)]: the grey stream decode writes them, the Y
    // kernel reads them)
    int chroma = DCT3D_CHROMA_444;
    dct3d::DevBuf d_c420;
    // RGB-domain distortion probe (dct3d_distortion_rgb_frames*): the decoded planes of one range of
    // stacks (pass 1 writes them, pass 2 reads them), the planes' per-cube squared errors and bits, the candidates'
    // plane slots, the per-cube RGB errors when the caller keeps none
    dct3d::DevBuf d_rgb_planes, d_rgb_psse, d_rgb_pbits, d_rgb_slots, d_rgb_cube;
    std::vector<int32_t> rgb_tables;
    // SSIM probe (dct3d_ssim_frames*): the 4 x 4 blocks' moments of one range of stacks and one channel
    // (per table the uint64 records, then the source's uint32 records) and the window kernel's partial sums; the RGB
    // and luma SSIM probe keeps a range's records of all its planes there ([plane][candidate], then [plane])
    dct3d::DevBuf d_ssim_blk, d_ssim_part;
    // RGB and luma SSIM probe (dct3d_ssim_rgb_frames*), planes mode with d_window_ssim: the plane
    // probe's windows, which the caller's [candidate][plane] layout is copied out of
    dct3d::DevBuf d_ssim_win;
};

// The runtime's helpers the probes call (defined, with their comments, in dct3d_runtime.cpp -- inside its extern "C"
// blocks, hence as extern "C++" there).
namespace dct3d {
namespace rt {
int stream_wait(dct3d_ctx* c);
void call_begin(dct3d_ctx* c);
void batch_begin(dct3d_ctx* c);
void batch_end(dct3d_ctx* c);
hipEvent_t* timer_begin(dct3d_ctx* c);
void timer_end(dct3d_ctx* c, hipEvent_t* ev);
void count_slot_used(dct3d_ctx* c, uint64_t units);
void fill_encode_params(dct3d_ctx* c, EncodeParams& P, const uint8_t* d_raster, int32_t* d_q, const Geom& g, uint64_t n_cubes);
void fill_decode_params(dct3d_ctx* c, DecodeParams& P, const int32_t* d_q, uint8_t* d_raster, const Geom& g, uint64_t n_cubes);
Variant stream_variant_of(const dct3d_ctx* c, const Geom& g);
bool colour_refused(const dct3d_ctx* c, int px);
bool c420_on(const dct3d_ctx* c, int px);
bool c420_refused(const dct3d_ctx* c, int px);
bool c420_geom(const Geom& g, int n_stacks, Geom* gc, uint64_t* n_cubes);
void c420_cube_fields(EncodeParams& P, const Geom& g, const Geom& gc);
int c420_edge(const Geom& g);
void probe_tables(dct3d_ctx* c, const int32_t* tables, int n_tables, bool want_steps);  // (dct3d_probes.cpp; the vq calls' palette too)
}  // namespace rt
}  // namespace dct3d
