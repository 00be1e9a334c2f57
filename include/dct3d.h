/*
 * dct3d.h -- C-ABI of the MI355X 3D-DCT hot path (libdct3d.so).
 *
 * Drop-in boundary for julianopiccoli/3dDCTVideoEncoding's per-stack device block.  The reference
 * C codec (3d-DCT-video-encoding-OpenCL/) does, per 8-frame stack:
 *     readCubes -> clEnqueueWriteBuffer -> dct_calculate_partial_sums -> dct_aggregate_partial_sums
 *     -> clEnqueueReadBuffer -> applyQuantization                       (encoder.c:206-260)
 *     applyDequantization -> clEnqueueWriteBuffer -> idct_calculate_partial_sums
 *     -> idct_aggregate_partial_sums -> clEnqueueReadBuffer -> writeCubes (decoder.c:246-295)
 * after a per-call OpenCL setup (encoder.c:147-197, decoder.c:153-202, OpenCLUtils.c:49-165).
 * Each entry point below names the reference region it replaces.
 *
 * Conventions (all entry points):
 *   - plain pointers and sizes, no framework types; 0 = DCT3D_OK, non-zero = DCT3D_E* code
 *     (the reference printf()s and returns 1, or exit(1)s inside OpenCLUtils.c; this library never
 *     prints and never exits -- the codec layer above prints, see codec.h);
 *   - a context owns its device buffers and its HIP stream (the reference creates its OpenCL objects
 *     per call and never releases them, encoder.c:165-197); one context per device, one host
 *     thread per context (a context is not thread-safe);
 *   - host-pointer entry points are synchronous on return (the reference's blocking
 *     clEnqueueWrite/ReadBuffer, encoder.c:209,254); *_dev entry points take device pointers and
 *     are asynchronous on the context stream (use dct3d_synchronize).  The context's own stream is a
 *     blocking stream (ordered with the legacy default stream); dct3d_ctx_set_stream selects another;
 *   - the *_stacks*, dct3d_encode_eg*, dct3d_decode_eg* and dct_opt entry points need a frame width that
 *     is a multiple of the block width and a height that is a multiple of the block height (1080 =
 *     135 * 8); the reference silently overruns otherwise, these calls return DCT3D_EINVAL.  Frames of
 *     any other size (1366 x 768, 1680 x 1050, ...) go through dct3d_encode_frames* / dct3d_decode_frames*
 *     (int32 cubes) or dct3d_encode_eg_frames* / dct3d_decode_eg_frames* (Exp-Golomb streams), which pad
 *     by edge replication and crop inside the transform kernels.
 *
 * Layouts:
 *   raster  : u8 frames, frame-major, row-major (the raw grayscale file format, encoder.c:21-27);
 *             a "stack" is DCT_BLOCK_DEPTH consecutive frames.
 *   cubes   : cube-major: for each stack, block-row by, block-col bx, then (z, y, x) inside the cube
 *             (readCubes order, encoder.c:29-41; Java Encoder.java:75-89).
 *
 * Numerics (parity target = the reference Java codec, BASELINE.json north_star):
 *   - dct3d_encode_stacks*: quantised int32 coefficients equal to the Java path
 *       Math.round(DCT.apply(...)[k] / max(1, 5(x+y+z)))          (Encoder.java:82, DCT.java:41-59)
 *     bit for bit: computed in fp32 under a rigorous per-coefficient error bound; any coefficient
 *     whose quotient is within that bound of a rounding tie is recomputed by replaying the Java
 *     fold exactly (fp64, HashMap group order), and the DC from the exact integer cube sum.
 *   - dct3d_decode_stacks*: u8 pixels equal to the Java path (byte) clamp(InverseDCT(...))
 *     (InverseDCT.java:33-82, Decoder.java:112) bit for bit, same certify-or-replay scheme (fp64).
 *   - float outputs (dct_opt, dct3d_forward_f32, dct3d_inverse_f32): fp64 internal arithmetic;
 *     |err| <= 1e-9 * max(1, |value|) before the final rounding to the output type.
 */
#ifndef DCT3D_H_
#define DCT3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCT3D_OK 0
#define DCT3D_EINVAL 1      /* bad argument / unsupported block dims / misaligned frame size */
#define DCT3D_EDEVICE 2     /* no such HIP device, or a HIP runtime error */
#define DCT3D_ENOMEM 3      /* device or host allocation failed */
#define DCT3D_EKERNEL 4     /* a kernel launch failed */
#define DCT3D_ENOSPC 5      /* an output buffer is too small (nothing was written past its end) */
#define DCT3D_ENODATA 6     /* an input stream ends before the requested data is complete */

#define DCT3D_ABI_VERSION 9

typedef struct dct3d_ctx dct3d_ctx;

/* Per-call statistics of the certify-or-replay scheme (last encode/decode call on the ctx). */
typedef struct {
    uint64_t n_units;          /* coefficients (encode) or pixels (decode) produced by the last call */
    uint64_t n_flagged;        /* units of the last call re-done by the exact Java fold (decode: the 32
                                  pixels of every lane with an uncertified pixel) */
    /* HIP-event timing of every encode/decode call since dct3d_reset_timers (profiling on) */
    uint64_t n_timed;          /* calls timed */
    double kernel_ms_total;    /* main transform kernel, summed */
    double aux_ms_total;       /* the call's auxiliary launch, summed (fused Exp-Golomb encode: the
                                  compaction kernel); 0 for single-launch calls */
    uint64_t n_rechecked;      /* 8x8x8 encode: units of the last call the fp32 certificate left open
                                  and the fp64 second certificate settled (not counted in n_flagged) */
} dct3d_stats;

/* Transform-plan introspection (host only, no device needed). */
typedef struct {
    int cube_size;
    int n_mults;          /* sum over coefficients of Java multiplication groups (11,567 for 8^3) */
    int treeified;        /* 1 if Java's HashMap would have treeified a bin (fold order then unverified) */
    double coef_dc;       /* the single DC group coefficient (DCT.java:110 with k = 0) */
    double dec_G, dec_E;  /* decode certification: margin = L1 * dec_G + dec_E, L1 = sum |q * step| of the cube */
    float enc_rstep[32];  /* encode certification per s = kx+ky+kz: fp32(1/step[s]) (reference: max(1,5s)) */
    float enc_G[32];      /*   threshold_s = 0.5 - (A * G_s + E_s), A = max|x - mean| of the cube */
    float enc_E[32];
    double enc_thr64[32]; /* 8x8x8 second certificate: settled iff |q64 - rint(q64)| < enc_thr64[s] */
    float dec_l1_max;     /* decode: a cube with L1 >= dec_l1_max takes the exact replay (|v| < 2^15) */
} dct3d_plan_info;

/* The plan for block dims (bw, bh, bd): the MI355X build's DCT.initialize (DCT.java:77-163) and
 * InverseDCT.initialize (InverseDCT.java:87-133).  Optional arrays (NULL to skip), cs = bw*bh*bd:
 *   ngroups [cs]       multiplication groups of each output coefficient k (fold length)
 *   coef    [cs * 64]  group coefficients of k in Java HashMap iteration (fold) order
 *   group_of[cs * cs]  fold index of input n in output k's fold (0xFF: dropped, key == 0)
 *   enc_K   [cs]       fp32 rounding-error bound of coefficient k per unit max|x - mean| */
int dct3d_plan_query(int bw, int bh, int bd, dct3d_plan_info *info, int32_t *ngroups, double *coef,
                     uint8_t *group_of, double *enc_K);

/* ABI version of the loaded library (DCT3D_ABI_VERSION). */
int dct3d_abi_version(void);
const char *dct3d_strerror(int code);

/* Replaces the per-call OpenCL setup: getDeviceId/getMaxWorkGroupSize (OpenCLUtils.c:69-104),
 * clCreateContext/buildKernel/clCreateBuffer/clCreateCommandQueue/clCreateKernel
 * (encoder.c:158-197, decoder.c:163-202).  `device` is a 0-based HIP ordinal (the codec layer
 * maps the reference's 1-based platformIndex, main.c:33-37).  Block dims are the codec.h macros
 * DCT_BLOCK_WIDTH/HEIGHT/DEPTH (codec.h:11-13); supported: 8 x 8 x 8 and 8 x 8 x 4. */
int dct3d_ctx_create(int device, int block_w, int block_h, int block_d, dct3d_ctx **out);
void dct3d_ctx_destroy(dct3d_ctx *ctx);

/* Use an external hipStream_t (e.g. a framework's current stream) instead of the ctx-owned one.
 * NULL restores the ctx-owned stream.  Work enqueued afterwards is ordered after the previous
 * stream's work by an event recorded on the previous stream, which therefore MUST STILL EXIST when
 * this is called: switch away from a caller's stream before destroying it.  (Should HIP reject the
 * previous handle, a device-wide synchronisation orders the work instead -- but a destroyed stream's
 * handle may already name a new stream, so that is no guarantee.) */
int dct3d_ctx_set_stream(dct3d_ctx *ctx, void *hip_stream);
/* The ctx's device ordinal, block depth and the hipStream_t its calls run on (any pointer may be
 * NULL).  Lets companion libraries (libdct3d_diag.so) queue work in order with the ctx's. */
int dct3d_ctx_info(const dct3d_ctx *ctx, int *device, int *block_d, void **hip_stream);
/* Test / diagnostic options of a ctx.  Each one changes only HOW later calls reach their results
 * (the results stay bit-identical): tests use them to drive the rare paths.  value 0 restores the
 * default.  Unknown options: DCT3D_EINVAL. */
#define DCT3D_OPT_DEC_MARGIN 2        /* added to the decode certification margin: lanes go to the in-wave
                                         exact replay */
#define DCT3D_OPT_ENC_NO_RECHECK 3    /* 1: the 8x8x8 encode skips its fp64 second certificate, so every
                                         coefficient the fp32 certificate leaves open takes the Java fold */
#define DCT3D_OPT_EG_TWO_STEP 5       /* 1: dct3d_encode_eg / dct3d_decode_eg through int32 cubes; also
                                         dct3d_encode_eg_frames, dct3d_decode_eg_frames[_dev] */
#define DCT3D_OPT_EG_NO_RESOLVE 6     /* 1: Exp-Golomb decode sync by plain confirming passes only */
#define DCT3D_OPT_EG_FORCE_RETRY 8    /* test: the Exp-Golomb decode's speculative front reports an unresolved
                                         pass 0, so the call takes its skip-and-rerun path (same results) */
#define DCT3D_OPT_EG_DEC_GROUPS 9     /* stream -> raster decode: groups of 2,048 values per wave, the next
                                         group's loads in flight during the current one (1, 2, 4, 8; 0: 8).
                                         Does not act on dct3d_decode_eg_frames*'s own kernels (grey frames
                                         of any size: always 8; packed RGB24: always 1) */
#define DCT3D_OPT_EG_FUSED_FRONT 10   /* 1: the Exp-Golomb decode's speculative front as ONE launch (the
                                         resolving sync pass, the chunk scan and the mark pass fused, a
                                         decoupled look-back for the chunks' value indices) instead of three
                                         (A/B: measured slower) */
#define DCT3D_OPT_QUANT_FORCE_TABLE 11 /* test: 1: a context whose quantiser is the reference table runs the
                                         table kernels (dct3d_ctx_set_quant) too, reading max(1, 5 s) from
                                         the table instead of having it in their text */
/* Not a test option: the colour transform of the packed RGB24 stream calls and the rate probe (additive to ABI
 * 9; see "YCbCr colour transform" below).  Values DCT3D_COLOUR_PLANES (0, the default) and DCT3D_COLOUR_YCBCR
 * (1); any other value: DCT3D_EINVAL. */
#define DCT3D_OPT_COLOUR 12
#define DCT3D_COLOUR_PLANES 0
#define DCT3D_COLOUR_YCBCR 1
int dct3d_ctx_set_option(dct3d_ctx *ctx, int option, double value);

/* ---------------------------------------------------------------------------------------------
 * YCbCr colour transform (additive to ABI 9).  With DCT3D_OPT_COLOUR =
 * DCT3D_COLOUR_YCBCR the three streams of a packed RGB24 call hold the Y, Cb and Cr planes of the frames
 * instead of their R, G and B planes.  The transform is JFIF full-range BT.601 in 16-bit fixed point and is
 * DEFINED by these integers (>> arithmetic, i.e. floor; all inputs and outputs bytes):
 *   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *   Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
 *   u = Cb - 128, v = Cr - 128
 *   R' = clamp(Y + (( 91881 v + 32768) >> 16), 0, 255)
 *   G' = clamp(Y + ((-22554 u - 46802 v + 32768) >> 16), 0, 255)
 *   B' = clamp(Y + ((116130 u + 32768) >> 16), 0, 255)
 * Write T for the forward transform of a packed raster (Y, Cb, Cr in the places of R, G, B) and T^-1 for the
 * inverse.  With channels == 3 and the option on:
 *   dct3d_encode_eg_frames[_dev], dct3d_encode_eg_frames_vq[_dev]  give, on `frames`, every result the same
 *       call gives with the option off on T(frames): the streams byte for byte, total_bits[ch], DCT3D_ENOSPC,
 *       the statistics;
 *   dct3d_rate_frames[_dev]  likewise: bits, d_cube_bits, n_flagged;
 *   dct3d_decode_eg_frames[_dev], dct3d_decode_eg_frames_vq[_dev]  write T^-1 of the frames the same call
 *       writes with the option off; end_bit[ch], the error codes and the statistics are unchanged.
 * The transform runs inside those calls' kernels, on the bytes a lane holds anyway: no launch and no memory
 * traffic is added.  A round trip T^-1(T(x)) is off by at most 1 per sample before any quantisation.
 * With channels == 1 the option does nothing (the same kernels run).  The calls that have no colour stage
 * refuse the option instead of ignoring it -- DCT3D_EINVAL, nothing launched, the next call unaffected:
 *   dct3d_encode_frames* / dct3d_decode_frames* with channels == 3 and dct3d_*_stacks_rgb* (int32 cubes);
 *   dct3d_distortion_frames* with channels == 3 (its error would be the Y, Cb, Cr planes', not the samples');
 *   the _eg_frames* calls with channels == 3 on a context that also has DCT3D_OPT_EG_TWO_STEP (the _vq calls
 *       refuse that option anyway).
 * DCT3D_OPT_DEC_MARGIN, DCT3D_OPT_EG_NO_RESOLVE and DCT3D_OPT_EG_FORCE_RETRY act as without the option.
 * ------------------------------------------------------------------------------------------- */

/* ---------------------------------------------------------------------------------------------
 * 4:2:0 chroma subsampling (additive to ABI 9).  A mode of the context, not a
 * DCT3D_OPT_* id, on top of DCT3D_OPT_COLOUR = DCT3D_COLOUR_YCBCR: with DCT3D_CHROMA_420 the Cb and Cr planes of
 * a packed RGB24 stream call are coded at a quarter of the samples.  With T and T^-1 the colour transform above,
 * on width x height frames, the mode is DEFINED by these integers:
 *   chroma size   cw = (width + 1) / 2, ch = (height + 1) / 2 (dct3d_chroma_size).  No temporal subsampling: the
 *                 block depth is the context's.
 *   subsample S   per frame and chroma plane p: pad p to even width and height by repeating its last column and
 *                 row, then c[j][i] = (p[2j][2i] + p[2j][2i+1] + p[2j+1][2i] + p[2j+1][2i+1] + 2) >> 2: a box
 *                 filter on the 8-bit Cb / Cr values of T (S after T, not a transform of summed R, G, B).
 *   upsample U    pixel replication, p[y][x] = c[y >> 1][x >> 1], cropped to width x height.
 *   the streams   0: the Y plane, width x height; 1: S(Cb), cw x ch; 2: S(Cr), cw x ch -- each with its own edge
 *                 padding (the next multiples of 8), its own cubes per stack, ceil(width / 8) ceil(height / 8) and
 *                 ceil(cw / 8) ceil(ch / 8), and its own length.
 * With channels == 3, the transform on and the mode on:
 *   dct3d_encode_eg_frames[_dev], dct3d_encode_eg_frames_vq[_dev]  stream k, total_bits[k] and DCT3D_ENOSPC are
 *       those of the grey call (channels == 1) on plane k of (Y, S(Cb), S(Cr)) of T(frames), under the same table
 *       and carry; the map of a _vq call is per stack and shared by the three channels;
 *   dct3d_decode_eg_frames[_dev], dct3d_decode_eg_frames_vq[_dev]  from three streams of those value counts, the
 *       frames are T^-1 of (Y, U(Cb), U(Cr)) of the three grey decodes at (width, height), (cw, ch), (cw, ch);
 *       end_bit[k] is the grey call's; a short or corrupt stream gives the code and end bits the 4:4:4 call gives
 *       for the same fault in the same stream, and the frames stay untouched when any stream is bad;
 *   dct3d_rate_frames[_dev]  bits[t][s][k] is the grey call's of plane k.  The per-cube layout is ragged: with a
 *       non-NULL d_cube_bits dct3d_rate_frames_dev returns DCT3D_EINVAL; only the totals are offered;
 *   dct3d_get_stats  n_units is the sum over the three grey calls.
 * With channels == 1 the mode does nothing.  With channels == 3 and DCT3D_COLOUR_PLANES those calls return
 * DCT3D_EINVAL before anything is queued.  The calls that refuse the colour option keep refusing it.
 *
 * dct3d_ctx_set_chroma: DCT3D_CHROMA_444 (the default) or DCT3D_CHROMA_420; a NULL context or any other value:
 *   DCT3D_EINVAL, nothing changes.  A context that never sets DCT3D_CHROMA_420 launches what it launched before.
 * dct3d_ctx_get_chroma: the mode.  dct3d_chroma_size: (cw, ch) of positive (w, h), no context needed.
 * ------------------------------------------------------------------------------------------- */
#define DCT3D_CHROMA_444 0
#define DCT3D_CHROMA_420 1
int dct3d_ctx_set_chroma(dct3d_ctx *ctx, int mode);
int dct3d_ctx_get_chroma(const dct3d_ctx *ctx, int *mode);
int dct3d_chroma_size(int w, int h, int *cw, int *ch);

/* ---------------------------------------------------------------------------------------------
 * Quantiser tables (additive to ABI 9).  A quantiser is one integer step per s = kx + ky + kz of a
 * coefficient's indices, 0 <= s <= bw + bh + bd - 3 (22 entries at 8x8x8, 18 at 8x8x4), each step in
 * [1, 255].  The reference codec's is step[s] = max(1, 5 s) (Encoder.java:75-89, Decoder.java:78-96),
 * and a context starts with it.  With any other table the values are DEFINED as that Java code's with
 * step[x + y + z] in place of Math.max(1, 5 * (x + y + z)):
 *   encode  q = Math.round(c_java / step)     (IEEE double division of the Java fold's value, the DC's
 *                                              included, then Math.round's exact half-up rounding)
 *   decode  (double) q * step, Java's InverseDCT fold, (byte) clamp
 * and every output is either certified equal to that definition or replayed exactly, as with the
 * reference table: there is no approximate mode.  Small steps certify less (the bound scales with
 * 1 / step), so more coefficients take the exact paths; dct3d_get_stats reports them.
 *
 * dct3d_ctx_set_quant: n must be bw + bh + bd - 2, every step in [1, 255] (else DCT3D_EINVAL, the table
 *   unchanged); steps == NULL restores the reference table (n is then ignored).  It waits for the
 *   context's stream, rebuilds the plan's certification tables and uploads them: it is a property of
 *   the context, not a per-call argument, and MUST NOT race a call in flight on this context from
 *   another thread.  A context whose table equals the reference table -- never set, or set explicitly --
 *   runs the same kernels as before this interface existed.
 * dct3d_ctx_get_quant: copies the table out (n as above).
 * dct3d_plan_query_quant: dct3d_plan_query for a table (steps == NULL: the reference table).
 *
 * Every raster call honours the context's table, in its _dev and host-pointer forms:
 * dct3d_encode_stacks*, dct3d_decode_stacks*, the _rgb calls, dct3d_encode_frames*, dct3d_decode_frames*,
 * dct3d_encode_eg*, dct3d_decode_eg*, the _eg_frames* calls, with or without DCT3D_OPT_EG_TWO_STEP.
 * (With a table other than the reference's, the grey stream decode runs 8 groups per wave whatever
 * DCT3D_OPT_EG_DEC_GROUPS says.)  Calls with no quantiser in them are unaffected: the float drop-ins
 * (dct3d_forward_f32*, dct3d_inverse_f32*), the dct_opt output of dct3d_encode_stacks*, and the entropy
 * stages on int32 cubes, dct3d_eg_encode_dev and dct3d_eg_decode_dev.  libdct3d_diag.so's kernels keep
 * the reference table. */
int dct3d_ctx_set_quant(dct3d_ctx *ctx, const int32_t *steps, int n);
int dct3d_ctx_get_quant(const dct3d_ctx *ctx, int32_t *steps, int n);
int dct3d_plan_query_quant(int bw, int bh, int bd, const int32_t *steps, int n, dct3d_plan_info *info,
                           int32_t *ngroups, double *coef, uint8_t *group_of, double *enc_K);
/* Enable HIP-event timing of the kernels (reported by dct3d_get_stats). */
int dct3d_ctx_set_profiling(dct3d_ctx *ctx, int on);
int dct3d_synchronize(dct3d_ctx *ctx);
/* Reads back the device counters of the last encode/decode and resolves the timing events
 * (synchronises the stream). */
int dct3d_get_stats(dct3d_ctx *ctx, dct3d_stats *out);
int dct3d_reset_timers(dct3d_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * Native fused path (B): replaces readCubes + H2D + dct kernels + D2H + applyQuantization
 * (encoder.c:206-260) for n_stacks consecutive stacks.
 *   raster : n_stacks * block_d frames of width*height u8
 *   q_cubes: n_stacks * (width/bw) * (height/bh) cubes of bw*bh*bd int32 (cube-major)
 *   dct_opt: optional (may be NULL) fp64 DCT coefficients, same cube-major layout (the Java
 *            dctCoeff values, Encoder.java:66, for the float-DCT parity check)
 * ------------------------------------------------------------------------------------------- */
int dct3d_encode_stacks(dct3d_ctx *ctx, const uint8_t *raster, int width, int height, int n_stacks,
                        int32_t *q_cubes, double *dct_opt);
int dct3d_encode_stacks_dev(dct3d_ctx *ctx, const uint8_t *d_raster, int width, int height,
                            int n_stacks, int32_t *d_q_cubes, double *d_dct_opt);

/* Replaces applyDequantization + H2D + idct kernels + D2H + writeCubes (decoder.c:246-295). */
int dct3d_decode_stacks(dct3d_ctx *ctx, const int32_t *q_cubes, int width, int height, int n_stacks,
                        uint8_t *raster);
int dct3d_decode_stacks_dev(dct3d_ctx *ctx, const int32_t *d_q_cubes, int width, int height,
                            int n_stacks, uint8_t *d_raster);

/* ---------------------------------------------------------------------------------------------
 * Packed RGB24 video (ABI 9): the upstream capture / player format, frame-major, row-major, 3 bytes
 * per pixel in R, G, B order: uint8 [n_stacks * D][height][width][3].  The colour split and mix are
 * fused into the transform kernels: every packed byte is read (encode) or written (decode) once.
 *   rgb      n_stacks stacks of D packed frames (width, height: pixels, multiples of 8)
 *   q_cubes  int32, cube-major, laid out [stack][channel][cube][cube_size], channel = 0 R, 1 G, 2 B
 * The values are defined by the grey calls: with the planar-stacked raster that holds, for every
 * stack, its D red frames, then its D green frames, then its D blue frames,
 *   planar = rgb.reshape(n, D, H, W, 3).transpose(0, 4, 1, 2, 3).reshape(3 * n * D, H, W)
 * dct3d_encode_stacks_rgb(rgb, n) writes exactly what dct3d_encode_stacks(planar, 3 n) writes, and
 * dct3d_decode_stacks_rgb(q, n) is dct3d_decode_stacks(q, 3 n) re-interleaved.  So each (stack,
 * channel) block is byte for byte the grey path's block for that plane's stack (it can go unchanged
 * to dct3d_entropy_enc_push or dct3d_eg_encode_dev), and chunks of whole stacks stay contiguous on
 * both sides.  Statistics cover the whole call (n_units = 3 * cubes * cube_size); the options act as
 * on the grey calls.  DCT3D_EINVAL when 3 * cubes exceeds the grey calls' cube limit.
 * Conventions as the grey calls: *_dev asynchronous on the context stream, the host calls
 * synchronous and chunked by stacks.
 * Encode replaces RGBUtils split (RGBUtils.java:39-84) + per plane the work of encoder.c:206-260;
 * decode replaces per plane decoder.c:246-295 + RGBUtils mix (RGBUtils.java:86-131).
 * ------------------------------------------------------------------------------------------- */
int dct3d_encode_stacks_rgb(dct3d_ctx *ctx, const uint8_t *rgb, int width, int height, int n_stacks,
                            int32_t *q_cubes);
int dct3d_encode_stacks_rgb_dev(dct3d_ctx *ctx, const uint8_t *d_rgb, int width, int height,
                                int n_stacks, int32_t *d_q_cubes);
int dct3d_decode_stacks_rgb(dct3d_ctx *ctx, const int32_t *q_cubes, int width, int height, int n_stacks,
                            uint8_t *rgb);
int dct3d_decode_stacks_rgb_dev(dct3d_ctx *ctx, const int32_t *d_q_cubes, int width, int height,
                                int n_stacks, uint8_t *d_rgb);

/* ---------------------------------------------------------------------------------------------
 * Frames of any size (additive to ABI 9; detect by symbol): width >= 1, height >= 1, channels = 1 (grey,
 * uint8 [n_stacks * D][height][width]) or 3 (packed RGB24, uint8 [n_stacks * D][height][width][3]),
 * dense (no row padding).  With Wp = 8 ceil(width / 8), Hp = 8 ceil(height / 8), the padded raster
 * repeats each frame's last column and last row up to Wp x Hp (per channel; numpy: np.pad(frames,
 * ((0, 0), (0, Hp - height), (0, Wp - width)), mode = "edge")).  It exists nowhere in memory: the
 * kernels clamp their loads and crop their stores, and the host copies move the unpadded bytes only.
 *   encode  writes exactly what dct3d_encode_stacks (channels = 1) or dct3d_encode_stacks_rgb
 *           (channels = 3) writes for the padded raster at Wp x Hp: (Wp / 8) (Hp / 8) cubes per stack
 *           (RGB: per stack and channel, [stack][channel][cube]);
 *   decode  writes the top-left height x width part of what dct3d_decode_stacks[_rgb] writes at
 *           Wp x Hp, densely, and nothing else.
 * When width and height are multiples of 8 these calls are the *_stacks* calls (the same kernels).
 * Statistics count the padded work (n_units = cubes * cube_size, x 3 for RGB); the options act as on
 * the *_stacks* calls.  DCT3D_EINVAL: NULL context or buffers, channels not 1 or 3, width or height
 * <= 0, channels * padded cubes past the cube limit.  Conventions as the *_stacks* calls: *_dev
 * asynchronous on the context stream, the host calls synchronous and chunked by stacks.
 * ------------------------------------------------------------------------------------------- */
int dct3d_encode_frames(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int channels,
                        int n_stacks, int32_t *q_cubes);
int dct3d_encode_frames_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int channels,
                            int n_stacks, int32_t *d_q_cubes);
int dct3d_decode_frames(dct3d_ctx *ctx, const int32_t *q_cubes, int width, int height, int channels,
                        int n_stacks, uint8_t *frames);
int dct3d_decode_frames_dev(dct3d_ctx *ctx, const int32_t *d_q_cubes, int width, int height, int channels,
                            int n_stacks, uint8_t *d_frames);

/* ---------------------------------------------------------------------------------------------
 * Reference-faithful drop-in (A): the exact data flow of the OpenCL block, float cube-major in,
 * float cube-major out (kernelInputData -> kernelOutputData, encoder.c:165-254 / decoder.c:
 * 170-292).  The caller keeps readCubes/applyQuantization (forward) and applyDequantization/
 * writeCubes (inverse) on the host, exactly as the reference does.
 *   dct3d_forward_f32: orthonormal 3D DCT-II of each cube (dct_* kernels, 3dDCT.cl:43-143)
 *   dct3d_inverse_f32: 3D inverse DCT clamped to [0,255] (idct_* kernels, 3dDCT.cl:164-265)
 * ------------------------------------------------------------------------------------------- */
int dct3d_forward_f32(dct3d_ctx *ctx, const float *cubes, size_t n_cubes, float *coeffs);
int dct3d_inverse_f32(dct3d_ctx *ctx, const float *coeffs, size_t n_cubes, float *pixels);
int dct3d_forward_f32_dev(dct3d_ctx *ctx, const float *d_cubes, size_t n_cubes, float *d_coeffs);
int dct3d_inverse_f32_dev(dct3d_ctx *ctx, const float *d_coeffs, size_t n_cubes, float *d_pixels);

/* ---- Exp-Golomb stage on the device -----------------------------------------
 * Replaces applyExpGolombCoding (encoder.c:60-71) over expGolomb_writeValue (ExpGolomb.c:32-64) /
 * ExpGolombWriter.java:19-49: the signed order-0 Exp-Golomb stream of n_cubes consecutive cube-major
 * int32 cubes, each in diagonal-slice order (cubeUtils_diagonalSlices, CubeUtils.c:5-46), MSB first,
 * continuing a stream whose partial byte holds `carry_byte` with `carry_bits` (0..7) bits used (the
 * byte the reference carries from stack to stack, expGolomb_freeBuffer, ExpGolomb.c:112-130).
 * d_out (device, 4-byte aligned, out_cap bytes) receives ceil(total_bits / 32) little-endian words,
 * i.e. the stream bytes followed by zero padding; *total_bits = carry_bits + the bits written.
 * Values must satisfy |v| < 2^30 (quantised 8-bit content stays below 2^13), else DCT3D_EINVAL.
 * DCT3D_ENOSPC when out_cap is too small (*total_bits is still set; d_out is untouched).
 * Returns once *total_bits is known (the last kernel, eg_stitch_kernel, hands it to the host as it
 * starts); the last words of d_out complete on the context stream (dct3d_synchronize, or stream order).
 * d_q and d_out must stay valid, and d_q unchanged, until the context stream reaches that point. */
int dct3d_eg_encode_dev(dct3d_ctx *ctx, const int32_t *d_q, uint64_t n_cubes, uint8_t carry_byte, int carry_bits,
                        uint8_t *d_out, uint64_t out_cap, uint64_t *total_bits);

/* Host raster in, Exp-Golomb stream kept on the device: encoder.c:206-274 up to (not including) the
 * deflate -- readCubes + DCT + quantisation + applyExpGolombCoding for n_stacks stacks, one H2D copy
 * of the raw bytes.  *total_bits as above; fetch the bytes with dct3d_eg_fetch. */
int dct3d_encode_eg(dct3d_ctx *ctx, const uint8_t *raster, int width, int height, int n_stacks, uint8_t carry_byte,
                    int carry_bits, uint64_t *total_bits);

/* Device raster in, device stream out, fused: encoder.c:206-274 up to the deflate
 * (readCubes + DCT + quantisation + applyExpGolombCoding) for n_stacks stacks of d_raster, without
 * the int32 cube-major intermediate -- uncertified coefficients are replayed exactly inside the
 * transform kernel, and each wave codes its 8 cubes straight into the stream.  The stream format,
 * carry, d_out and *total_bits are those of dct3d_eg_encode_dev (the bytes are identical to
 * dct3d_encode_stacks_dev followed by dct3d_eg_encode_dev).  DCT3D_ENOSPC when out_cap is too small
 * (*total_bits is still set; d_out is untouched).  Returns as dct3d_eg_encode_dev: once *total_bits is
 * known, the last words completing on the context stream; d_raster and d_out must stay valid, and d_raster
 * unchanged, until the context stream reaches that point. */
int dct3d_encode_eg_dev(dct3d_ctx *ctx, const uint8_t *d_raster, int width, int height, int n_stacks,
                        uint8_t carry_byte, int carry_bits, uint8_t *d_out, uint64_t out_cap, uint64_t *total_bits);

/* Copies the first `nbytes` bytes of the last dct3d_encode_eg stream to host memory. */
int dct3d_eg_fetch(dct3d_ctx *ctx, uint8_t *out, uint64_t nbytes);

/* Diagonal-slice order of a bw x bh x bd cube (CubeUtils.c:5-46): out[i] = x + bw*y + bw*bh*z of the
 * i-th position (introspection / tests). */
int dct3d_diagonal_order(int bw, int bh, int bd, uint16_t *out);

/* Inverse of the Exp-Golomb stage (expGolomb_readValue, ExpGolomb.c:66-110 / ExpGolombReader.java;
 * Decoder.java:78-96 places value i of a cube at diagonal position i; decoder.c:210-236): decodes
 * n_cubes cubes (n_cubes * cube_size values) from the device stream d_bytes (4-byte aligned,
 * nbytes) starting at bit start_bit, into cube-major int32 d_q.  Parallel: self-synchronising
 * chunks of the stream (no index is needed in the file).  *end_bit = the bit after the last value.
 * DCT3D_ENODATA if the stream ends first, DCT3D_EINVAL if it is corrupt (a code with 32 or more
 * leading zeros).  Synchronises the context stream. */
int dct3d_eg_decode_dev(dct3d_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes, uint64_t start_bit, uint64_t n_cubes,
                        int32_t *d_q, uint64_t *end_bit);

/* Device stream in, device raster out, fused: decoder.c:209-295 after the inflate
 * for n_stacks stacks -- Exp-Golomb decode, reorder, dequantisation, IDCT, clamp/truncate -- without the
 * int32 cube-major intermediate: the decode kernel parses each of its cubes from the stream directly.
 * Stream arguments, *end_bit and errors as dct3d_eg_decode_dev; the raster as dct3d_decode_stacks_dev:
 * the call returns once *end_bit and the verdict are known (the decode kernel hands them to the host as
 * it starts), and the raster completes asynchronously on the context stream (use dct3d_synchronize, or
 * read it in stream order).  d_bytes and d_raster must stay valid, and d_bytes unchanged, until the context
 * stream reaches that point: the decode kernel, and its rare exact replay, still read the stream after the
 * call has returned. */
int dct3d_decode_eg_dev(dct3d_ctx *ctx, const uint8_t *d_bytes, uint64_t nbytes, uint64_t start_bit, int width,
                        int height, int n_stacks, uint8_t *d_raster, uint64_t *end_bit);

/* Host stream in, raster out: decoder.c:209-295 after the inflate -- Exp-Golomb decode, reorder,
 * dequantisation, IDCT, clamp/truncate and writeCubes for n_stacks stacks, on the device; only the
 * stream and the u8 frames cross PCIe.  bytes[0..nbytes) holds the stream from bit start_bit (0..7). */
int dct3d_decode_eg(dct3d_ctx *ctx, const uint8_t *bytes, uint64_t nbytes, int start_bit, int width, int height,
                    int n_stacks, uint8_t *raster, uint64_t *end_bit);

/* The cost of the last stream decode call on the context (additive to ABI 9; detect by symbol; DESIGN.md
 * section 4b): the sync launches its fronts issued, the speculative attempt and its rerun together.  A front
 * issues 1 on a stream whose chunks all fall into step (every encoder's output), and at most
 * ceil(n_chunks / 256) + 3 on any stream, n_chunks = ceil((8 nbytes - start_bit) / 512).  A call with three
 * streams (packed RGB24) has a front per stream: *max_per_front is the largest of their counts, *sum their sum;
 * one stream: both are its count.  0 before the first such call.  No device work, no synchronisation. */
int dct3d_eg_sync_launches(const dct3d_ctx *ctx, uint64_t *max_per_front, uint64_t *sum);

/* ---------------------------------------------------------------------------------------------
 * Fused stream encode and decode for frames of any size, grey or packed RGB24 (additive to ABI 9; detect by
 * symbol): raster -> Exp-Golomb streams and back with no int32 intermediate, as dct3d_encode_eg* /
 * dct3d_decode_eg* do for grey frames at multiples of 8.  width, height >= 1, channels = 1 or 3, frames
 * dense, as for dct3d_encode_frames.  Arrays marked [] have `channels` entries.
 * ONE STREAM PER CHANNEL (the codec's file format: .red, .green, .blue, each the grey format of its plane).
 * With q = dct3d_encode_frames(frames) viewed as [n_stacks][channels][C][cube_size], C the cubes of the
 * padded raster per stack and channel:
 *   encode  stream ch is exactly what dct3d_eg_encode_dev writes for the n_stacks * C cubes q[:, ch] in stack
 *           order, continuing carry_byte[ch] / carry_bits[ch]; word padding, 4-byte alignment of d_out[ch]
 *           and total_bits[ch] as there.  Cube g of stream ch is RGB cube g.
 *   decode  the inverse: d_frames receives what dct3d_decode_frames gives for the q whose channel blocks
 *           the streams hold -- the cropped height x width frames and nothing else.  end_bit[ch] as
 *           dct3d_decode_eg_dev's.
 * Errors.  DCT3D_EINVAL: the cases of dct3d_encode_frames, a NULL array, a misaligned d_out[ch] /
 * d_bytes[ch], carry_bits[ch] outside 0..7 (start_bit[ch] outside 0..7 for the host decode).  DCT3D_ENOSPC:
 * some out_cap[ch] is too small; every total_bits[ch] is still set and no byte at or past any out_cap[ch] is
 * written (channels that fit may have been written).  DCT3D_ENODATA / DCT3D_EINVAL: a stream is short /
 * corrupt; end_bit[ch] is set for every stream whose own verdict is good (the others keep start_bit[ch]), the
 * first bad stream's code is returned, and the frames are then unspecified.
 * With channels == 1 and width, height multiples of 8 the calls ARE dct3d_encode_eg[_dev] /
 * dct3d_decode_eg[_dev] (handed over before anything else: the same code, the same early return).
 * Returns (otherwise):
 *   dct3d_encode_eg_frames_dev  one launch chain per channel, back to back on the context stream; the call
 *       waits for each chain's total before it queues the next and returns once the last total_bits[ch] is
 *       known, as dct3d_encode_eg_dev: the last channel's last words complete on the context stream.
 *   dct3d_decode_eg_frames_dev  channels == 1: as dct3d_decode_eg_dev, once the verdict is known, the frames
 *       completing on the context stream.  channels == 3: only after all its stream work is queued and
 *       the three verdicts are read back (a copy behind the decode kernel: the frames are complete then).
 *   In every case d_frames, d_out[ch] / d_bytes[ch] must stay valid, and the inputs unchanged, until the
 *   context stream reaches that point (dct3d_synchronize, or stream order).
 *   The host calls are synchronous on return as dct3d_encode_eg (fetch with dct3d_eg_fetch_channel) /
 *   dct3d_decode_eg: one copy of the unpadded frames in, per-channel device streams, the decode in chunks of
 *   stacks.  dct3d_eg_fetch stays as is and equals channel 0.
 * Statistics count the padded work of all channels (n_units); n_flagged counts the exact replays of these
 * calls' own kernels, encode included (dct3d_encode_eg_dev's kernel reports none).  DCT3D_OPT_DEC_MARGIN,
 * DCT3D_OPT_EG_NO_RESOLVE and DCT3D_OPT_EG_FORCE_RETRY act as on the grey calls, on every channel.
 * ------------------------------------------------------------------------------------------- */
int dct3d_encode_eg_frames_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int channels,
                               int n_stacks, const uint8_t carry_byte[], const int carry_bits[],
                               uint8_t *const d_out[], const uint64_t out_cap[], uint64_t total_bits[]);
int dct3d_encode_eg_frames(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int channels,
                           int n_stacks, const uint8_t carry_byte[], const int carry_bits[], uint64_t total_bits[]);
/* Copies the first `nbytes` bytes of channel `channel`'s stream of the last dct3d_encode_eg_frames (or, channel
 * 0, dct3d_encode_eg) to host memory. */
int dct3d_eg_fetch_channel(dct3d_ctx *ctx, int channel, uint8_t *out, uint64_t nbytes);
int dct3d_decode_eg_frames_dev(dct3d_ctx *ctx, const uint8_t *const d_bytes[], const uint64_t nbytes[],
                               const uint64_t start_bit[], int width, int height, int channels, int n_stacks,
                               uint8_t *d_frames, uint64_t end_bit[]);
int dct3d_decode_eg_frames(dct3d_ctx *ctx, const uint8_t *const bytes[], const uint64_t nbytes[],
                           const int start_bit[], int width, int height, int channels, int n_stacks,
                           uint8_t *frames, uint64_t end_bit[]);

/* -------------------------------------------------------------------------------------------
 * Rate probe (additive to ABI 9: detect it by symbol).  The exact size of the Exp-Golomb streams under
 * several quantiser tables, from one transform per cube and with no stream written.
 *   frames, width, height, channels, n_stacks   as dct3d_encode_eg_frames*.
 *   tables    host, [n_tables][bw + bh + bd - 2] steps, each in [1, 255]; NULL with n_tables == 1: the
 *             context's current table.  1 <= n_tables <= DCT3D_RATE_MAX_TABLES.
 *   bits      host, [n_tables][n_stacks][channels]: bits[t][s][ch] is the number of bits that
 *             dct3d_encode_eg_frames appends to stream ch for stack s on a context whose table is tables[t]
 *             -- over the cubes q[s, ch] of dct3d_encode_frames under that table, the sum of the code widths
 *             (2n - 1 for a code of n bits, code = max(2v, 1 - 2v)).  Summed over the stacks it is that call's
 *             total_bits[ch] - carry_bits[ch].  Exact; there is no estimate.
 *   d_cube_bits   optional device memory, [n_tables][n_stacks][channels][C] (C: the padded cubes per stack and
 *             channel): the same sum per cube (a cube costs < 2^15 bits).
 * The call neither reads (tables != NULL) nor changes the context's quantiser and is synchronous on return; the
 * host-pointer call moves the frames in chunks of whole stacks (64 MiB of staging at most, or one stack), its
 * numbers and statistics those of one call.
 * Errors.  DCT3D_EINVAL: the cases of dct3d_encode_frames, n_tables outside 1..DCT3D_RATE_MAX_TABLES, tables
 * == NULL with n_tables != 1, bits == NULL, a step outside [1, 255] (nothing is launched then).
 * Statistics: n_units = padded coefficients of all channels x n_tables; n_flagged = the coefficient values
 * settled by the exact Java fold, counted per table that left the coefficient open.  With n_tables == 1 it is
 * what dct3d_encode_eg_frames_dev reports for the same frames under that table, where that call counts.
 * ------------------------------------------------------------------------------------------- */
#define DCT3D_RATE_MAX_TABLES 32
int dct3d_rate_frames_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int channels,
                          int n_stacks, const int32_t *tables, int n_tables,
                          uint64_t *bits, uint16_t *d_cube_bits);
int dct3d_rate_frames(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int channels,
                      int n_stacks, const int32_t *tables, int n_tables, uint64_t *bits);

/* ---------------------------------------------------------------------------------------------
 * Distortion probe (additive to ABI 9; detect by symbol): the exact squared error of encode + decode under
 * several quantiser tables, from one row load and one forward transform per cube; no coefficient and no
 * decoded raster is written.  With y_t = dct3d_decode_frames(dct3d_encode_frames(x)), both on
 * a context whose table is tables[t]:
 *   frames, width, height, channels, n_stacks, tables, n_tables   as dct3d_rate_frames*.
 *   sse       host, [n_tables][n_stacks][channels]: sse[t][s][ch] = sum (x - y_t)^2, as integers, over the
 *             unpadded samples of stack s, channel ch (padded columns and rows are coded, not counted).
 *   bits      host, the same shape, or NULL: exactly what dct3d_rate_frames returns for the same arguments.
 *   d_cube_sse    optional device memory, uint32 [n_tables][n_stacks][channels][C] (d_cube_bits' layout): the
 *             same sum per cube over its samples inside the frame (512 x 255^2 < 2^32).
 * The call writes no stream, neither reads (tables != NULL) nor changes the context's quantiser, honours
 * DCT3D_OPT_DEC_MARGIN as dct3d_decode_frames does, and is synchronous on return; the host-pointer call
 * moves the frames in chunks of whole stacks, as dct3d_rate_frames does.
 * Errors.  DCT3D_EINVAL: the cases of dct3d_rate_frames, with sse in the place of bits.
 * Statistics: n_units = padded coefficients of all channels x n_tables; n_flagged = the coefficient values
 * settled by the exact Java fold, counted per table as in the rate call, plus what the decode's exact replay
 * counts (32 samples per replayed lane, as dct3d_decode_frames).
 * ------------------------------------------------------------------------------------------- */
int dct3d_distortion_frames_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int channels,
                                int n_stacks, const int32_t *tables, int n_tables,
                                uint64_t *sse, uint64_t *bits, uint32_t *d_cube_sse);
int dct3d_distortion_frames(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int channels,
                            int n_stacks, const int32_t *tables, int n_tables, uint64_t *sse, uint64_t *bits);

/* ---------------------------------------------------------------------------------------------
 * RGB-domain distortion probe (additive to ABI 9; detect by symbol): the exact squared error, in
 * the RGB pixels, of the packed RGB24 stream encode + decode under a list of (Y, Cb, Cr) table triples, in all
 * three colour modes of the context: planes, DCT3D_COLOUR_YCBCR, and DCT3D_CHROMA_420 on top.  Let y_c be what
 * dct3d_decode_eg_frames_vqc(dct3d_encode_eg_frames_vqc(x)) returns when every row of the [n_stacks][3] map is
 * cand[c], in the context's colour and chroma mode.
 *   frames, width, height, n_stacks   packed RGB24 frames of any size, as dct3d_rate_frames* with channels == 3.
 *   tables, n_tables   the palette, as dct3d_rate_frames* (NULL with n_tables == 1: the context's table).
 *   cand      host, [n_cand][3] palette indices (Y | R, Cb | G, Cr | B), 1 <= n_cand <= DCT3D_RATE_MAX_TABLES;
 *             NULL: n_cand == n_tables and candidate i = (i, i, i).
 *   sse       host, [n_cand][n_stacks], required: sse[c][s] = sum (x - y_c)^2, as integers, over the unpadded
 *             pixels of stack s and their three bytes.
 *   plane_sse host, [n_tables][n_stacks][3], or NULL: the error of plane k under tables[t] in the plane's own
 *             domain, over the plane's own unpadded samples (ceil(w / 2) x ceil(h / 2) for chroma under 4:2:0);
 *             in planes mode exactly dct3d_distortion_frames' sse.
 *   bits      host, the same shape, or NULL: exactly dct3d_rate_frames' result in the same mode.
 *   d_cube_sse    optional device memory, uint32 [n_cand][n_stacks][C] (C: the padded cubes per stack of the
 *             frames' grid): sse per 8 x 8 x D cube over its pixels inside the frame (512 x 3 x 255^2 < 2^32).
 * When plane_sse or bits is asked for, every (table, plane) pair is coded; otherwise (YCbCr modes) only the pairs
 * some candidate uses.  The results are exact; the call writes no stream, neither reads (tables != NULL) nor
 * changes the context's quantiser, colour or chroma mode, honours DCT3D_OPT_DEC_MARGIN as the decode calls do and
 * is synchronous on return; the host-pointer call moves the frames in chunks of whole stacks, as
 * dct3d_rate_frames does.  In the YCbCr modes the decoded planes of a range of stacks live in a buffer the context
 * owns (DCT3D_RGB_PLANE_BUDGET bytes at most, or one stack's): the call walks the stacks in ranges.
 * Errors.  DCT3D_EINVAL: the cases of dct3d_rate_frames with sse in the place of bits, n_cand outside
 * 1..DCT3D_RATE_MAX_TABLES, a candidate index >= n_tables, cand == NULL with n_cand != n_tables, 4:2:0 set
 * without the colour transform.
 * Statistics: n_units = padded coefficients x tables of every launch; n_flagged as the distortion probe counts.
 * ------------------------------------------------------------------------------------------- */
#define DCT3D_RGB_PLANE_BUDGET (64u << 20)
int dct3d_distortion_rgb_frames_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int n_stacks,
                                    const int32_t *tables, int n_tables, const uint8_t *cand, int n_cand,
                                    uint64_t *sse, uint64_t *plane_sse, uint64_t *bits, uint32_t *d_cube_sse);
int dct3d_distortion_rgb_frames(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int n_stacks,
                                const int32_t *tables, int n_tables, const uint8_t *cand, int n_cand,
                                uint64_t *sse, uint64_t *plane_sse, uint64_t *bits);

/* ---------------------------------------------------------------------------------------------
 * SSIM probe (additive to ABI 9; detect by symbol): the exact windowed SSIM of encode + decode
 * under several quantiser tables, from the distortion probe's one row load and one forward transform per cube.
 *
 * Definition.  Take one plane of one frame, w x h; x is the source, y what
 * dct3d_decode_frames(dct3d_encode_frames(x)) returns under the table.  Only samples inside the frame count
 * (padded columns and rows are coded, not counted, as in dct3d_distortion_frames).
 *   Blocks.  The 4 x 4 grid has nbx = ceil(w / 4) columns and nby = ceil(h / 4) rows; block (bx, by) has the
 *   integer moments n (1 .. 16), Sx, Sy, Sxx, Syy, Sxy over its samples inside the frame.
 *   Windows.  nwx = max(nbx - 1, 1) by nwy = max(nby - 1, 1) windows (dct3d_ssim_windows); window (i, j) sums the
 *   moments of blocks i .. min(i + 1, nbx - 1) by j .. min(j + 1, nby - 1): 8 x 8 windows at a stride of 4, with
 *   fewer than 64 samples at the right and bottom edges and in frames under 5 samples wide or high.
 *   Value.  In int64, with c1 = 6.5025 and c2 = 58.5225 scaled by 10^4:
 *     A = 20000 Sx Sy + 65025 n^2                          B = 20000 (n Sxy - Sx Sy) + 585225 n^2
 *     C = 10000 (Sx^2 + Sy^2) + 65025 n^2                  D = 10000 (n Sxx - Sx^2 + n Syy - Sy^2) + 585225 n^2
 *   (every term below 2^43 in magnitude; C, D > 0).  The window's SSIM in fp64 is s = fl(fl(A B) / fl(C D)): two
 *   IEEE multiplications and one IEEE division of exactly converted integers, no addition, nothing to contract.
 *   |s| <= 1, and s == 1 for x == y.  The window's number is v = floor(s 2^24), an int32 in [-2^24, 2^24].
 *   Result.  ssim[t][s][ch] is the int64 sum of v over the windows of the D frames of stack s, plane ch, under
 *   tables[t]; the mean SSIM is sum / (2^24 D nwx nwy).  Exact; there is no estimate mode.
 *
 *   frames, width, height, channels, n_stacks, tables, n_tables   as dct3d_distortion_frames*.
 *   ssim      host, int64 [n_tables][n_stacks][channels], required.
 *   sse, bits host, the same shape, or NULL: exactly dct3d_distortion_frames' numbers for the same arguments.
 *   d_window_ssim   optional device memory, int32 [n_tables][n_stacks][channels][D][nwy][nwx]: the v of every window.
 * The call writes no stream, neither reads (tables != NULL) nor changes the context's quantiser, honours
 * DCT3D_OPT_DEC_MARGIN as dct3d_decode_frames does, and is synchronous on return; the host-pointer call moves the
 * frames in chunks of whole stacks, as dct3d_rate_frames does.  The blocks' moments live in a buffer the context
 * owns: per stack and channel D nbx nby (8 n_tables + 4) bytes, DCT3D_SSIM_BLOCK_BUDGET bytes at most (or one
 * stack's); the call walks the stacks in ranges and the channels reuse the buffer.
 * Errors.  DCT3D_EINVAL: the cases of dct3d_distortion_frames with ssim in the place of sse; with channels == 3,
 * DCT3D_OPT_COLOUR other than planes or DCT3D_CHROMA_420 set on the context (luma SSIM in the YCbCr modes is
 * not built).  dct3d_ssim_windows: DCT3D_EINVAL for w < 1, h < 1 or a NULL result.
 * Statistics: as dct3d_distortion_frames counts them.
 * ------------------------------------------------------------------------------------------- */
#define DCT3D_SSIM_BLOCK_BUDGET (16u << 20)
int dct3d_ssim_frames_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int channels,
                          int n_stacks, const int32_t *tables, int n_tables,
                          int64_t *ssim, uint64_t *sse, uint64_t *bits, int32_t *d_window_ssim);
int dct3d_ssim_frames(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int channels,
                      int n_stacks, const int32_t *tables, int n_tables,
                      int64_t *ssim, uint64_t *sse, uint64_t *bits);
int dct3d_ssim_windows(int w, int h, int *nwx, int *nwy);

/* ---------------------------------------------------------------------------------------------
 * RGB and luma SSIM probe (additive to ABI 9; detect by symbol): the SSIM above, taken on the RGB
 * bytes the packed RGB24 stream decode would write, under a list of (Y, Cb, Cr) table triples, in all three colour
 * modes of the context: planes, DCT3D_COLOUR_YCBCR, and DCT3D_CHROMA_420 on top.  The arguments are
 * dct3d_distortion_rgb_frames*'; y_c is, as there, what dct3d_decode_eg_frames_vqc(dct3d_encode_eg_frames_vqc(x))
 * returns when every row of the map is cand[c].
 *   ssim      host, int64 [n_cand][n_stacks][3], required: ssim[c][s][k] is the sum of v (the definition above) over
 *             the dct3d_ssim_windows(width, height) windows of the D frames of stack s, between plane k (R, G, B)
 *             of x and plane k of y_c.
 *   ssim_y    host, int64 [n_cand][n_stacks], or NULL (YCbCr modes only): the same sum between the luma plane of
 *             the colour transform of x (the plane the encode codes) and the decoded Y plane under
 *             tables[cand[c][0]].
 *   sse       host, [n_cand][n_stacks], or NULL: exactly dct3d_distortion_rgb_frames' sse.
 *   bits      host, [n_tables][n_stacks][3], or NULL: exactly dct3d_distortion_rgb_frames' bits.
 *   d_window_ssim   optional device memory, int32 [n_cand][3][n_stacks][D][nwy][nwx]: the v of every window.
 * Exact; the call writes no stream, neither reads (tables != NULL) nor changes the context's quantiser, colour or
 * chroma mode, honours DCT3D_OPT_DEC_MARGIN and is synchronous on return; the host-pointer call moves the frames in
 * chunks of whole stacks.  The blocks' moments of a range of stacks live in the SSIM probe's buffer: per stack
 * D nbx nby (8 n_cand + 4) P bytes, P = 3, or 4 with ssim_y; the call walks the stacks in ranges that fit both
 * DCT3D_RGB_PLANE_BUDGET (the decoded planes) and DCT3D_SSIM_BLOCK_BUDGET (the records), or one stack at a time.
 * When bits is asked for, every (table, plane) pair is coded; otherwise only the pairs some candidate uses.
 * Errors.  DCT3D_EINVAL: the cases of dct3d_distortion_rgb_frames with ssim in the place of sse; ssim_y != NULL in
 * planes mode (there is no luma plane).
 * Statistics: as dct3d_distortion_rgb_frames counts them, over the pairs that are coded.
 * ------------------------------------------------------------------------------------------- */
int dct3d_ssim_rgb_frames_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int n_stacks,
                              const int32_t *tables, int n_tables, const uint8_t *cand, int n_cand,
                              int64_t *ssim, int64_t *ssim_y, uint64_t *sse, uint64_t *bits, int32_t *d_window_ssim);
int dct3d_ssim_rgb_frames(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int n_stacks,
                          const int32_t *tables, int n_tables, const uint8_t *cand, int n_cand,
                          int64_t *ssim, int64_t *ssim_y, uint64_t *sse, uint64_t *bits);

/* ---------------------------------------------------------------------------------------------
 * Per-stack quantiser tables in the fused stream calls (additive to ABI 9; detect by symbol).
 * The four dct3d_*_eg_frames* calls with three more host arguments, copied before the call returns:
 *   tables       [n_tables][bw + bh + bd - 2] steps, each in [1, 255]: a palette of 1 <= n_tables <=
 *                DCT3D_RATE_MAX_TABLES tables (the layout the probes take).
 *   stack_table  [n_stacks], each entry < n_tables: stack s of EVERY channel is coded with
 *                tables[stack_table[s]].
 * Channel ch's stream is the stream dct3d_encode_eg_frames writes when, stack by stack, the context's table is
 * tables[stack_table[s]]: the chain of n_stacks single-stack base calls with dct3d_ctx_set_quant before each
 * and the carry of each handed to the next, byte for byte; the decode is the inverse under the same map.  Every
 * value is certified or replayed exactly under its own stack's table, as with one table.  The calls neither
 * read nor change the context's quantiser (as the probes), rebuild no plan and wait for nothing a base call
 * does not wait for.  Everything else -- frames, streams, carries, return points, DCT3D_ENOSPC with every
 * total_bits[ch] set, DCT3D_ENODATA with the good streams' end_bit[ch] -- is the base call's; n_units and
 * n_flagged are the sums the chain of base calls reports.
 * DCT3D_EINVAL in addition to the base calls' cases: a NULL among the three, n_tables outside 1..32, a step
 * outside [1, 255], a stack_table entry >= n_tables, or DCT3D_OPT_EG_TWO_STEP set on the context (the int32
 * intermediate has no table per stack: the option is refused, not ignored).  DCT3D_OPT_EG_FORCE_RETRY,
 * DCT3D_OPT_EG_NO_RESOLVE and DCT3D_OPT_DEC_MARGIN act as on the base calls.
 * dct3d_eg_fetch_channel serves dct3d_encode_eg_frames_vq as it serves dct3d_encode_eg_frames.
 * ------------------------------------------------------------------------------------------- */
int dct3d_encode_eg_frames_vq_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int channels,
                                  int n_stacks, const int32_t *tables, int n_tables, const uint8_t *stack_table,
                                  const uint8_t carry_byte[], const int carry_bits[], uint8_t *const d_out[],
                                  const uint64_t out_cap[], uint64_t total_bits[]);
int dct3d_encode_eg_frames_vq(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int channels,
                              int n_stacks, const int32_t *tables, int n_tables, const uint8_t *stack_table,
                              const uint8_t carry_byte[], const int carry_bits[], uint64_t total_bits[]);
int dct3d_decode_eg_frames_vq_dev(dct3d_ctx *ctx, const uint8_t *const d_bytes[], const uint64_t nbytes[],
                                  const uint64_t start_bit[], int width, int height, int channels, int n_stacks,
                                  const int32_t *tables, int n_tables, const uint8_t *stack_table,
                                  uint8_t *d_frames, uint64_t end_bit[]);
int dct3d_decode_eg_frames_vq(dct3d_ctx *ctx, const uint8_t *const bytes[], const uint64_t nbytes[],
                              const int start_bit[], int width, int height, int channels, int n_stacks,
                              const int32_t *tables, int n_tables, const uint8_t *stack_table, uint8_t *frames,
                              uint64_t end_bit[]);

/* ---------------------------------------------------------------------------------------------
 * A quantiser table per (stack, channel) in the fused stream calls (additive to ABI 9; detect by symbol;
 * DESIGN.md 4r).  The four _vq calls with `table_map` in the place of `stack_table`:
 *   table_map    [n_stacks][channels], each entry < n_tables: stack s of channel ch is coded with
 *                tables[table_map[s * channels + ch]].  Copied before the call returns.
 * Write col(k) for the [n_stacks] column k of the map, and plane k for channel k of the frames
 * (DCT3D_COLOUR_PLANES), plane k of rgb_to_ycbcr(frames) (DCT3D_COLOUR_YCBCR), or plane k of
 * rgb_to_ycbcr420(frames) (DCT3D_CHROMA_420 on top).  Then
 *   encode: stream k, total_bits[k] and the DCT3D_ENOSPC behaviour are those of the grey (channels == 1)
 *       dct3d_encode_eg_frames_vq call on plane k with the same palette, col(k) and carry k;
 *   decode: the frames are what the colour mode composes (the merge, T^-1, or ycbcr420_to_rgb) from the three
 *       grey _vq decodes, each under its col(k); end_bit[k] is the grey call's; a short or corrupt stream gives
 *       the _vq call's code and end bits and leaves the frames untouched.
 * With all columns equal every output is the _vq call's with that column, byte for byte; with channels == 1
 * the call is the _vq call.  Every value is certified or replayed exactly under the table of its own (stack,
 * channel).  n_units is the sum over the three grey calls; the decode's n_flagged is their sum; the encode's
 * equals the sum where all three planes are ragged and is at least the sum elsewhere (as the 4:2:0 calls').
 * DCT3D_EINVAL: the _vq calls' cases, with a table_map entry >= n_tables in the place of the stack_table one
 * (DCT3D_OPT_EG_TWO_STEP and three channels with 4:2:0 on but the colour transform off included); nothing is
 * queued.  DCT3D_OPT_EG_FORCE_RETRY, DCT3D_OPT_EG_NO_RESOLVE and DCT3D_OPT_DEC_MARGIN act as on the base calls.
 * dct3d_eg_fetch_channel serves dct3d_encode_eg_frames_vqc as it serves dct3d_encode_eg_frames.
 * ------------------------------------------------------------------------------------------- */
int dct3d_encode_eg_frames_vqc_dev(dct3d_ctx *ctx, const uint8_t *d_frames, int width, int height, int channels,
                                   int n_stacks, const int32_t *tables, int n_tables, const uint8_t *table_map,
                                   const uint8_t carry_byte[], const int carry_bits[], uint8_t *const d_out[],
                                   const uint64_t out_cap[], uint64_t total_bits[]);
int dct3d_encode_eg_frames_vqc(dct3d_ctx *ctx, const uint8_t *frames, int width, int height, int channels,
                               int n_stacks, const int32_t *tables, int n_tables, const uint8_t *table_map,
                               const uint8_t carry_byte[], const int carry_bits[], uint64_t total_bits[]);
int dct3d_decode_eg_frames_vqc_dev(dct3d_ctx *ctx, const uint8_t *const d_bytes[], const uint64_t nbytes[],
                                   const uint64_t start_bit[], int width, int height, int channels, int n_stacks,
                                   const int32_t *tables, int n_tables, const uint8_t *table_map,
                                   uint8_t *d_frames, uint64_t end_bit[]);
int dct3d_decode_eg_frames_vqc(dct3d_ctx *ctx, const uint8_t *const bytes[], const uint64_t nbytes[],
                               const int start_bit[], int width, int height, int channels, int n_stacks,
                               const int32_t *tables, int n_tables, const uint8_t *table_map, uint8_t *frames,
                               uint64_t end_bit[]);

#ifdef __cplusplus
}
#endif

#endif /* DCT3D_H_ */
