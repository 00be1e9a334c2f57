/*
 * codec.h -- reference-compatible codec entry points and block dimensions
 * (replaces 3d-DCT-video-encoding-OpenCL/codec.h:11-20).
 *
 * Same macro names as the reference; FACE_SIZE / CUBE_SIZE are parenthesised here (the reference's
 * unparenthesised `#define CUBE_SIZE FACE_SIZE * DCT_BLOCK_DEPTH` silently breaks `x / CUBE_SIZE`).
 * DCT_BLOCK_DEPTH may be overridden at compile time (8 or 4); the *_ex entry points
 * take it at run time.
 */
#ifndef DCT3D_CODEC_H_
#define DCT3D_CODEC_H_

#define DCT_BLOCK_WIDTH 8
#define DCT_BLOCK_HEIGHT 8
#ifndef DCT_BLOCK_DEPTH
#define DCT_BLOCK_DEPTH 8
#endif

#define FACE_SIZE (DCT_BLOCK_WIDTH * DCT_BLOCK_HEIGHT)
#define CUBE_SIZE (FACE_SIZE * DCT_BLOCK_DEPTH)

#ifdef __cplusplus
extern "C" {
#endif

/* encoder.c:88 / decoder.c:85.  platformIndex is the reference's 1-based device selector
 * (main.c:33-37); here it selects HIP device (platformIndex - 1).  Returns 0 on success, 1 on
 * failure after printing the reason (the reference's convention). */
int encode(char *inputFileName, char *outputFileName, int width, int height, int framesToEncode, int platformIndex);
int decode(char *inputFileName, char *outputFileName, int width, int height, int framesToDecode, int platformIndex);

/* Same, with the block depth (8 or 4) and the number of stacks per device call explicit.
 * width and height may be any size >= 1.  Multiples of 8 are coded as the reference codes them.  Any other size
 * (the reference overruns its buffers there) is padded to the next multiples of 8 by repeating each frame's last
 * column and last row inside the device transform (dct3d_encode_frames), and cropped again by decode_ex
 * (dct3d_decode_frames): the .bin is byte for byte the one encode_ex writes for the edge-padded video.  The
 * same holds for encode_rgb_ex / decode_rgb_ex; encode_multi / decode_multi need multiples of 8. */
int encode_ex(const char *inputFileName, const char *outputFileName, int width, int height, int framesToEncode,
              int platformIndex, int blockDepth, int stacksPerBatch);
int decode_ex(const char *inputFileName, const char *outputFileName, int width, int height, int framesToDecode,
              int platformIndex, int blockDepth, int stacksPerBatch);

/* Several devices (platformIndices[0 .. nDevices-1], 1-based; a device may repeat), one host thread and
 * one context each.  encode_multi: batches round-robin over the devices, their streams joined in order:
 * the same .bin as encode_ex.  decode_multi: the batches' device decodes chain on the stream position
 * (the stream has no index) and alternate over the devices; only the previous batch's raster write
 * overlaps a decode (with two or more devices), so decoding does not scale with devices.  Same return
 * convention. */
int encode_multi(const char *inputFileName, const char *outputFileName, int width, int height, int framesToEncode,
                 const int *platformIndices, int nDevices, int blockDepth, int stacksPerBatch);
int decode_multi(const char *inputFileName, const char *outputFileName, int width, int height, int framesToDecode,
                 const int *platformIndices, int nDevices, int blockDepth, int stacksPerBatch);

/* Packed RGB24 video (the upstream capture format: 3 bytes per pixel, R, G, B) <-> three streams named as
 * RGBUtils names the split planes: <namePattern>.red, .green, .blue.  Each is byte for byte the .bin that
 * encode_ex writes for that plane after `RGBUtils split`; decode_rgb_ex writes what `RGBUtils mix` makes of
 * the three decode_ex outputs.  The split and the mix run inside the device transform
 * (dct3d_encode_stacks_rgb / dct3d_decode_stacks_rgb).  One device, host entropy coder.  Same return
 * convention. */
int encode_rgb_ex(const char *inputFileName, const char *outputNamePattern, int width, int height, int framesToEncode,
                  int platformIndex, int blockDepth, int stacksPerBatch);
int decode_rgb_ex(const char *inputNamePattern, const char *outputFileName, int width, int height, int framesToDecode,
                  int platformIndex, int blockDepth, int stacksPerBatch);

/* The quantiser (dct3d.h, dct3d_ctx_set_quant): one integer step in [1, 255] per s = x + y + z of a
 * coefficient's position in its cube, blockDepth + 14 of them; the reference's is max(1, 5 s).  The .bin has no
 * header -- width, height, frame count and block depth are already the caller's to repeat at decode -- and the
 * quantiser joins them: the file format stays the reference's, and a file is decoded with the quantiser it was
 * encoded with.  With none given, every file is byte for byte what it was before quantisers existed.
 *
 * codec_parse_quant: the one parser of a quantiser given as text: "q=<int>" is step[s] = max(1, <int> * s)
 *   clipped to 255 (q=5: the reference's; <int> in [0, 255]), or a comma-separated list of exactly
 *   blockDepth + 14 steps, each in [1, 255].  Returns 0 and fills steps[0 .. blockDepth + 13], or 1 (steps
 *   untouched) on anything else.
 * codec_set_quant: the quantiser of every later encode / decode call of this process (every entry point above,
 *   on every device), as such a text; NULL or "": none.  It overrides the environment variable
 *   DCT3D_CODEC_QUANT, which holds the same text for callers that cannot add a call.  The text is parsed when
 *   a call starts, against that call's block depth: a call whose quantiser does not parse prints the reason
 *   and returns 1.  Returns 1 if the text is too long to keep (nothing changes then). */
#include <stdint.h>
int codec_parse_quant(const char *text, int blockDepth, int32_t *steps);
int codec_set_quant(const char *text);

/* A rate target in place of a quantiser (single-device encodes: encode, encode_ex, encode_rgb_ex): "rate=<bits
 * per pixel>", a positive decimal number.  The target is bpp * width * height * frames bits, counted in unpadded
 * pixels over all channels together, and it is measured on the Exp-Golomb bits BEFORE the deflate (the .bin is
 * usually smaller).  The encode makes two passes over its input file: the first prices every batch under the
 * fixed ladder q in {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64} (dct3d_rate_frames), sums the bits
 * over the file and the channels, picks the smallest q whose bits are <= the target (the largest q when none
 * fits) and prints one line "rate: q=<n> bits=<total>"; the second pass encodes as q=<n> does, byte for byte.
 * The .bin stays headerless: decode it with the printed q=<n>.
 *
 * codec_parse_rate: 0 and *bpp for "rate=<positive number>"; 1 (*bpp untouched) on anything else ("rate=",
 *   "rate=-1", "rate=abc", a quantiser's text).
 * codec_set_rate: the rate target of every later encode call of this process, as such a text; NULL or "": none.
 *   It overrides the environment variable DCT3D_CODEC_RATE.  A quantiser and a rate target exclude each other:
 *   1 (nothing changes) while codec_set_quant holds a text, and a call that finds both (either by these calls
 *   or by the environment) prints the reason and returns 1, as does a decode or a multi-device call that finds
 *   a rate target.  Also 1 if the text is too long to keep. */
int codec_parse_rate(const char *text, double *bpp);
int codec_set_rate(const char *text);

/* A PSNR target in place of a quantiser (the same single-device encodes): "psnr=<dB>", a positive decimal number.
 * The encode makes two passes over its input file: the first runs the distortion probe (dct3d_distortion_frames)
 * per batch over the rate target's ladder of q, sums the squared errors and the bits over the file and the
 * channels, takes each q's PSNR = 10 log10(255^2 N / sse) over all N unpadded samples of all channels together
 * (the zero-filled frames of a short last stack count), picks the largest q whose PSNR is >= the target (the
 * smallest q when none reaches it) and prints one line "psnr: q=<n> psnr=<dB, 3 decimals> bits=<total>"; the
 * second pass encodes as q=<n> does, byte for byte.  The .bin stays headerless: decode it with the printed q=<n>.
 *
 * codec_parse_psnr: 0 and *db for "psnr=<positive number>"; 1 (*db untouched) on anything else, as
 *   codec_parse_rate.
 * codec_set_psnr: the PSNR target of every later encode call of this process, as such a text; NULL or "": none.
 *   It overrides the environment variable DCT3D_CODEC_PSNR.  A quantiser, a rate target and a PSNR target
 *   exclude each other: 1 (nothing changes) while codec_set_quant or codec_set_rate holds a text (and
 *   codec_set_rate returns 1 while this holds one), and a call that finds two of them (either by these calls or
 *   by the environment) prints the reason and returns 1, as does a decode or a multi-device call that finds a
 *   PSNR target.  Also 1 if the text is too long to keep. */
int codec_parse_psnr(const char *text, double *db);
int codec_set_psnr(const char *text);

/* An RGB-domain PSNR target in place of a quantiser (encode_rgb_ex on one device, in every colour mode: planes,
 * ycc=1, ycc=1 chroma=420): "psnr_rgb=<dB>", a positive decimal number.  The first pass runs the RGB-domain distortion
 * probe (dct3d_distortion_rgb_frames) per batch over the rate target's ladder, candidate i = (rung i, rung j, rung j)
 * with j = min(i + k, 15) (k: cq=<k> beside qmap3=, else 0), and sums the squared errors of the pixels and the
 * candidates' bits over the file.  PSNR = 10 log10(255^2 * 3 * width * height * frames / sse), the zero-filled frames
 * of a short last stack counting as frames; the pick is the PSNR target's rule (the largest q whose PSNR is >= <dB>,
 * the smallest when none reaches it).  It prints one line "psnr_rgb: q=<qY>,<qCb>,<qCr> psnr=<dB, 3 decimals>
 * bits=<total>"; the second pass encodes as q=<n> does, byte for byte.  With qmap=<path> the rule is applied per
 * stack with one quality for all planes and the map is written as rate= writes it; with qmap3=<path> [cq=<k>] per
 * stack with the triples (i, j, j).  With ycc=0 the numbers are psnr=<dB>'s.
 * codec_parse_psnr_rgb: 0 and *db for "psnr_rgb=<positive number>"; 1 (*db untouched) on anything else.
 * codec_set_psnr_rgb: the target of every later encode call of this process; NULL or "": none.  It overrides the
 *   environment variable DCT3D_CODEC_PSNR_RGB.  It excludes a quantiser, a rate target and a PSNR target as those
 *   exclude each other.  A call refuses it, before any file is made, on a decode, on a grey encode, on several
 *   devices and with DCT3D_CODEC_HOST_EG=1. */
int codec_parse_psnr_rgb(const char *text, double *db);
int codec_set_psnr_rgb(const char *text);

/* An SSIM target in place of a quantiser (the single-device encodes, grey or R, G, B planes): "ssim=<target>", a plain
 * decimal in (0, 1].  It takes psnr='s two passes with the SSIM probe (dct3d_ssim_frames; dct3d.h states the SSIM:
 * 8 x 8 windows at a stride of 4, exact) in the distortion probe's place: the sums of the ladder's q are added over
 * the file and the channels, a q's mean SSIM is sum / (2^24 * windows) over all windows (dct3d_ssim_windows per frame
 * and channel; the zero-filled frames of a short last stack count as frames), the pick is the largest q whose mean is
 * >= the target (the smallest q when none reaches it).  It prints one line "ssim: q=<n> ssim=<mean, 6 decimals>
 * bits=<total>"; the second pass encodes as q=<n> does, byte for byte.  With qmap=<path> the rule is applied per stack
 * (the mean over the stack's windows of all channels) and the map is written, as for psnr= with qmap=.
 * codec_parse_ssim: 0 and *target for "ssim=<decimal in (0, 1]>"; 1 (*target untouched) on anything else.
 * codec_set_ssim: the target of every later encode call of this process; NULL or "": none.  It overrides the
 *   environment variable DCT3D_CODEC_SSIM.  It excludes a quantiser, a rate target and both PSNR targets as those
 *   exclude each other.  A call refuses it, before any file is made, on a decode, on several devices, with ycc=1 and
 *   with chroma=420 (luma SSIM in the YCbCr modes is not built). */
int codec_parse_ssim(const char *text, double *target);
int codec_set_ssim(const char *text);

/* An RGB SSIM target in place of a quantiser (encode_rgb_ex on one device, in every colour mode: planes, ycc=1, ycc=1
 * chroma=420): "ssim_rgb=<target>", a plain decimal in (0, 1].  It is psnr_rgb='s first pass with the RGB and luma SSIM
 * probe (dct3d_ssim_rgb_frames) in the probe's place: candidate i = (rung i, rung j, rung j), j = min(i + k, 15) (k:
 * cq=<k> beside qmap3=, else 0); the sums are added over the file and over R, G and B, the mean is taken over all
 * windows of the three planes (dct3d_ssim_windows per frame and plane; the zero-filled frames of a short last stack
 * count as frames), the pick is ssim='s rule.  It prints one line "ssim_rgb: q=<qY>,<qCb>,<qCr> ssim=<mean, 6 decimals>
 * ssim_y=<mean, 6 decimals> bits=<total>", ssim_y= (the luma plane's mean under the pick) only in the YCbCr modes; the
 * second pass encodes as q=<n> does, byte for byte.  With qmap=<path> the rule is applied per stack with one quality for
 * all planes, with qmap3=<path> [cq=<k>] per stack with the triples; the maps are written as psnr_rgb= writes them.
 * codec_parse_ssim_rgb: 0 and *target for "ssim_rgb=<decimal in (0, 1]>"; 1 (*target untouched) on anything else.
 * codec_set_ssim_rgb: the target of every later encode call of this process; NULL or "": none.  It overrides the
 *   environment variable DCT3D_CODEC_SSIM_RGB.  It excludes a quantiser and every other target as those exclude each
 *   other.  A call refuses it, before any file is made, on a decode, on a grey encode, on several devices and with
 *   DCT3D_CODEC_HOST_EG=1. */
int codec_parse_ssim_rgb(const char *text, double *target);
int codec_set_ssim_rgb(const char *text);

/* A quality per stack (the single-device calls: encode, encode_ex, encode_rgb_ex and their decodes): "qmap=<path>"
 * names a text file with one line per stack, in stack order, each a quality of the ladder above; stack s of every
 * channel is coded as q=<that quality> codes it (dct3d_encode_eg_frames_vq / dct3d_decode_eg_frames_vq, the ladder
 * as the palette).  The map travels beside the .bin as width, height, frame count, block depth and q= do: the .bin
 * stays the reference's headerless format, and with no map every file is byte for byte what it was.
 *   encode with rate= or psnr= AND qmap=   the first pass applies the target's rule per stack and WRITES the map:
 *       the rate target's budget is bpp * width * height * blockDepth bits for every stack, the stack's bits summed
 *       over the channels; the PSNR is taken over the stack's unpadded samples of all channels (the zero-filled
 *       frames of a short last stack count).  Prints "qmap: stacks=<n> bits=<total>"; the second pass encodes with
 *       the map.
 *   encode with qmap= alone, decode with qmap=   READ the map.  A constant map gives the q=<n> file byte for byte.
 * Errors (a line printed, 1 returned, before any output file is made): qmap= together with a quantiser, on the
 * several-device calls, with DCT3D_CODEC_HOST_EG=1, a file whose line count is not the stack count, a line that is
 * no quality of the ladder.
 *
 * codec_parse_qmap: reads the file `path` (the path itself, without "qmap="): 0 and qualities[0 .. nStacks-1], or
 *   1 (qualities untouched) if the file cannot be read, is empty, has another line count, or holds a line that is
 *   not exactly a ladder quality in decimal.
 * codec_set_qmap: the map of every later single-device call of this process, as the text "qmap=<path>"; NULL or
 *   "": none.  It overrides the environment variable DCT3D_CODEC_QMAP.  1 (nothing changes) while codec_set_quant
 *   holds a text, or if the text is too long to keep. */
int codec_parse_qmap(const char *path, int nStacks, int *qualities);
int codec_set_qmap(const char *text);

/* The colour transform of the packed RGB24 calls on one device (encode_rgb_ex, decode_rgb_ex): "ycc=1" codes the Y,
 * Cb and Cr planes of the frames (dct3d.h, DCT3D_OPT_COLOUR = DCT3D_COLOUR_YCBCR: JFIF full-range BT.601 in 16-bit
 * fixed point, computed inside the device stream calls) in place of their R, G and B planes; "ycc=0" is none.  The
 * three files then hold Y, Cb, Cr under the names .red / .green / .blue; they are byte for byte what encode_rgb_ex
 * without it writes for the transformed frames.  The .bin does not record the mode, as it does not record the
 * quantiser: decode with the ycc= of the encode.  rate=, and rate= with qmap=, price the transformed planes.
 * Errors (a line printed, 1 returned, before any output file is made): a text that is neither "ycc=0" nor "ycc=1";
 * ycc=1 on a grey call or a several-device call; ycc=1 with psnr= (the distortion probe measures planes, and the
 * Y, Cb, Cr planes' error is not the samples'); ycc=1 with DCT3D_CODEC_HOST_EG=1 (the int32 path has no colour
 * stage).
 * codec_set_colour: the mode of every later call of this process, as such a text; NULL or "": none.  It overrides
 *   the environment variable DCT3D_CODEC_YCC ("1" or "0", or the text itself).  1 (nothing changes) if the text is
 *   too long to keep. */
int codec_set_colour(const char *text);

/* 4:2:0 chroma subsampling of the packed RGB24 calls on one device (encode_rgb_ex, decode_rgb_ex), on top of ycc=1:
 * "chroma=420" codes the Cb and Cr planes at a quarter of the samples (dct3d.h, dct3d_ctx_set_chroma =
 * DCT3D_CHROMA_420: a 2 x 2 box mean on the way in, pixel replication on the way back, both inside the device stream
 * calls); "chroma=444" is none.  The .green / .blue files then hold the (width + 1) / 2 x (height + 1) / 2 planes,
 * each the .bin of encode_ex for that plane.  The .bin does not record the mode: decode with the ycc= and the chroma=
 * of the encode.  rate=, and rate= with qmap=, price and code the subsampled planes.
 * Errors (a line printed, 1 returned, before any output file is made): a text that is neither "chroma=420" nor
 * "chroma=444"; chroma=420 without ycc=1, on a grey call or a several-device call, or with DCT3D_CODEC_HOST_EG=1.
 * codec_set_chroma: the mode of every later call of this process, as such a text; NULL or "": none.  It overrides
 *   the environment variable DCT3D_CODEC_CHROMA ("420" or "444", or the text itself).  1 (nothing changes) if the
 *   text is too long to keep. */
int codec_set_chroma(const char *text);

/* A quality per (stack, channel) of the packed RGB24 calls on one device (encode_rgb_ex, decode_rgb_ex):
 * "qmap3=<path>" names a text file with one line per stack, in stack order, each three qualities of the ladder
 * separated by single spaces: those of the .red, .green and .blue files' planes (R, G, B; with ycc=1 Y, Cb, Cr).  Stack
 * s of plane ch is coded as q=<that quality> codes it (dct3d_encode_eg_frames_vqc / dct3d_decode_eg_frames_vqc, the
 * ladder as the palette).  The map travels beside the .bin, as qmap='s does; a map of three equal columns gives the
 * files of qmap= with that column.
 *   encode with rate= AND qmap3= [cq=<k>]   the first pass prices every stack's candidates i = 0 .. 15: plane 0 at rung
 *       i of the ladder, planes 1 and 2 at rung j = min(i + k, 15) (k in 0..15, 0 without cq=), the cost the three
 *       planes' bits under those rungs; it picks the smallest rung whose cost fits qmap='s budget (bpp * width *
 *       height * blockDepth bits), the largest when none does, WRITES the map (lines "q_i q_j q_j") and prints
 *       "qmap3: stacks=<n> bits=<total>"; the second pass encodes with the map.
 *   encode with qmap3= alone, decode with qmap3=   READ the map.
 * Errors (a line printed, 1 returned, before any output file is made): qmap3= together with qmap=, a quantiser or
 * psnr=; on a grey call or a several-device call; with DCT3D_CODEC_HOST_EG=1; a malformed file; cq= without ycc=1, or
 * without rate= and qmap3=.
 *
 * codec_parse_qmap3: reads the file `path`: 0 and qualities[3 s + ch], or 1 (qualities untouched) if the file cannot
 *   be read, has another line count, or holds a line that is not exactly three ladder qualities in decimal with one
 *   space between them.
 * codec_set_qmap3: the map of every later call of this process, as the text "qmap3=<path>"; NULL or "": none.  It
 *   overrides the environment variable DCT3D_CODEC_QMAP3.  1 (nothing changes) if the text is too long to keep.  What it
 *   excludes is refused by the call that finds both, as listed above: the rules live in one place.
 * codec_set_cq: the chroma offset, as the text "cq=<k>"; NULL or "": none.  It overrides DCT3D_CODEC_CQ. */
int codec_parse_qmap3(const char *path, int nStacks, int *qualities);
int codec_set_qmap3(const char *text);
int codec_set_cq(const char *text);

#ifdef __cplusplus
}
#endif

#endif /* DCT3D_CODEC_H_ */
