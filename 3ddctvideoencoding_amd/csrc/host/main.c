/* main.c -- CLI with the reference's argument convention (main.c:5-49):
 *   dct3d_codec list_devices
 *   dct3d_codec encode|decode <input> <output> <width> <height> <frames> [device_index (1-based)] [block_depth 8|4]
 *   dct3d_codec encode_rgb <rgb24 file> <name pattern> <width> <height> <frames> [device_index] [block_depth 8|4]
 *   dct3d_codec decode_rgb <name pattern> <rgb24 file> <width> <height> <frames> [device_index] [block_depth 8|4]
 *     (packed RGB24 <-> <name pattern>.red / .green / .blue, the RGBUtils plane names; one device)
 *   every command takes a quantiser after the block depth (codec.h, codec_parse_quant): q=<int>, i.e. step
 *   max(1, <int> s) clipped to 255 (q=5: the reference's), or block_depth + 14 comma-separated steps in 1..255;
 *   the file does not record it: decode with the quantiser of the encode
 *   the single-device encodes take rate=<bits per pixel> in the quantiser's place (codec.h, codec_parse_rate): two
 *   passes, the first picks q from a fixed ladder and prints "rate: q=<n> bits=<total>"; decode with that q=<n>
 *   ... or psnr=<dB> (codec_parse_psnr): the first pass picks the largest q of the ladder whose PSNR reaches the
 *   target and prints "psnr: q=<n> psnr=<dB> bits=<total>"
 *   the single-device commands take qmap=<path> (codec.h, codec_set_qmap): one ladder quality per stack, one per
 *   line; written by an encode that also has rate= or psnr= (the rule applied per stack), read by an encode without
 *   a target and by a decode; not together with q= or several devices
 *   encode_rgb and decode_rgb take ycc=1 (codec.h, codec_set_colour): the three files hold the Y, Cb, Cr planes,
 *   the transform computed inside the device calls; not recorded in the file: decode with ycc=1 too; not with psnr=
 *   ... and chroma=420 beside ycc=1 (codec.h, codec_set_chroma): .green / .blue hold the Cb and Cr planes at a quarter
 *   of the samples, (width + 1) / 2 x (height + 1) / 2; not recorded either: decode with the same two tokens
 *   ... and qmap3=<path> (codec.h, codec_set_qmap3): three ladder qualities per stack and line, one per plane; written
 *   by an encode_rgb that also has rate= (and cq=<k>: the chroma planes k rungs coarser), else read; not with qmap=,
 *   q= or psnr=
 *   encode_rgb takes psnr_rgb=<dB> (codec.h, codec_parse_psnr_rgb) in the quantiser's place, in every colour mode: the
 *   first pass measures the squared error in the RGB pixels (the RGB-domain distortion probe) and prints
 *   "psnr_rgb: q=<qY>,<qCb>,<qCr> psnr=<dB> bits=<total>"; with qmap= or qmap3= [cq=<k>] it writes the map
 *   the single-device encodes take ssim=<target in (0, 1]> (codec.h, codec_parse_ssim) in the quantiser's place: the
 *   first pass picks the largest q whose mean SSIM (the SSIM probe) reaches the target and prints
 *   "ssim: q=<n> ssim=<mean> bits=<total>"; with qmap= it writes the map; not with ycc=1 or chroma=420
 *   encode_rgb takes ssim_rgb=<target in (0, 1]> (codec.h, codec_parse_ssim_rgb) in the quantiser's place, in every
 *   colour mode: psnr_rgb='s passes with the RGB and luma SSIM probe; prints "ssim_rgb: q=<qY>,<qCb>,<qCr> ssim=<mean>
 *   [ssim_y=<mean>] bits=<total>"; with qmap= or qmap3= [cq=<k>] it writes the map
 *   width and height: any size >= 1 on one device (a size that is no multiple of 8 is padded by repeating the
 *   last column and row inside the device transform, and cropped on the way back); multiples of 8 on several
 * (list_platforms is accepted as an alias of list_devices.)  device_index may be a comma-separated list
 * ("1,2,3"): encode_multi / decode_multi over those devices. */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "codec.h"
#include "dct3d.h"

static void usage(void) {
    printf("Usage\n\n");
    printf("dct3d_codec list_devices -> List available HIP devices\n");
    printf("dct3d_codec encode|decode <input file> <output file> <width> <height> <nr of frames> "
           "<device_index (optional, 1-based; a list a,b,... uses several)> <block depth 8|4 (optional)> -> "
           "Encode/Decode given file\n");
    printf("dct3d_codec encode_rgb <rgb24 file> <name pattern> <width> <height> <nr of frames> "
           "<device_index (optional)> <block depth 8|4 (optional)> -> Encode packed RGB24 into "
           "<name pattern>.red/.green/.blue\n");
    printf("dct3d_codec decode_rgb <name pattern> <rgb24 file> <width> <height> <nr of frames> "
           "<device_index (optional)> <block depth 8|4 (optional)> -> Decode <name pattern>.red/.green/.blue "
           "into packed RGB24\n");
    printf("Every command takes a quantiser after the block depth: q=<int> (steps max(1, <int> * (x+y+z)), at most "
           "255; q=5 is the reference's) or <block depth + 14> comma-separated steps in 1..255.  The file does not "
           "record it: decode with the quantiser of the encode\n");
    printf("encode and encode_rgb on one device take rate=<bits per pixel> in the quantiser's place: the target is "
           "<bits per pixel> * width * height * frames (unpadded pixels, all channels together), measured on the "
           "Exp-Golomb bits before the deflate.  A first pass over the input prices the ladder q = 1, 2, 3, 4, 5, 6, 8, "
           "10, 12, 16, 20, 24, 32, 40, 48, 64, picks the smallest q that fits (64 when none does) and prints "
           "'rate: q=<n> bits=<total>'; the second pass encodes as q=<n>.  Decode with that q=<n>: rate= on a decode, "
           "together with q=, or with several devices is an error\n");
    printf("... or psnr=<dB>: the first pass measures the exact squared error of encode + decode under the same ladder, "
           "takes each q's PSNR over all unpadded samples of all channels together, picks the largest q whose PSNR is "
           ">= <dB> (1 when none reaches it) and prints 'psnr: q=<n> psnr=<dB> bits=<total>'; the second pass encodes as "
           "q=<n>.  psnr= on a decode, together with q= or rate=, or with several devices is an error\n");
    printf("The commands on one device take qmap=<path>, a text file of one ladder quality per stack (one per line, in "
           "stack order): stack s of every channel is coded as q=<that quality> codes it.  With rate= or psnr= the "
           "first pass applies the target's rule per stack (budget <bits per pixel> * width * height * block depth "
           "per stack; PSNR over the stack's samples), WRITES the map and prints 'qmap: stacks=<n> bits=<total>'; an "
           "encode without a target and a decode READ it.  qmap= together with q=, with several devices, or a file "
           "with another line count or a quality outside the ladder is an error\n");
    printf("encode_rgb and decode_rgb take ycc=1: the three files hold the Y, Cb and Cr planes of the frames (JFIF "
           "full-range BT.601 in 16-bit fixed point, computed inside the device calls) in place of R, G and B.  The file "
           "does not record it: decode with ycc=1 too.  rate= and qmap= price and code those planes; ycc=1 together with "
           "psnr=, on encode or decode, or with several devices is an error\n");
    printf("encode_rgb and decode_rgb take chroma=420 together with ycc=1: the .green and .blue files hold the Cb and Cr "
           "planes at a quarter of the samples, (width + 1) / 2 x (height + 1) / 2 (a 2 x 2 box mean on the way in, pixel "
           "replication on the way back, inside the device calls); chroma=444 is the default.  The file does not record "
           "it: decode with the same tokens.  rate= and qmap= price and code the subsampled planes; chroma=420 without "
           "ycc=1, on encode or decode, or with several devices is an error\n");
    printf("encode_rgb and decode_rgb take qmap3=<path>, a text file of three ladder qualities per stack (one line per "
           "stack, single spaces between them): those of the .red, .green and .blue planes (Y, Cb, Cr with ycc=1).  "
           "With rate= the first pass prices per stack the candidates 'plane 0 at rung i of the ladder, planes 1 and 2 at "
           "rung min(i + k, 15)' (cq=<k>, 0..15, default 0; it needs ycc=1), picks the smallest rung that fits qmap='s "
           "budget, WRITES the map and prints 'qmap3: stacks=<n> bits=<total>'; an encode without a target and a decode "
           "READ it.  qmap3= together with qmap=, q= or psnr=, on encode or decode, with several devices, or a malformed "
           "file is an error; so is cq= without ycc=1 or without rate= and qmap3=\n");
    printf("encode_rgb on one device takes psnr_rgb=<dB> in the quantiser's place, with or without ycc=1 and chroma=420: "
           "the first pass measures, per rung of the ladder, the exact squared error of encode + decode in the RGB pixels "
           "(all three bytes of every unpadded pixel), picks the largest q whose PSNR is >= <dB> (1 when none reaches it) "
           "and prints 'psnr_rgb: q=<qY>,<qCb>,<qCr> psnr=<dB> bits=<total>'; the second pass encodes as q=<n>.  With "
           "qmap=<path> the rule is applied per stack and the map is WRITTEN; with qmap3=<path> [cq=<k>] the candidates "
           "are 'plane 0 at rung i, planes 1 and 2 at rung min(i + k, 15)' and the three-column map is written.  "
           "psnr_rgb= on a decode, on a grey command, together with q=, rate= or psnr=, or with several devices is an "
           "error\n");
    printf("encode and encode_rgb on one device take ssim=<target>, a decimal in (0, 1], in the quantiser's place: the "
           "first pass measures, per rung of the ladder, the exact SSIM of encode + decode (8 x 8 windows at a stride of "
           "4 over every frame of every plane), takes each q's mean over all windows, picks the largest q whose mean is "
           ">= <target> (1 when none reaches it) and prints 'ssim: q=<n> ssim=<mean> bits=<total>'; the second pass "
           "encodes as q=<n>.  With qmap=<path> the rule is applied per stack and the map is WRITTEN.  ssim= on a "
           "decode, together with q=, rate=, psnr= or psnr_rgb=, with ycc=1 or chroma=420, or with several devices is an "
           "error\n");
    printf("encode_rgb on one device takes ssim_rgb=<target>, a decimal in (0, 1], in the quantiser's place, with or "
           "without ycc=1 and chroma=420: the first pass measures, per rung of the ladder, the exact SSIM of encode + "
           "decode on the R, G and B bytes the decode writes (and, with ycc=1, on the luma plane), picks the largest q "
           "whose mean over the windows of R, G and B is >= <target> (1 when none reaches it) and prints 'ssim_rgb: "
           "q=<qY>,<qCb>,<qCr> ssim=<mean> ssim_y=<mean> bits=<total>' (no ssim_y= without ycc=1); the second pass encodes "
           "as q=<n>.  With qmap=<path> the rule is applied per stack and the map is WRITTEN; with qmap3=<path> [cq=<k>] "
           "the candidates are psnr_rgb='s triples and the three-column map is written.  ssim_rgb= on a decode, on a grey "
           "command, together with q=, rate=, psnr=, psnr_rgb= or ssim=, or with several devices is an error\n");
    printf("<width> and <height> may be any size >= 1: a size that is no multiple of 8 is padded by repeating the "
           "last column and row (the stream is that of the padded video) and cropped again by decode; with "
           "several devices they must be multiples of 8\n");
}

/* "1" or "1,2,3": 1-based device numbers (the reference's platformIndex, main.c:33-37).  Every entry must
 * be a positive decimal number; an empty entry, trailing junk, a value <= 0 or more than max entries is
 * an error (non-zero return). */
static int parse_devices(const char *arg, int *devs, int max, int *n) {
    *n = 0;
    const char *p = arg;
    for (;;) {
        char *end = NULL;
        errno = 0;
        const long v = strtol(p, &end, 10);
        if (end == p || errno || v <= 0 || v > 1 << 20 || *n >= max) return -1;
        devs[(*n)++] = (int)v;
        if (*end == '\0') return 0;
        if (*end != ',') return -1;
        p = end + 1;
    }
}

int main(int argc, char *argv[]) {
    if (argc < 2) {
        usage();
        return 0;
    }
    if (!strcmp(argv[1], "list_devices") || !strcmp(argv[1], "list_platforms")) {
        for (int d = 0;; d++) {
            dct3d_ctx *c = NULL;
            if (dct3d_ctx_create(d, 8, 8, 8, &c)) {
                if (d == 0) printf("No HIP device available\n");
                break;
            }
            printf("%d - HIP device %d\n", d + 1, d);
            dct3d_ctx_destroy(c);
        }
        return 0;
    }
    if (argc < 7) {
        usage();
        return 1;
    }
    const int width = atoi(argv[4]), height = atoi(argv[5]), frames = atoi(argv[6]);
    int devs[64], n_dev = 0;
    if (argc > 7 && parse_devices(argv[7], devs, 64, &n_dev)) {
        printf("Invalid device list '%s': 1-based device numbers, comma-separated, at most 64\n", argv[7]);
        usage();
        return 1;
    }
    if (n_dev == 0) devs[n_dev++] = 1;
    const int depth = argc > 8 ? atoi(argv[8]) : DCT_BLOCK_DEPTH;
    int have_quant = 0, have_rate = 0, have_psnr = 0, have_qmap = 0, have_ycc = 0, have_chroma = 0, have_qmap3 = 0, have_cq = 0, have_prgb = 0, have_ssim = 0, have_srgb = 0;
    for (int a = 9; a < argc && a < 15 && (depth == 8 || depth == 4); a++) { /* (any other depth: the entry point reports the geometry) */
        int32_t steps[32];
        double v;
        const int is_rate = !strncmp(argv[a], "rate=", 5), is_psnr = !strncmp(argv[a], "psnr=", 5);
        const int is_qmap = !strncmp(argv[a], "qmap=", 5), is_ycc = !strncmp(argv[a], "ycc=", 4);
        const int is_chroma = !strncmp(argv[a], "chroma=", 7);
        const int is_qmap3 = !strncmp(argv[a], "qmap3=", 6), is_cq = !strncmp(argv[a], "cq=", 3);
        const int is_prgb = !strncmp(argv[a], "psnr_rgb=", 9);
        if (is_prgb) { /* the RGB-domain PSNR target: refused here before any file is made */
            if (have_prgb) break;
            if (codec_parse_psnr_rgb(argv[a], &v)) {
                printf("Invalid psnr_rgb target '%s': psnr_rgb=<dB>, a positive number\n", argv[a]);
                usage();
                return 1;
            }
            if (strcmp(argv[1], "encode_rgb") || n_dev > 1) {
                printf("psnr_rgb= applies to encode_rgb on one device: decode with the q=<n> or the map that the encode "
                       "printed or wrote\n");
                return 1;
            }
            have_prgb = a;
            continue;
        }
        if (!strncmp(argv[a], "ssim_rgb=", 9)) { /* the RGB SSIM target: refused here before any file is made */
            if (have_srgb) break;
            if (codec_parse_ssim_rgb(argv[a], &v)) {
                printf("Invalid ssim_rgb target '%s': ssim_rgb=<target>, a decimal in (0, 1]\n", argv[a]);
                usage();
                return 1;
            }
            if (strcmp(argv[1], "encode_rgb") || n_dev > 1) {
                printf("ssim_rgb= applies to encode_rgb on one device: decode with the q=<n> or the map that the encode "
                       "printed or wrote\n");
                return 1;
            }
            have_srgb = a;
            continue;
        }
        if (!strncmp(argv[a], "ssim=", 5)) { /* the SSIM target: refused here before any file is made */
            if (have_ssim) break;
            if (codec_parse_ssim(argv[a], &v)) {
                printf("Invalid ssim target '%s': ssim=<target>, a decimal in (0, 1]\n", argv[a]);
                usage();
                return 1;
            }
            if (argv[1][0] != 'e' || n_dev > 1) {
                printf("ssim= applies to encode and encode_rgb on one device: decode with the q=<n> that the encode printed\n");
                return 1;
            }
            have_ssim = a;
            continue;
        }
        if (a >= 10 && (is_qmap3 ? have_qmap3 : is_cq ? have_cq : 0)) break;
        if (is_qmap3 || is_cq) { /* collected here; the entry points check them (codec.c: call_qmap3, reject_qmap3) */
            if (is_qmap3) have_qmap3 = a;
            else have_cq = a;
            continue;
        }
        if (a >= 10 && (is_rate ? have_rate : is_psnr ? have_psnr : is_qmap ? have_qmap : is_ycc ? have_ycc : is_chroma ? have_chroma : have_quant)) break; /* (a second argument counts only as another kind) */
        if (is_ycc) {
            if (strcmp(argv[a], "ycc=0") && strcmp(argv[a], "ycc=1")) {
                printf("Invalid colour mode '%s': ycc=0 or ycc=1\n", argv[a]);
                usage();
                return 1;
            }
            if (argv[a][4] == '1' && ((strcmp(argv[1], "encode_rgb") && strcmp(argv[1], "decode_rgb")) || n_dev > 1)) {
                printf("ycc= applies to encode_rgb and decode_rgb on one device\n");
                return 1;
            }
            have_ycc = a;
        } else if (is_chroma) {
            if (strcmp(argv[a], "chroma=420") && strcmp(argv[a], "chroma=444")) {
                printf("Invalid chroma mode '%s': chroma=420 or chroma=444\n", argv[a]);
                usage();
                return 1;
            }
            if (argv[a][9] == '0' && ((strcmp(argv[1], "encode_rgb") && strcmp(argv[1], "decode_rgb")) || n_dev > 1)) {
                printf("chroma= applies to encode_rgb and decode_rgb on one device\n");
                usage();
                return 1;
            }
            have_chroma = a;
        } else if (is_qmap) {
            if (!argv[a][5]) {
                printf("Invalid quality map '%s': qmap=<path>\n", argv[a]);
                usage();
                return 1;
            }
            if (n_dev > 1) {
                printf("qmap= applies to the commands on one device\n");
                return 1;
            }
            have_qmap = a;
        } else if (is_rate || is_psnr) {
            if (is_rate ? codec_parse_rate(argv[a], &v) : codec_parse_psnr(argv[a], &v)) {
                if (is_rate) printf("Invalid rate target '%s': rate=<bits per pixel>, a positive number\n", argv[a]);
                else printf("Invalid psnr target '%s': psnr=<dB>, a positive number\n", argv[a]);
                usage();
                return 1;
            }
            if (argv[1][0] != 'e' || n_dev > 1) {
                printf("%s applies to encode and encode_rgb on one device: decode with the q=<n> that the encode printed\n",
                       is_rate ? "rate=" : "psnr=");
                return 1;
            }
            if (is_rate) have_rate = a;
            else have_psnr = a;
        } else if (codec_parse_quant(argv[a], depth, steps)) {
            printf("Invalid quantiser '%s': q=<0..255>, or block depth + 14 comma-separated steps in 1..255\n", argv[a]);
            usage();
            return 1;
        } else {
            have_quant = a;
        }
    }
    if ((have_quant != 0) + (have_rate != 0) + (have_psnr != 0) > 1) {
        printf("%s and %s exclude each other\n", have_quant ? "q=" : "rate=", have_psnr ? "psnr=" : "rate=");
        return 1;
    }
    if (have_prgb && (have_quant || have_rate || have_psnr)) {
        printf("%s and psnr_rgb= exclude each other\n", have_quant ? "q=" : have_rate ? "rate=" : "psnr=");
        return 1;
    }
    if (have_ssim && (have_quant || have_rate || have_psnr || have_prgb)) {
        printf("%s and ssim= exclude each other\n", have_quant ? "q=" : have_rate ? "rate=" : have_psnr ? "psnr=" : "psnr_rgb=");
        return 1;
    }
    if (have_srgb && (have_quant || have_rate || have_psnr || have_prgb || have_ssim)) {
        printf("%s and ssim_rgb= exclude each other\n",
               have_quant ? "q=" : have_rate ? "rate=" : have_psnr ? "psnr=" : have_prgb ? "psnr_rgb=" : "ssim=");
        return 1;
    }
    if (have_ssim && ((have_ycc && argv[have_ycc][4] == '1') || (have_chroma && argv[have_chroma][9] == '0'))) {
        printf("%s and ssim= exclude each other: the SSIM probe measures the R, G, B planes (luma SSIM is not built)\n",
               have_ycc && argv[have_ycc][4] == '1' ? "ycc=1" : "chroma=420");
        return 1;
    }
    if (have_ycc && argv[have_ycc][4] == '1' && have_psnr) {
        printf("ycc=1 and psnr= exclude each other: the distortion probe would measure the Y, Cb, Cr planes, not the RGB "
               "samples\n");
        return 1;
    }
    if (have_chroma && argv[have_chroma][9] == '0' && !(have_ycc && argv[have_ycc][4] == '1') && !getenv("DCT3D_CODEC_YCC")) {
        printf("chroma=420 needs ycc=1: it subsamples the Cb and Cr planes of the colour transform\n");
        usage();
        return 1;
    }
    if (have_quant && have_qmap) {
        printf("q= and qmap= exclude each other\n");
        return 1;
    }
    if ((have_quant && codec_set_quant(argv[have_quant])) || (have_rate && codec_set_rate(argv[have_rate])) ||
        (have_psnr && codec_set_psnr(argv[have_psnr])) || (have_qmap && codec_set_qmap(argv[have_qmap])) ||
        (have_ycc && codec_set_colour(argv[have_ycc])) || (have_chroma && codec_set_chroma(argv[have_chroma])) ||
        (have_qmap3 && codec_set_qmap3(argv[have_qmap3])) || (have_cq && codec_set_cq(argv[have_cq])) ||
        (have_prgb && codec_set_psnr_rgb(argv[have_prgb])) || (have_ssim && codec_set_ssim(argv[have_ssim])) ||
        (have_srgb && codec_set_ssim_rgb(argv[have_srgb]))) {
        printf("Argument too long\n");
        return 1;
    }
    if (!strcmp(argv[1], "encode"))
        return n_dev > 1 ? encode_multi(argv[2], argv[3], width, height, frames, devs, n_dev, depth, 0)
                         : encode_ex(argv[2], argv[3], width, height, frames, devs[0], depth, 0);
    if (!strcmp(argv[1], "decode"))
        return n_dev > 1 ? decode_multi(argv[2], argv[3], width, height, frames, devs, n_dev, depth, 0)
                         : decode_ex(argv[2], argv[3], width, height, frames, devs[0], depth, 0);
    if (!strcmp(argv[1], "encode_rgb") || !strcmp(argv[1], "decode_rgb")) {
        if (n_dev > 1) {
            if (have_qmap3 || have_cq) printf("qmap3= and cq= apply to encode_rgb and decode_rgb on one device\n");
            printf("%s runs on one device\n", argv[1]);
            return 1;
        }
        return argv[1][0] == 'e' ? encode_rgb_ex(argv[2], argv[3], width, height, frames, devs[0], depth, 0)
                                 : decode_rgb_ex(argv[2], argv[3], width, height, frames, devs[0], depth, 0);
    }
    usage();
    return 1;
}
