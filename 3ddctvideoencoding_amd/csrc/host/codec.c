/* codec.c -- encode()/decode(): the reference codec's pipeline (encoder.c:88-293,
 * decoder.c:85-314) with the OpenCL block replaced by the libdct3d C-ABI.
 *
 * encode: per batch of stacks: fread -> the device (fused DCT + quantisation, Java semantics, and by
 *         default diagonal order + Exp-Golomb) -> per channel: deflate (codec_entropy.c).
 * decode: inflate per channel -> the device (Exp-Golomb + reorder, fused dequantisation + IDCT + clamp +
 *         truncation) -> fwrite.
 * One body per direction (encode_any / decode_any) serves every frame size, grey and packed RGB24.
 * A stack is DCT_BLOCK_DEPTH frames; a short last stack is zero-filled (the reference reads
 * uninitialised bytes there, encoder.c:21-27).  Frames to encode are rounded up to whole stacks,
 * as in the reference loop (encoder.c:203).  Errors: printf + return 1 (the reference convention);
 * never exit().
 *
 * encode_multi / decode_multi: the same pipelines over several devices, one host thread and one
 * dct3d_ctx per device (a ctx is single-threaded; SURVEY.md §8b "one host thread per ctx").  Encode:
 * batches go round-robin to the devices, each coded from a zero carry; the calling thread joins the
 * batch streams in order, shifting each by the running partial byte, into the one zlib stream -- the
 * same .bin as encode_ex.  Decode: a batch's first bit is known only when the previous batch is
 * decoded (the stream has no index), so the device calls chain and alternate over the devices; the only
 * overlap is the previous batch's raster write (several devices) -- the next window is inflated after
 * the running decode returns.  Decoding does not get faster with more devices. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "codec.h"
#include "codec_entropy.h"
#include "dct3d.h"

/* DCT3D_CODEC_TIMING=1: encode_any / decode_any print one JSON line of per-stage wall seconds to stderr
 * (tools/codec_e2e.py): which stage bounds the reference-identical .bin end to end */
static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static int timing_on(void) {
    const char *e = getenv("DCT3D_CODEC_TIMING");
    return e && e[0] == '1';
}
#define STAGE(acc, stmt)              \
    do {                              \
        const double t_0_ = now_s();  \
        stmt;                         \
        (acc) += now_s() - t_0_;      \
    } while (0)

/* every frame size, grey (channels = 1) or packed RGB24 (3): see "packed RGB24 and frames of any size" below */
static int encode_any(const char *inName, const char *outName, int width, int height, int frames, int platformIndex,
                      int depth, int batch, int channels);
static int decode_any(const char *inName, const char *outName, int width, int height, int frames, int platformIndex,
                      int depth, int batch, int channels);
static int host_eg_on(void);
static int geometry_ok(int width, int height, int frames, int depth) {
    return width > 0 && height > 0 && frames > 0 && (depth == 8 || depth == 4);
}
static int invalid_geometry(int width, int height, int frames, int depth) {
    printf("Invalid geometry: %dx%d, %d frames, block depth %d (width, height and frames must be positive, the "
           "block depth 8 or 4)\n", width, height, frames, depth);
    return 1;
}

/* ---- the quantiser (codec.h) ------------------------------------------------------------------- */
#define QUANT_MAX_STEPS 22 /* block depth 8: 8 + 8 + 8 - 2 */

int codec_parse_quant(const char *text, int depth, int32_t *steps) {
    if (!text || !steps || (depth != 8 && depth != 4)) return 1;
    const int n = depth + 14;
    int32_t t[QUANT_MAX_STEPS];
    char *end = NULL;
    if (!strncmp(text, "q=", 2)) {
        if (text[2] < '0' || text[2] > '9') return 1; /* (strtol would take a sign or blanks) */
        const long q = strtol(text + 2, &end, 10);
        if (*end != '\0' || q > 255) return 1;
        for (int s = 0; s < n; s++) t[s] = q * s < 1 ? 1 : q * s > 255 ? 255 : (int32_t)(q * s);
    } else {
        const char *p = text;
        for (int s = 0; s < n; s++) {
            if (*p < '0' || *p > '9') return 1;
            const long v = strtol(p, &end, 10);
            if (v < 1 || v > 255 || *end != (s == n - 1 ? '\0' : ',')) return 1;
            t[s] = (int32_t)v;
            p = end + 1;
        }
    }
    memcpy(steps, t, sizeof(int32_t) * (size_t)n);
    return 0;
}

static char g_quant_text[QUANT_MAX_STEPS * 4 + 8]; /* codec_set_quant's text; "": none */

int codec_set_quant(const char *text) {
    if (text && strlen(text) >= sizeof(g_quant_text)) return 1;
    snprintf(g_quant_text, sizeof(g_quant_text), "%s", text ? text : "");
    return 0;
}

/* The quantiser of a call at block depth `depth`: codec_set_quant's text, else DCT3D_CODEC_QUANT.  *set = 0:
 * none given (the context keeps the reference table).  1 after printing when the text does not parse. */
static int call_quant(int depth, int32_t *steps, int *set) {
    const char *text = g_quant_text[0] ? g_quant_text : getenv("DCT3D_CODEC_QUANT");
    *set = text && text[0];
    if (*set && codec_parse_quant(text, depth, steps)) {
        printf("Invalid quantiser '%s': q=<0..255>, or %d comma-separated steps in 1..255\n", text, depth + 14);
        return 1;
    }
    return 0;
}

/* ... and set on a context right after its creation; 1 after printing on an error */
static int ctx_apply_quant(dct3d_ctx *ctx, int depth) {
    int32_t steps[QUANT_MAX_STEPS];
    int set;
    if (call_quant(depth, steps, &set)) return 1;
    const int rc = set ? dct3d_ctx_set_quant(ctx, steps, depth + 14) : DCT3D_OK;
    if (rc) printf("Error setting the quantiser: %s\n", dct3d_strerror(rc));
    return rc != DCT3D_OK;
}

/* the table of a context as text for the DCT3D_CODEC_TIMING line: "[1, 5, 10, ...]" */
static void quant_json(const dct3d_ctx *ctx, int depth, char *buf, size_t cap) {
    int32_t steps[QUANT_MAX_STEPS];
    size_t o = 0;
    buf[0] = '\0';
    if (!ctx || dct3d_ctx_get_quant(ctx, steps, depth + 14)) {
        snprintf(buf, cap, "null");
        return;
    }
    for (int s = 0; s < depth + 14 && o + 8 < cap; s++)
        o += (size_t)snprintf(buf + o, cap - o, "%s%d", s ? ", " : "[", (int)steps[s]);
    snprintf(buf + o, cap - o, "]");
}

/* ---- the rate target (codec.h) ------------------------------------------------------------------ */
/* "<prefix><plain positive decimal>": no sign, blanks, exponent or hexadecimal; 0 < value <= 1e9 */
static int parse_positive(const char *text, const char *prefix, double *value) {
    const size_t n = strlen(prefix);
    if (!text || !value || strncmp(text, prefix, n)) return 1;
    const char *p = text + n;
    if (!((*p >= '0' && *p <= '9') || (*p == '.' && p[1] >= '0' && p[1] <= '9'))) return 1;
    for (const char *c = p; *c; c++)
        if (!((*c >= '0' && *c <= '9') || *c == '.')) return 1;
    char *end = NULL;
    const double v = strtod(p, &end);
    if (*end != '\0' || !(v > 0.0) || v > 1e9) return 1;
    *value = v;
    return 0;
}

/* What selects a call's quantiser: the table itself or one of the targets.  A target is "<prefix><number>"; q=,
 * rate= and psnr= exclude each other: one may not be set (codec_set_*) while another is, and a call that finds
 * one (set or in the environment) beside an entry before it in this list refuses. */
static char g_rate_text[64]; /* codec_set_rate's text; "": none */
static char g_psnr_text[64]; /* codec_set_psnr's text; "": none */
static char g_psnr_rgb_text[64]; /* codec_set_psnr_rgb's text; "": none */
static char g_ssim_text[64]; /* codec_set_ssim's text; "": none */
static char g_ssim_rgb_text[64]; /* codec_set_ssim_rgb's text; "": none */
enum { SEL_QUANT, SEL_RATE, SEL_PSNR, SEL_PSNR_RGB, SEL_SSIM, SEL_SSIM_RGB, SEL_N };
static const struct {
    const char *prefix, *env, *noun, *unit, *range;
    char *text;
    size_t cap;
} kSel[SEL_N] = {
    {"q=", "DCT3D_CODEC_QUANT", "quantiser", NULL, NULL, g_quant_text, sizeof(g_quant_text)},
    {"rate=", "DCT3D_CODEC_RATE", "rate target", "bits per pixel", "a positive number", g_rate_text, sizeof(g_rate_text)},
    {"psnr=", "DCT3D_CODEC_PSNR", "PSNR target", "dB", "a positive number", g_psnr_text, sizeof(g_psnr_text)},
    {"psnr_rgb=", "DCT3D_CODEC_PSNR_RGB", "RGB PSNR target", "dB", "a positive number", g_psnr_rgb_text, sizeof(g_psnr_rgb_text)},
    {"ssim=", "DCT3D_CODEC_SSIM", "SSIM target", "target", "a decimal in (0, 1]", g_ssim_text, sizeof(g_ssim_text)},
    {"ssim_rgb=", "DCT3D_CODEC_SSIM_RGB", "RGB SSIM target", "target", "a decimal in (0, 1]", g_ssim_rgb_text, sizeof(g_ssim_rgb_text)},
};
static const char *sel_text(int i) { return kSel[i].text[0] ? kSel[i].text : getenv(kSel[i].env); }

int codec_parse_rate(const char *text, double *bpp) { return parse_positive(text, kSel[SEL_RATE].prefix, bpp); }
int codec_parse_psnr(const char *text, double *db) { return parse_positive(text, kSel[SEL_PSNR].prefix, db); }
int codec_parse_psnr_rgb(const char *text, double *db) { return parse_positive(text, kSel[SEL_PSNR_RGB].prefix, db); }
/* a plain decimal in (0, 1] behind the prefix */
static int parse_unit(const char *text, const char *prefix, double *target) {
    double v;
    if (!target || parse_positive(text, prefix, &v) || v > 1.0) return 1;
    *target = v;
    return 0;
}
int codec_parse_ssim(const char *text, double *target) { return parse_unit(text, kSel[SEL_SSIM].prefix, target); }
int codec_parse_ssim_rgb(const char *text, double *target) { return parse_unit(text, kSel[SEL_SSIM_RGB].prefix, target); }
/* target i's text -> its value: 1 when it does not parse */
static int parse_target(int i, const char *text, double *value) {
    return i == SEL_SSIM || i == SEL_SSIM_RGB ? parse_unit(text, kSel[i].prefix, value) : parse_positive(text, kSel[i].prefix, value);
}

static int set_target(int i, const char *text) {
    if (text && strlen(text) >= kSel[i].cap) return 1;
    for (int o = 0; o < SEL_N; o++)
        if (o != i && text && text[0] && kSel[o].text[0]) return 1;
    snprintf(kSel[i].text, kSel[i].cap, "%s", text ? text : "");
    return 0;
}
int codec_set_rate(const char *text) { return set_target(SEL_RATE, text); }
int codec_set_psnr(const char *text) { return set_target(SEL_PSNR, text); }
int codec_set_psnr_rgb(const char *text) { return set_target(SEL_PSNR_RGB, text); }
int codec_set_ssim(const char *text) { return set_target(SEL_SSIM, text); }
int codec_set_ssim_rgb(const char *text) { return set_target(SEL_SSIM_RGB, text); }

/* Target i of a call: codec_set_*'s text, else the environment variable.  *set = 0: none given.  1 after printing
 * when the text does not parse or a quantiser or an earlier target is given too. */
static int call_target(int i, double *value, int *set) {
    const char *text = sel_text(i);
    *set = text && text[0];
    if (!*set) return 0;
    for (int o = 0; o < i; o++) {
        const char *ot = sel_text(o);
        if (ot && ot[0]) {
            printf("A %s ('%s') and a %s ('%s') exclude each other\n", kSel[o].noun, ot, kSel[i].noun, text);
            return 1;
        }
    }
    if (parse_target(i, text, value)) {
        printf("Invalid %.*s target '%s': %s<%s>, %s\n", (int)strlen(kSel[i].prefix) - 1, kSel[i].prefix, text,
               kSel[i].prefix, kSel[i].unit, kSel[i].range);
        return 1;
    }
    return 0;
}
/* the commands that take no target: 1 after printing when one is given */
static int reject_targets(const char *what) {
    for (int i = SEL_RATE; i < SEL_N; i++) {
        double v;
        int set;
        if (call_target(i, &v, &set)) return 1;
        if (set) {
            printf("%s applies to single-device encodes only (%s): decode with the q=<n> that the encode printed\n",
                   kSel[i].prefix, what);
            return 1;
        }
    }
    return 0;
}

/* The first pass of an encode with a rate target: the rate probe (dct3d_rate_frames) per batch over the fixed
 * ladder of qualities, the bits summed over the file and the channels; the pick is the smallest quality whose
 * bits fit bpp * width * height * frames (unpadded pixels, all channels together, Exp-Golomb bits before the
 * deflate), or the largest when none fits.  Prints "rate: q=<n> bits=<total>", sets the context's quantiser to
 * q=<n> and rewinds the input.  1 after printing on an error.
 * METRIC_PSNR: the first pass of an encode with a PSNR target instead: the distortion probe (dct3d_distortion_frames)
 * per batch over the same ladder, the squared errors and the bits summed over the file and the channels; the PSNR
 * of a quality is taken over all unpadded samples of all channels together (the zero-filled frames of a short last
 * stack count as frames); the pick is the largest quality whose PSNR is >= target, or the smallest when none
 * reaches it.  Prints "psnr: q=<n> psnr=<dB> bits=<total>".
 * METRIC_SSIM: an SSIM target (ssim=<target>): the SSIM probe (dct3d_ssim_frames) in the distortion probe's place, its
 * sums added over the file and the channels, the mean over all windows (dct3d_ssim_windows per frame and channel; the
 * zero-filled frames count); psnr='s rule on the means.  Prints "ssim: q=<n> ssim=<6 decimals> bits=<total>". */
enum { METRIC_RATE, METRIC_PSNR, METRIC_SSIM }; /* what the first pass measures and picks by */
static const int kRateLadder[] = {1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64};
#define RATE_LADDER_N ((int)(sizeof(kRateLadder) / sizeof(kRateLadder[0])))
static double psnr_of(uint64_t sse, double n_samples) {
    return sse ? 10.0 * log10(255.0 * 255.0 * n_samples / (double)sse) : INFINITY;
}
/* the ladder's tables, [RATE_LADDER_N][depth + 14]: step[s] = max(1, q s) clipped to 255, as q=<n> */
static void ladder_tables(int depth, int32_t *tabs) {
    const int n = depth + 14;
    for (int i = 0; i < RATE_LADDER_N; i++)
        for (int s = 0; s < n; s++) {
            const int v = kRateLadder[i] * s;
            tabs[i * n + s] = v < 1 ? 1 : v > 255 ? 255 : v;
        }
}
/* the two rules over one ladder of sums (a file's, or a stack's): the smallest quality whose bits fit, the
 * largest when none does; the largest quality whose PSNR reaches the target, the smallest when none does */
static int pick_by_rate(const uint64_t *tot, double target_bits) {
    int pick = RATE_LADDER_N - 1; /* none fits: the largest quality (the ladder ascends) */
    for (int i = RATE_LADDER_N - 1; i >= 0; i--)
        if ((double)tot[i] <= target_bits) pick = i; /* the smallest that fits, whatever the order of the sizes */
    return pick;
}
static int pick_by_psnr(const uint64_t *err, double n_samples, double target_db) {
    int pick = 0; /* none reaches the target: the smallest quality (the ladder ascends) */
    for (int i = 0; i < RATE_LADDER_N; i++)
        if (psnr_of(err[i], n_samples) >= target_db) pick = i; /* the largest that reaches it, whatever the order */
    return pick;
}
/* the SSIM probe's sums: the mean over n_windows windows, and psnr='s rule on it */
static double ssim_of(int64_t sum, double n_windows) { return (double)sum / (16777216.0 * n_windows); }
static int pick_by_ssim(const int64_t *sum, double n_windows, double target) {
    int pick = 0;
    for (int i = 0; i < RATE_LADDER_N; i++)
        if (ssim_of(sum[i], n_windows) >= target) pick = i;
    return pick;
}

/* ---- the per-stack quality map (codec.h) ---------------------------------------------------------- */
static char g_qmap_text[4096]; /* codec_set_qmap's text; "": none */

int codec_set_qmap(const char *text) {
    if (text && strlen(text) >= sizeof(g_qmap_text)) return 1;
    if (text && text[0] && g_quant_text[0]) return 1; /* a quantiser is set */
    snprintf(g_qmap_text, sizeof(g_qmap_text), "%s", text ? text : "");
    return 0;
}

static int ladder_index(long q) {
    for (int i = 0; i < RATE_LADDER_N; i++)
        if (kRateLadder[i] == q) return i;
    return -1;
}

int codec_parse_qmap(const char *path, int n_stacks, int *qualities) {
    if (!path || !path[0] || n_stacks <= 0 || !qualities) return 1;
    FILE *f = fopen(path, "r");
    if (!f) return 1;
    int *q = (int *)malloc(sizeof(int) * (size_t)n_stacks);
    int n = 0, bad = q == NULL;
    char line[64];
    while (!bad && fgets(line, sizeof(line), f)) {
        size_t len = strlen(line);
        if (len && line[len - 1] == '\n') line[--len] = '\0';
        if (len && line[len - 1] == '\r') line[--len] = '\0';
        char *end = NULL;
        const long v = (line[0] >= '0' && line[0] <= '9') ? strtol(line, &end, 10) : -1;
        if (v < 0 || *end != '\0' || ladder_index(v) < 0 || n >= n_stacks) bad = 1; /* (n >= n_stacks: a line too many) */
        else q[n++] = (int)v;
    }
    fclose(f);
    if (!bad && n != n_stacks) bad = 1;
    if (!bad) memcpy(qualities, q, sizeof(int) * (size_t)n_stacks);
    free(q);
    return bad;
}

/* The map of a call: codec_set_qmap's text, else DCT3D_CODEC_QMAP.  *path = NULL: none given.  1 after printing when
 * the text is no "qmap=<path>", a quantiser is given too, or the call runs the host Exp-Golomb path. */
static int call_qmap(const char **path) {
    const char *text = g_qmap_text[0] ? g_qmap_text : getenv("DCT3D_CODEC_QMAP");
    *path = NULL;
    if (!text || !text[0]) return 0;
    if (strncmp(text, "qmap=", 5) || !text[5]) {
        printf("Invalid quality map '%s': qmap=<path>\n", text);
        return 1;
    }
    const char *qt = sel_text(SEL_QUANT);
    if (qt && qt[0]) {
        printf("A quantiser ('%s') and a quality map ('%s') exclude each other\n", qt, text);
        return 1;
    }
    const char *he = getenv("DCT3D_CODEC_HOST_EG");
    if (he && he[0] == '1') {
        printf("qmap= needs the device stream calls (DCT3D_CODEC_HOST_EG=1 is set)\n");
        return 1;
    }
    *path = text + 5;
    return 0;
}
/* the commands that take no map: 1 after printing when one is given */
static int reject_qmap(const char *what) {
    const char *text = g_qmap_text[0] ? g_qmap_text : getenv("DCT3D_CODEC_QMAP");
    if (!text || !text[0]) return 0;
    printf("qmap= applies to single-device encodes and decodes only (%s)\n", what);
    return 1;
}

/* ---- the per-(stack, channel) quality map of encode_rgb / decode_rgb (codec.h) ---------------------- */
static char g_qmap3_text[4096]; /* codec_set_qmap3's text; "": none */
static char g_cq_text[16];      /* codec_set_cq's text; "": none */

int codec_set_qmap3(const char *text) {
    if (text && strlen(text) >= sizeof(g_qmap3_text)) return 1;
    snprintf(g_qmap3_text, sizeof(g_qmap3_text), "%s", text ? text : "");
    return 0;
}
int codec_set_cq(const char *text) {
    if (text && strlen(text) >= sizeof(g_cq_text)) return 1;
    snprintf(g_cq_text, sizeof(g_cq_text), "%s", text ? text : "");
    return 0;
}

int codec_parse_qmap3(const char *path, int n_stacks, int *qualities) {
    if (!path || !path[0] || n_stacks <= 0 || !qualities) return 1;
    FILE *f = fopen(path, "r");
    if (!f) return 1;
    int *q = (int *)malloc(sizeof(int) * 3 * (size_t)n_stacks);
    int n = 0, bad = q == NULL;
    char line[64];
    while (!bad && fgets(line, sizeof(line), f)) {
        size_t len = strlen(line);
        if (len && line[len - 1] == '\n') line[--len] = '\0';
        if (len && line[len - 1] == '\r') line[--len] = '\0';
        if (n >= n_stacks) bad = 1; /* a line too many */
        const char *p = line;
        for (int k = 0; k < 3 && !bad; k++) { /* three numbers, one space between, nothing else */
            char *end = NULL;
            const long v = (*p >= '0' && *p <= '9') ? strtol(p, &end, 10) : -1;
            if (v < 0 || ladder_index(v) < 0 || *end != (k < 2 ? ' ' : '\0')) bad = 1;
            else {
                q[3 * n + k] = (int)v;
                p = end + 1;
            }
        }
        if (!bad) n++;
    }
    fclose(f);
    if (!bad && n != n_stacks) bad = 1;
    if (!bad) memcpy(qualities, q, sizeof(int) * 3 * (size_t)n_stacks);
    free(q);
    return bad;
}

static const char *qmap3_text(void) { return g_qmap3_text[0] ? g_qmap3_text : getenv("DCT3D_CODEC_QMAP3"); }
static const char *cq_text(void) { return g_cq_text[0] ? g_cq_text : getenv("DCT3D_CODEC_CQ"); }
/* The three-column map of a call on `channels` channels: codec_set_qmap3's text, else DCT3D_CODEC_QMAP3; and the
 * chroma offset cq=<k> (codec_set_cq, else DCT3D_CODEC_CQ).  *path = NULL: none given; *cq = k (0 without cq=).  1
 * after printing when a text does not parse, the map stands beside a quantiser, a per-stack map or a PSNR target, on a
 * grey call (what names it) or on the host Exp-Golomb path, or cq= stands without ycc=1 or without rate= and qmap3=. */
static int call_qmap3(const char *what, int channels, int writes_map, int psnr_set, int ycc, const char **path, int *cq) {
    /* (writes_map: the call has a target whose first pass writes the map -- rate=, or psnr_rgb=) */
    const char *text = qmap3_text(), *ct = cq_text();
    *path = NULL;
    *cq = 0;
    if (ct && ct[0]) {
        const char *v = strncmp(ct, "cq=", 3) ? ct : ct + 3;
        char *end = NULL;
        const long k = (v[0] >= '0' && v[0] <= '9') ? strtol(v, &end, 10) : -1;
        if (k < 0 || k > 15 || *end) {
            printf("Invalid chroma offset '%s': cq=<0..15>, rungs of the ladder\n", ct);
            return 1;
        }
        if (!ycc) {
            printf("cq= needs ycc=1: it codes the Cb and Cr planes more coarsely than Y\n");
            return 1;
        }
        if (!writes_map || !text || !text[0]) {
            printf("cq= applies to an encode_rgb with rate= and qmap3= (%s)\n", what);
            return 1;
        }
        *cq = (int)k;
    }
    if (!text || !text[0]) return 0;
    if (strncmp(text, "qmap3=", 6) || !text[6]) {
        printf("Invalid quality map '%s': qmap3=<path>\n", text);
        return 1;
    }
    if (channels != 3) {
        printf("qmap3= and cq= apply to encode_rgb and decode_rgb on one device (%s)\n", what);
        return 1;
    }
    const char *qt = sel_text(SEL_QUANT), *mt = g_qmap_text[0] ? g_qmap_text : getenv("DCT3D_CODEC_QMAP");
    if ((qt && qt[0]) || (mt && mt[0]) || psnr_set) {
        printf("qmap3= excludes q=, qmap= and psnr= ('%s')\n", text);
        return 1;
    }
    if (host_eg_on()) {
        printf("qmap3= needs the device stream calls (DCT3D_CODEC_HOST_EG=1 is set)\n");
        return 1;
    }
    *path = text + 6;
    return 0;
}
/* the commands that take no three-column map: 1 after printing when one, or cq=, is given */
static int reject_qmap3(const char *what) {
    const char *text = qmap3_text(), *ct = cq_text();
    if ((!text || !text[0]) && (!ct || !ct[0])) return 0;
    printf("qmap3= and cq= apply to encode_rgb and decode_rgb on one device (%s)\n", what);
    return 1;
}
/* the call's three-column map as ladder indices, [n_stacks][3]: 1 after printing on an error */
static int read_qmap3(const char *path, int n_stacks, uint8_t *index) {
    int *q = (int *)malloc(sizeof(int) * 3 * (size_t)n_stacks);
    if (!q || codec_parse_qmap3(path, n_stacks, q)) {
        printf("Invalid quality map file '%s': %d lines, one per stack, each three qualities of the ladder separated by "
               "single spaces\n", path, n_stacks);
        free(q);
        return 1;
    }
    for (int i = 0; i < 3 * n_stacks; i++) index[i] = (uint8_t)ladder_index(q[i]);
    free(q);
    return 0;
}
static int write_qmap3(const char *path, int n_stacks, const uint8_t *index) {
    FILE *f = fopen(path, "w");
    if (!f) {
        printf("Cannot open output file %s\n", path);
        return 1;
    }
    for (int s = 0; s < n_stacks; s++)
        fprintf(f, "%d %d %d\n", kRateLadder[index[3 * s]], kRateLadder[index[3 * s + 1]], kRateLadder[index[3 * s + 2]]);
    if (fflush(f) || fclose(f)) {
        printf("Error writing the quality map %s\n", path);
        return 1;
    }
    return 0;
}

static char g_colour_text[16]; /* codec_set_colour's text; "": none */

int codec_set_colour(const char *text) {
    if (text && strlen(text) >= sizeof(g_colour_text)) return 1;
    snprintf(g_colour_text, sizeof(g_colour_text), "%s", text ? text : "");
    return 0;
}
/* The colour mode of a call on `channels` channels: codec_set_colour's text, else DCT3D_CODEC_YCC ("1", "0" or the
 * text).  *ycc = 1: the Y, Cb, Cr planes.  1 after printing when the text is no "ycc=0|1", or the mode is on for a
 * call that has no colour stage: grey (what names it), a PSNR target, the host Exp-Golomb path. */
static int call_colour(const char *what, int channels, int target_sel, int *ycc) { /* (target_sel: 0 | SEL_PSNR | SEL_SSIM) */
    const char *text = g_colour_text[0] ? g_colour_text : getenv("DCT3D_CODEC_YCC");
    *ycc = 0;
    if (!text || !text[0]) return 0;
    const char *v = strncmp(text, "ycc=", 4) ? text : text + 4;
    if ((v[0] != '0' && v[0] != '1') || v[1]) {
        printf("Invalid colour mode '%s': ycc=0 or ycc=1\n", text);
        return 1;
    }
    if (v[0] == '0') return 0;
    if (channels != 3) {
        printf("ycc= applies to encode_rgb and decode_rgb on one device (%s)\n", what);
        return 1;
    }
    if (target_sel == SEL_SSIM) {
        printf("ycc=1 and ssim= exclude each other: the SSIM probe measures the R, G, B planes (luma SSIM is not built)\n");
        return 1;
    }
    if (target_sel == SEL_PSNR) {
        printf("ycc=1 and psnr= exclude each other: the distortion probe would measure the Y, Cb, Cr planes, not the "
               "RGB samples\n");
        return 1;
    }
    if (host_eg_on()) {
        printf("ycc=1 needs the device stream calls (DCT3D_CODEC_HOST_EG=1 is set)\n");
        return 1;
    }
    *ycc = 1;
    return 0;
}
/* the context of a call codes the Y, Cb, Cr planes: 1 after printing on an error */
static int ctx_apply_colour(dct3d_ctx *ctx, int ycc) {
    if (!ycc) return 0;
    const int rc = dct3d_ctx_set_option(ctx, DCT3D_OPT_COLOUR, DCT3D_COLOUR_YCBCR);
    if (rc) printf("Error setting the colour transform: %s\n", dct3d_strerror(rc));
    return rc != 0;
}
static char g_chroma_text[16]; /* codec_set_chroma's text; "": none */

int codec_set_chroma(const char *text) {
    if (text && strlen(text) >= sizeof(g_chroma_text)) return 1;
    snprintf(g_chroma_text, sizeof(g_chroma_text), "%s", text ? text : "");
    return 0;
}
/* The chroma mode of a call on `channels` channels whose colour mode is ycc: codec_set_chroma's text, else
 * DCT3D_CODEC_CHROMA ("420", "444" or the text).  *c420 = 1: Cb and Cr at a quarter of the samples.  1 after
 * printing when the text is no "chroma=420|444", or 4:2:0 is asked of a call that cannot do it: grey or several
 * devices (what names it), without ycc=1, the host Exp-Golomb path. */
static int call_chroma(const char *what, int channels, int ycc, int *c420) {
    const char *text = g_chroma_text[0] ? g_chroma_text : getenv("DCT3D_CODEC_CHROMA");
    *c420 = 0;
    if (!text || !text[0]) return 0;
    const char *v = strncmp(text, "chroma=", 7) ? text : text + 7;
    if (strcmp(v, "420") && strcmp(v, "444")) {
        printf("Invalid chroma mode '%s': chroma=420 or chroma=444\n", text);
        return 1;
    }
    if (!strcmp(v, "444")) return 0;
    if (channels != 3) {
        printf("chroma= applies to encode_rgb and decode_rgb on one device (%s)\n", what);
        return 1;
    }
    if (host_eg_on()) {
        printf("chroma=420 needs the device stream calls (DCT3D_CODEC_HOST_EG=1 is set)\n");
        return 1;
    }
    if (!ycc) {
        printf("chroma=420 needs ycc=1: it subsamples the Cb and Cr planes of the colour transform\n");
        return 1;
    }
    *c420 = 1;
    return 0;
}
/* the context of a call codes Cb and Cr at 4:2:0: 1 after printing on an error */
static int ctx_apply_chroma(dct3d_ctx *ctx, int c420) {
    if (!c420) return 0;
    const int rc = dct3d_ctx_set_chroma(ctx, DCT3D_CHROMA_420);
    if (rc) printf("Error setting the chroma mode: %s\n", dct3d_strerror(rc));
    return rc != 0;
}
/* reads the call's map into ladder indices, one per stack: 1 after printing on an error */
static int read_qmap(const char *path, int n_stacks, uint8_t *index) {
    int *q = (int *)malloc(sizeof(int) * (size_t)n_stacks);
    if (!q || codec_parse_qmap(path, n_stacks, q)) {
        printf("Invalid quality map file '%s': %d lines, one per stack, each a quality of the ladder\n", path, n_stacks);
        free(q);
        return 1;
    }
    for (int s = 0; s < n_stacks; s++) index[s] = (uint8_t)ladder_index(q[s]);
    free(q);
    return 0;
}
static int write_qmap(const char *path, int n_stacks, const uint8_t *index) {
    FILE *f = fopen(path, "w");
    if (!f) {
        printf("Cannot open output file %s\n", path);
        return 1;
    }
    for (int s = 0; s < n_stacks; s++) fprintf(f, "%d\n", kRateLadder[index[s]]);
    if (fflush(f) || fclose(f)) {
        printf("Error writing the quality map %s\n", path);
        return 1;
    }
    return 0;
}

/* stack_pick (with a quality map): the rules per stack instead -- stack s's bits and squared error summed over the
 * channels, the rate target's budget that of `depth` frames, the PSNR over the stack's unpadded samples of all
 * channels (the zero-filled frames of a short last stack count); stack_pick[s] = the ladder index.  Prints
 * "qmap: stacks=<n> bits=<total>" and leaves the context's quantiser alone.
 * cq >= 0 (a three-column map, rate target, three channels): stack_pick is [n_stacks][3]; candidate i of a stack codes
 * channel 0 at rung i and channels 1 and 2 at rung j = min(i + cq, last), costs the three channels' bits under those
 * rungs, and the rate rule picks among the candidates; stack_pick[s] = {i, j, j}.  Prints "qmap3: ...". */
static int rate_first_pass(dct3d_ctx *ctx, FILE *in, uint8_t *fr, int width, int height, int frames, int depth, int batch,
                           int channels, double target, int metric, uint8_t *stack_pick, int cq) {
    const int n = depth + 14, n_stacks = (frames + depth - 1) / depth;
    const size_t stack_bytes = (size_t)channels * width * height * depth;
    int32_t tabs[RATE_LADDER_N * QUANT_MAX_STEPS];
    uint64_t tot[RATE_LADDER_N], err[RATE_LADDER_N], map_bits = 0;
    ladder_tables(depth, tabs);
    int64_t sim[RATE_LADDER_N]; /* METRIC_SSIM: the sums of v over the file */
    int nwx = 1, nwy = 1;
    if (metric == METRIC_SSIM) (void)dct3d_ssim_windows(width, height, &nwx, &nwy);
    const double n_win = (double)nwx * (double)nwy; /* windows of one frame and channel */
    for (int i = 0; i < RATE_LADDER_N; i++) tot[i] = err[i] = 0, sim[i] = 0;
    const size_t n_sums = (size_t)RATE_LADDER_N * batch * channels;
    uint64_t *bits = (uint64_t *)malloc(sizeof(uint64_t) * n_sums * 2), *sse = bits ? bits + n_sums : NULL;
    int64_t *ssim = (int64_t *)malloc(sizeof(int64_t) * (metric == METRIC_SSIM ? n_sums : 1));
    if (!bits || !ssim) {
        printf("Out of memory\n");
        free(bits);
        free(ssim);
        return 1;
    }
    int status = 0;
    for (int s0 = 0; !status && s0 < n_stacks; s0 += batch) {
        const int nb = (n_stacks - s0) < batch ? (n_stacks - s0) : batch;
        size_t got = 0, r;
        const size_t want = stack_bytes * nb;
        while (got < want && (r = fread(fr + got, 1, want - got, in)) > 0) got += r;
        if (got < want) memset(fr + got, 0, want - got); /* a short last stack is zero-filled, as the encode's */
        const int rc = metric == METRIC_SSIM ? dct3d_ssim_frames(ctx, fr, width, height, channels, nb, tabs, RATE_LADDER_N, ssim, NULL, bits)
                       : metric == METRIC_PSNR ? dct3d_distortion_frames(ctx, fr, width, height, channels, nb, tabs, RATE_LADDER_N, sse, bits)
                                               : dct3d_rate_frames(ctx, fr, width, height, channels, nb, tabs, RATE_LADDER_N, bits);
        if (rc) {
            printf("Error running the %s probe: %s\n", metric == METRIC_SSIM ? "SSIM" : metric == METRIC_PSNR ? "distortion" : "rate",
                   dct3d_strerror(rc));
            status = 1;
            break;
        }
        for (int i = 0; i < RATE_LADDER_N; i++)
            for (int k = 0; k < nb * channels; k++) {
                tot[i] += bits[(size_t)i * nb * channels + k];
                if (metric == METRIC_PSNR) err[i] += sse[(size_t)i * nb * channels + k];
                if (metric == METRIC_SSIM) sim[i] += ssim[(size_t)i * nb * channels + k];
            }
        for (int s = 0; stack_pick && s < nb; s++) { /* the same rules on this stack's sums */
            uint64_t sb[RATE_LADDER_N], se[RATE_LADDER_N];
            int64_t sm[RATE_LADDER_N];
            for (int i = 0; i < RATE_LADDER_N; i++) {
                sb[i] = se[i] = 0, sm[i] = 0;
                for (int ch = 0; ch < channels; ch++) {
                    sb[i] += bits[((size_t)i * nb + s) * channels + ch];
                    if (metric == METRIC_PSNR) se[i] += sse[((size_t)i * nb + s) * channels + ch];
                    if (metric == METRIC_SSIM) sm[i] += ssim[((size_t)i * nb + s) * channels + ch];
                }
            }
            const double px = (double)width * (double)height * (double)depth;
            if (cq >= 0) {
                for (int i = 0; i < RATE_LADDER_N; i++) {
                    const int j = i + cq < RATE_LADDER_N ? i + cq : RATE_LADDER_N - 1;
                    sb[i] = bits[((size_t)i * nb + s) * 3] + bits[((size_t)j * nb + s) * 3 + 1] + bits[((size_t)j * nb + s) * 3 + 2];
                }
                const int p = pick_by_rate(sb, target * px), j = p + cq < RATE_LADDER_N ? p + cq : RATE_LADDER_N - 1;
                stack_pick[3 * (s0 + s)] = (uint8_t)p;
                stack_pick[3 * (s0 + s) + 1] = stack_pick[3 * (s0 + s) + 2] = (uint8_t)j;
                map_bits += sb[p];
                continue;
            }
            const int p = metric == METRIC_SSIM ? pick_by_ssim(sm, n_win * (double)depth * (double)channels, target)
                          : metric == METRIC_PSNR ? pick_by_psnr(se, px * (double)channels, target)
                                                  : pick_by_rate(sb, target * px);
            stack_pick[s0 + s] = (uint8_t)p;
            map_bits += sb[p];
        }
    }
    free(bits);
    free(ssim);
    if (status) return 1;
    if (stack_pick) {
        printf("%s: stacks=%d bits=%llu\n", cq >= 0 ? "qmap3" : "qmap", n_stacks, (unsigned long long)map_bits);
    } else {
        int pick;
        if (metric == METRIC_SSIM) {
            const double n_windows = n_win * (double)channels * (double)n_stacks * (double)depth;
            pick = pick_by_ssim(sim, n_windows, target);
            printf("ssim: q=%d ssim=%.6f bits=%llu\n", kRateLadder[pick], ssim_of(sim[pick], n_windows), (unsigned long long)tot[pick]);
        } else if (metric == METRIC_PSNR) {
            const double n_samples = (double)width * (double)height * (double)channels * (double)n_stacks * (double)depth;
            pick = pick_by_psnr(err, n_samples, target);
            printf("psnr: q=%d psnr=%.3f bits=%llu\n", kRateLadder[pick], psnr_of(err[pick], n_samples), (unsigned long long)tot[pick]);
        } else {
            pick = pick_by_rate(tot, target * (double)width * (double)height * (double)frames);
            printf("rate: q=%d bits=%llu\n", kRateLadder[pick], (unsigned long long)tot[pick]);
        }
        const int rc = dct3d_ctx_set_quant(ctx, tabs + pick * n, n);
        if (rc) {
            printf("Error setting the quantiser: %s\n", dct3d_strerror(rc));
            return 1;
        }
    }
    if (fseek(in, 0, SEEK_SET)) {
        printf("Cannot rewind the input file for the second pass\n");
        return 1;
    }
    return 0;
}

/* The first pass of an encode_rgb with an RGB-domain PSNR target (psnr_rgb=<dB>; codec.h): the RGB-domain
 * distortion probe (dct3d_distortion_rgb_frames) per batch over the ladder, candidate i = (rung i, rung j, rung j), j =
 * min(i + cq, last) (cq: with a three-column map; else 0), in the context's colour and chroma mode; the squared
 * errors of the pixels and the candidates' bits summed over the file.  PSNR = 10 log10(255^2 3 w h frames / sse), the
 * zero-filled frames of a short last stack counting as frames; the pick is pick_by_psnr's.  Without a map it prints
 * "psnr_rgb: q=<qY>,<qCb>,<qCr> psnr=<dB> bits=<total>" and sets the context's quantiser to the pick.  stack_pick
 * ([n_stacks], or [n_stacks][3] with qw == 3): the rule per stack over the stack's pixels instead; prints "qmap: ..."
 * or "qmap3: ..." as the rate target does.  Rewinds the input.  1 after printing on an error. */
/* metric == METRIC_SSIM: an RGB SSIM target instead (ssim_rgb=<target>; codec.h): the RGB and luma SSIM probe
 * (dct3d_ssim_rgb_frames) in the probe's place, the same candidates; the sums of R, G and B added, the mean over all
 * windows of the three planes (dct3d_ssim_windows per frame and plane; the zero-filled frames count); the pick is
 * pick_by_ssim's.  luma (the YCbCr modes): the luma sums are taken too.  Prints "ssim_rgb: q=<qY>,<qCb>,<qCr>
 * ssim=<6 decimals> [ssim_y=<6 decimals> ]bits=<total>". */
static int psnr_rgb_first_pass(dct3d_ctx *ctx, FILE *in, uint8_t *fr, int width, int height, int frames, int depth, int batch,
                               double target, int metric, int luma, uint8_t *stack_pick, int qw, int cq) {
    const int n = depth + 14, n_stacks = (frames + depth - 1) / depth;
    const size_t stack_bytes = (size_t)3 * width * height * depth;
    int32_t tabs[RATE_LADDER_N * QUANT_MAX_STEPS];
    uint8_t cand[3 * RATE_LADDER_N];
    int jof[RATE_LADDER_N];
    uint64_t tot[RATE_LADDER_N], err[RATE_LADDER_N], map_bits = 0;
    int64_t sim[RATE_LADDER_N], sim_y[RATE_LADDER_N]; /* METRIC_SSIM: the sums of v over the file */
    int nwx = 1, nwy = 1;
    if (metric == METRIC_SSIM) (void)dct3d_ssim_windows(width, height, &nwx, &nwy);
    const double n_win = (double)nwx * (double)nwy; /* windows of one frame and plane */
    ladder_tables(depth, tabs);
    for (int i = 0; i < RATE_LADDER_N; i++) {
        tot[i] = err[i] = 0;
        sim[i] = sim_y[i] = 0;
        jof[i] = i + cq < RATE_LADDER_N ? i + cq : RATE_LADDER_N - 1;
        cand[3 * i] = (uint8_t)i;
        cand[3 * i + 1] = cand[3 * i + 2] = (uint8_t)jof[i];
    }
    const size_t n_sse = (size_t)RATE_LADDER_N * batch, n_bits = n_sse * 3;
    uint64_t *sse = (uint64_t *)malloc(sizeof(uint64_t) * (n_sse + n_bits)), *bits = sse ? sse + n_sse : NULL;
    int64_t *ssim = (int64_t *)malloc(sizeof(int64_t) * (metric == METRIC_SSIM ? 4 * n_sse : 1)), *ssim_y = ssim ? ssim + 3 * n_sse : NULL;
    if (!sse || !ssim) {
        printf("Out of memory\n");
        free(sse);
        free(ssim);
        return 1;
    }
    int status = 0;
    for (int s0 = 0; !status && s0 < n_stacks; s0 += batch) {
        const int nb = (n_stacks - s0) < batch ? (n_stacks - s0) : batch;
        size_t got = 0, r;
        const size_t want = stack_bytes * nb;
        while (got < want && (r = fread(fr + got, 1, want - got, in)) > 0) got += r;
        if (got < want) memset(fr + got, 0, want - got); /* a short last stack is zero-filled, as the encode's */
        const int rc = metric == METRIC_SSIM
                           ? dct3d_ssim_rgb_frames(ctx, fr, width, height, nb, tabs, RATE_LADDER_N, cand, RATE_LADDER_N, ssim,
                                                   luma ? ssim_y : NULL, NULL, bits)
                           : dct3d_distortion_rgb_frames(ctx, fr, width, height, nb, tabs, RATE_LADDER_N, cand, RATE_LADDER_N, sse,
                                                         NULL, bits);
        if (rc) {
            printf("Error running the RGB %s probe: %s\n", metric == METRIC_SSIM ? "SSIM" : "distortion", dct3d_strerror(rc));
            status = 1;
            break;
        }
        for (int s = 0; s < nb; s++) {
            uint64_t sb[RATE_LADDER_N], se[RATE_LADDER_N];
            int64_t sm[RATE_LADDER_N];
            for (int i = 0; i < RATE_LADDER_N; i++) {
                const int j = jof[i];
                se[i] = 0, sm[i] = 0;
                if (metric == METRIC_SSIM) {
                    for (int k = 0; k < 3; k++) sm[i] += ssim[((size_t)i * nb + s) * 3 + k];
                    if (luma) sim_y[i] += ssim_y[(size_t)i * nb + s];
                } else {
                    se[i] = sse[(size_t)i * nb + s];
                }
                sb[i] = bits[((size_t)i * nb + s) * 3] + bits[((size_t)j * nb + s) * 3 + 1] + bits[((size_t)j * nb + s) * 3 + 2];
                err[i] += se[i];
                sim[i] += sm[i];
                tot[i] += sb[i];
            }
            if (!stack_pick) continue;
            const int p = metric == METRIC_SSIM ? pick_by_ssim(sm, 3.0 * n_win * (double)depth, target)
                                                : pick_by_psnr(se, 3.0 * (double)width * (double)height * (double)depth, target);
            if (qw == 3) {
                stack_pick[3 * (s0 + s)] = (uint8_t)p;
                stack_pick[3 * (s0 + s) + 1] = stack_pick[3 * (s0 + s) + 2] = (uint8_t)jof[p];
            } else {
                stack_pick[s0 + s] = (uint8_t)p;
            }
            map_bits += sb[p];
        }
    }
    free(sse);
    free(ssim);
    if (status) return 1;
    if (stack_pick) {
        printf("%s: stacks=%d bits=%llu\n", qw == 3 ? "qmap3" : "qmap", n_stacks, (unsigned long long)map_bits);
    } else {
        const double n_samples = 3.0 * (double)width * (double)height * (double)n_stacks * (double)depth;
        const double n_windows = n_win * (double)n_stacks * (double)depth; /* of one plane */
        const int pick = metric == METRIC_SSIM ? pick_by_ssim(sim, 3.0 * n_windows, target) : pick_by_psnr(err, n_samples, target);
        if (metric == METRIC_SSIM) {
            printf("ssim_rgb: q=%d,%d,%d ssim=%.6f ", kRateLadder[pick], kRateLadder[jof[pick]], kRateLadder[jof[pick]],
                   ssim_of(sim[pick], 3.0 * n_windows));
            if (luma) printf("ssim_y=%.6f ", ssim_of(sim_y[pick], n_windows));
            printf("bits=%llu\n", (unsigned long long)tot[pick]);
        } else
            printf("psnr_rgb: q=%d,%d,%d psnr=%.3f bits=%llu\n", kRateLadder[pick], kRateLadder[jof[pick]], kRateLadder[jof[pick]],
                   psnr_of(err[pick], n_samples), (unsigned long long)tot[pick]);
        const int rc = dct3d_ctx_set_quant(ctx, tabs + pick * n, n);
        if (rc) {
            printf("Error setting the quantiser: %s\n", dct3d_strerror(rc));
            return 1;
        }
    }
    if (fseek(in, 0, SEEK_SET)) {
        printf("Cannot rewind the input file for the second pass\n");
        return 1;
    }
    return 0;
}

static int default_batch(void) {
    const char *e = getenv("DCT3D_CODEC_BATCH");
    int b = e ? atoi(e) : 16;
    return b > 0 ? b : 16;
}

int encode_ex(const char *inName, const char *outName, int width, int height, int frames, int platformIndex,
              int depth, int batch) {
    if (!geometry_ok(width, height, frames, depth)) return invalid_geometry(width, height, frames, depth);
    return encode_any(inName, outName, width, height, frames, platformIndex, depth, batch, 1);
}

int decode_ex(const char *inName, const char *outName, int width, int height, int frames, int platformIndex,
              int depth, int batch) {
    if (!geometry_ok(width, height, frames, depth)) return invalid_geometry(width, height, frames, depth);
    return decode_any(inName, outName, width, height, frames, platformIndex, depth, batch, 1);
}

/* ---- several devices ------------------------------------------------------------------------ */

typedef struct {
    dct3d_ctx *ctx;
    int width, height, decode;
    pthread_t th;
    int started;
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int state;  /* 0 idle, 1 job posted, 2 job done, 3 quit */
    int rc;
    int nb;                 /* stacks of the job */
    uint8_t *raster;        /* encode: input; decode: output (stack_px * batch) */
    unsigned char *eg;      /* encode: the batch's stream, fetched (grown as needed) */
    size_t eg_cap;
    uint64_t bits;          /* encode: stream bits; decode: bits consumed from the window */
    const unsigned char *win;  /* decode: the inflated window, its length and first bit */
    size_t win_len;
    int win_bit;
} dev_worker;

static void *dev_worker_main(void *arg) {
    dev_worker *w = (dev_worker *)arg;
    for (;;) {
        pthread_mutex_lock(&w->mu);
        while (w->state != 1 && w->state != 3) pthread_cond_wait(&w->cv, &w->mu);
        const int quit = w->state == 3;
        pthread_mutex_unlock(&w->mu);
        if (quit) return NULL;
        int rc;
        if (!w->decode) {
            uint64_t tb = 0;
            rc = dct3d_encode_eg(w->ctx, w->raster, w->width, w->height, w->nb, 0, 0, &tb);
            const size_t nbytes = (size_t)((tb + 7) / 8);
            if (!rc && nbytes > w->eg_cap) {
                free(w->eg);
                w->eg_cap = nbytes + nbytes / 4;
                w->eg = (unsigned char *)malloc(w->eg_cap);
                if (!w->eg) rc = DCT3D_ENOMEM;
            }
            if (!rc) rc = dct3d_eg_fetch(w->ctx, w->eg, nbytes);
            w->bits = tb;
        } else {
            uint64_t eb = 0;
            rc = dct3d_decode_eg(w->ctx, w->win, w->win_len, w->win_bit, w->width, w->height, w->nb, w->raster, &eb);
            w->bits = eb;
        }
        pthread_mutex_lock(&w->mu);
        w->rc = rc;
        w->state = 2;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
    }
}

static void dev_post(dev_worker *w) {
    pthread_mutex_lock(&w->mu);
    w->state = 1;
    pthread_cond_broadcast(&w->cv);
    pthread_mutex_unlock(&w->mu);
}

static int dev_wait(dev_worker *w) {
    pthread_mutex_lock(&w->mu);
    while (w->state != 2) pthread_cond_wait(&w->cv, &w->mu);
    w->state = 0;
    const int rc = w->rc;
    pthread_mutex_unlock(&w->mu);
    return rc;
}

static void dev_workers_destroy(dev_worker *ws, int n) {
    if (!ws) return;
    for (int i = 0; i < n; i++) {
        dev_worker *w = &ws[i];
        if (w->started) {
            pthread_mutex_lock(&w->mu);
            while (w->state == 1) pthread_cond_wait(&w->cv, &w->mu);  /* a posted job finishes first */
            w->state = 3;
            pthread_cond_broadcast(&w->cv);
            pthread_mutex_unlock(&w->mu);
            pthread_join(w->th, NULL);
            pthread_mutex_destroy(&w->mu);
            pthread_cond_destroy(&w->cv);
        }
        dct3d_ctx_destroy(w->ctx);
        free(w->raster);
        free(w->eg);
    }
    free(ws);
}

/* one ctx + thread per device (platform indices 1-based, as encode_ex); NULL after printing on failure */
static dev_worker *dev_workers_create(const int *platformIndices, int n, int width, int height, int depth,
                                      size_t raster_bytes, int decode) {
    dev_worker *ws = (dev_worker *)calloc((size_t)n, sizeof(dev_worker));
    if (!ws) {
        printf("Out of memory\n");
        return NULL;
    }
    for (int i = 0; i < n; i++) {
        dev_worker *w = &ws[i];
        w->width = width;
        w->height = height;
        w->decode = decode;
        const int idx = platformIndices[i];
        int rc = dct3d_ctx_create(idx > 0 ? idx - 1 : 0, 8, 8, depth, &w->ctx);
        if (rc) {
            printf("Error creating the device context (device %d): %s\n", idx, dct3d_strerror(rc));
            dev_workers_destroy(ws, n);
            return NULL;
        }
        if (ctx_apply_quant(w->ctx, depth)) {
            dev_workers_destroy(ws, n);
            return NULL;
        }
        w->raster = (uint8_t *)malloc(raster_bytes);
        if (!w->raster || pthread_mutex_init(&w->mu, NULL) || pthread_cond_init(&w->cv, NULL)) {
            printf("Out of memory\n");
            dev_workers_destroy(ws, n);
            return NULL;
        }
        if (pthread_create(&w->th, NULL, dev_worker_main, w)) {
            pthread_mutex_destroy(&w->mu);
            pthread_cond_destroy(&w->cv);
            printf("Cannot start a device thread\n");
            dev_workers_destroy(ws, n);
            return NULL;
        }
        w->started = 1;
    }
    return ws;
}

/* `bits` stream bits coded from a zero carry, re-aligned behind the c (0..7) bits of the partial byte
 * cb (MSB first): out[0] = cb | s[0] >> c, out[i] = s[i-1] << (8 - c) | s[i] >> c; returns the bits */
static uint64_t join_carry(const unsigned char *s, uint64_t bits, uint8_t cb, int c, unsigned char *out) {
    const size_t n = (size_t)((bits + 7) / 8), m = (size_t)((bits + (uint64_t)c + 7) / 8);
    if (c == 0) {
        memcpy(out, s, n);
        return bits;
    }
    unsigned prev = cb >> (8 - c);
    for (size_t i = 0; i < m; i++) {
        const unsigned cur = i < n ? s[i] : 0u;
        out[i] = (unsigned char)((prev << (8 - c)) | (cur >> c));
        prev = cur;
    }
    return bits + (uint64_t)c;
}

int encode_multi(const char *inName, const char *outName, int width, int height, int frames,
                 const int *platformIndices, int nDevices, int depth, int batch) {
    if (!platformIndices || nDevices <= 0) {
        printf("No device given\n");
        return 1;
    }
    if (width <= 0 || height <= 0 || width % 8 || height % 8 || frames <= 0 || (depth != 8 && depth != 4)) {
        printf("Invalid geometry: %dx%d, %d frames, block depth %d (several devices: width/height must be multiples "
               "of 8)\n", width, height, frames, depth);
        return 1;
    }
    if (reject_targets("encode_multi") || reject_qmap("encode_multi") || reject_qmap3("encode_multi")) return 1;
    int ycc;
    int c420;
    if (call_colour("encode_multi", 1, 0, &ycc) || call_chroma("encode_multi", 1, ycc, &c420)) return 1;
    if (batch <= 0) batch = default_batch();
    FILE *in = fopen(inName, "rb");
    if (!in) {
        printf("Cannot open input file %s\n", inName);
        return 1;
    }
    FILE *out = fopen(outName, "wb");
    if (!out) {
        printf("Cannot open output file %s\n", outName);
        fclose(in);
        return 1;
    }
    const size_t frame = (size_t)width * height, stack_px = frame * depth;
    const int n_stacks = (frames + depth - 1) / depth;
    const int n_batches = (n_stacks + batch - 1) / batch;
    dev_worker *ws = dev_workers_create(platformIndices, nDevices, width, height, depth, stack_px * batch, 0);
    if (!ws) {
        fclose(in);
        fclose(out);
        return 1;
    }
    dct3d_entropy_enc *ent = dct3d_entropy_enc_create(width, height, depth, out);
    const char *dt = getenv("DCT3D_CODEC_DEFLATE_THREADS");
    int status = 0;
    if (ent && dct3d_entropy_enc_set_threads(ent, dt ? atoi(dt) : 1, 0)) {
        dct3d_entropy_enc_destroy(ent);
        ent = NULL;
    }
    unsigned char *joined = NULL;
    size_t joined_cap = 0;
    if (!ent) {
        printf("Out of memory\n");
        status = 1;
    }
    /* batch k runs on device k % n; up to n batches in flight, joined in order */
    int posted = 0;
    for (int k = 0; !status && k < n_batches; k++) {
        for (; posted < n_batches && posted < k + nDevices; posted++) {
            dev_worker *w = &ws[posted % nDevices];
            const int s0 = posted * batch, nb = (n_stacks - s0) < batch ? (n_stacks - s0) : batch;
            size_t got = 0, r;
            const size_t want = stack_px * (size_t)nb;
            while (got < want && (r = fread(w->raster + got, 1, want - got, in)) > 0) got += r;
            if (got < want) memset(w->raster + got, 0, want - got);
            w->nb = nb;
            dev_post(w);
        }
        dev_worker *w = &ws[k % nDevices];
        const int rc = dev_wait(w);
        if (rc) {
            printf("Error running the 3D DCT: %s\n", dct3d_strerror(rc));
            status = 1;
            break;
        }
        uint8_t cb;
        int cbits;
        dct3d_entropy_enc_carry(ent, &cb, &cbits);
        const size_t need = (size_t)((w->bits + 7 + 7) / 8);
        if (need > joined_cap) {
            free(joined);
            joined_cap = need + need / 4;
            joined = (unsigned char *)malloc(joined_cap);
            if (!joined) {
                printf("Out of memory\n");
                status = 1;
                break;
            }
        }
        const uint64_t tb = join_carry(w->eg, w->bits, cb, cbits, joined);
        if (dct3d_entropy_enc_push_stream(ent, joined, tb, k == n_batches - 1)) {
            printf("Error in the entropy coder\n");
            status = 1;
            break;
        }
        for (int s = 0; s < w->nb; s++) printf("Frames processed: %d\n", (k * batch + s + 1) * depth);
    }
    dev_workers_destroy(ws, nDevices);  /* waits for jobs still in flight after an error */
    dct3d_entropy_enc_destroy(ent);
    free(joined);
    fclose(in);
    if (fflush(out) || fclose(out)) status = 1;
    if (!status) printf("Encoding process completed\n");
    return status;
}

/* fwrite of decoded batch k (its device's raster buffer); clears *pending; 1 on a write error */
static int write_batch(dev_worker *ws, int n, int k, int batch, int n_stacks, size_t stack_px, int depth, FILE *out,
                       int *pending) {
    const dev_worker *w = &ws[k % n];
    const int nb = (n_stacks - k * batch) < batch ? (n_stacks - k * batch) : batch;
    *pending = -1;
    if (fwrite(w->raster, 1, stack_px * nb, out) != stack_px * nb) {
        printf("Error writing the output file\n");
        return 1;
    }
    printf("Frames processed: %d\n", (k * batch + nb) * depth);
    return 0;
}

int decode_multi(const char *inName, const char *outName, int width, int height, int frames,
                 const int *platformIndices, int nDevices, int depth, int batch) {
    if (!platformIndices || nDevices <= 0) {
        printf("No device given\n");
        return 1;
    }
    if (width <= 0 || height <= 0 || width % 8 || height % 8 || frames <= 0 || (depth != 8 && depth != 4)) {
        printf("Invalid geometry: %dx%d, %d frames, block depth %d\n", width, height, frames, depth);
        return 1;
    }
    if (reject_targets("decode_multi") || reject_qmap("decode_multi") || reject_qmap3("decode_multi")) return 1;
    int ycc;
    int c420;
    if (call_colour("decode_multi", 1, 0, &ycc) || call_chroma("decode_multi", 1, ycc, &c420)) return 1;
    if (batch <= 0) batch = default_batch();
    FILE *in = fopen(inName, "rb");
    if (!in) {
        printf("Cannot open input file %s\n", inName);
        return 1;
    }
    FILE *out = fopen(outName, "wb");
    if (!out) {
        printf("Cannot open output file %s\n", outName);
        fclose(in);
        return 1;
    }
    const size_t frame = (size_t)width * height, stack_px = frame * depth;
    const int n_stacks = (frames + depth - 1) / depth;
    const int n_batches = (n_stacks + batch - 1) / batch;
    dev_worker *ws = dev_workers_create(platformIndices, nDevices, width, height, depth, stack_px * batch, 1);
    if (!ws) {
        fclose(in);
        fclose(out);
        return 1;
    }
    dct3d_entropy_dec *ent = dct3d_entropy_dec_create(width, height, depth, in, NULL, 0);
    int status = 0;
    if (!ent) {
        printf("Out of memory\n");
        status = 1;
    }
    double bits_per_value = 4.0;  /* window estimate for the first batch; then the measured rate */
    int pending = -1;             /* the decoded batch whose raster is not written yet */
    for (int k = 0; !status && k < n_batches; k++) {
        dev_worker *w = &ws[k % nDevices];
        const int s0 = k * batch, nb = (n_stacks - s0) < batch ? (n_stacks - s0) : batch;
        const double values = (double)stack_px * nb;
        size_t need = (size_t)(values * bits_per_value / 8 * 1.25) + 65536;
        int rc;
        int first = 1;
        for (;;) {
            if (dct3d_entropy_dec_window(ent, need, &w->win, &w->win_len, &w->win_bit)) {
                rc = DCT3D_EINVAL;
                break;
            }
            w->nb = nb;
            /* the previous batch's raster is written while this one decodes -- before the post when both
             * use the same (only) device's buffer */
            if (first && pending >= 0 && nDevices == 1) status = write_batch(ws, nDevices, pending, batch, n_stacks,
                                                                           stack_px, depth, out, &pending);
            dev_post(w);
            if (first && pending >= 0) status |= write_batch(ws, nDevices, pending, batch, n_stacks, stack_px, depth,
                                                            out, &pending);
            first = 0;
            rc = dev_wait(w);
            if (rc == DCT3D_ENODATA && !dct3d_entropy_dec_eof(ent) && w->win_len >= need) {
                need *= 2;  /* the batch needs more of the stream than estimated */
                continue;
            }
            if (!rc) {
                dct3d_entropy_dec_consume(ent, w->bits);
                bits_per_value = (double)(w->bits - (uint64_t)w->win_bit) / values;
            }
            break;
        }
        if (status) break;
        if (rc == DCT3D_ENODATA || rc == DCT3D_EINVAL) {
            printf("Truncated or corrupt input stream\n");
            status = 1;
            break;
        }
        if (rc) {
            printf("Error running the inverse 3D DCT: %s\n", dct3d_strerror(rc));
            status = 1;
            break;
        }
        pending = k;
    }
    if (!status && pending >= 0) status = write_batch(ws, nDevices, pending, batch, n_stacks, stack_px, depth, out,
                                                      &pending);
    dev_workers_destroy(ws, nDevices);
    dct3d_entropy_dec_destroy(ent);
    fclose(in);
    if (fflush(out) || fclose(out)) status = 1;
    if (!status) printf("Decoding process completed\n");
    return status;
}

/* ---- packed RGB24 and frames of any size ------------------------------------------------------ */
/* The upstream colour workflow (RGBUtils split -> encode each plane -> decode each -> RGBUtils mix) with
 * the split and the mix fused into the device transform: one packed RGB24 file <-> three streams named
 * as RGBUtils names its planes, <pattern>.red / .green / .blue, each the very .bin of encode_ex for that
 * plane.  And a width or height that is no multiple of 8, grey (channels = 1: one stream, outName / inName)
 * or packed RGB24: the device pads by repeating each frame's last column and last row up to wp x hp (the
 * next multiples of 8) inside its kernels and crops on the way back; the entropy coder works on wp x hp, so
 * the streams are, byte for byte, what the same command writes for the edge-padded video at wp x hp.
 * Both, and grey at multiples of 8 (where the frames calls are the *_stacks / grey stream calls), go through
 * encode_any / decode_any.  Default: the fused stream calls (dct3d_encode_eg_frames / dct3d_decode_eg_frames)
 * -- each channel's Exp-Golomb stream is built and parsed on the device, only the frames and the streams
 * cross PCIe.  DCT3D_CODEC_HOST_EG=1: the quantised ints over PCIe (dct3d_encode_frames /
 * dct3d_decode_frames) and the host entropy coder per stack; the same files. */
static const char *const kRgbSuffix[3] = {".red", ".green", ".blue"};

static FILE *open_plane(const char *pattern, int ch, const char *mode) {
    const size_t n = strlen(pattern) + 8;
    char *name = (char *)malloc(n);
    if (!name) return NULL;
    snprintf(name, n, "%s%s", pattern, kRgbSuffix[ch]);
    FILE *f = fopen(name, mode);
    if (!f) printf("Cannot open %s file %s\n", mode[0] == 'r' ? "input" : "output", name);
    free(name);
    return f;
}

int encode_rgb_ex(const char *inName, const char *outPattern, int width, int height, int frames, int platformIndex,
                  int depth, int batch) {
    if (!geometry_ok(width, height, frames, depth)) return invalid_geometry(width, height, frames, depth);
    return encode_any(inName, outPattern, width, height, frames, platformIndex, depth, batch, 3);
}

int decode_rgb_ex(const char *inPattern, const char *outName, int width, int height, int frames, int platformIndex,
                  int depth, int batch) {
    if (!geometry_ok(width, height, frames, depth)) return invalid_geometry(width, height, frames, depth);
    return decode_any(inPattern, outName, width, height, frames, platformIndex, depth, batch, 3);
}

static FILE *open_stream(const char *name, int channels, int ch, const char *mode) {
    if (channels == 3) return open_plane(name, ch, mode);
    FILE *f = fopen(name, mode);
    if (!f) printf("Cannot open %s file %s\n", mode[0] == 'r' ? "input" : "output", name);
    return f;
}

static int host_eg_on(void) {
    const char *he = getenv("DCT3D_CODEC_HOST_EG");
    return he && he[0] == '1';
}

static int encode_any(const char *inName, const char *outName, int width, int height, int frames, int platformIndex,
                      int depth, int batch, int channels) {
    double rate_bpp = 0.0;
    int rate_set = 0;
    if (call_target(SEL_RATE, &rate_bpp, &rate_set)) return 1;
    double psnr_db = 0.0;
    int psnr_set = 0;
    if (call_target(SEL_PSNR, &psnr_db, &psnr_set)) return 1;
    /* the RGB-domain PSNR target: packed RGB24 on the device stream calls alone -- refused before any file is made */
    double prgb_db = 0.0;
    int prgb_set = 0;
    if (call_target(SEL_PSNR_RGB, &prgb_db, &prgb_set)) return 1;
    if (prgb_set && channels != 3) {
        printf("psnr_rgb= applies to encode_rgb on one device (encode): a grey encode takes psnr=\n");
        return 1;
    }
    if (prgb_set && host_eg_on()) {
        printf("psnr_rgb= needs the device stream calls (DCT3D_CODEC_HOST_EG=1 is set)\n");
        return 1;
    }
    /* the SSIM target: psnr='s place and passes, the SSIM probe's numbers */
    double ssim_target = 0.0;
    int ssim_set = 0;
    if (call_target(SEL_SSIM, &ssim_target, &ssim_set)) return 1;
    /* the RGB SSIM target: psnr_rgb='s place, passes and conditions, the RGB and luma SSIM probe's numbers */
    double srgb_target = 0.0;
    int srgb_set = 0;
    if (call_target(SEL_SSIM_RGB, &srgb_target, &srgb_set)) return 1;
    if (srgb_set && channels != 3) {
        printf("ssim_rgb= applies to encode_rgb on one device (encode): a grey encode takes ssim=\n");
        return 1;
    }
    if (srgb_set && host_eg_on()) {
        printf("ssim_rgb= needs the device stream calls (DCT3D_CODEC_HOST_EG=1 is set)\n");
        return 1;
    }
    int ycc;
    if (call_colour("encode", channels, ssim_set ? SEL_SSIM : psnr_set ? SEL_PSNR : 0, &ycc)) return 1;
    int c420;
    if (call_chroma("encode", channels, ycc, &c420)) return 1;
    /* a quality map: written by the first pass of a rate or PSNR target, else read -- before any file is made */
    const char *qmap_path = NULL, *qmap3_path = NULL;
    int cq = 0;
    if (call_qmap3("encode", channels, rate_set || prgb_set || srgb_set, psnr_set || ssim_set, ycc, &qmap3_path, &cq)) return 1;
    if (call_qmap(&qmap_path)) return 1;
    const int qw = qmap3_path ? 3 : 1; /* the map's entries per stack */
    if (qmap3_path) qmap_path = qmap3_path;
    uint8_t *qmap = NULL;
    int32_t qmap_tabs[RATE_LADDER_N * QUANT_MAX_STEPS];
    if (qmap_path) {
        const int ns = (frames + depth - 1) / depth;
        qmap = (uint8_t *)calloc((size_t)ns * qw, 1);
        if (!qmap) {
            printf("Out of memory\n");
            return 1;
        }
        if (!rate_set && !psnr_set && !ssim_set && !prgb_set && !srgb_set && (qw == 3 ? read_qmap3(qmap_path, ns, qmap) : read_qmap(qmap_path, ns, qmap))) {
            free(qmap);
            return 1;
        }
        ladder_tables(depth, qmap_tabs);
    }
    if (batch <= 0) batch = default_batch();
    FILE *in = fopen(inName, "rb");
    if (!in) {
        printf("Cannot open input file %s\n", inName);
        free(qmap);
        return 1;
    }
    const int wp = (width + 7) / 8 * 8, hp = (height + 7) / 8 * 8;
    /* chroma=420: channels 1 and 2 are the subsampled planes, (width + 1) / 2 x (height + 1) / 2, padded likewise */
    const int wpc = c420 ? ((width + 1) / 2 + 7) / 8 * 8 : wp, hpc = c420 ? ((height + 1) / 2 + 7) / 8 * 8 : hp;
    /* DCT3D_CODEC_HOST_EG=1: Exp-Golomb on the host from the quantised ints (A/B and tests); default: the
     * device Exp-Golomb stage, the same bytes */
    const int host_eg = host_eg_on();
    /* DCT3D_CODEC_DEFLATE_THREADS=N (N > 1): parallel deflate in every channel's coder -- the same inflated
     * payload, a different .bin; default: one zlib stream, the reference encoder's bytes */
    const char *dt = getenv("DCT3D_CODEC_DEFLATE_THREADS");
    const int deflate_threads = dt ? atoi(dt) : 1;
    FILE *out[3] = {NULL, NULL, NULL};
    dct3d_entropy_enc *ent[3] = {NULL, NULL, NULL};
    dct3d_ctx *ctx = NULL;
    uint8_t *fr = NULL;
    int32_t *q = NULL;
    unsigned char *eg = NULL;
    size_t eg_cap = 0;
    int status = 0;
    const double t_start = now_s();
    double t_ctx = 0, t_read = 0, t_dev = 0, t_fetch = 0, t_ent = 0;
    for (int ch = 0; ch < channels && !status; ch++)
        if (!(out[ch] = open_stream(outName, channels, ch, "wb"))) status = 1;
    if (!status) {
        int rc;
        STAGE(t_ctx, rc = dct3d_ctx_create(platformIndex > 0 ? platformIndex - 1 : 0, 8, 8, depth, &ctx));
        if (rc) {
            printf("Error creating the device context: %s\n", dct3d_strerror(rc));
            status = 1;
        } else {
            STAGE(t_ctx, status = ctx_apply_quant(ctx, depth) || ctx_apply_colour(ctx, ycc) || ctx_apply_chroma(ctx, c420));
        }
    }
    const size_t stack_bytes = (size_t)channels * width * height * depth; /* of the frames as they are */
    const size_t stack_px = (size_t)wp * hp * depth;                       /* values of a padded plane's stack */
    const int n_stacks = (frames + depth - 1) / depth;
    if (!status) {
        fr = (uint8_t *)malloc(stack_bytes * batch);
        if (host_eg) q = (int32_t *)malloc(channels * stack_px * batch * sizeof(int32_t));
        eg_cap = stack_px * batch / 2 + 64;
        if (!host_eg) eg = (unsigned char *)malloc(eg_cap);
        int ok = fr && (host_eg ? q != NULL : eg != NULL);
        for (int ch = 0; ch < channels; ch++)
            if (!(ent[ch] = dct3d_entropy_enc_create(ch ? wpc : wp, ch ? hpc : hp, depth, out[ch])) ||
                dct3d_entropy_enc_set_threads(ent[ch], deflate_threads, 0))
                ok = 0;
        if (!ok) {
            printf("Out of memory\n");
            status = 1;
        }
    }
    /* a rate target: the first pass picks the quality, the second encodes as q=<n> does */
    if (!status && (rate_set || psnr_set || ssim_set))
        STAGE(t_dev, status = rate_first_pass(ctx, in, fr, width, height, frames, depth, batch, channels,
                                              ssim_set ? ssim_target : psnr_set ? psnr_db : rate_bpp,
                                              ssim_set ? METRIC_SSIM : psnr_set ? METRIC_PSNR : METRIC_RATE, qmap, qw == 3 ? cq : -1));
    if (!status && (prgb_set || srgb_set))
        STAGE(t_dev, status = psnr_rgb_first_pass(ctx, in, fr, width, height, frames, depth, batch, srgb_set ? srgb_target : prgb_db,
                                                  srgb_set ? METRIC_SSIM : METRIC_PSNR, ycc, qmap, qw, qw == 3 ? cq : 0));
    if (!status && qmap && (rate_set || psnr_set || ssim_set || prgb_set || srgb_set))
        status = qw == 3 ? write_qmap3(qmap_path, n_stacks, qmap) : write_qmap(qmap_path, n_stacks, qmap);
    for (int s0 = 0; !status && s0 < n_stacks; s0 += batch) {
        const int nb = (n_stacks - s0) < batch ? (n_stacks - s0) : batch;
        size_t got = 0, r;
        const size_t want = stack_bytes * nb;
        STAGE(t_read, while (got < want && (r = fread(fr + got, 1, want - got, in)) > 0) got += r);
        if (got < want) memset(fr + got, 0, want - got); /* a short last stack is zero-filled */
        const int last = s0 + nb == n_stacks;
        int rc;
        if (host_eg) { /* quantised ints over PCIe, Exp-Golomb on the host */
            STAGE(t_dev, rc = dct3d_encode_frames(ctx, fr, width, height, channels, nb, q));
            if (rc) {
                printf("Error running the 3D DCT: %s\n", dct3d_strerror(rc));
                status = 1;
                break;
            }
            const double t_e0 = now_s();
            for (int s = 0; s < nb && !status; s++)
                for (int ch = 0; ch < channels; ch++) /* block (s, ch) of the [stack][channel] layout */
                    if (dct3d_entropy_enc_push(ent[ch], q + stack_px * ((size_t)channels * s + ch),
                                               s0 + s == n_stacks - 1)) {
                        printf("Error in the entropy coder\n");
                        status = 1;
                        break;
                    }
            t_ent += now_s() - t_e0;
        } else { /* each channel's stream built on the device, continuing its file's partial byte */
            uint8_t cb[3] = {0, 0, 0};
            int cbits[3] = {0, 0, 0};
            uint64_t tb[3] = {0, 0, 0};
            for (int ch = 0; ch < channels; ch++) dct3d_entropy_enc_carry(ent[ch], &cb[ch], &cbits[ch]);
            if (qw == 3) /* stack s0 + s of channel ch under the ladder's table qmap[3 (s0 + s) + ch] */
                STAGE(t_dev, rc = dct3d_encode_eg_frames_vqc(ctx, fr, width, height, channels, nb, qmap_tabs, RATE_LADDER_N,
                                                             qmap + 3 * (size_t)s0, cb, cbits, tb));
            else if (qmap) /* stack s0 + s under the ladder's table qmap[s0 + s] */
                STAGE(t_dev, rc = dct3d_encode_eg_frames_vq(ctx, fr, width, height, channels, nb, qmap_tabs, RATE_LADDER_N,
                                                            qmap + s0, cb, cbits, tb));
            else
                STAGE(t_dev, rc = dct3d_encode_eg_frames(ctx, fr, width, height, channels, nb, cb, cbits, tb));
            for (int ch = 0; ch < channels && !rc; ch++) {
                const size_t nbytes = (size_t)((tb[ch] + 7) / 8);
                if (nbytes > eg_cap) {
                    free(eg);
                    eg_cap = nbytes + nbytes / 4;
                    eg = (unsigned char *)malloc(eg_cap);
                    if (!eg) {
                        rc = DCT3D_ENOMEM;
                        break;
                    }
                }
                STAGE(t_fetch, rc = dct3d_eg_fetch_channel(ctx, ch, eg, nbytes));
                if (rc) break;
                int perr;
                STAGE(t_ent, perr = dct3d_entropy_enc_push_stream(ent[ch], eg, tb[ch], last));
                if (perr) {
                    printf("Error in the entropy coder\n");
                    status = 1;
                    break;
                }
            }
            if (rc) {
                printf("Error running the 3D DCT: %s\n", dct3d_strerror(rc));
                status = 1;
                break;
            }
        }
        for (int s = 0; !status && s < nb; s++) printf("Frames processed: %d\n", (s0 + s + 1) * depth);
    }
    for (int ch = 0; ch < channels; ch++) {
        if (ent[ch]) STAGE(t_ent, dct3d_entropy_enc_destroy(ent[ch])); /* the last deflate output and its write */
        if (out[ch] && (fflush(out[ch]) || fclose(out[ch]))) status = 1;
    }
    free(fr);
    free(q);
    free(eg);
    free(qmap);
    char qtext[QUANT_MAX_STEPS * 5 + 8];
    quant_json(ctx, depth, qtext, sizeof(qtext));
    if (ctx) dct3d_ctx_destroy(ctx);
    fclose(in);
    if (timing_on())
        fprintf(stderr,
                "{\"stage_s\": {\"ctx_create\": %.6f, \"read\": %.6f, \"device\": %.6f, \"eg_fetch\": %.6f, "
                "\"%s\": %.6f}, \"total_s\": %.6f, \"host_eg\": %d, \"deflate_threads\": %d, \"channels\": %d, "
                "\"quant\": %s}\n",
                t_ctx, t_read, t_dev, t_fetch, host_eg ? "eg_deflate_write" : "deflate_write", t_ent, now_s() - t_start,
                host_eg, deflate_threads, channels, qtext);
    if (!status) printf("Encoding process completed\n");
    return status;
}

static int decode_any(const char *inName, const char *outName, int width, int height, int frames, int platformIndex,
                      int depth, int batch, int channels) {
    if (reject_targets("decode")) return 1;
    int ycc;
    if (call_colour("decode", channels, 0, &ycc)) return 1;
    int c420;
    if (call_chroma("decode", channels, ycc, &c420)) return 1;
    const char *qmap_path = NULL, *qmap3_path = NULL;
    int cq = 0;
    if (call_qmap3("decode", channels, 0, 0, ycc, &qmap3_path, &cq)) return 1; /* (cq=: an encode's, refused) */
    if (call_qmap(&qmap_path)) return 1;
    const int qw = qmap3_path ? 3 : 1; /* the map's entries per stack */
    if (qmap3_path) qmap_path = qmap3_path;
    uint8_t *qmap = NULL;
    int32_t qmap_tabs[RATE_LADDER_N * QUANT_MAX_STEPS];
    if (qmap_path) { /* read before any file is made */
        const int ns = (frames + depth - 1) / depth;
        qmap = (uint8_t *)calloc((size_t)ns * qw, 1);
        if (!qmap) {
            printf("Out of memory\n");
            return 1;
        }
        if (qw == 3 ? read_qmap3(qmap_path, ns, qmap) : read_qmap(qmap_path, ns, qmap)) {
            free(qmap);
            return 1;
        }
        ladder_tables(depth, qmap_tabs);
    }
    if (batch <= 0) batch = default_batch();
    const int wp = (width + 7) / 8 * 8, hp = (height + 7) / 8 * 8;
    /* chroma=420: channels 1 and 2 are the subsampled planes, (width + 1) / 2 x (height + 1) / 2, padded likewise */
    const int wpc = c420 ? ((width + 1) / 2 + 7) / 8 * 8 : wp, hpc = c420 ? ((height + 1) / 2 + 7) / 8 * 8 : hp;
    const int host_eg = host_eg_on();
    FILE *in[3] = {NULL, NULL, NULL};
    dct3d_entropy_dec *ent[3] = {NULL, NULL, NULL};
    FILE *out = NULL;
    dct3d_ctx *ctx = NULL;
    uint8_t *fr = NULL;
    int32_t *q = NULL;
    int status = 0;
    const double t_start = now_s();
    double t_ctx = 0, t_inf = 0, t_dev = 0, t_write = 0;
    for (int ch = 0; ch < channels && !status; ch++)
        if (!(in[ch] = open_stream(inName, channels, ch, "rb"))) status = 1;
    if (!status && !(out = fopen(outName, "wb"))) {
        printf("Cannot open output file %s\n", outName);
        status = 1;
    }
    if (!status) {
        int rc;
        STAGE(t_ctx, rc = dct3d_ctx_create(platformIndex > 0 ? platformIndex - 1 : 0, 8, 8, depth, &ctx));
        if (rc) {
            printf("Error creating the device context: %s\n", dct3d_strerror(rc));
            status = 1;
        } else {
            STAGE(t_ctx, status = ctx_apply_quant(ctx, depth) || ctx_apply_colour(ctx, ycc) || ctx_apply_chroma(ctx, c420));
        }
    }
    const size_t stack_bytes = (size_t)channels * width * height * depth;
    const size_t stack_px = (size_t)wp * hp * depth;
    const int n_stacks = (frames + depth - 1) / depth;
    double bits_per_value = 4.0; /* window estimate for the first batch; then the measured rate */
    if (!status) {
        fr = (uint8_t *)malloc(stack_bytes * batch);
        if (host_eg) q = (int32_t *)malloc(channels * stack_px * batch * sizeof(int32_t));
        int ok = fr && (!host_eg || q);
        for (int ch = 0; ch < channels; ch++)
            if (!(ent[ch] = dct3d_entropy_dec_create(ch ? wpc : wp, ch ? hpc : hp, depth, in[ch], NULL, 0))) ok = 0;
        if (!ok) {
            printf("Out of memory\n");
            status = 1;
        }
    }
    for (int s0 = 0; !status && s0 < n_stacks; s0 += batch) {
        const int nb = (n_stacks - s0) < batch ? (n_stacks - s0) : batch;
        int rc = 0;
        if (host_eg) {
            const double t_i0 = now_s();
            for (int s = 0; s < nb && !status; s++)
                for (int ch = 0; ch < channels; ch++)
                    if (dct3d_entropy_dec_pull(ent[ch], q + stack_px * ((size_t)channels * s + ch))) {
                        printf("Truncated or corrupt input stream\n");
                        status = 1;
                        break;
                    }
            t_inf += now_s() - t_i0;
            if (status) break;
            STAGE(t_dev, rc = dct3d_decode_frames(ctx, q, width, height, channels, nb, fr));
        } else { /* the device parses each channel's inflated stream, refilled and run again on ENODATA */
            const double values = (double)stack_px * nb;
            size_t need = (size_t)(values * bits_per_value / 8 * 1.25) + 65536;
            for (;;) {
                const unsigned char *p[3] = {NULL, NULL, NULL};
                uint64_t len[3] = {0, 0, 0}, eb[3] = {0, 0, 0};
                int bit[3] = {0, 0, 0};
                int werr = 0;
                for (int ch = 0; ch < channels && !werr; ch++) {
                    size_t l = 0;
                    STAGE(t_inf, werr = dct3d_entropy_dec_window(ent[ch], need, &p[ch], &l, &bit[ch]));
                    len[ch] = l;
                }
                if (werr) {
                    rc = DCT3D_EINVAL;
                    break;
                }
                if (qw == 3)
                    STAGE(t_dev, rc = dct3d_decode_eg_frames_vqc(ctx, p, len, bit, width, height, channels, nb, qmap_tabs,
                                                                 RATE_LADDER_N, qmap + 3 * (size_t)s0, fr, eb));
                else if (qmap)
                    STAGE(t_dev, rc = dct3d_decode_eg_frames_vq(ctx, p, len, bit, width, height, channels, nb, qmap_tabs,
                                                                RATE_LADDER_N, qmap + s0, fr, eb));
                else
                    STAGE(t_dev, rc = dct3d_decode_eg_frames(ctx, p, len, bit, width, height, channels, nb, fr, eb));
                if (rc == DCT3D_ENODATA) { /* some channel needs more of its stream than estimated? */
                    int more = 0;
                    for (int ch = 0; ch < channels; ch++)
                        if (!dct3d_entropy_dec_eof(ent[ch]) && len[ch] >= need) more = 1;
                    if (more) {
                        need *= 2;
                        continue;
                    }
                }
                if (!rc) {
                    bits_per_value = 0.0;
                    for (int ch = 0; ch < channels; ch++) {
                        dct3d_entropy_dec_consume(ent[ch], eb[ch]);
                        const double b = (double)(eb[ch] - (uint64_t)bit[ch]) / (ch ? (double)wpc * hpc * depth * nb : values);
                        if (b > bits_per_value) bits_per_value = b;
                    }
                }
                break;
            }
            if (rc == DCT3D_ENODATA || rc == DCT3D_EINVAL) {
                printf("Truncated or corrupt input stream\n");
                status = 1;
                break;
            }
        }
        if (rc) {
            printf("Error running the inverse 3D DCT: %s\n", dct3d_strerror(rc));
            status = 1;
            break;
        }
        size_t wrote;
        STAGE(t_write, wrote = fwrite(fr, 1, stack_bytes * nb, out));
        if (wrote != stack_bytes * nb) {
            printf("Error writing the output file\n");
            status = 1;
            break;
        }
        printf("Frames processed: %d\n", (s0 + nb) * depth);
    }
    for (int ch = 0; ch < channels; ch++) {
        if (ent[ch]) dct3d_entropy_dec_destroy(ent[ch]);
        if (in[ch]) fclose(in[ch]);
    }
    free(fr);
    free(q);
    free(qmap);
    char qtext[QUANT_MAX_STEPS * 5 + 8];
    quant_json(ctx, depth, qtext, sizeof(qtext));
    if (ctx) dct3d_ctx_destroy(ctx);
    STAGE(t_write, if (out && (fflush(out) || fclose(out))) status = 1);
    if (timing_on())
        fprintf(stderr,
                "{\"stage_s\": {\"ctx_create\": %.6f, \"%s\": %.6f, \"device\": %.6f, \"write\": %.6f}, "
                "\"total_s\": %.6f, \"host_eg\": %d, \"channels\": %d, \"quant\": %s}\n",
                t_ctx, host_eg ? "read_inflate_eg" : "read_inflate", t_inf, t_dev, t_write, now_s() - t_start, host_eg,
                channels, qtext);
    if (!status) printf("Decoding process completed\n");
    return status;
}

int encode(char *inName, char *outName, int width, int height, int frames, int platformIndex) {
    return encode_ex(inName, outName, width, height, frames, platformIndex, DCT_BLOCK_DEPTH, 0);
}

int decode(char *inName, char *outName, int width, int height, int frames, int platformIndex) {
    return decode_ex(inName, outName, width, height, frames, platformIndex, DCT_BLOCK_DEPTH, 0);
}
