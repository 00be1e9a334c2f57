"""Shared by test_cert_common.py (CPU), test_gpu_certificates.py, test_gpu_probe_certificates.py,
test_gpu_distortion_rgb_certificates.py and test_gpu_ssim_certificates.py (GPU): what the
host emulations of the kernels' arithmetic predict for the counts dct3d_get_stats reports -- which coefficients the
fp32 encode certificate leaves open, which lanes the decode certificate flags, how the 8x8x8 second certificate splits
the open ones, what the rate and distortion probes count under several tables, what the RGB-domain distortion
probe counts per plane of the colour transform and coded table, and what the two SSIM probes count, across their
ranges of stacks and under the planes mode's compacted tables.

The emulations are tests/native/emulate_encode.cpp and emulate_decode_quant.cpp, built here as test_emulation.py
builds them (g++ -O2 -ffp-contract=off -fno-fast-math, into a temporary directory).  With contraction off on both
sides and the same butterfly source, IEEE fp32 / fp64 arithmetic is deterministic: the device's counts must equal
these predictions exactly.  No GPU is needed by anything in this module."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

import quant_common as qc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "3ddctvideoencoding_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native")
GXX = ["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-std=c++17", "-shared", "-fPIC", "-I", CSRC]


@functools.lru_cache(maxsize=None)
def _libs():
    """(emulate_encode's library, emulate_decode_quant's), built once per process"""
    d = tempfile.mkdtemp(prefix="cert_emu_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    out = []
    for src in ("emulate_encode.cpp", "emulate_decode_quant.cpp"):
        so = os.path.join(d, src.replace(".cpp", ".so"))
        subprocess.run(GXX + [os.path.join(NATIVE, src), "-o", so], check=True)
        out.append(C.CDLL(so))
    out[0].emulate_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    out[1].emulate_decode_quant_w.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return tuple(out)


def steps_of(steps, depth):
    """the table as int32 (None: the reference's max(1, 5 s))"""
    return qc.pkg().quant_table(5, depth) if steps is None else np.ascontiguousarray(steps, np.int32)


@functools.lru_cache(maxsize=None)
def _plan_of(depth, key):
    return qc.pkg().plan_query(8, 8, depth, None if key is None else np.frombuffer(key, np.int32))


def plan_of(depth, steps):
    """plan_query for the table (None: the reference's), made once per table: the planner's analysis takes ~0.4 s"""
    return _plan_of(depth, None if steps is None else np.ascontiguousarray(steps, np.int32).tobytes())


def raster_of(frames, depth):
    """frames [F, h, w] or packed [F, h, w, 3], any h, w -> the edge-padded raster the calls are defined on, RGB as
    the planar-stacked raster of dct3d.h (per stack: its R, G, B frames): [channels F, Hp, Wp]"""
    pad = qc.pkg().pad_frames(np.asarray(frames, np.uint8))
    return np.ascontiguousarray(pad if pad.ndim == 3 else qc.planar(pad, depth))


def encode_emulate(frames, depth, steps=None, channels=1, shift=0):
    """the emulated fp32 kernel on the cubes of raster_of(frames): (q, open, cubes).  open[cube][kz][ky][kx] is the
    fp32 certificate's verdict, DC cleared; cubes in the calls' output order [stack][channel][by][bx].
    shift (the sensitivity check only): the threshold tables G, E read at s + shift, clamped to the table."""
    import oracle
    assert channels == (3 if np.asarray(frames).ndim == 4 else 1)
    p = plan_of(depth, steps)
    cubes = np.ascontiguousarray(oracle.to_cubes(raster_of(frames, depth), 8, 8, depth), np.uint8)
    n = cubes.shape[0]
    q = np.empty(cubes.size, np.int32)
    fl = np.empty(cubes.size, np.uint8)
    val = np.empty(cubes.size, np.float32)
    A = np.empty(n, np.float32)
    ns = qc.n_steps(depth)
    idx = np.minimum(np.arange(32) + shift, ns - 1)
    t = [np.ascontiguousarray(p["enc_rstep"], np.float32), np.ascontiguousarray(p["enc_G"][idx], np.float32),
         np.ascontiguousarray(p["enc_E"][idx], np.float32)]
    _libs()[0].emulate_encode(cubes.ctypes.data, n, depth, t[0].ctypes.data, t[1].ctypes.data, t[2].ctypes.data,
                              p["coef_dc"], q.ctypes.data, fl.ctypes.data, val.ctypes.data, A.ctypes.data)
    shape = (n, depth, 8, 8)
    op = fl.reshape(shape).astype(bool)
    op[:, 0, 0, 0] = False
    q = q.reshape(shape)
    # the DC as the kernels make it: JavaRound(S * coef_dc / step[0]) in fp64 (the emulation has step[0] = 1 in its text)
    dc = (cubes.reshape(n, -1).sum(axis=1, dtype=np.int64).astype(np.float64) * p["coef_dc"]) / float(steps_of(steps, depth)[0])
    q[:, 0, 0, 0] = (np.floor(dc) + (dc - np.floor(dc) >= 0.5)).astype(np.int32)
    return q, op, cubes


def encode_open(frames, depth, steps=None, channels=1):
    """bool [cube][kz][ky][kx]: the coefficients the fp32 certificate leaves open (the DC never is)"""
    return encode_emulate(frames, depth, steps, channels)[1]


def dct_cubes(frames, depth):
    """the oracle's fp64 DCT (Java semantics) of raster_of(frames), as cubes"""
    import oracle
    return oracle.to_cubes(qc.plan(depth).dct(raster_of(frames, depth)), 8, 8, depth)


TIE, BAND = 1e-12, 1e-9  # split_8x8x8: 0.5 - d <= TIE is a tie; (TIE, BAND) must be empty


def split_8x8x8(frames, open_mask, steps, dct=None):
    """With the second certificate on (8x8x8), which open coefficients stay open for the Java fold and which the
    fp64 recheck settles, from the oracle's fp64 DCT alone (not the kernel's fp64 path): with
    d = |c / step - rint(c / step)|, an open coefficient with 0.5 - d < 1e-9 is an exact tie (fold); every other
    one is rechecked.  Precondition (asserted): no open coefficient in the ambiguous band 1e-12 < 0.5 - d < 1e-9.
    Returns (fold mask, rechecked mask); the predicted (n_flagged, n_rechecked) are their sums."""
    d = dct_cubes(frames, 8) if dct is None else dct
    v = d / qc.step_cube(steps_of(steps, 8), 8)
    gap = 0.5 - np.abs(v - np.rint(v))
    amb = open_mask & (gap > TIE) & (gap < BAND)
    assert not amb.any(), f"{int(amb.sum())} open coefficients in the ambiguous band: another seed"
    fold = open_mask & (gap < BAND)
    return fold, open_mask & ~fold


# ---- decode ---------------------------------------------------------------------------------------------------------

L1_FACTOR = 1.0 + 2.0 ** -19  # decode_tile: the fp32 cube sum times (1.0f + 0x1p-19f)
L1_SLACK = 2.0 ** -20         # the fp64 lane sums, the conversion and the five fp32 roundings: < 6 * 2^-24


def _mi(l1f, G, E):
    """decode_tile: m = fmin((double)l1_f * dec_G + dec_E, 0.5); mi = (uint32)ceil(fma(m, 2^32, 0.5)) + 1
    (m * 2^32 is exact, so the fma is the plain sum's one rounding)"""
    m = np.minimum(l1f * G + E, 0.5)
    return np.ceil(m * 4294967296.0 + 0.5).astype(np.int64) + 1


def decode_emulate(q, depth, steps, extra_margin):
    """The decode certificate (decode_tile, dct3d_decode_dev.h) on int32 cubes q [n, depth, 8, 8]: the mask of
    flagged lanes [n, lanes per cube] (the predicted n_flagged is 32 x its sum), and the bytes [n, depth, 8, 8] the kernel
    packs from w's high word (the low half as a signed 16-bit value, saturated to [0, 255]).

    Ownership (layout C, dec_b_to_c / dec_store_tile): a lane owns 32 pixels of one row y of its cube over every
    depth z -- 8x8x8: 16 lanes per cube, lane (y, h) the pixels x = 4h .. 4h + 3 of z = 0 .. 7 (mask index 2 y + h);
    8x8x4: 8 lanes per cube, lane y the pixels x = 0 .. 7 of z = 0 .. 3.  A lane is flagged when the low word of
    w = v + kFixMagic of one of its pixels is < mi or > 2^32 - 1 - mi, or when its cube's L1 reaches dec_l1_max
    (then all lanes of the cube).  DCT3D_OPT_DEC_MARGIN is added to dec_E on the host, in fp64.

    The kernel's fp32 reduction of L1 is not restated: l1_f lies within L1 (1 + 2^-19) (1 +- 2^-20).  Asserted
    preconditions: both ends give the same mi for every cube, and no cube's L1 lies that close to dec_l1_max."""
    lanes, byte = decode_emulate_margins(q, depth, steps, (extra_margin,))
    return lanes[0], byte


def decode_emulate_margins(q, depth, steps, margins):
    """decode_emulate for several margins from one run of the emulated transform (w does not depend on the margin):
    ([the mask of flagged lanes per margin], the bytes); the preconditions are asserted for every margin"""
    p = plan_of(depth, steps)
    st = steps_of(steps, depth)
    q = np.ascontiguousarray(q, np.int32).reshape(-1, depth, 8, 8)
    n = q.shape[0]
    w = np.empty(q.size, np.float64)
    l1e = np.empty(n, np.float64)
    _libs()[1].emulate_decode_quant_w(q.ctypes.data, n, depth, st.ctypes.data, w.ctypes.data, l1e.ctypes.data)
    l1 = qc.l1(q, st, depth).astype(np.float64)  # exact integers (< 2^49)
    assert np.array_equal(l1, l1e)
    lo_l, hi_l = l1 * L1_FACTOR * (1.0 - L1_SLACK), l1 * L1_FACTOR * (1.0 + L1_SLACK)
    lmax = float(p["dec_l1_max"])
    assert not ((lo_l < lmax) & (hi_l >= lmax)).any(), "a cube's L1 within 2^-20 of dec_l1_max"
    lo = (w.view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64).reshape(n, depth, 8, 8)
    # a lane's verdict needs only the least and the greatest low word of its 32 pixels (the kernel's lo_min, lo_max)
    if depth == 8:
        lo = lo.reshape(n, 8, 8, 2, 4)
        lo_min, lo_max = lo.min(axis=(1, 4)).reshape(n, 16), lo.max(axis=(1, 4)).reshape(n, 16)  # [y][h]
    else:
        lo_min, lo_max = lo.min(axis=(1, 3)), lo.max(axis=(1, 3))  # [y]
    out = []
    for extra_margin in margins:
        E = p["dec_E"] + float(extra_margin)
        mi = _mi(lo_l, p["dec_G"], E)
        assert np.array_equal(mi, _mi(hi_l, p["dec_G"], E)), "mi depends on the fp32 L1 reduction: another seed"
        lanes = (lo_min < mi[:, None]) | (lo_max > 0xFFFFFFFF - mi[:, None])
        out.append(lanes | (lo_l >= lmax)[:, None])
    h16 = ((w.view(np.uint64) >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64)
    byte = np.clip(np.where(h16 >= 32768, h16 - 65536, h16), 0, 255).astype(np.uint8).reshape(n, depth, 8, 8)
    return out, byte


def decode_open(q, depth, steps, extra_margin):
    """the mask of flagged lanes alone (decode_emulate)"""
    return decode_emulate(q, depth, steps, extra_margin)[0]


def lane_pixels(lanes, depth):
    """flagged lanes [n, lanes per cube] -> the mask of the pixels they own [n, depth, 8, 8]"""
    n = lanes.shape[0]
    if depth == 8:
        return np.broadcast_to(lanes.reshape(n, 1, 8, 2, 1), (n, 8, 8, 2, 4)).reshape(n, 8, 8, 8)
    return np.broadcast_to(lanes.reshape(n, 1, 8, 1), (n, 4, 8, 8))


def guard_cubes(depth, name):
    """the L1 guard case: four cubes, two just under and two just over dec_l1_max (quant_common.guard_cube, 2^-10 either
    side: far outside decode_emulate's 2^-20 band): (q [4, depth, 8, 8], the mask of the cubes over the guard)"""
    T = steps_of(table(name, depth), depth)
    rng = np.random.default_rng(4100 + depth)
    lmax = qc.l1_max(depth)
    q = np.stack([qc.guard_cube(T, depth, rng, lmax * (1 + s * 2.0 ** -10)) for s in (-1, 1, 1, -1)])
    over = qc.l1(q, T, depth) >= lmax
    assert over.tolist() == [False, True, True, False]
    return q, over


# ---- bands ----------------------------------------------------------------------------------------------------------

def band_counts(mask, stacks, channels, nby):
    """per-unit mask [cube, ...] in the calls' order [stack][channel][by][bx] -> int64 [nby]: the count of each
    horizontal band of one block row (over every stack and channel)"""
    m = mask.reshape(stacks, channels, nby, -1)
    return m.sum(axis=(0, 1, 3)).astype(np.int64)


def band_frames(frames, by):
    """block row by of the frames, cropped (the last band of a ragged height is shorter: the calls pad it)"""
    return np.ascontiguousarray(frames[:, 8 * by:8 * by + 8])


def band_cubes(q, stacks, channels, nby, by):
    """the cubes of block row by, in the order the calls take for the cropped frames"""
    s = q.shape[1:]
    return np.ascontiguousarray(q.reshape((stacks, channels, nby, -1) + s)[:, :, by]).reshape((-1,) + s)


def is_rich(counts):
    """a case can see a shifted threshold: >= 20 open units in all, a non-zero count in >= a quarter of its bands"""
    counts = np.asarray(counts)
    return int(counts.sum()) >= 20 and 4 * int((counts > 0).sum()) >= counts.size


def first_difference(pred, got, mask, stacks, channels, nby):
    """for a failing case: the first band whose counts differ and the emulation's open positions in it
    (pred, got: one row of counts per band)"""
    pred, got = np.asarray(pred).reshape(nby, -1), np.asarray(got).reshape(nby, -1)
    by = int(np.nonzero((pred != got).any(axis=1))[0][0])
    m = mask.reshape((stacks, channels, nby, -1) + mask.shape[1:])[:, :, by]
    return f"band {by}: predicted {pred[by].tolist()}, device {got[by].tolist()}; the emulation's open units " \
           f"(stack, channel, bx, ...) {np.argwhere(m)[:16].tolist()}"


# ---- the inputs and cases of test_gpu_certificates.py (checked on the CPU by test_cert_common.py) ----------------------

TABLES = ("ref", "q1", "q12", "seeded")  # ref: no table set (None)


def table(name, depth):
    """ref: None; qt<n>: quant_table(n); every other name: quant_common.tables"""
    if name == "ref":
        return None
    return qc.pkg().quant_table(int(name[2:]), depth) if name.startswith("qt") else qc.tables(depth)[name]


@functools.lru_cache(maxsize=None)
def content(kind, depth, channels, w, h, stacks, seed=0):
    """seeded frames [stacks depth, h, w] (channels = 3: [.., 3]), never modified.  uniform: pkg.synthetic's noise,
    the content whose coefficients come near rounding ties (~1e-4 of them open under the reference table);
    ties4: test_encode_8x8x4_inwave_replay's exact ties in half of the cubes; ramp_crop: block rows 58-65 and block
    columns 186-193 of the 1080p ramp stack at frame 200, around cube 14829's exact tie
    (test_encode_8x8x8_exact_tie_takes_java_fold)"""
    p = qc.pkg()
    f = stacks * depth

    def plane(i):
        if kind == "uniform":
            return p.synthetic.frames(w, h, f, seed=0xC357 + 131 * i + seed, frame0=7 + 3 * i + seed, kind="uniform")
        if kind == "ties4":
            z, y, x = np.meshgrid(np.arange(f), np.arange(h), np.arange(w), indexing="ij")
            v = 100 + ((x // 8 + y // 8) % 3) * 2 + 8 * ((z % 4 == 0) & ((y % 8 == 0) | ((y % 8 == 1) & (x % 8 < 2))))
            v += 16 * ((z % 4 == 3) & (x % 8 == 4) & (y % 8 < 5) & ((x // 8) % 2 == 1))
            return v.astype(np.uint8)
        assert kind == "ramp_crop" and (w, h, f) == (64, 64, 8)
        return p.synthetic.frames(1920, 1080, 8, kind="ramp", frame0=200)[:, 58 * 8:66 * 8, 186 * 8:194 * 8]

    fr = plane(0) if channels == 1 else np.stack([plane(0), plane(1), plane(2)], axis=-1)
    fr = np.ascontiguousarray(fr, np.uint8)
    fr.setflags(write=False)
    return fr


class Case:
    """one input of a call family; rich: the tables under which the case must be rich (is_rich, asserted)"""

    def __init__(self, kind, depth, channels, w, h, stacks, rich=(), seed=0):
        self.kind, self.depth, self.channels, self.w, self.h, self.stacks = kind, depth, channels, w, h, stacks
        self.rich, self.seed = tuple(rich), seed
        self.nby = (h + 7) // 8
        self.id = f"{kind}-{w}x{h}x{stacks}-{'rgb' if channels == 3 else 'grey'}-d{depth}"

    def frames(self):
        return content(self.kind, self.depth, self.channels, self.w, self.h, self.stacks, self.seed)

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=4)
def _case_dct(kind, depth, channels, w, h, stacks, seed):
    d = dct_cubes(content(kind, depth, channels, w, h, stacks, seed), depth)
    d.setflags(write=False)
    return d


def case_dct(c):
    """the oracle's fp64 DCT of the case's padded (planar) raster as cubes, shared by the case's tables"""
    return _case_dct(c.kind, c.depth, c.channels, c.w, c.h, c.stacks, c.seed)


@functools.lru_cache(maxsize=8)
def _case_open(kind, depth, channels, w, h, stacks, seed, name, shift):
    q, op, _ = encode_emulate(content(kind, depth, channels, w, h, stacks, seed), depth, table(name, depth), channels, shift)
    q.setflags(write=False)
    op.setflags(write=False)
    return q, op


def case_open(c, name, shift=0):
    """(the emulation's q, its open mask) of the case under table `name`"""
    return _case_open(c.kind, c.depth, c.channels, c.w, c.h, c.stacks, c.seed, name, shift)


def case_q_ref(c, name):
    """the reference's coefficients (quant_common.py): the oracle's Java DCT, then the numpy quantiser"""
    return qc.pkg().quantize_ref(case_dct(c), steps_of(table(name, c.depth), c.depth))


# the encode cases, by call family (test_gpu_certificates.py a-f); RICH8 / RICH4: the tables under which the 8x8x8 /
# 8x8x4 cases of these sizes are rich (q12, and at 8x8x4 the seeded table, leave too few coefficients open)
RICH8, RICH4 = ("ref", "q1", "seeded"), ("ref", "q1")
STACKS8 = [Case("uniform", 8, 1, 200, 72, 4, RICH8), Case("uniform", 8, 1, 24, 16, 5), Case("uniform", 8, 1, 8, 8, 1),
           Case("ramp_crop", 8, 1, 64, 64, 1), Case("uniform", 8, 1, 1920, 1080, 1, TABLES)]
STACKS4 = [Case("uniform", 4, 1, 200, 72, 4, RICH4), Case("uniform", 4, 1, 24, 16, 5), Case("uniform", 4, 1, 8, 8, 1),
           Case("ties4", 4, 1, 200, 72, 3), Case("uniform", 4, 1, 1920, 1080, 1, TABLES)]
RGB = [Case("uniform", 8, 3, 200, 72, 2, RICH8), Case("uniform", 8, 3, 24, 16, 5), Case("uniform", 8, 3, 8, 8, 1),
       Case("uniform", 4, 3, 200, 72, 2, RICH4), Case("uniform", 4, 3, 24, 16, 5), Case("uniform", 4, 3, 8, 8, 1)]
EDGE = [Case("uniform", d, ch, w, h, st, rich)
        for d in (8, 4) for ch in (1, 3)
        for (w, h, st, rich) in ((1366, 24, 2 if ch == 1 else 1, RICH8 if d == 8 else RICH4), (13, 11, 1, ()), (1, 1, 1, ()))]
# the stream encode kernels that count: grey at sizes that are no multiple of 8, RGB at any size
EG = [Case("uniform", d, 1, w, h, st, rich)
      for d in (8, 4) for (w, h, st, rich) in ((1366, 24, 2, RICH8 if d == 8 else RICH4), (13, 11, 1, ()))] + \
     [Case("uniform", d, 3, w, h, st, rich)
      for d in (8, 4) for (w, h, st, rich) in ((200, 72, 2, RICH8 if d == 8 else RICH4), (24, 16, 5, ()), (13, 11, 1, ()))]

# DCT3D_OPT_DEC_MARGIN values.  A lane owns 32 pixels and is flagged when one of them has its fractional part within
# m of an integer: for fractional parts spread evenly a share 1 - (1 - 2 m)^32 of the lanes, so m = (1 - (1 - p)^(1/32)) / 2
# gives 1.57e-4, 1.64e-3 and 1.07e-2 for p = 1 %, 10 % and 50 %.  Rounded, on the decode of uniform noise's coefficients
# (200 x 72, cert_common.decode_open on the CPU) they flag 0.7-1.1 %, 9.0-10.0 % and 50.1-51.1 % of the lanes.
MARGINS = (1.5e-4, 1.6e-3, 1.1e-2)
DEC = [Case("uniform", d, ch, w, h, 1) for d in (8, 4) for ch in (1, 3) for (w, h) in ((200, 72), (1366, 24), (13, 11))]


# ---- the rate and distortion probes (test_gpu_probe_certificates.py) ------------------------------------------------
# rate_kernel and distortion_kernel certify in loops of their own, from table rows that probe-only host code builds
# (dct3d_rate_frames_dev, dct3d_distortion_frames_dev), and add what they fold into the same counter.

# 11 tables: two launches of up to 8.  (quant_table(24), not 20: under 20 one lane of the 200 x 72 x 4 case at 8x8x8
# decodes within the margin-0 certificate's reach, and the distortion count at margin 0 is to be the encode term alone.)
PROBE_TABLES = TABLES + ("all255", "ones", "q2", "qt3", "qt7", "qt24", "qt64")
PROBE_SETS = dict({n: (n,) for n in PROBE_TABLES}, four=TABLES, eleven=PROBE_TABLES)


def with_total(v):
    """per-band counts -> the same with the whole raster's count last"""
    v = np.asarray(v, np.int64)
    return np.concatenate([v, [v.sum()]])


@functools.lru_cache(maxsize=None)
def probe_open_counts(c, name, shift=0):
    """int64 [nby + 1]: the coefficients the emulation leaves open under table `name`, per band and in all (kept
    per case and table: the sets share them)"""
    v = with_total(band_counts(case_open(c, name, shift)[1], c.stacks, c.channels, c.nby))
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def probe_decode_lanes(c, name, margins):
    """the lanes the decode certificate flags on the reference's coefficients under table `name`, one mask
    [cube, lanes per cube] per margin (a tuple of margins; kept per case and table).  The probe's decode tile runs
    with EDGE = 0 on whole padded cubes of the integers the encode side staged (the reference's, once the folds have
    settled the open ones); its constants do not depend on the table, DCT3D_OPT_DEC_MARGIN is added as
    decode_emulate adds it."""
    return tuple(decode_emulate_margins(case_q_ref(c, name), c.depth, table(name, c.depth), margins)[0])


def probe_lane_counts(c, name, margin):
    """int64 [nby + 1]: the lanes probe_decode_lanes flags at `margin`, per band and in all (the margins of
    PROBE_MARGINS from one run of the emulation)"""
    ms = PROBE_MARGINS if margin in PROBE_MARGINS else (margin,)
    return with_total(band_counts(probe_decode_lanes(c, name, ms)[ms.index(margin)], c.stacks, c.channels, c.nby))


def rate_probe_counts(c, names, shift=0):
    """rate_kernel's n_flagged for the tables `names` in one call, int64 [nby + 1] (per band, then the whole raster):
    a coefficient open under k of the tables is folded once and counted k times -- the sum over the tables of the
    open coefficients; the DC is never counted; every geometry counts"""
    return sum(probe_open_counts(c, n, shift) for n in names)


def distortion_probe_counts(c, names, margin, shift=0):
    """distortion_kernel's n_flagged, int64 [nby + 1]: per table the open coefficients (every one takes the fold, at
    8x8x8 too: the probe has no second certificate) plus 32 per lane the decode tile replays"""
    return sum(probe_open_counts(c, n, shift) + 32 * probe_lane_counts(c, n, margin) for n in names)


PROBE_MARGINS = (0.0,) + MARGINS[:2]
# grey at multiples of 8 (which the stream encode does not count, and the probes do), the ragged and RGB lists of
# EG, 1 x 1, and the grey 1080p stack of each depth.  The sets a case runs under: probe_sets.
PROBE_CASES = STACKS8[:3] + STACKS4[:3] + EG + [c for c in EDGE if (c.w, c.h) == (1, 1)] + [STACKS8[4], STACKS4[4]]


def probe_sets(c):
    """the table sets of a probe case: each of TABLES alone, the four in one call, the 11 in one call.  At 1080p the
    seven other tables run alone as well, before the 11: a table's reference there costs about a second of host
    time, and each case then pays for one table's"""
    if (c.w, c.h) == (1920, 1080):
        return TABLES + ("four",) + PROBE_TABLES[4:] + ("eleven",)
    return TABLES + ("four", "eleven")


def probe_rich(c, set_name):
    """whether the case claims richness under the set: a set is rich when one of its tables is"""
    return any(n in c.rich for n in PROBE_SETS[set_name])


# distortion_sum_kernel (and rate_sum_kernel): 256 threads, thread i sums the run's values i, i + 256, ...; a butterfly
# over 1, 2, 4, 8, 16, 32 lanes inside each wave of 64, the uint64 partial sent as two 32-bit halves.
SUM_BLOCK = 256


def sum_partials(values, lanes):
    """int64 [256 / lanes]: the partial sums each aligned group of `lanes` lanes holds after the butterfly's steps
    below `lanes`, for one run of per-cube values"""
    v = np.asarray(values, np.int64).reshape(-1)
    pad = np.zeros(-(-v.size // SUM_BLOCK) * SUM_BLOCK, np.int64)
    pad[:v.size] = v
    return pad.reshape(-1, SUM_BLOCK).sum(axis=0).reshape(-1, lanes).sum(axis=1)


# the case whose partial sums pass 2^32 while shuffles remain: uniform noise under all255, one grey stack; every
# 8-lane partial of every wave >= 2^32 (asserted from the reference's cube sums by the test).  The sizes: the
# smallest multiple-of-8 height at widths 2560 / 3840 that meets the condition, measured on the reference:
# a cube costs 1,981,851 (8x8x8) / 990,577 (8x8x4) on average, the least 8-lane partial is 1.0019 / 1.0035 x 2^32
# (one block row less: 0.9982 / 0.9998).
BIG_SUM = {8: (2560, 1744), 4: (3840, 2328)}


# ---- the RGB-domain distortion probe in the colour modes (test_gpu_distortion_rgb_certificates.py) ---------------------
# distortion_plane_kernel (dct3d_distortion_rgb.hip) is a copy of distortion_kernel's certificate loop with a forward
# transform, a reload source, a table loop and a fold count of its own; probe_rgb_ycc_dev decides on the host which
# (table, plane) pairs are coded at all.  The prediction treats every plane of the colour transform as a grey clip.

COLOUR_MODES = ("planes", "ycc", "c420")


class ColourCase:
    """packed RGB24 content("uniform", depth, 3, w, h, stacks) in one colour mode of a context.  band: the frame rows
    of one band -- one block row (8), in c420 mode 16: two Y block rows over one chroma block row, so that a crop at a
    band's start has the whole frame's Y and chroma cubes.  rich: the shape claims richness under q1."""

    def __init__(self, mode, depth, w, h, stacks, rich=False):
        assert mode in COLOUR_MODES
        self.mode, self.depth, self.w, self.h, self.stacks, self.rich = mode, depth, w, h, stacks, rich
        self.band = 16 if mode == "c420" else 8
        self.nb = (h + self.band - 1) // self.band
        self.rgb = Case("uniform", depth, 3, w, h, stacks)  # planes mode: the plane probe's case
        self.id = f"{mode}-{w}x{h}x{stacks}-d{depth}"

    def frames(self):
        return self.rgb.frames()

    def __repr__(self):
        return self.id


@functools.lru_cache(maxsize=None)
def colour_planes(c):
    """the case's three planes as grey clips [F, ph, pw]: R, G, B | rgb_to_ycbcr's | rgb_to_ycbcr420's (the chroma
    at chroma_size); never modified"""
    p, fr = qc.pkg(), c.frames()
    if c.mode == "c420":
        pl = list(p.rgb_to_ycbcr420(fr))
    else:
        t = fr if c.mode == "planes" else p.rgb_to_ycbcr(fr)
        pl = [t[..., k] for k in range(3)]
    pl = tuple(np.ascontiguousarray(a, np.uint8) for a in pl)
    if c.mode == "c420":
        assert pl[1].shape[1:] == qc.pkg().chroma_size(c.w, c.h)[::-1]
    for a in pl:
        a.setflags(write=False)
    return pl


def colour_plane_cubes(c, k):
    """(padded cubes per stack, block rows) of plane k"""
    _, ph, pw = colour_planes(c)[k].shape
    return ((pw + 7) // 8) * ((ph + 7) // 8), (ph + 7) // 8


@functools.lru_cache(maxsize=None)
def colour_plane_dct(c, k):
    d = dct_cubes(colour_planes(c)[k], c.depth)
    d.setflags(write=False)
    return d


def colour_plane_q_ref(c, k, name):
    """the reference's coefficients of plane k under table `name`"""
    return qc.pkg().quantize_ref(colour_plane_dct(c, k), steps_of(table(name, c.depth), c.depth))


@functools.lru_cache(maxsize=None)
def colour_plane_open(c, k, name, shift=0):
    """(the emulation's q, its open mask) of plane k under table `name`, kept per (case, plane, table)"""
    q, op, _ = encode_emulate(colour_planes(c)[k], c.depth, table(name, c.depth), 1, shift)
    q.setflags(write=False)
    op.setflags(write=False)
    return q, op


@functools.lru_cache(maxsize=None)
def colour_plane_lanes(c, k, name):
    """the lanes the decode certificate flags on the reference's coefficients of plane k, one mask per margin of
    PROBE_MARGINS (probe_decode_lanes on the plane; the preconditions are asserted inside)"""
    return tuple(decode_emulate_margins(colour_plane_q_ref(c, k, name), c.depth, table(name, c.depth), PROBE_MARGINS)[0])


def _plane_bands(c, k, mask):
    """per-unit mask of plane k [cube, ...] -> int64 [nb + 1]: the count per band of the frames, then the plane's.
    Block row r of the plane lies in the frame rows from 8 r (chroma of c420: 16 r) on."""
    _, nby = colour_plane_cubes(c, k)
    rows = mask.reshape(c.stacks, nby, -1).sum(axis=(0, 2)).astype(np.int64)
    sub = 2 if (c.mode == "c420" and k > 0) else 1
    v = np.zeros(c.nb, np.int64)
    np.add.at(v, (8 * sub * np.arange(nby)) // c.band, rows)
    return with_total(v)


@functools.lru_cache(maxsize=None)
def colour_open_counts(c, k, name, shift=0):
    v = _plane_bands(c, k, colour_plane_open(c, k, name, shift)[1])
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def colour_lane_counts(c, k, name, margin):
    v = _plane_bands(c, k, colour_plane_lanes(c, k, name)[PROBE_MARGINS.index(margin)])
    v.setflags(write=False)
    return v


def coded_tables(n_tables, cand, all_pairs):
    """probe_rgb_ycc_dev's lists L[k]: the tables plane k is coded under, in the order of their first use -- the
    distinct tables some candidate names for plane k; every table when the planes' errors or the bits are asked for
    (all_pairs) or no candidates are given (candidate i = (i, i, i))"""
    if cand is None or all_pairs:
        return [list(range(n_tables)) for _ in range(3)]
    L = [[], [], []]
    for cd in cand:
        for k in range(3):
            if cd[k] not in L[k]:
                L[k].append(int(cd[k]))
    return L


def colour_distortion_counts(c, names, cand, margin, all_pairs=False, shift=0):
    """n_flagged of one distortion_rgb_frames[_dev] call, int64 [nb + 1] (per band, then the whole raster).
    ycc, c420: the sum over the planes k and the tables of L[k] of (the open coefficients + 32 x the lanes the decode
    tile replays): a table several candidates name is coded and counted once, a table no candidate names for the plane
    not at all.  planes: the plane probe under every table, whatever the candidates say."""
    if c.mode == "planes":
        return distortion_probe_counts(c.rgb, names, margin, shift)
    L = coded_tables(len(names), cand, all_pairs)
    return sum(colour_open_counts(c, k, names[t], shift) + 32 * colour_lane_counts(c, k, names[t], margin)
               for k in range(3) for t in L[k])


def colour_rate_counts(c, names, shift=0):
    """n_flagged of rate_frames_dev in ycc or c420 mode: the rate probe's rule, every table on every plane"""
    return sum(colour_open_counts(c, k, n, shift) for k in range(3) for n in names)


def colour_units(c, names, cand, all_pairs=False, rows=None):
    """n_units of the call on the frames cropped to `rows` frame rows (None: whole): per plane |L[k]| x padded cubes
    x 64 depth x stacks (planes mode: every table)"""
    p = qc.pkg()
    h = c.h if rows is None else rows
    sizes = [(c.w, h)] + [p.chroma_size(c.w, h) if c.mode == "c420" else (c.w, h)] * 2
    L = coded_tables(len(names), None if c.mode == "planes" else cand, all_pairs)
    return sum(len(L[k]) * ((pw + 7) // 8) * ((ph + 7) // 8) for k, (pw, ph) in enumerate(sizes)) * 64 * c.depth * c.stacks


def colour_rich(c, names, cand, all_pairs=False):
    """a (case, table set) is rich: is_rich of the summed per-band open counts of the coded pairs, and every plane
    has >= 12 open coefficients under some table of the set"""
    L = coded_tables(len(names), cand, all_pairs)
    total = sum(colour_open_counts(c, k, names[t]) for k in range(3) for t in L[k])
    return is_rich(total[:-1]) and all(max(int(colour_open_counts(c, k, n)[-1]) for n in names) >= 12 for k in range(3))


# (w, h, stacks, rich under q1); planes mode runs at two of them: its kernel is the plane probe's
COLOUR_SHAPES = ((200, 72, 2, True), (208, 80, 2, True), (244, 54, 2, True), (1366, 24, 1, True), (24, 16, 5, False),
                 (13, 11, 1, False), (1, 1, 1, False))
COLOUR_PROBE_CASES = [ColourCase(m, d, w, h, st, rich) for d in (8, 4) for m in ("ycc", "c420")
                      for (w, h, st, rich) in COLOUR_SHAPES] + \
                     [ColourCase("planes", d, w, h, st) for d in (8, 4) for (w, h, st) in ((200, 72, 2), (13, 11, 1))]
# name -> (table names, candidates or None, ask for the planes' errors).  subsets: each plane a different proper
# subset of the four, table 3 coded for no plane; planes4: the same with every pair coded
_SUBSETS = ((0, 1, 2), (2, 1, 0), (0, 1, 0))
COLOUR_SETS = {
    "q1": (("q1",), ((0, 0, 0),), False),
    "ref": (("ref",), ((0, 0, 0),), False),
    "subsets": (TABLES, _SUBSETS, False),
    "planes4": (TABLES, _SUBSETS, True),
    "eleven": (PROBE_TABLES, None, False),
    "repeat": (("q1", "q12", "seeded"), ((0, 1, 2), (2, 2, 0), (0, 1, 2)), False),
}
COLOUR_RICH_SETS = ("q1", "planes4", "eleven")  # the sets that code q1 on all three planes


# ---- the SSIM probes (test_gpu_ssim_certificates.py) -------------------------------------------------------------------
# dct3d_ssim_frames[_dev] launches distortion_kernel's SSIM = 1 instantiations from ssim_dev, the only plane probe that
# walks the stacks in ranges (range x channel x batch of 8 tables into one counter slot, window and sum launches
# between the counting ones); dct3d_ssim_rgb_frames[_dev] reuses rgb_ycc_dev with a second budget on the ranges and,
# in planes mode, codes only the tables some candidate names.

# the probe cases without the two 1080p ones (the host-call tests are the 1080p coverage: their count is held to the
# distortion probe's, which test_gpu_probe_certificates.py holds to the emulation at 1080p)
SSIM_PROBE_CASES = [c for c in PROBE_CASES if (c.w, c.h) != (1920, 1080)]
SSIM_PROBE_SETS = ("q1", "four", "eleven")
# 32 tables in one call: the 11 cycled.  A prediction sums per name, so a name counts with its multiplicity and 11
# emulations pay for the 32
RANGE_NAMES = tuple(PROBE_TABLES[i % len(PROBE_TABLES)] for i in range(32))
RANGE_CAND = tuple((i, (i + 5) % 32, (i + 11) % 32) for i in range(32))  # every plane codes all 32


def ssim_probe_counts(c, names, margin, shift=0):
    """the plane SSIM probe's n_flagged, int64 [nby + 1]: "statistics are the distortion probe's"  -- the
    SSIM arm certifies and replays exactly as distortion_kernel does, whatever the ranges, want_sse and want_bits"""
    return distortion_probe_counts(c, names, margin, shift)


def ssim_probe_units(c, names, rows=None):
    """the plane SSIM probe's n_units on the frames cropped to `rows` rows (None: whole): tables x padded samples"""
    wp, hp = qc.pkg().padded_size(c.w, c.h if rows is None else rows)
    return len(names) * wp * hp * c.channels * c.depth * c.stacks


def ssim_record_bytes(depth, w, h, n, planes=1):
    """the block records of one stack (and, plane probe, one channel): D nbx nby (8 n + 4) bytes per record plane over
    the 4 x 4 block grid (dct3d.h)"""
    return depth * ((w + 3) // 4) * ((h + 3) // 4) * (8 * n + 4) * planes


def ssim_ranges(depth, w, h, stacks, n, planes=1, plane_bytes=0):
    """the stacks of each range of a call: as many as fit DCT3D_SSIM_BLOCK_BUDGET (and, colour modes, the decoded
    planes DCT3D_RGB_PLANE_BUDGET: plane_bytes of one stack), one at least"""
    p = qc.pkg()
    per = max(1, min(stacks, p.DCT3D_SSIM_BLOCK_BUDGET // ssim_record_bytes(depth, w, h, n, planes)))
    if plane_bytes:
        per = max(1, min(per, p.DCT3D_RGB_PLANE_BUDGET // plane_bytes))
    return [min(per, stacks - s0) for s0 in range(0, stacks, per)]


def _range_stacks(depth):
    """one stack more than the block budget holds at 256 x 176 under 32 tables: 3 at 8x8x8, 6 at 8x8x4"""
    return qc.pkg().DCT3D_SSIM_BLOCK_BUDGET // ssim_record_bytes(depth, 256, 176, 32) + 1


# the range cases, whole raster only (a band of 8 rows has no second range)
SSIM_RANGE_CASES = [Case("uniform", d, ch, 256, 176, _range_stacks(d)) for d in (8, 4) for ch in (1, 3)]
# test_gpu_ssim_rgb.py::test_stack_ranges' shapes: the records of 32 candidates split the stacks 3 + 2 (2 + 2 + 1 with
# the luma's record plane), the decoded planes alone would not
SSIM_RGB_RANGE_CASES = [ColourCase(m, d, 128, h, 5) for (d, h) in ((8, 88), (4, 176)) for m in ("ycc", "c420")]


def stack_counts(mask, stacks):
    """per-unit mask [cube, ...] in the calls' order (the stack outermost) -> int64 [stacks]"""
    return mask.reshape(stacks, -1).sum(axis=1).astype(np.int64)


def ssim_range_stack_counts(c, names, margin):
    """the plane probe's prediction of a range case per stack, int64 [stacks] (its sum: ssim_probe_counts' last)"""
    ms = PROBE_MARGINS
    return sum(stack_counts(case_open(c, n)[1], c.stacks) +
               32 * stack_counts(probe_decode_lanes(c, n, ms)[ms.index(margin)], c.stacks) for n in names)


def colour_range_stack_counts(c, names, cand, margin):
    """colour_distortion_counts of a colour range case per stack, int64 [stacks]"""
    L = coded_tables(len(names), cand, False)
    i = PROBE_MARGINS.index(margin)
    return sum(stack_counts(colour_plane_open(c, k, names[t])[1], c.stacks) +
               32 * stack_counts(colour_plane_lanes(c, k, names[t])[i], c.stacks) for k in range(3) for t in L[k])


def ssim_rgb_planes_tables(n_tables, cand, want_bits):
    """rgb_planes_dev's compaction under the SSIM probe: the tables the plane probe is run with -- the distinct tables
    any candidate names for any plane, in the order of first use over the flattened candidate list; every table when
    the bits are asked for or no candidates are given (candidate i = (i, i, i)).  (The RGB distortion probe's planes
    mode does not compact: colour_distortion_counts' planes arm.)"""
    if cand is None or want_bits:
        return list(range(n_tables))
    used = []
    for cd in cand:
        for t in cd:
            if int(t) not in used:
                used.append(int(t))
    return used


def ssim_rgb_counts(c, names, cand, margin, want_bits=False, shift=0):
    """n_flagged of one ssim_rgb_frames[_dev] call, int64 [nb + 1].  ycc, c420: colour_distortion_counts with every
    pair coded when the bits are asked for -- neither the luma nor want_sse changes L[k].  planes: the plane probe
    under the compacted tables, every coded table on all three planes."""
    if c.mode == "planes":
        used = ssim_rgb_planes_tables(len(names), cand, want_bits)
        return distortion_probe_counts(c.rgb, [names[t] for t in used], margin, shift)
    return colour_distortion_counts(c, names, cand, margin, want_bits, shift)


def ssim_rgb_units(c, names, cand, want_bits=False, rows=None):
    """n_units of the call on the frames cropped to `rows` frame rows (None: whole).  planes: the coded tables x the
    padded raster of the three planes"""
    if c.mode == "planes":
        used = ssim_rgb_planes_tables(len(names), cand, want_bits)
        return ssim_probe_units(c.rgb, used, rows)
    return colour_units(c, names, cand, want_bits, rows)
