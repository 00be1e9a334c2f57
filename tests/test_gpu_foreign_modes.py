"""GPU: streams no encoder of 8-bit frames writes through every stream decode built after test_gpu_eg_fused.py and
test_gpu_quant_foreign.py: the per-stack and per-(stack, channel) table calls (_vq, _vqc; QT = 2), the YCbCr calls
(CT = 1) and the 4:2:0 calls (decode_eg_y420_kernel), beside the grey and RGB24 base calls (QT = 0, 1).

The inputs are foreign_common.py's, and every condition on them is asserted on the CPU by test_foreign_common.py:

  boundary   groups of 2,048 values whose window spans are WIN - 1, WIN, WIN + 1 and around them (the LDS window
             against the global-memory parse, in each of the three copies of the window logic); every group holds
             long cubes (|q| >= 2^18: replayed whole from the stream) and ONE dense ordinary cube, in range and under
             the guard, whose bytes come straight from the one-pass parse of that window
  guard      one cube in two consecutive stacks, under the L1 guard with one stack's table and over it with the other's

The reference is foreign_common.ref_modes: quant_common.ref_decode_frames (dequantize_ref, the oracle's Java fold, the
byte clamp, the crop) per stack and channel under that entry's table, then the mode's numpy composition.  The streams
are test_gpu_vq.ref_streams of the cubes.  Every comparison is np.array_equal; every device output lies between 4 KiB
canary bands and is written twice over different fills (test_gpu_vq.decode_dev, test_gpu_vqc.decode_dev); every call is
made in the host form and in the device form."""
import contextlib
import functools

import numpy as np
import pytest

import foreign_common as fc
import quant_common as qc
import test_gpu_vq as vq
import test_gpu_vqc as vqc
from conftest import ctx_option

pytestmark = pytest.mark.gpu

BAND = vq.BAND
STACKS = 2
SIZES = {"aligned": (64, 48), "ragged": (61, 45)}  # 48 cubes a stack; 4:2:0: 12 chroma cubes a stack at both
START = (3, 0, 5)
KINDS = ("ref", "set", "vq")  # QT = 0, 1, 2


def _own_contexts(pkg):
    """(get, close): contexts made on first use, the table, the options and the chroma mode reset on each get"""
    made = {}

    def get(depth):
        if depth not in made:
            try:
                made[depth] = pkg.Context(0, 8, 8, depth)
            except Exception as e:
                pytest.fail(f"HIP context for 8x8x{depth} could not be created: {e}")
        ctx = made[depth]
        ctx.set_stream(None)
        ctx.set_quant(None)
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
        for opt in (pkg.DCT3D_OPT_QUANT_FORCE_TABLE, pkg.DCT3D_OPT_EG_TWO_STEP, pkg.DCT3D_OPT_DEC_MARGIN,
                    pkg.DCT3D_OPT_EG_DEC_GROUPS, pkg.DCT3D_OPT_EG_FORCE_RETRY, pkg.DCT3D_OPT_EG_NO_RESOLVE,
                    pkg.DCT3D_OPT_COLOUR):
            ctx.set_option(opt, 0)
        return ctx

    def close():
        for c in made.values():
            c.close()

    return get, close


@pytest.fixture(scope="module")
def fctx(pkg):
    """contexts of this module's own for the calls under test"""
    get, close = _own_contexts(pkg)
    yield get
    close()


@pytest.fixture(scope="module")
def chain_ctx(pkg):
    """contexts of their own for the chains of single-stack base calls, whose quantiser the chain sets stack by stack
    (as test_gpu_vq.py's chain_ctx)"""
    get, close = _own_contexts(pkg)
    yield get
    close()


@contextlib.contextmanager
def _mode(ctx, pkg, mode):
    if mode != "planes":
        ctx.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR)
    if mode == "c420":
        ctx.set_chroma(pkg.DCT3D_CHROMA_420)
    try:
        yield ctx
    finally:
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
        ctx.set_option(pkg.DCT3D_OPT_COLOUR, 0)


def _stats(ctx):
    st = ctx.stats()
    return st["n_units"], st["n_flagged"]


def _tables(depth, kind, stacks=STACKS):
    """(palette, map [stacks, 3]) of a table kind: ref -- the reference table, set -- the seeded table through
    set_quant, vq -- foreign_common.guard_palette cycling with the stack (three equal columns), vqc -- m[s, k] =
    (s + k) % 3"""
    s, k = np.arange(stacks)[:, None], np.arange(3)[None, :]
    if kind in ("ref", "set"):
        T = qc.pkg().quant_table(5, depth) if kind == "ref" else qc.tables(depth)["seeded"]
        return np.asarray(T, np.int32)[None], np.zeros((stacks, 3), np.uint8)
    m = (s + 0 * k) % 3 if kind == "vq" else (s + k) % 3
    return fc.guard_palette(depth), np.ascontiguousarray(m, np.uint8)


def decode_both(ctx, pkg, streams, sb, w, h, stacks, kind, pal, m, mode="planes"):
    """the host form and the device form of the call of `kind` under the colour mode: [(frames, end bits, (n_units,
    n_flagged))]; the device form's bands are intact"""
    ch = len(streams)
    by, sb = [b for b, _ in streams], list(sb)
    col = np.ascontiguousarray(m[:, 0])
    res = []
    if kind == "set":
        ctx.set_quant(pal[0])
    elif kind == "ref":
        assert np.array_equal(ctx.quant(), pal[0])
    try:
        with _mode(ctx, pkg, mode):
            if kind == "vq":
                out, eb = ctx.decode_eg_frames_vq(by, w, h, stacks, pal, col, sb)
            elif kind == "vqc":
                out, eb = ctx.decode_eg_frames_vqc(by, w, h, stacks, pal, m, sb)
            else:
                out, eb = ctx.decode_eg_frames(by, w, h, stacks, sb)
            res.append((out, eb, _stats(ctx)))
            if kind == "vqc":
                out, eb, ok = vqc.decode_dev(ctx, streams, sb, w, h, stacks, pal, m)
            else:
                out, eb, ok = vq.decode_dev(ctx, streams, sb, w, h, ch, stacks, pal if kind == "vq" else None,
                                            col if kind == "vq" else None, vq=kind == "vq")
            assert ok, "the device form wrote outside its output"
            res.append((out, eb, _stats(ctx)))
    finally:
        ctx.set_quant(None)
    return res


def _check(res, ref, ends, min_flagged, what=""):
    for form, (out, eb, (_, flagged)) in zip(("host", "device"), res):
        assert eb == ends, (what, form, eb, ends)
        assert np.array_equal(out, ref), f"{what} {form} form: {(out != ref).sum()} bytes differ"
        assert flagged >= min_flagged, (what, form, flagged, min_flagged)


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ---- (a) the window boundary, grey ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _grey_case(depth, use, size, kind):
    """(streams, reference frames, the long cubes' pixels) of the boundary stream `use` as 2 stacks of SIZES[size]"""
    w, h = SIZES[size]
    q, ordinary, sb = fc.boundary_use(depth, use)
    q = q.reshape(STACKS, 1, -1, depth, 8, 8)
    pal, m = _tables(depth, kind)
    ref = fc.ref_modes(q, w, h, STACKS, depth, pal, m[:, :1], "planes")
    _freeze(ref)
    return fc.streams_of(q, depth, [sb]), ref, 64 * depth * int((~ordinary).sum())


@pytest.mark.parametrize("use", ["grey0", "grey5"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", ["aligned", "ragged"])
@pytest.mark.parametrize("depth", [8, 4])
def test_window_boundary_grey(pkg, fctx, depth, size, kind, use):
    """decode_eg_kernel's open_window at EDGE = 0 and 1 and QT = 0, 1, 2, from start bits 0 and 5"""
    w, h = SIZES[size]
    streams, ref, long_px = _grey_case(depth, use, size, kind)
    pal, m = _tables(depth, kind)
    sb = fc.BOUNDARY_USES[use][1]
    ctx = fctx(depth)
    _check(decode_both(ctx, pkg, streams, [sb], w, h, STACKS, kind, pal, m), ref, [streams[0][1]], long_px)


@pytest.mark.parametrize("groups", [1, 2, 4, 8])
@pytest.mark.parametrize("use", ["grey0", "grey5"])
@pytest.mark.parametrize("depth", [8, 4])
def test_window_boundary_groups_per_wave(pkg, fctx, depth, use, groups):
    """the aligned QT = 0 stream call (decode_eg, decode_eg_dev), on which DCT3D_OPT_EG_DEC_GROUPS acts: a wave's
    successive rounds are groups g and g + 4, whose windows fit and do not fit in all four combinations, the second
    one's look-ahead words in flight during the first one's transform"""
    import torch
    w, h = SIZES["aligned"]
    streams, ref, long_px = _grey_case(depth, use, "aligned", "ref")
    (data, end), sb = streams[0], fc.BOUNDARY_USES[use][1]
    ctx = fctx(depth)
    pad = np.zeros((len(data) + 3) // 4 * 4 + 4, np.uint8)
    pad[:len(data)] = np.frombuffer(data, np.uint8)
    d_s = torch.from_numpy(pad).cuda()
    with ctx_option(ctx, pkg.DCT3D_OPT_EG_DEC_GROUPS, groups):
        out, eb = ctx.decode_eg(data, w, h, STACKS, sb)
        assert eb == end and np.array_equal(out, ref), f"host form: {(out != ref).sum()} bytes differ"
        assert ctx.stats()["n_flagged"] >= long_px
        outs = []
        for fill in (0xA5, 0x5A):
            buf, mid = qc.banded(torch, ref.size, fill, BAND)
            eb = ctx.decode_eg_dev(d_s, len(data), sb, w, h, STACKS, mid)
            ctx.synchronize()
            got, intact = qc.bands_intact(buf, ref.size, fill, BAND)
            assert intact and eb == end
            outs.append(got.reshape(ref.shape))
        assert np.array_equal(outs[0], ref) and np.array_equal(outs[1], ref)
        assert ctx.stats()["n_flagged"] >= long_px


# ---- (b) the window boundary, RGB kernel ------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rgb_q(depth, k):
    """q [stack][channel][cube]: the boundary content on channel k, ordinary and sparse long on the other two"""
    n = fc.BOUNDARY_CUBES
    others = iter([fc.ordinary_stream_cubes(depth, n, 301 + depth + k), fc.long_cubes(depth, n, 401 + depth + k)])
    chans = [fc.boundary_use(depth, f"ch{k}")[0] if c == k else next(others) for c in range(3)]
    q = np.ascontiguousarray(np.stack([c.reshape(STACKS, -1, depth, 8, 8) for c in chans], axis=1))
    _freeze(q)
    return q


@functools.lru_cache(maxsize=None)
def _rgb_case(depth, k, size, kind):
    """(streams, reference in planes mode, the boundary channel's long pixels)"""
    w, h = SIZES[size]
    q = _rgb_q(depth, k)
    pal, m = _tables(depth, kind)
    ref = fc.ref_modes(q, w, h, STACKS, depth, pal, m, "planes")
    _freeze(ref)
    ordinary = fc.boundary_use(depth, f"ch{k}")[1]
    return fc.streams_of(q, depth, START), ref, 64 * depth * int((~ordinary).sum())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", ["aligned", "ragged"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("depth", [8, 4])
def test_window_boundary_rgb(pkg, fctx, depth, k, size, kind):
    """the channel loop of decode_eg_rgb_kernel at CT = 0 and 1, EDGE = 0 and 1, QT = 0, 1, 2; under the colour
    transform additionally test_gpu_ycc.py's identity against mode off"""
    w, h = SIZES[size]
    streams, ref, long_px = _rgb_case(depth, k, size, kind)
    pal, m = _tables(depth, kind)
    ends = [t for _, t in streams]
    ctx = fctx(depth)
    off = decode_both(ctx, pkg, streams, START, w, h, STACKS, kind, pal, m, "planes")
    _check(off, ref, ends, long_px, "planes")
    on = decode_both(ctx, pkg, streams, START, w, h, STACKS, kind, pal, m, "ycc")
    _check(on, pkg.ycbcr_to_rgb(ref), ends, long_px, "ycc")
    for (o_on, _, st_on), (o_off, _, st_off) in zip(on, off):
        assert np.array_equal(o_on, pkg.ycbcr_to_rgb(o_off)) and st_on == st_off


# ---- (c) the window boundary, y420 kernel -----------------------------------------------------------------------------

C420_SIZES = dict(SIZES, chroma=(128, 96))  # chroma: the boundary stream's 48 cubes a stack are the Cb plane's


@functools.lru_cache(maxsize=None)
def _c420_q(depth, size):
    """per channel [stack][cube]: the boundary content on stream 0 at (w, h), long and limit content on streams 1 and 2 at
    the chroma geometry; size "chroma": long content on stream 0, the boundary content on stream 1, limit on 2"""
    p = qc.pkg()
    w, h = C420_SIZES[size]
    n = [STACKS * (-(-pw // 8)) * (-(-ph // 8)) for pw, ph in [(w, h)] + [p.chroma_size(w, h)] * 2]
    if size == "chroma":
        assert n[1] == fc.BOUNDARY_CUBES
        chans = [fc.long_cubes(depth, n[0], 501 + depth), fc.boundary_use(depth, "ch1")[0], fc.limit_cubes(depth, n[2], 601 + depth)]
    else:
        assert n[0] == fc.BOUNDARY_CUBES
        chans = [fc.boundary_use(depth, "ch0")[0], fc.long_cubes(depth, n[1], 501 + depth), fc.limit_cubes(depth, n[2], 601 + depth)]
    chans = tuple(np.ascontiguousarray(c.reshape(STACKS, -1, depth, 8, 8)) for c in chans)
    _freeze(*chans)
    return chans


@functools.lru_cache(maxsize=None)
def _c420_case(depth, size, kind):
    w, h = C420_SIZES[size]
    q = _c420_q(depth, size)
    pal, m = _tables(depth, kind)
    ref = fc.ref_modes(q, w, h, STACKS, depth, pal, m, "c420")
    _freeze(ref)
    ordinary = fc.boundary_use(depth, "ch1" if size == "chroma" else "ch0")[1]
    return fc.streams_of(q, depth, START), ref, 64 * depth * int((~ordinary).sum())


@pytest.mark.parametrize("size,kind", [(s, k) for s in ("aligned", "ragged") for k in KINDS + ("vqc",)] +
                         [("chroma", "ref"), ("chroma", "vqc")])
@pytest.mark.parametrize("depth", [8, 4])
def test_window_boundary_c420(pkg, fctx, depth, size, kind):
    """decode_eg_y420_kernel's window on stream 0 (multiples of 16, and odd w and h) under every table kind, after
    whole-cube replays in all three streams; size "chroma": the boundary stream is Cb, which the grey decode takes at
    the chroma geometry into the context's planes"""
    w, h = C420_SIZES[size]
    streams, ref, long_px = _c420_case(depth, size, kind)
    pal, m = _tables(depth, kind)
    ctx = fctx(depth)
    _check(decode_both(ctx, pkg, streams, START, w, h, STACKS, kind, pal, m, "c420"), ref, [t for _, t in streams], long_px)


# ---- (d) the sides of the guard under per-stack and per-channel tables -------------------------------------------------

def _channel_sizes(pkg, mode, w, h, channels):
    return [(w, h)] + [pkg.chroma_size(w, h) if mode == "c420" else (w, h)] * (channels - 1)


@functools.lru_cache(maxsize=None)
def _guard_case(depth, w, h, stacks, variant, mode):
    """(per-channel q, streams, the map, reference frames)"""
    p = qc.pkg()
    channels = 1 if variant == "grey_vq" else 3
    pal, gm = fc.guard_palette(depth), fc.guard_map(stacks)
    m = gm if variant == "rgb_vqc" else np.ascontiguousarray(np.repeat(gm[:, :1], 3, axis=1))
    q = []
    for k, (pw, ph) in enumerate(_channel_sizes(p, mode, w, h, channels)):
        cps = (-(-pw // 8)) * (-(-ph // 8))
        q.append(fc.split_guard_cubes(depth, pal, m[:, k], cps, 5, k))
    ref = fc.ref_modes(q, w, h, stacks, depth, pal, m[:, :channels], mode)
    _freeze(ref, m, *q)
    return tuple(q), fc.streams_of(q, depth, START[:channels]), m, ref


_CHAINS = {}


def _grey_chain(ctx, depth, q, stream, sb, w, h, stacks, pal, col):
    """test_gpu_vq.chain_decode of one grey stream under a map column: single-stack base calls, set_quant before each
    (kernels that test_gpu_quant_foreign.py holds to the reference on this kind of input): (end bit, n_flagged,
    n_units), made once per stream.  The chain's frames are held to ref_modes of the channel on its own: the yardstick
    of the counts is right on the very inputs whose counts it vouches for."""
    key = (depth, stream[0], sb, w, h, col.tobytes())
    if key not in _CHAINS:
        out, pos, flagged, units = vq.chain_decode(ctx, [stream], [sb], w, h, 1, stacks, pal, col)
        ref = fc.ref_modes([q], w, h, stacks, depth, pal, col[:, None], "planes")
        assert np.array_equal(out, ref), f"the chain of base calls: {(out != ref).sum()} bytes differ"
        _CHAINS[key] = (pos[0], flagged, units)
    return _CHAINS[key]


GUARD_CASES = [(w, h, st, "grey_vq", "planes") for w, h, st in fc.GUARD_SIZES[:2]] + \
              [(w, h, st, v, md) for w, h, st in fc.GUARD_SIZES for v in ("rgb_vq", "rgb_vqc") for md in ("planes", "ycc", "c420")]


@pytest.mark.parametrize("w,h,stacks,variant,mode", GUARD_CASES)
@pytest.mark.parametrize("depth", [8, 4])
def test_guard_sides_under_per_stack_and_per_channel_tables(pkg, fctx, chain_ctx, depth, w, h, stacks, variant, mode):
    """QT = 2 on foreign values: vq_lane_steps with the table changing inside a wave (8 x 8: with every cube), the
    lane's integer L1 under its own stack's steps, ReloadStreamVq's table of the replayed cube, vq_channel's column.
    Frames equal ref_modes; n_units and n_flagged equal the sums over the channels' grey chains of single-stack base
    calls, as test_gpu_vq.py and test_gpu_vqc.py pin them for an encoder's streams."""
    q, streams, m, ref = _guard_case(depth, w, h, stacks, variant, mode)
    channels = len(q)
    pal = fc.guard_palette(depth)
    ctx = fctx(depth)
    sizes = _channel_sizes(pkg, mode, w, h, channels)
    chains = [_grey_chain(chain_ctx(depth), depth, q[k], streams[k], START[k], sizes[k][0], sizes[k][1], stacks, pal,
                          np.ascontiguousarray(m[:, k])) for k in range(channels)]
    ends = [t for _, t in streams]
    assert [c[0] for c in chains] == ends
    want = (sum(c[2] for c in chains), sum(c[1] for c in chains))
    # a cube over the guard is replayed whole: its pixels at the least are flagged, in every stack where it is over
    over = sum(int((qc.l1(q[k][s], pal[m[s, k]], depth) >= qc.l1_max(depth)).sum()) for k in range(channels) for s in range(stacks))
    assert over >= len(fc.guard_places(stacks, q[0].shape[1])) // 2 and want[1] >= 64 * depth * over
    kind = "vqc" if variant == "rgb_vqc" else "vq"
    if channels == 1:
        res = decode_both(ctx, pkg, streams, START[:1], w, h, stacks, "vq", pal, m, mode)
    else:
        res = decode_both(ctx, pkg, streams, START, w, h, stacks, kind, pal, m, mode)
    _check(res, ref, ends, 0)
    for form, (_, _, st) in zip(("host", "device"), res):
        assert st == want, (form, st, want)


# ---- (e) errors keep their meaning ------------------------------------------------------------------------------------

def _damage(depth, stream, fault, q=None, sb=0):
    """a stream cut ("cut") or with 64 zero bits spliced in ("zeros").  With the channel's cubes q: inside, or in front
    of, the first code of a long cube in the middle of the stream; else at the middle byte."""
    b, total = stream
    if q is None:
        at = 8 * (len(b) // 2)
    else:
        vals = fc.stream_values(q, depth)
        c = next(i for i in range(len(vals) // 2, len(vals)) if abs(int(vals[i, 0])) > qc.Q15)
        width = qc.code_bits(vals)
        at = sb + int(width[:c].sum())
        assert width[c, 0] >= 39
    if fault == "cut":
        nb = (at + 20) // 8 if q is not None else at // 8
        assert q is None or 8 * nb > at + 8, "inside the code's zeros"
        return b[:nb], 0
    bits = np.unpackbits(np.frombuffer(b, np.uint8))
    bits = np.concatenate([bits[:at], np.zeros(64, np.uint8), bits[at:]])
    return np.packbits(bits).tobytes(), 0


def _vqc_dev_error(ctx, pkg, streams, sb, w, h, stacks, pal, m):
    """decode_eg_frames_vqc_dev into a banded buffer, an error expected: the error, the bands intact"""
    import torch
    d_s = vqc._dev_streams(streams)
    n = stacks * ctx.bd * h * w * 3
    buf, mid = qc.banded(torch, n, 0xA5, BAND)
    with pytest.raises(pkg.Dct3dError) as e:
        ctx.decode_eg_frames_vqc_dev(d_s, [len(b) for b, _ in streams], list(sb), w, h, stacks, pal, m, mid)
    ctx.synchronize()
    assert qc.bands_intact(buf, n, 0xA5, BAND)[1], "wrote outside its output"
    return e.value


@pytest.mark.parametrize("bad", ["first", "last", "all"])
@pytest.mark.parametrize("fault", ["cut", "zeros"])
@pytest.mark.parametrize("call", ["ycc_vqc", "c420"])
@pytest.mark.parametrize("depth", [8, 4])
def test_errors_keep_their_meaning(pkg, fctx, depth, call, fault, bad):
    """the boundary stream cut inside a long code is DCT3D_ENODATA, with 64 zero bits spliced in DCT3D_EINVAL: on one
    channel of a YCbCr _vqc call (the boundary channel: first, last, or the middle one with all three streams damaged)
    and in a 4:2:0 call whose stream 0 is the boundary stream (stream 0 damaged, stream 2, or all three).  Host and
    device form; the bands stay intact, the good streams' end bits are reported, and the next call on the same
    context, the good input of (b) or (c), is correct."""
    w, h = SIZES["ragged"]
    ctx = fctx(depth)
    hit = {"first": [0], "last": [2], "all": [0, 1, 2]}[bad]
    if call == "ycc_vqc":
        k = {"first": 0, "last": 2, "all": 1}[bad]
        kind, mode = "vqc", "ycc"
        q = [_rgb_q(depth, k)[:, c] for c in range(3)]
        pal, m = _tables(depth, kind)
        streams = fc.streams_of(q, depth, START)
        ref = pkg.ycbcr_to_rgb(fc.ref_modes(q, w, h, STACKS, depth, pal, m, "planes"))
    else:
        k, kind, mode = 0, "ref", "c420"
        q = _c420_q(depth, "ragged")
        pal, m = _tables(depth, kind)
        streams, ref, _ = _c420_case(depth, "ragged", kind)
    ends = [t for _, t in streams]
    damaged = [_damage(depth, s, fault, q[c] if c == k else None, START[c]) if c in hit else s for c, s in enumerate(streams)]
    code = pkg.DCT3D_ENODATA if fault == "cut" else pkg.DCT3D_EINVAL
    with _mode(ctx, pkg, mode):
        with pytest.raises(pkg.Dct3dError) as e:
            if kind == "vqc":
                ctx.decode_eg_frames_vqc([b for b, _ in damaged], w, h, STACKS, pal, m, list(START))
            else:
                ctx.decode_eg_frames([b for b, _ in damaged], w, h, STACKS, list(START))
        assert e.value.code == code, ("host form", e.value.code, code)
        if kind == "vqc":
            err = _vqc_dev_error(ctx, pkg, damaged, START, w, h, STACKS, pal, m)
        else:
            with pytest.raises(pkg.Dct3dError) as e:
                vq.decode_dev(ctx, damaged, list(START), w, h, 3, STACKS, None, None, vq=False)  # (checks the bands)
            err = e.value
        assert err.code == code, ("device form", err.code, code)
        assert [err.end_bits[c] for c in range(3) if c not in hit] == [ends[c] for c in range(3) if c not in hit]
    _check(decode_both(ctx, pkg, streams, START, w, h, STACKS, kind, pal, m, mode), ref, ends, 1, "the call after")
