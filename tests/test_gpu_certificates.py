"""GPU: the device's certificates decide exactly what the host emulations decide.

Every encode and decode kernel is certify-or-replay, and dct3d_get_stats reports what the certificates left open.
The parity tests compare outputs, which a loosened certificate changes only when a quotient lies within ~1e-4 of a
rounding tie and on the wrong side of the threshold; the counts see every such coefficient.  With contraction off on
both sides and one butterfly source, the counts must equal cert_common.py's predictions (the host emulations
tests/native/emulate_encode.cpp and emulate_decode_quant.cpp) exactly: every assertion here is an equality of
integers, after the output itself has been compared with the oracle as the parity tests do.

  encode, int32   n_flagged + n_rechecked = the coefficients the fp32 certificate left open (8x8x8; with
                  DCT3D_OPT_ENC_NO_RECHECK, and at 8x8x4, n_flagged alone); with the second certificate on the pair
                  is split_8x8x8's: exact ties to the Java fold, every other open coefficient rechecked
  encode, stream  n_flagged = the open coefficients, for the kernels that count: frames that are no multiple of 8
                  (EDGE) and packed RGB24 (PX = 3).  The grey multiple-of-8 stream kernel (dct3d_encode_eg_dev's)
                  reports no count (dct3d.h): it shares this source through `if constexpr`, but its instantiation is
                  not covered by this module.
  decode          n_flagged = 32 x the lanes with an uncertified pixel (cert_common.decode_open), int32 and stream
                  calls alike: every decode kernel reports its replays, none is left out.

Localisation: besides the whole raster, every case repeats the call on each horizontal band of one block row (host
calls on cropped frames / that row's cubes) and compares the vector of per-band counts; a failure names the first
differing band and the emulation's open positions in it.  Rich cases (>= 20 open units, a non-zero count in a quarter
of the bands; asserted) are the ones a threshold read one entry off changes (test_cert_common.py shows that on the
CPU); the small shapes are there for the kernels' geometry: ragged 4- and 8-cube waves, a single cube, edge cubes.
1080p is the largest case of the grey int32 families only (an RGB 1080p stack triples the host's share of the time).
"""
import numpy as np
import pytest

import cert_common as cc
import quant_common as qc
from cert_common import DEC, EDGE, EG, MARGINS, RGB, STACKS4, STACKS8
from test_gpu_eg import _expected

pytestmark = pytest.mark.gpu

MODES = ("ref", "ref_forced") + cc.TABLES[1:]  # ref_forced: the QT = 1 kernels on the reference table


def _table_name(mode):
    return "ref" if mode == "ref_forced" else mode


@pytest.fixture(scope="module")
def cctx(pkg):
    """contexts of this module's own, handed out with the table of `mode` set and every option at its default"""
    made = {}

    def get(depth, mode):
        if depth not in made:
            try:
                made[depth] = pkg.Context(0, 8, 8, depth)
            except Exception as e:
                pytest.fail(f"HIP context for 8x8x{depth} could not be created: {e}")
        ctx = made[depth]
        for opt in (pkg.DCT3D_OPT_QUANT_FORCE_TABLE, pkg.DCT3D_OPT_EG_TWO_STEP, pkg.DCT3D_OPT_ENC_NO_RECHECK,
                    pkg.DCT3D_OPT_DEC_MARGIN):
            ctx.set_option(opt, 0)
        ctx.set_quant(cc.table(_table_name(mode), depth))
        if mode == "ref_forced":
            ctx.set_option(pkg.DCT3D_OPT_QUANT_FORCE_TABLE, 1)
        return ctx

    yield get
    for c in made.values():
        c.close()


def _streams(q, depth, channels, stacks):
    """the oracle's Exp-Golomb stream of each channel's cubes of q [stack][channel][cube]"""
    import oracle
    blocks = q.reshape(stacks, channels, -1, 64 * depth)
    return [_expected(oracle, qc.pkg(), np.ascontiguousarray(blocks[:, ch]), depth) for ch in range(channels)]


def _pair(st):
    return int(st["n_flagged"]), int(st["n_rechecked"])


def _equal_counts(c, what, pred, got, mask):
    """pred, got: per-band vectors of (n_flagged, n_rechecked), the whole raster's pair last"""
    pred, got = np.asarray(pred, np.int64), np.asarray(got, np.int64)
    print(f"{c.id} {what}: predicted {pred[-1].tolist()}, device {got[-1].tolist()}")
    if not np.array_equal(pred[:-1], got[:-1]):
        pytest.fail(f"{c.id} {what}: " + cc.first_difference(pred[:-1], got[:-1], mask, c.stacks, c.channels, c.nby) +
                    f"\npredicted per band {pred[:-1].tolist()}\ndevice per band {got[:-1].tolist()}")
    assert np.array_equal(pred[-1], got[-1]), f"{c.id} {what}: the bands agree, the whole raster does not"


# ---- encode ---------------------------------------------------------------------------------------------------------

def _encode_call(api):
    return {"stacks": lambda ctx, fr: ctx.encode_stacks(fr), "stacks_rgb": lambda ctx, fr: ctx.encode_stacks_rgb(fr),
            "frames": lambda ctx, fr: ctx.encode_frames(fr), "eg": lambda ctx, fr: ctx.encode_eg_frames(fr)}[api]


def _encode_counts(ctx, c, api, q_ref):
    """the call on the whole raster and on every band, each output compared with the reference: the counts"""
    call, fr = _encode_call(api), c.frames()
    got = []
    for by in list(range(c.nby)) + [None]:
        f = fr if by is None else cc.band_frames(fr, by)
        ref = q_ref if by is None else cc.band_cubes(q_ref, c.stacks, c.channels, c.nby, by)
        out = call(ctx, f)
        st = ctx.stats()
        if api == "eg":
            assert out == _streams(ref, c.depth, c.channels, c.stacks), f"{c.id} band {by}: stream"
        else:
            assert np.array_equal(out, ref), f"{c.id} band {by}: {(out != ref).sum()} coefficients differ"
        got.append(_pair(st))
    return got


def _bands(c, *masks):
    """per-band (and, last, whole-raster) count pairs of the masks (one mask: the second count is 0)"""
    cols = [cc.band_counts(m, c.stacks, c.channels, c.nby) for m in masks]
    if len(cols) == 1:
        cols.append(np.zeros_like(cols[0]))
    v = np.stack(cols, axis=1)
    return np.concatenate([v, v.sum(axis=0, keepdims=True)])


def _predict(c, mode):
    name = _table_name(mode)
    _, op = cc.case_open(c, name)
    if name in c.rich:
        assert cc.is_rich(cc.band_counts(op, c.stacks, c.channels, c.nby)), f"{c.id} {name} is not rich"
    return op, cc.case_q_ref(c, name)


def _check_open(pkg, ctx, c, api, mode, what):
    """n_flagged = the open coefficients, n_rechecked = 0"""
    op, q_ref = _predict(c, mode)
    _equal_counts(c, what, _bands(c, op), _encode_counts(ctx, c, api, q_ref), op)


def _check_split(pkg, ctx, c, api, mode, what):
    """8x8x8, second certificate on: (n_flagged, n_rechecked) = split_8x8x8's (exact ties, the rest)"""
    op, q_ref = _predict(c, mode)
    fold, rechk = cc.split_8x8x8(c.frames(), op, cc.table(_table_name(mode), 8), cc.case_dct(c))
    _equal_counts(c, what, _bands(c, fold, rechk), _encode_counts(ctx, c, api, q_ref), op)
    return fold


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", STACKS8, ids=repr)
def test_encode_8x8x8(pkg, cctx, c, mode):
    """a: encode_stacks.  Second certificate off: every open coefficient is folded; on: the pair is split_8x8x8's.
    The ramp crop holds cube 14829's exact tie, which only the fold settles: its predicted n_flagged is >= 1."""
    ctx = cctx(8, mode)
    ctx.set_option(pkg.DCT3D_OPT_ENC_NO_RECHECK, 1)
    _check_open(pkg, ctx, c, "stacks", mode, f"{mode} no recheck")
    ctx.set_option(pkg.DCT3D_OPT_ENC_NO_RECHECK, 0)
    fold = _check_split(pkg, ctx, c, "stacks", mode, f"{mode} recheck")
    if c.kind == "ramp_crop" and _table_name(mode) == "ref":
        assert fold.sum() >= 1 and fold[3 * 8 + 3, 0, 2, 2]  # cube 14829 = block (61, 189): (3, 3) of the crop


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", STACKS4, ids=repr)
def test_encode_8x8x4(pkg, cctx, c, mode):
    """b: encode_stacks at 8x8x4 (encode_body, enc4_replay): n_flagged = open, n_rechecked = 0"""
    _check_open(pkg, cctx(4, mode), c, "stacks", mode, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", RGB, ids=repr)
def test_encode_rgb(pkg, cctx, c, mode):
    """c: encode_stacks_rgb: the count is the sum over the three planes (the prediction runs on the planar-stacked
    raster)"""
    ctx = cctx(c.depth, mode)
    if c.depth == 8:
        _check_split(pkg, ctx, c, "stacks_rgb", mode, f"{mode} recheck")
        ctx.set_option(pkg.DCT3D_OPT_ENC_NO_RECHECK, 1)
    _check_open(pkg, ctx, c, "stacks_rgb", mode, f"{mode} no recheck")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", EDGE, ids=repr)
def test_encode_edge(pkg, cctx, c, mode):
    """d: encode_frames at sizes that are no multiple of 8: the prediction is made on the edge-padded raster"""
    ctx = cctx(c.depth, mode)
    if c.depth == 8:
        _check_split(pkg, ctx, c, "frames", mode, f"{mode} recheck")
        ctx.set_option(pkg.DCT3D_OPT_ENC_NO_RECHECK, 1)
    _check_open(pkg, ctx, c, "frames", mode, f"{mode} no recheck")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", EG, ids=repr)
def test_encode_stream(pkg, cctx, c, mode):
    """e: encode_eg_frames through the stream kernels that count (EDGE, PX = 3), both depths: every open coefficient
    takes the exact fold, n_flagged = open"""
    _check_open(pkg, cctx(c.depth, mode), c, "eg", mode, mode)


@pytest.mark.parametrize("mode", ["ref", "q1"])
@pytest.mark.parametrize("c", [EG[0], EG[2]], ids=repr)
def test_encode_stream_two_step(pkg, cctx, c, mode):
    """f: DCT3D_OPT_EG_TWO_STEP: the same streams through the int32 kernels, whose counts the call then reports"""
    ctx = cctx(c.depth, mode)
    ctx.set_option(pkg.DCT3D_OPT_EG_TWO_STEP, 1)
    if c.depth == 8:
        _check_split(pkg, ctx, c, "eg", mode, f"{mode} two-step")
    else:
        _check_open(pkg, ctx, c, "eg", mode, f"{mode} two-step")


# ---- decode ---------------------------------------------------------------------------------------------------------

def _decode_call(c, api):
    if api == "eg":
        return lambda ctx, q, h: ctx.decode_eg_frames([b for b, _ in _streams(q, c.depth, c.channels, c.stacks)], c.w, h,
                                                      c.stacks)[0]
    if api == "eg_grey":
        return lambda ctx, q, h: ctx.decode_eg(_streams(q, c.depth, 1, c.stacks)[0][0], c.w, h, c.stacks)[0]
    if c.w % 8 or c.h % 8:
        return lambda ctx, q, h: ctx.decode_frames(q, c.w, h, c.stacks, c.channels)
    if c.channels == 3:
        return lambda ctx, q, h: ctx.decode_stacks_rgb(q, c.w, h, c.stacks)
    return lambda ctx, q, h: ctx.decode_stacks(q, c.w, h, c.stacks)


def _check_decode(pkg, ctx, c, mode, margin, api="int32"):
    """n_flagged = 32 x the flagged lanes, whole raster and per band; the frames are the reference's either way"""
    name = _table_name(mode)
    T = cc.table(name, c.depth)
    q = cc.case_q_ref(c, name)
    lanes = cc.decode_open(q, c.depth, T, margin)  # (asserts its preconditions before any GPU call)
    out_ref = qc.ref_decode_frames(q, c.w, c.h, c.stacks, c.channels, cc.steps_of(T, c.depth), c.depth)
    call = _decode_call(c, api)
    ctx.set_option(pkg.DCT3D_OPT_DEC_MARGIN, margin)
    got = []
    for by in list(range(c.nby)) + [None]:
        qb = q if by is None else cc.band_cubes(q, c.stacks, c.channels, c.nby, by)
        ref = out_ref if by is None else out_ref[:, 8 * by:8 * by + 8]
        out = call(ctx, qb, ref.shape[1])
        st = ctx.stats()
        assert np.array_equal(out, ref), f"{c.id} band {by}: {(out != ref).sum()} bytes differ"
        got.append(_pair(st))
    ctx.set_option(pkg.DCT3D_OPT_DEC_MARGIN, 0)
    pred = _bands(c, lanes)
    pred[:, 0] *= 32
    _equal_counts(c, f"{mode} {api} margin {margin}", pred, got, lanes)
    return int(pred[-1, 0])


@pytest.mark.parametrize("mode", ["ref", "seeded"])
@pytest.mark.parametrize("c", DEC, ids=repr)
def test_decode(pkg, cctx, c, mode):
    """g: decode_stacks[_rgb] (multiples of 8) and decode_frames (any size) on the reference encoder's output: no lane
    is flagged at margin 0, and at each of MARGINS exactly the lanes the emulation flags"""
    ctx = cctx(c.depth, mode)
    assert _check_decode(pkg, ctx, c, mode, 0.0) == 0
    n = [_check_decode(pkg, ctx, c, mode, m) for m in MARGINS]
    if (c.w, c.h) == (200, 72):
        assert 0 < n[0] < n[1] < n[2]


@pytest.mark.parametrize("mode", ["ref", "seeded"])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_l1_guard(pkg, cctx, depth, mode):
    """g: two cubes just under and two just over dec_l1_max (quant_common.guard_cube, 2^-10 either side): the cubes
    over it are replayed whole, n_flagged = 32 x (the flagged lanes of the under cubes) + 64 depth x 2"""
    T = cc.steps_of(cc.table(mode, depth), depth)
    q, over = cc.guard_cubes(depth, mode)
    ctx = cctx(depth, mode)
    ref = qc.ref_decode(q, 32, 8, depth, T, depth)
    for margin in (0.0, MARGINS[1]):
        lanes = cc.decode_open(q, depth, cc.table(mode, depth), margin)
        assert lanes[over].all()
        ctx.set_option(pkg.DCT3D_OPT_DEC_MARGIN, margin)
        out = ctx.decode_stacks(q, 32, 8, 1)
        st = ctx.stats()
        ctx.set_option(pkg.DCT3D_OPT_DEC_MARGIN, 0)
        assert np.array_equal(out, ref)
        assert st["n_flagged"] == 32 * int(lanes[~over].sum()) + 64 * depth * 2 == 32 * int(lanes.sum()), (margin, st)


@pytest.mark.parametrize("mode", ["ref", "seeded"])
@pytest.mark.parametrize("c", DEC, ids=repr)
def test_decode_stream(pkg, cctx, c, mode):
    """h: decode_eg_frames (and, grey at multiples of 8, decode_eg) at the 10 % margin: the fused stream decode runs
    decode_tile on the parsed codes and reports its replays in every geometry -- the same equality"""
    ctx = cctx(c.depth, mode)
    n = _check_decode(pkg, ctx, c, mode, MARGINS[1], "eg")
    assert n > 0 or (c.w, c.h) != (200, 72)
    if c.channels == 1 and not (c.w % 8 or c.h % 8):
        _check_decode(pkg, ctx, c, mode, MARGINS[1], "eg_grey")
