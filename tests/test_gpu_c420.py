"""GPU: 4:2:0 chroma subsampling fused into the YCbCr stream calls and the rate probe (dct3d_ctx_set_chroma =
DCT3D_CHROMA_420 on top of DCT3D_OPT_COLOUR = DCT3D_COLOUR_YCBCR).  The feature is stated as identities
against the GREY calls as they are, on the three planes (Y, S(Cb), S(Cr)) = rgb_to_ycbcr420(frames) (the numpy
definitions, tests/test_c420_ref.py), of sizes (w, h), (cw, ch), (cw, ch):

  encode   mode on, on frames          ==  the grey call on plane k: stream k, total bits, ENOSPC
  rate     mode on, on frames          ==  the grey probe on plane k: bits[t, s, k]
  decode   mode on, from three streams ==  ycbcr420_to_rgb of the three grey decodes; end bits equal

All comparisons are exact equalities of bytes and integers.  The grey side is covered against the oracle by the other
modules (test_gpu_eg_frames.py, test_gpu_quant.py, test_gpu_vq.py, test_gpu_rate.py).

Statistics.  n_units of a call is the sum over the three grey calls.  n_flagged: a grey stream ENCODE at multiples of
8 runs the plain kernel, which reports no count (dct3d.h), while every chain of a packed call counts; so the encode's
n_flagged equals the sum of the grey calls' where all three planes are ragged and is at least that sum elsewhere.  The
decode's and the rate probe's kernels count in every geometry: their n_flagged is the sum.

Shapes (w, h, stacks): see SHAPES.  FOLD_SHAPE is one at which the exact fold runs in both chroma chains, found on the
CPU with cert_common's emulation on the subsample_420 planes of the uniform content (reference table): open
coefficients [Y, Cb, Cr] = [18, 2, 4] at 8x8x8 and [15, 4, 5] at 8x8x4; all three planes are ragged there, so the grey
runs count them (asserted).  FOLD_ALIGNED (multiples of 16: the aligned loader's reload) predicts [22, 4, 4] and
[15, 4, 7]; its grey runs are the plain kernel's, so the packed call's count is checked against the prediction."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import quant_common as qc
from conftest import ctx_option
from test_gpu_vq import decode_dev, encode_dev
from test_gpu_ycc import CARRY, NO_CARRY, SEED, colour

pytestmark = pytest.mark.gpu

FOLD_SHAPE = (244, 54, 2)
FOLD_ALIGNED = (208, 80, 2)
FOLD_OPEN = {(FOLD_SHAPE, 8): [18, 2, 4], (FOLD_SHAPE, 4): [15, 4, 5], (FOLD_ALIGNED, 8): [22, 4, 4], (FOLD_ALIGNED, 4): [15, 4, 7]}
SHAPES = [
    (1, 1, 1),       # one sample everywhere
    (2, 2, 1),
    (7, 5, 2),       # width under 8
    (15, 9, 2),      # width under 16: the byte path; cw = 8 exactly
    (16, 16, 1),     # no edge in any plane, one chroma cube
    (17, 16, 1),     # a chroma cube column holding one sample that comes from a replicated pixel
    (24, 16, 5),     # Y aligned, chroma ragged; an odd nbx; several stacks
    (32, 32, 2),     # both aligned; even nbx: the block stores
    (61, 27, 2),     # both ragged; a packed row stride that is no multiple of 4
    (1366, 24, 1),
    FOLD_SHAPE,
    FOLD_ALIGNED,
]


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


@functools.lru_cache(maxsize=None)
def planes(kind, depth, w, h, stacks):
    """(Y, S(Cb), S(Cr)) of the colour content: the reference's inputs, made once (read-only)"""
    out = qc.pkg().rgb_to_ycbcr420(colour(kind, depth, w, h, stacks))
    for a in out:
        a.setflags(write=False)
    return out


def _sizes(pkg, w, h):
    cw, ch = pkg.chroma_size(w, h)
    return [(w, h), (cw, ch), (cw, ch)]


def _caps(pkg, w, h, depth, stacks):
    """a capacity per stream that holds any content: 4 bytes per value of the padded plane (a code has 27 bits at most)"""
    return [(-(-pw // 8) * 8) * (-(-ph // 8) * 8) * depth * stacks * 4 + 64 for pw, ph in _sizes(pkg, w, h)]


def _table(pkg, depth, name):
    return None if name == "ref" else pkg.quant_table(int(name[1:]), depth)


def _stats(ctx):
    st = ctx.stats()
    return st["n_units"], st["n_flagged"]


class _on:
    """the colour transform and 4:2:0 for the duration of a block"""

    def __init__(self, ctx, pkg):
        self.ctx, self.pkg = ctx, pkg

    def __enter__(self):
        self.ctx.set_option(self.pkg.DCT3D_OPT_COLOUR, self.pkg.DCT3D_COLOUR_YCBCR)
        self.ctx.set_chroma(self.pkg.DCT3D_CHROMA_420)
        return self.ctx

    def __exit__(self, *a):
        self.ctx.set_chroma(self.pkg.DCT3D_CHROMA_444)
        self.ctx.set_option(self.pkg.DCT3D_OPT_COLOUR, 0)


def _ragged(w, h):
    return bool(w % 8 or h % 8)


def _check_encode_stats(pkg, w, h, got, grey):
    """got: (n_units, n_flagged) of the packed call; grey: the three grey calls'"""
    print("encode statistics: packed", got, "grey", grey)
    assert got[0] == sum(u for u, _ in grey)
    if all(_ragged(*s) for s in _sizes(pkg, w, h)):
        assert got[1] == sum(f for _, f in grey)
    else:
        assert got[1] >= sum(f for _, f in grey)


# ---- 1: encode ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", ["ref", "q1"])
@pytest.mark.parametrize("kind", ["ramp", "uniform"])
@pytest.mark.parametrize("w,h,stacks", SHAPES)
@pytest.mark.parametrize("depth", [8, 4])
def test_encode_identity(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks, kind, table):
    """host and device entry points, the device one under non-zero carries: stream k and its total bits equal the grey
    call's on plane k"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, pl, sz = colour(kind, depth, w, h, stacks), planes(kind, depth, w, h, stacks), _sizes(pkg, w, h)
    fold = (w, h, stacks) in (FOLD_SHAPE, FOLD_ALIGNED) and kind == "uniform" and table == "ref"
    caps = _caps(pkg, w, h, depth, stacks)
    ctx.set_quant(_table(pkg, depth, table))
    try:
        want_h, want_d, st_h, st_d = [], [], [], []
        for k in range(3):
            want_h.append(ctx.encode_eg_frames(pl[k])[0])
            st_h.append(_stats(ctx))
            got, ok = encode_dev(ctx, pl[k], sz[k][0], sz[k][1], 1, stacks, None, None, [CARRY[k]], caps=[caps[k]], vq=False)
            st_d.append(_stats(ctx))
            assert ok
            want_d.append(got[0])
        if fold and (w, h, stacks) == FOLD_SHAPE:
            assert [f for _, f in st_h] == [f for _, f in st_d] == FOLD_OPEN[(FOLD_SHAPE, depth)], "the grey runs must take the predicted folds"
        with _on(ctx, pkg):
            got_h = ctx.encode_eg_frames(fr)
            gst_h = _stats(ctx)
            got_d, ok = encode_dev(ctx, fr, w, h, 3, stacks, None, None, CARRY, caps=caps, vq=False)
            gst_d = _stats(ctx)
            assert ok
        assert got_h == want_h and got_d == want_d
        assert [t for _, t in got_h] != [0, 0, 0]
        _check_encode_stats(pkg, w, h, gst_h, st_h)
        _check_encode_stats(pkg, w, h, gst_d, st_d)
        if fold:
            assert gst_h[1] == gst_d[1] == sum(FOLD_OPEN[((w, h, stacks), depth)])
    finally:
        ctx.set_quant(None)


@pytest.mark.parametrize("depth", [8, 4])
def test_encode_enospc_is_the_same(pkg, gpu_ctx8, gpu_ctx4, depth):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 61, 27, 2
    fr, pl, sz = colour("uniform", depth, w, h, stacks), planes("uniform", depth, w, h, stacks), _sizes(pkg, w, h)
    full = [ctx.encode_eg_frames(pl[k])[0][1] for k in range(3)]
    caps = [64, ((full[1] + 31) // 32) * 4 + 64, 64]  # the middle stream fits, the others do not
    grey = []
    for k in range(3):
        try:
            got, _ = encode_dev(ctx, pl[k], sz[k][0], sz[k][1], 1, stacks, None, None, NO_CARRY[:1], caps=[caps[k]], vq=False)
            grey.append((pkg.DCT3D_OK, got[0][1]))
        except pkg.Dct3dError as e:
            grey.append((e.code, e.total_bits[0]))
    assert [c for c, _ in grey] == [pkg.DCT3D_ENOSPC, pkg.DCT3D_OK, pkg.DCT3D_ENOSPC]
    with _on(ctx, pkg):
        with pytest.raises(pkg.Dct3dError) as e:
            encode_dev(ctx, fr, w, h, 3, stacks, None, None, NO_CARRY, caps=caps, vq=False)
        assert e.value.code == pkg.DCT3D_ENOSPC and e.value.total_bits == [t for _, t in grey] == full
        # and with room everywhere the call after it is right
        got, ok = encode_dev(ctx, fr, w, h, 3, stacks, None, None, NO_CARRY, caps=_caps(pkg, w, h, depth, stacks), vq=False)
    assert ok and [t for _, t in got] == full


# ---- 2: decode ----------------------------------------------------------------------------------------------------

_STREAMS = {}


def _unrelated(kind, depth, w, h, stacks, k):
    """a synthetic plane of plane k's size that has nothing to do with the other two"""
    return qc.pkg().synthetic.frames(w, h, stacks * depth, seed=SEED + 104729 * (k + 1), frame0=5 * k, kind=kind)


def _streams_of(ctx, pkg, depth, w, h, stacks, source):
    """three grey encodes (reference table), made once per shape: of the planes of the colour ramp ("ramp": what the
    4:2:0 encode writes), or of unrelated uniform planes of the right sizes ("uniform")"""
    key = (depth, w, h, stacks, source)
    if key not in _STREAMS:
        sz = _sizes(pkg, w, h)
        pl = planes("ramp", depth, w, h, stacks) if source == "ramp" else [_unrelated("uniform", depth, sz[k][0], sz[k][1], stacks, k) for k in range(3)]
        _STREAMS[key] = tuple(ctx.encode_eg_frames(pl[k])[0] for k in range(3))
    return _STREAMS[key]


def _grey_decodes(ctx, pkg, streams, w, h, stacks):
    """the three grey decodes: (planes, end bits, statistics)"""
    outs, ebs, sts = [], [], []
    for (b, _), (pw, ph) in zip(streams, _sizes(pkg, w, h)):
        out, eb = ctx.decode_eg_frames([b], pw, ph, stacks)
        outs.append(out)
        ebs.append(eb[0])
        sts.append(_stats(ctx))
    return outs, ebs, sts


def _decode_on(ctx, pkg, streams, w, h, stacks, dev):
    with _on(ctx, pkg):
        if dev:
            out, eb, ok = decode_dev(ctx, streams, [0, 0, 0], w, h, 3, stacks, None, None, vq=False)
            assert ok, "a write outside the frames"
        else:
            out, eb = ctx.decode_eg_frames([b for b, _ in streams], w, h, stacks)
        return out, eb, _stats(ctx)


def _check_decode(pkg, got, grey):
    (on, eb, st), (outs, ebs, sts) = got, grey
    assert np.array_equal(on, pkg.ycbcr420_to_rgb(*outs))
    assert eb == ebs
    assert st == (sum(u for u, _ in sts), sum(f for _, f in sts)), (st, sts)


@pytest.mark.parametrize("source", ["ramp", "uniform"])
@pytest.mark.parametrize("w,h,stacks", SHAPES)
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_identity(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks, source):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    streams = _streams_of(ctx, pkg, depth, w, h, stacks, source)
    grey = _grey_decodes(ctx, pkg, streams, w, h, stacks)
    assert grey[1] == [t for _, t in streams]
    if source == "uniform" and w * h >= 35:
        # (a stack of a few pixels has too few samples for this; every other shape must show the clamp at work)
        outs = grey[0]
        pre = pkg.ycbcr_to_rgb_unclamped(np.stack((outs[0], pkg.upsample_420(outs[1], w, h), pkg.upsample_420(outs[2], w, h)), axis=-1))
        pre = pre.reshape(-1, 3)
        assert (pre.min(axis=0) < 0).all() and (pre.max(axis=0) > 255).all(), (pre.min(axis=0), pre.max(axis=0))
    for dev in (False, True):
        _check_decode(pkg, _decode_on(ctx, pkg, streams, w, h, stacks, dev), grey)


def test_the_encoder_s_streams_decode(pkg, gpu_ctx8):
    """the round trip through the 4:2:0 calls alone: within the quantiser's error of the frames (a sanity bound, not
    an identity: mean absolute error under 12 of 255 for the smooth ramp at the reference table)"""
    ctx, (w, h, stacks) = gpu_ctx8, (61, 27, 2)
    fr = colour("ramp", 8, w, h, stacks)
    with _on(ctx, pkg):
        streams = ctx.encode_eg_frames(fr)
        out, eb = ctx.decode_eg_frames([b for b, _ in streams], w, h, stacks)
    assert eb == [t for _, t in streams]
    assert np.abs(out.astype(np.int32) - fr.astype(np.int32)).mean() < 12.0


@pytest.mark.parametrize("option,value", [("DCT3D_OPT_DEC_MARGIN", 0.45), ("DCT3D_OPT_EG_FORCE_RETRY", 1),
                                          ("DCT3D_OPT_EG_NO_RESOLVE", 1)])
@pytest.mark.parametrize("w,h,stacks", [(24, 16, 5), (32, 32, 2), (61, 27, 2)])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_identity_under_the_options(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks, option, value):
    """a margin that sends nearly every lane through the exact replay, and the front's skip-and-rerun path"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    for source in ("ramp", "uniform"):
        streams = _streams_of(ctx, pkg, depth, w, h, stacks, source)
        with ctx_option(ctx, getattr(pkg, option), value):
            grey = _grey_decodes(ctx, pkg, streams, w, h, stacks)
            got_d = _decode_on(ctx, pkg, streams, w, h, stacks, True)
            got_h = _decode_on(ctx, pkg, streams, w, h, stacks, False)
        if option == "DCT3D_OPT_DEC_MARGIN":
            assert all(2 * f > u for u, f in grey[2]), "the margin must flag most lanes on the reference side"
        _check_decode(pkg, got_d, grey)
        _check_decode(pkg, got_h, grey)


@pytest.mark.parametrize("bad", [0, 1, 2])
@pytest.mark.parametrize("depth", [8, 4])
def test_truncated_stream(pkg, gpu_ctx8, gpu_ctx4, depth, bad):
    """a truncated Y stream and a truncated chroma stream: DCT3D_ENODATA, the end bits of the good streams, what the
    4:4:4 call gives for the same fault in the same stream; a sentinel-filled device raster stays untouched; and the
    next call is good"""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 61, 27, 2
    streams = list(_streams_of(ctx, pkg, depth, w, h, stacks, "ramp"))
    good = _decode_on(ctx, pkg, streams, w, h, stacks, True)
    totals = [t for _, t in streams]

    def cut(ss):
        b, t = ss[bad]
        out = list(ss)
        out[bad] = (b[:-1], t)  # truncated by a byte
        return out

    def run(ss):
        """(code, end bits, the raster untouched)"""
        d_s = []
        for b, _ in ss:
            a = np.zeros((len(b) + 3) // 4 * 4 + 4, np.uint8)
            a[:len(b)] = np.frombuffer(b, np.uint8)
            d_s.append(torch.from_numpy(a).cuda())
        d_out = torch.full((stacks * depth * h * w * 3,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.decode_eg_frames_dev(d_s, [len(b) for b, _ in ss], [0, 0, 0], w, h, stacks, d_out)
        ctx.synchronize()
        return e.value.code, e.value.end_bits, bool((d_out == 0xA5).all().item())

    # the 4:4:4 call, on three streams of its own value counts (the Y plane three times), the same stream cut
    with ctx_option(ctx, pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR):
        code444, eb444, clean444 = run(cut([streams[0]] * 3))
    with _on(ctx, pkg):
        code, eb, clean = run(cut(streams))
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.decode_eg_frames([b for b, _ in cut(streams)], w, h, stacks)
        assert e.value.code == code
    assert code == code444 == pkg.DCT3D_ENODATA and clean and clean444
    assert eb == [0 if k == bad else totals[k] for k in range(3)]
    assert eb444 == [0 if k == bad else totals[0] for k in range(3)]
    again = _decode_on(ctx, pkg, streams, w, h, stacks, True)
    assert np.array_equal(again[0], good[0]) and again[1] == good[1] == totals


# ---- 3: the per-stack table calls ------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,stacks", [(24, 16, 5), (61, 27, 3)])
@pytest.mark.parametrize("depth", [8, 4])
def test_vq_calls(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks):
    """a map that uses several tables, shared by the three channels: every stream is the grey vq call's on its plane,
    and the decode is ycbcr420_to_rgb of the grey vq decodes"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    pal = np.stack([pkg.quant_table(q, depth) for q in (5, 12, 2)]).astype(np.int32)
    m = (np.arange(stacks) % 3).astype(np.uint8)
    sz, caps = _sizes(pkg, w, h), _caps(pkg, w, h, depth, stacks)
    for kind in ("ramp", "uniform"):
        fr, pl = colour(kind, depth, w, h, stacks), planes(kind, depth, w, h, stacks)
        want_h = [ctx.encode_eg_frames_vq(pl[k], pal, m)[0] for k in range(3)]
        want_d = []
        for k in range(3):
            got, ok = encode_dev(ctx, pl[k], sz[k][0], sz[k][1], 1, stacks, pal, m, [CARRY[k]], caps=[caps[k]])
            assert ok
            want_d.append(got[0])
        assert want_h != [ctx.encode_eg_frames(pl[k])[0] for k in range(3)]  # (the other tables are in use)
        outs, ebs, sts = [], [], []
        for k in range(3):
            out, eb = ctx.decode_eg_frames_vq([want_h[k][0]], sz[k][0], sz[k][1], stacks, pal, m)
            outs.append(out)
            ebs.append(eb[0])
            sts.append(_stats(ctx))
        with _on(ctx, pkg):
            assert ctx.encode_eg_frames_vq(fr, pal, m) == want_h
            got_d, ok = encode_dev(ctx, fr, w, h, 3, stacks, pal, m, CARRY, caps=caps)
            assert ok and got_d == want_d
            on_h, eb_h = ctx.decode_eg_frames_vq([b for b, _ in want_h], w, h, stacks, pal, m)
            st_h = _stats(ctx)
            on_d, eb_d, ok = decode_dev(ctx, want_h, [0, 0, 0], w, h, 3, stacks, pal, m)
            st_d = _stats(ctx)
        assert ok
        _check_decode(pkg, (on_h, eb_h, st_h), (outs, ebs, sts))
        _check_decode(pkg, (on_d, eb_d, st_d), (outs, ebs, sts))


# ---- 4: the rate probe ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ramp", "uniform"])
@pytest.mark.parametrize("w,h,stacks", SHAPES)
@pytest.mark.parametrize("depth", [8, 4])
def test_rate_identity(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks, kind):
    """four tables in one call: bits[t, s, k] equals the grey probe's of plane k, host and device; only totals: a
    caller's per-cube buffer is refused"""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, pl = colour(kind, depth, w, h, stacks), planes(kind, depth, w, h, stacks)
    tabs = [pkg.quant_table(q, depth) for q in (5, 1, 12, 64)]
    want, sts = [], []
    for k in range(3):
        want.append(ctx.rate_frames(pl[k], tabs)[:, :, 0])
        sts.append(_stats(ctx))
    want = np.stack(want, axis=-1)
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    with _on(ctx, pkg):
        host = ctx.rate_frames(fr, tabs)
        st_h = _stats(ctx)
        dev = ctx.rate_frames_dev(d_fr, w, h, 3, stacks, tabs)
        st_d = _stats(ctx)
        tb = [t for _, t in ctx.encode_eg_frames(fr)]
        d_cubes = torch.zeros(4 * stacks * 3 * ((w + 7) // 8) * ((h + 7) // 8), dtype=torch.int16, device="cuda")
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.rate_frames_dev(d_fr, w, h, 3, stacks, tabs, d_cubes)
        assert e.value.code == pkg.DCT3D_EINVAL
        ctx.synchronize()
        assert not d_cubes.any().item()
        assert np.array_equal(ctx.rate_frames_dev(d_fr, w, h, 3, stacks, tabs), dev)  # the call after the refusal
    assert host.shape == (4, stacks, 3) and np.array_equal(host, want) and np.array_equal(dev, want)
    total = (sum(u for u, _ in sts), sum(f for _, f in sts))
    assert st_h == st_d == total, (st_h, st_d, sts)
    if (w, h, stacks) == FOLD_SHAPE and kind == "uniform":
        assert total[1] > 0
    # and the probe prices what the encode writes (the context's table is the first of the four)
    assert host[0].sum(axis=0).tolist() == tb


# ---- 5: refusals ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [8, 4])
def test_refusals_and_the_call_after(pkg, gpu_ctx8, gpu_ctx4, depth):
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 13, 11, 3
    fr, pl = colour("ramp", depth, w, h, stacks), planes("ramp", depth, w, h, stacks)
    want = [ctx.encode_eg_frames(pl[k])[0] for k in range(3)]
    streams = [b for b, _ in want]
    pal = np.stack([pkg.quant_table(5, depth), pkg.quant_table(12, depth)]).astype(np.int32)
    m = np.zeros(stacks, np.uint8)
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    d_out = [torch.zeros(4096, dtype=torch.uint8, device="cuda") for _ in range(3)]
    d_q = torch.from_numpy(ctx.encode_frames(fr)).cuda()
    E = pkg.DCT3D_EINVAL

    def on420():
        with _on(ctx, pkg):
            return ctx.encode_eg_frames(fr)

    def refused(f, *a, **k):
        before = _stats(ctx)
        with pytest.raises(pkg.Dct3dError) as e:
            f(*a, **k)
        assert e.value.code == E, f.__name__
        ctx.synchronize()
        assert _stats(ctx) == before, f.__name__  # nothing was launched: the statistics are the last good call's

    assert ctx.chroma() == pkg.DCT3D_CHROMA_444
    for bad in (2, -1, 420):
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.set_chroma(bad)
        assert e.value.code == E and ctx.chroma() == pkg.DCT3D_CHROMA_444
    assert on420() == want
    # three channels, the mode on, the colour transform off: refused before anything is queued
    ctx.set_chroma(pkg.DCT3D_CHROMA_420)
    try:
        assert ctx.chroma() == pkg.DCT3D_CHROMA_420
        ctx.encode_eg_frames(pl[0])  # (a good call, whose statistics must stand)
        refused(ctx.encode_eg_frames, fr)
        refused(ctx.encode_eg_frames_dev, d_fr, w, h, 3, stacks, d_out, [4096] * 3)
        refused(ctx.decode_eg_frames, streams, w, h, stacks)
        refused(ctx.decode_eg_frames_dev, d_out, [len(b) for b in streams], [0] * 3, w, h, stacks, d_fr)
        refused(ctx.rate_frames, fr)
        refused(ctx.rate_frames_dev, d_fr, w, h, 3, stacks)
        refused(ctx.encode_eg_frames_vq, fr, pal, m)
        refused(ctx.decode_eg_frames_vq, streams, w, h, stacks, pal, m)
        assert np.array_equal(fr, d_fr.cpu().numpy()) and not any(t.any().item() for t in d_out)  # nothing was written
        # one channel: the mode does nothing
        assert ctx.encode_eg_frames(pl[1])[0] == want[1]
        out, eb = ctx.decode_eg_frames([streams[0]], w, h, stacks)
        assert eb == [want[0][1]]
        assert np.array_equal(ctx.rate_frames(pl[2]), _rate_off(ctx, pkg, pl[2]))
        # the calls that refuse the colour option keep refusing it, with the mode on as well
        with ctx_option(ctx, pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR):
            assert ctx.encode_eg_frames(fr) == want
            refused(ctx.encode_frames, fr)
            refused(ctx.decode_frames_dev, d_q, w, h, 3, stacks, d_fr)
            refused(ctx.distortion_frames, fr)
            with ctx_option(ctx, pkg.DCT3D_OPT_EG_TWO_STEP, 1):
                for f, a in ((ctx.encode_eg_frames, (fr,)), (ctx.decode_eg_frames, (streams, w, h, stacks))):
                    with pytest.raises(pkg.Dct3dError) as e:
                        f(*a)
                    assert e.value.code == E, f.__name__
            assert ctx.encode_eg_frames(fr) == want
    finally:
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
    # the mode off again: the 4:4:4 calls are what they were
    with ctx_option(ctx, pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR):
        t = pkg.rgb_to_ycbcr(fr)
        got = ctx.encode_eg_frames(fr)
        assert got[0] == want[0]  # (the Y stream is the same in both modes)
        assert got[1] == ctx.encode_eg_frames(np.ascontiguousarray(t[..., 1]))[0] and got[1] != want[1]


def _rate_off(ctx, pkg, plane):
    ctx.set_chroma(pkg.DCT3D_CHROMA_444)
    try:
        return ctx.rate_frames(plane)
    finally:
        ctx.set_chroma(pkg.DCT3D_CHROMA_420)


# ---- 6: the codec's chroma=420 ----------------------------------------------------------------------------------------

LADDER = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64)
SUFFIXES = (".red", ".green", ".blue")


def _cli(pkg, *args, env=None):
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _files(tmp_path, name):
    return [(tmp_path / (name + s)).read_bytes() for s in SUFFIXES]


@pytest.mark.parametrize("depth", [8, 4])
def test_cli_round_trip(pkg, gpu_ctx8, gpu_ctx4, tmp_path, depth):
    """encode_rgb ... ycc=1 chroma=420: each file is the .bin the grey encode command writes for that plane (beside q=,
    and through the environment variables); decode_rgb with the same tokens writes the frames the Python calls give"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 61, 27, 2
    fr, pl, sz = colour("ramp", depth, w, h, stacks), planes("ramp", depth, w, h, stacks), _sizes(pkg, w, h)
    raw = tmp_path / "in.rgb"
    fr.tofile(raw)
    geo = (w, h, stacks * depth, 1, depth)
    _cli(pkg, "encode_rgb", raw, tmp_path / "on", *geo, "q=3", "ycc=1", "chroma=420")
    env = dict(os.environ, DCT3D_CODEC_YCC="1", DCT3D_CODEC_CHROMA="420")
    _cli(pkg, "encode_rgb", raw, tmp_path / "env", *geo, "q=3", env=env)
    grey = []
    for k in range(3):
        pl[k].tofile(tmp_path / f"p{k}.raw")
        _cli(pkg, "encode", tmp_path / f"p{k}.raw", tmp_path / f"p{k}.bin", sz[k][0], sz[k][1], stacks * depth, 1, depth, "q=3")
        grey.append((tmp_path / f"p{k}.bin").read_bytes())
    assert _files(tmp_path, "on") == _files(tmp_path, "env") == grey and all(len(b) > 0 for b in grey)
    _cli(pkg, "decode_rgb", tmp_path / "on", tmp_path / "dec.rgb", *geo, "q=3", "ycc=1", "chroma=420")
    ctx.set_quant(pkg.quant_table(3, depth))
    try:
        with _on(ctx, pkg):
            streams = ctx.encode_eg_frames(fr)
            want, _ = ctx.decode_eg_frames([b for b, _ in streams], w, h, stacks)
    finally:
        ctx.set_quant(None)
    assert np.array_equal(np.fromfile(tmp_path / "dec.rgb", np.uint8).reshape(fr.shape), want)


def test_cli_rate_with_a_quality_map(pkg, gpu_ctx8, tmp_path):
    """rate= with qmap= under chroma=420 prices and codes the subsampled planes: the bits it prints are the Python
    encode's under the map it wrote, an encode that reads the map writes the same files, and the decode with the map
    gives the Python decode's frames"""
    ctx, depth = gpu_ctx8, 8
    w, h, stacks = 61, 27, 2
    fr = colour("ramp", depth, w, h, stacks)
    raw = tmp_path / "in.rgb"
    fr.tofile(raw)
    geo = (w, h, stacks * depth, 1, depth)
    tok = ("ycc=1", "chroma=420")
    out = _cli(pkg, "encode_rgb", raw, tmp_path / "m", *geo, "rate=1.5", f"qmap={tmp_path / 'm.map'}", *tok)
    m = re.search(r"^qmap: stacks=(\d+) bits=(\d+)$", out, re.M)
    assert m and int(m.group(1)) == stacks, out
    quals = [int(x) for x in (tmp_path / "m.map").read_text().split()]
    assert len(quals) == stacks and all(q in LADDER for q in quals)
    pal = np.stack([pkg.quant_table(q, depth) for q in LADDER]).astype(np.int32)
    idx = np.array([LADDER.index(q) for q in quals], np.uint8)
    with _on(ctx, pkg):
        streams = ctx.encode_eg_frames_vq(fr, pal, idx)
        want, _ = ctx.decode_eg_frames_vq([b for b, _ in streams], w, h, stacks, pal, idx)
        bits = ctx.rate_frames(fr, list(pal))
    assert int(m.group(2)) == sum(t for _, t in streams) == sum(int(bits[idx[s], s].sum()) for s in range(stacks))
    _cli(pkg, "encode_rgb", raw, tmp_path / "r", *geo, f"qmap={tmp_path / 'm.map'}", *tok)
    assert _files(tmp_path, "m") == _files(tmp_path, "r")
    _cli(pkg, "decode_rgb", tmp_path / "m", tmp_path / "dec.rgb", *geo, f"qmap={tmp_path / 'm.map'}", *tok)
    assert np.array_equal(np.fromfile(tmp_path / "dec.rgb", np.uint8).reshape(fr.shape), want)
