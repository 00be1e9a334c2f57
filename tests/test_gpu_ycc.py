"""GPU: the YCbCr colour transform fused into the packed RGB24 stream calls and the rate probe (DCT3D_OPT_COLOUR;
DESIGN 4o).  The whole feature is three identities against the calls as they are without the option, with T =
rgb_to_ycbcr and T^-1 = ycbcr_to_rgb (the numpy definitions, tests/test_ycc_ref.py):

  encode   mode on, on frames          ==  mode off, on T(frames): streams, total bits, ENOSPC, statistics
  rate     mode on, on frames          ==  mode off, on T(frames): bits, cube bits, n_flagged
  decode   mode on, from some streams  ==  T^-1 of mode off from the same streams; end bits and statistics equal

All comparisons are exact equalities of bytes and integers.  The mode-off side is covered against the oracle by the
other modules (test_gpu_eg_frames.py, test_gpu_quant.py, test_gpu_vq.py, test_gpu_rate.py).

Content: "ramp" and "uniform", three synthetic planes of different seeds interleaved.  Shapes (w, h, stacks): the
smallest frame; both edges and several stacks; aligned with an odd and an even number of cubes per row (the decode's
per-lane stores and its block stores); edges with several block rows; a packed row stride that is no multiple of 4;
and enough cubes that the encode's exact fold runs (asserted on the mode-off side, predicted on the CPU with
cert_common's emulation: 12 open coefficients at 8x8x8, 39 at 8x8x4 under the reference table)."""
import functools
import re
import subprocess

import numpy as np
import pytest

import quant_common as qc
from conftest import ctx_option
from test_gpu_vq import decode_dev, encode_dev

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (13, 11, 3), (24, 16, 5), (32, 16, 2), (61, 27, 2), (1366, 24, 1), (200, 72, 4)]
FOLD_SHAPE = (200, 72, 4)
CARRY = [(0xB4, 3), (0x5F, 7), (0x80, 1)]
NO_CARRY = [(0, 0)] * 3
SEED = 0x3DDC7


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


@functools.lru_cache(maxsize=None)
def colour(kind, depth, w, h, stacks):
    """packed frames [stacks * depth, h, w, 3]: three synthetic planes of different seeds, interleaved (read-only)"""
    p = qc.pkg()
    fr = np.stack([p.synthetic.frames(w, h, stacks * depth, seed=SEED + 7919 * i, frame0=3 * i, kind=kind)
                   for i in range(3)], axis=-1)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def transformed(kind, depth, w, h, stacks):
    t = qc.pkg().rgb_to_ycbcr(colour(kind, depth, w, h, stacks))
    t.setflags(write=False)
    return t


def _table(pkg, depth, name):
    return None if name == "ref" else pkg.quant_table(int(name[1:]), depth)


def _stats(ctx):
    st = ctx.stats()
    return st["n_units"], st["n_flagged"]


def _on(ctx, pkg):
    return ctx_option(ctx, pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR)


# ---- 1: encode ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("table", ["ref", "q1"])
@pytest.mark.parametrize("kind", ["ramp", "uniform"])
@pytest.mark.parametrize("w,h,stacks", SHAPES)
@pytest.mark.parametrize("depth", [8, 4])
def test_encode_identity(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks, kind, table):
    """host and device entry points, the device one under non-zero carries: streams, total bits and statistics of
    mode on equal those of mode off on the transformed frames"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, tf = colour(kind, depth, w, h, stacks), transformed(kind, depth, w, h, stacks)
    ctx.set_quant(_table(pkg, depth, table))
    try:
        want_h = ctx.encode_eg_frames(tf)
        st_h = _stats(ctx)
        want_d, ok = encode_dev(ctx, tf, w, h, 3, stacks, None, None, CARRY, vq=False)
        st_d = _stats(ctx)
        assert ok
        if (w, h, stacks) == FOLD_SHAPE and kind == "ramp":
            assert st_h[1] > 0 and st_d[1] > 0, "the reference run must take the exact fold (its reloads are under test)"
        with _on(ctx, pkg):
            got_h = ctx.encode_eg_frames(fr)
            assert _stats(ctx) == st_h
            got_d, ok = encode_dev(ctx, fr, w, h, 3, stacks, None, None, CARRY, vq=False)
            assert ok and _stats(ctx) == st_d
        assert got_h == want_h and got_d == want_d
        assert [t for _, t in got_h] != [0, 0, 0]
    finally:
        ctx.set_quant(None)


@pytest.mark.parametrize("depth", [8, 4])
def test_encode_enospc_is_the_same(pkg, gpu_ctx8, gpu_ctx4, depth):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 61, 27, 2
    fr, tf = colour("uniform", depth, w, h, stacks), transformed("uniform", depth, w, h, stacks)
    full = [t for _, t in ctx.encode_eg_frames(tf)]
    caps = [64, ((full[1] + 31) // 32) * 4 + 64, 64]  # the middle stream fits, the others do not
    res = []
    for frames, mode in ((tf, 0), (fr, 1)):
        with ctx_option(ctx, pkg.DCT3D_OPT_COLOUR, mode):
            with pytest.raises(pkg.Dct3dError) as e:
                encode_dev(ctx, frames, w, h, 3, stacks, None, None, NO_CARRY, caps=caps, vq=False)
        assert e.value.code == pkg.DCT3D_ENOSPC
        res.append(e.value.total_bits)
    assert res[0] == res[1] == full


@pytest.mark.parametrize("depth", [8, 4])
def test_grey_frames_have_constant_chroma(pkg, gpu_ctx8, gpu_ctx4, depth):
    """R = G = B: Cb = Cr = 128 exactly, so streams 1 and 2 are the stream the grey call writes for a constant-128
    plane, and stream 0 the grey call's for the plane itself"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 61, 27, 2
    plane = pkg.synthetic.frames(w, h, stacks * depth, seed=SEED, kind="ramp")
    flat = ctx.encode_eg_frames(np.full_like(plane, 128))[0]
    luma = ctx.encode_eg_frames(plane)[0]
    with _on(ctx, pkg):
        got = ctx.encode_eg_frames(np.stack([plane] * 3, axis=-1))
    assert got == [luma, flat, flat]


# ---- 2: decode ----------------------------------------------------------------------------------------------------

_STREAMS = {}


def _streams_of(ctx, depth, w, h, stacks, source):
    """the mode-off encode (reference table) of (i) the transformed colour ramp, (ii) uniform planes as they are; made
    once per shape"""
    key = (depth, w, h, stacks, source)
    if key not in _STREAMS:
        fr = transformed("ramp", depth, w, h, stacks) if source == "ramp" else colour("uniform", depth, w, h, stacks)
        _STREAMS[key] = tuple(ctx.encode_eg_frames(fr))
    return _STREAMS[key]


def _decode_pair(ctx, pkg, streams, w, h, stacks, dev):
    """(frames, end bits, statistics) with the mode off and on, host or device entry point"""
    res = []
    for mode in (0, 1):
        with ctx_option(ctx, pkg.DCT3D_OPT_COLOUR, mode):
            if dev:
                out, eb, ok = decode_dev(ctx, streams, [0, 0, 0], w, h, 3, stacks, None, None, vq=False)
                assert ok, "a write outside the frames"
            else:
                out, eb = ctx.decode_eg_frames([b for b, _ in streams], w, h, stacks)
            res.append((out, eb, _stats(ctx)))
    return res


@pytest.mark.parametrize("source", ["ramp", "uniform"])
@pytest.mark.parametrize("w,h,stacks", SHAPES)
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_identity(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks, source):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    streams = _streams_of(ctx, depth, w, h, stacks, source)
    for dev in (False, True):
        (off, eb0, st0), (on, eb1, st1) = _decode_pair(ctx, pkg, streams, w, h, stacks, dev)
        if source == "uniform" and w * h > 1:
            # (a frame of one pixel has too few samples for this; every other shape must show the clamp at work)
            pre = pkg.ycbcr_to_rgb_unclamped(off).reshape(-1, 3)
            assert (pre.min(axis=0) < 0).all() and (pre.max(axis=0) > 255).all(), (pre.min(axis=0), pre.max(axis=0))
        assert np.array_equal(on, pkg.ycbcr_to_rgb(off))
        assert eb1 == eb0 == [t for _, t in streams] and st1 == st0


@pytest.mark.parametrize("option,value", [("DCT3D_OPT_DEC_MARGIN", 0.45), ("DCT3D_OPT_EG_FORCE_RETRY", 1),
                                          ("DCT3D_OPT_EG_NO_RESOLVE", 1)])
@pytest.mark.parametrize("w,h,stacks", [(24, 16, 5), (32, 16, 2), (61, 27, 2)])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_identity_under_the_options(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks, option, value):
    """a margin that sends nearly every lane through the exact replay, and the front's skip-and-rerun path"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    for source in ("ramp", "uniform"):
        streams = _streams_of(ctx, depth, w, h, stacks, source)
        with ctx_option(ctx, getattr(pkg, option), value):
            (off, eb0, st0), (on, eb1, st1) = _decode_pair(ctx, pkg, streams, w, h, stacks, True)
        if option == "DCT3D_OPT_DEC_MARGIN":
            assert 2 * st0[1] > st0[0], "the margin must flag most lanes on the reference side"
        assert np.array_equal(on, pkg.ycbcr_to_rgb(off)) and eb1 == eb0 and st1 == st0


# ---- 3: the per-stack table calls ------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,stacks", [(24, 16, 5), (61, 27, 2)])
@pytest.mark.parametrize("depth", [8, 4])
def test_vq_calls(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    pal = np.stack([pkg.quant_table(5, depth), pkg.quant_table(12, depth)]).astype(np.int32)
    m = (np.arange(stacks) % 2).astype(np.uint8)
    for kind in ("ramp", "uniform"):
        fr, tf = colour(kind, depth, w, h, stacks), transformed(kind, depth, w, h, stacks)
        want_h = ctx.encode_eg_frames_vq(tf, pal, m)
        st_h = _stats(ctx)
        want_d, ok = encode_dev(ctx, tf, w, h, 3, stacks, pal, m, CARRY)
        st_d = _stats(ctx)
        assert ok and want_h != ctx.encode_eg_frames(tf)  # (the second table is in use)
        with _on(ctx, pkg):
            assert ctx.encode_eg_frames_vq(fr, pal, m) == want_h and _stats(ctx) == st_h
            got_d, ok = encode_dev(ctx, fr, w, h, 3, stacks, pal, m, CARRY)
            assert ok and got_d == want_d and _stats(ctx) == st_d
        # decode: the streams just made (the ramp's are the transformed frames', the uniform's taken as they are)
        streams = want_h if kind == "ramp" else ctx.encode_eg_frames_vq(fr, pal, m)
        off_h, eb0 = ctx.decode_eg_frames_vq([b for b, _ in streams], w, h, stacks, pal, m)
        off_d, ebd0, ok0 = decode_dev(ctx, streams, [0, 0, 0], w, h, 3, stacks, pal, m)
        st0 = _stats(ctx)
        with _on(ctx, pkg):
            on_h, eb1 = ctx.decode_eg_frames_vq([b for b, _ in streams], w, h, stacks, pal, m)
            on_d, ebd1, ok1 = decode_dev(ctx, streams, [0, 0, 0], w, h, 3, stacks, pal, m)
            st1 = _stats(ctx)
        assert ok0 and ok1 and np.array_equal(off_h, off_d)
        assert np.array_equal(on_h, pkg.ycbcr_to_rgb(off_h)) and np.array_equal(on_d, pkg.ycbcr_to_rgb(off_d))
        assert eb1 == eb0 == ebd0 == ebd1 == [t for _, t in streams] and st1 == st0


# ---- 4: the rate probe ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ramp", "uniform"])
@pytest.mark.parametrize("w,h,stacks", SHAPES)
@pytest.mark.parametrize("depth", [8, 4])
def test_rate_identity(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, stacks, kind):
    """four tables in one call: bits, cube bits and n_flagged equal the mode-off probe's on the transformed frames"""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, tf = colour(kind, depth, w, h, stacks), transformed(kind, depth, w, h, stacks)
    tabs = [pkg.quant_table(q, depth) for q in (5, 1, 12, 64)]
    wp, hp = pkg.padded_size(w, h)
    n = 4 * stacks * 3 * (wp // 8) * (hp // 8) * 2

    def dev(frames):
        buf, mid = qc.banded(torch, n, 0xA5)
        bits = ctx.rate_frames_dev(torch.from_numpy(np.array(frames)).cuda(), w, h, 3, stacks, tabs, mid)
        st = _stats(ctx)
        cubes, intact = qc.bands_intact(buf, n, 0xA5)
        assert intact, "a write outside d_cube_bits"
        return bits, cubes.copy(), st

    want_bits, want_cubes, want_st = dev(tf)
    want_host = ctx.rate_frames(tf, tabs)
    host_st = _stats(ctx)
    if (w, h, stacks) == FOLD_SHAPE and kind == "ramp":
        assert want_st[1] > 0
    with _on(ctx, pkg):
        bits, cubes, st = dev(fr)
        host = ctx.rate_frames(fr, tabs)
        assert _stats(ctx) == host_st
    assert np.array_equal(bits, want_bits) and np.array_equal(cubes, want_cubes) and st == want_st
    assert np.array_equal(host, want_host) and np.array_equal(host, bits)
    # and the probe prices what the encode writes (the context's table is the first of the four)
    with _on(ctx, pkg):
        tb = [t for _, t in ctx.encode_eg_frames(fr)]
    assert bits[0].sum(axis=0).tolist() == tb


# ---- 5: refusals ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [8, 4])
def test_refusals_and_the_call_after(pkg, gpu_ctx8, gpu_ctx4, depth):
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 13, 11, 3
    fr, tf = colour("ramp", depth, w, h, stacks), transformed("ramp", depth, w, h, stacks)
    fr8 = colour("ramp", depth, 16, 8, 1)
    want = ctx.encode_eg_frames(tf)
    q = ctx.encode_frames(fr)
    q8 = ctx.encode_stacks_rgb(fr8)
    d_fr, d_fr8 = torch.from_numpy(np.array(fr)).cuda(), torch.from_numpy(np.array(fr8)).cuda()
    d_q, d_q8 = torch.from_numpy(q).cuda(), torch.from_numpy(q8).cuda()
    d_sse = torch.zeros(stacks * 3 * 4, dtype=torch.int32, device="cuda")
    streams = [b for b, _ in want]
    E = pkg.DCT3D_EINVAL

    def refused(f, *a, **k):
        before = _stats(ctx)
        with pytest.raises(pkg.Dct3dError) as e:
            f(*a, **k)
        assert e.value.code == E, f.__name__
        ctx.synchronize()
        # nothing was launched (the statistics are the last good call's) and the next call is right
        assert _stats(ctx) == before, f.__name__
        assert ctx.encode_eg_frames(fr) == want, f.__name__

    for bad in (2, 3, 0.5):
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.set_option(pkg.DCT3D_OPT_COLOUR, bad)
        assert e.value.code == E
        assert ctx.encode_eg_frames(tf) == want  # the mode is still off
    with _on(ctx, pkg):
        assert ctx.encode_eg_frames(fr) == want
        # the int32 raster calls on packed frames
        refused(ctx.encode_frames, fr)
        refused(ctx.decode_frames, q, w, h, stacks, 3)
        refused(ctx.encode_frames_dev, d_fr, w, h, 3, stacks, d_q)
        refused(ctx.decode_frames_dev, d_q, w, h, 3, stacks, d_fr)
        refused(ctx.encode_stacks_rgb, fr8)
        refused(ctx.decode_stacks_rgb, q8, 16, 8, 1)
        refused(ctx.encode_stacks_rgb_dev, d_fr8, 16, 8, 1, d_q8)
        refused(ctx.decode_stacks_rgb_dev, d_q8, 16, 8, 1, d_fr8)
        # the distortion probe on packed frames
        refused(ctx.distortion_frames, fr)
        refused(ctx.distortion_frames_dev, d_fr, w, h, 3, stacks, None, d_sse)
        # the stream calls through the int32 intermediate
        with ctx_option(ctx, pkg.DCT3D_OPT_EG_TWO_STEP, 1):
            for f, a in ((ctx.encode_eg_frames, (fr,)), (ctx.decode_eg_frames, (streams, w, h, stacks)),
                         (ctx.decode_eg_frames_dev, ([d_fr] * 3, [len(b) for b in streams], [0] * 3, w, h, stacks, d_fr)),
                         (ctx.encode_eg_frames_dev, (d_fr, w, h, 3, stacks, [d_q] * 3, [1024] * 3))):
                with pytest.raises(pkg.Dct3dError) as e:
                    f(*a)
                assert e.value.code == E, f.__name__
        assert ctx.encode_eg_frames(fr) == want
        assert np.array_equal(fr, d_fr.cpu().numpy()) and np.array_equal(q, d_q.cpu().numpy())  # nothing was written
    # the grey calls still work with the mode on, and give the bytes of the mode off
    grey = np.ascontiguousarray(fr[..., 1])
    grey8 = np.ascontiguousarray(fr8[..., 1])
    g_stream, g_q, g_sse = ctx.encode_eg_frames(grey), ctx.encode_frames(grey), ctx.distortion_frames(grey)
    g8_stream, g_rate = ctx.encode_eg(grey8), ctx.rate_frames(grey)
    g_out = ctx.decode_eg_frames([g_stream[0][0]], w, h, stacks)
    with _on(ctx, pkg):
        assert ctx.encode_eg_frames(grey) == g_stream and np.array_equal(ctx.encode_frames(grey), g_q)
        assert np.array_equal(ctx.distortion_frames(grey), g_sse) and np.array_equal(ctx.rate_frames(grey), g_rate)
        assert ctx.encode_eg(grey8) == g8_stream  # (multiples of 8: handed to the grey stream call as before)
        assert ctx.encode_eg_frames(grey8) == [g8_stream]
        got = ctx.decode_eg_frames([g_stream[0][0]], w, h, stacks)
        assert np.array_equal(got[0], g_out[0]) and got[1] == g_out[1]
        with ctx_option(ctx, pkg.DCT3D_OPT_EG_TWO_STEP, 1):  # grey through the int32 cubes: no colour stage needed
            assert ctx.encode_eg_frames(grey) == g_stream
    # the raster calls work again once the mode is off
    assert np.array_equal(ctx.encode_frames(fr), q)


# ---- 6: the codec's ycc=1 ---------------------------------------------------------------------------------------------

def _cli(pkg, *args, env=None):
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


SUFFIXES = (".red", ".green", ".blue")


def _files(tmp_path, name):
    return [(tmp_path / (name + s)).read_bytes() for s in SUFFIXES]


def _cli_case(tmp_path, depth):
    """the frames file, the transformed frames file and the common arguments of a 61 x 27 clip of 2 stacks"""
    w, h, stacks = 61, 27, 2
    fr, tf = colour("ramp", depth, w, h, stacks), transformed("ramp", depth, w, h, stacks)
    raw, traw = tmp_path / "in.rgb", tmp_path / "t.rgb"
    fr.tofile(raw)
    tf.tofile(traw)
    return fr, raw, traw, (w, h, stacks * depth, 1, depth)


@pytest.mark.parametrize("depth", [8, 4])
def test_cli_encode(pkg, tmp_path, depth):
    """encode_rgb ... ycc=1 on a frames file == encode_rgb without it on the transformed file, byte for byte (beside
    q=, and through the environment variable)"""
    import os
    fr, raw, traw, geo = _cli_case(tmp_path, depth)
    _cli(pkg, "encode_rgb", raw, tmp_path / "on", *geo, "q=3", "ycc=1")
    _cli(pkg, "encode_rgb", traw, tmp_path / "off", *geo, "q=3")
    _cli(pkg, "encode_rgb", raw, tmp_path / "env", *geo, "q=3", env=dict(os.environ, DCT3D_CODEC_YCC="1"))
    assert _files(tmp_path, "on") == _files(tmp_path, "off") == _files(tmp_path, "env")
    assert all(len(b) > 0 for b in _files(tmp_path, "on"))


@pytest.mark.parametrize("depth", [8, 4])
def test_cli_decode(pkg, tmp_path, depth):
    """decode_rgb ... ycc=1 == ycbcr_to_rgb of the plain decode of the same files"""
    fr, raw, traw, geo = _cli_case(tmp_path, depth)
    _cli(pkg, "encode_rgb", raw, tmp_path / "on", *geo, "ycc=1")
    _cli(pkg, "decode_rgb", tmp_path / "on", tmp_path / "dec_on.rgb", *geo, "ycc=1")
    _cli(pkg, "decode_rgb", tmp_path / "on", tmp_path / "dec_off.rgb", *geo)
    on = np.fromfile(tmp_path / "dec_on.rgb", np.uint8).reshape(fr.shape)
    off = np.fromfile(tmp_path / "dec_off.rgb", np.uint8).reshape(fr.shape)
    assert np.array_equal(on, pkg.ycbcr_to_rgb(off)) and not np.array_equal(on, off)


@pytest.mark.parametrize("depth", [8, 4])
def test_cli_rate(pkg, tmp_path, depth):
    """rate=... ycc=1 prints a q whose encode is the file q=<n> ycc=1 writes"""
    fr, raw, traw, geo = _cli_case(tmp_path, depth)
    out = _cli(pkg, "encode_rgb", raw, tmp_path / "r", *geo, "rate=1.5", "ycc=1")
    m = re.search(r"^rate: q=(\d+) bits=(\d+)$", out, re.M)
    assert m, out
    _cli(pkg, "encode_rgb", raw, tmp_path / "rq", *geo, f"q={m.group(1)}", "ycc=1")
    assert _files(tmp_path, "r") == _files(tmp_path, "rq")


def test_cli_rate_with_a_quality_map(pkg, tmp_path):
    """rate= with qmap= under the option: the map and the files are those of the transformed frames without it"""
    fr, raw, traw, geo = _cli_case(tmp_path, 8)
    _cli(pkg, "encode_rgb", raw, tmp_path / "m", *geo, "rate=1.5", f"qmap={tmp_path / 'm.map'}", "ycc=1")
    _cli(pkg, "encode_rgb", traw, tmp_path / "mt", *geo, "rate=1.5", f"qmap={tmp_path / 'mt.map'}")
    assert (tmp_path / "m.map").read_text() == (tmp_path / "mt.map").read_text()
    assert _files(tmp_path, "m") == _files(tmp_path, "mt")
