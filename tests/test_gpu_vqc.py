"""GPU: a quantiser table per (stack, channel) in the fused stream calls (dct3d_*_eg_frames_vqc*), stated
as identities against the GREY _vq calls as they are.  Write col(k) for column k of the [n_stacks, 3] map, and plane k
for channel k of the frames (mode "planes"), of rgb_to_ycbcr(frames) ("ycc") or of rgb_to_ycbcr420(frames) ("420"):

  encode   on frames, under the map      ==  the grey _vq call on plane k under col(k), carry k: stream, total bits
  decode   from three streams            ==  the mode's composition (merge, ycbcr_to_rgb, ycbcr420_to_rgb) of the three
                                             grey _vq decodes, each under its col(k); end bits equal
  equal columns                          ==  the _vq call with that column, byte for byte

All comparisons are exact equalities.  The grey side is covered against the oracle by test_gpu_vq.py; at 61 x 45, mode
"planes", the streams and frames are compared with test_gpu_vq's numpy reference too (quant_common.ref_frames per stack
and channel under that entry's table, the Exp-Golomb bits written in numpy), so that not every check is one device path
against another.

Content: test_gpu_vq.frames -- stacks in turn ramp, uniform noise and flat -- 11 stacks, so that the last wave is
ragged; test_gpu_ycc.colour's uniform noise at the two shapes (2 stacks) where DESIGN 4q's emulation predicts open
coefficients in every plane.  Maps over palettes of 3, 8 and 32 tables: "differ" m[s, ch] = (s + 3 ch) % T (for T = 3,
where that has three equal columns, (s + ch) % T: the columns differ at every stack), "const" (three distinct tables,
one per channel), "runs3" (runs of 3 stacks, a phase per channel), "equal" (all columns s % T), and "fold" (the fold
shapes' own: see FOLD_OPEN).

Statistics: n_units is the sum over the three grey calls; the decode's n_flagged is their sum; the encode's equals the
sum where all three planes are ragged and is at least the sum elsewhere (a grey encode at multiples of 8 runs the
plain kernel, which reports no count: DESIGN 4q)."""
import contextlib
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import quant_common as qc
import test_gpu_vq as vq
from conftest import ctx_option
from test_gpu_ycc import CARRY, NO_CARRY, SEED, colour

pytestmark = pytest.mark.gpu

STACKS = vq.STACKS  # 11
LADDER = vq.LADDER
BAND = vq.BAND
MODES = ("planes", "ycc", "420")
SHAPES_444 = [(8, 8), (24, 24), (61, 45), (64, 64)]
SHAPES_420 = [(16, 16), (17, 16), (61, 27), (32, 32)]
FOLD_SHAPES = [(244, 54), (208, 80)]  # 2 stacks of test_gpu_ycc.colour("uniform")
# The open coefficients [Y, Cb, Cr] that cert_common.encode_open predicts on the CPU for the planes of those clips under
# palette(depth, 8) and table_map("fold", 8, 2) -- tables 0, 3 and 5 (q1, q2, ones), under which every stack of every
# plane has some: each chain's exact fold, and its replay's reload, runs under the chain's own column.  At 244 x 54 all
# planes are ragged and the grey runs must report exactly these; at 208 x 80 the grey runs are the plain kernel's.
FOLD_OPEN = {((244, 54), 8): [73, 84, 74], ((244, 54), 4): [59, 56, 59], ((208, 80), 8): [84, 63, 95], ((208, 80), 4): [68, 40, 66]}
# (tables in the palette, map)
COMBOS = [(3, "differ"), (3, "const"), (8, "differ"), (8, "equal"), (32, "runs3"), (32, "differ")]


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


@functools.lru_cache(maxsize=None)
def palette(depth, n):
    """n distinct tables from the pool test_gpu_vq.palette draws from, in its order (read-only)"""
    p = qc.pkg()
    t = qc.tables(depth)
    pool = [t[k] for k in ("q1", "all255", "seeded", "q2", "q12", "ones")]
    pool += [p.quant_table(q, depth) for q in LADDER if q not in (1, 2, 12)]
    pool += [p.quant_table(q, depth) for q in range(65, 65 + 32)]
    out = np.stack(pool[:n]).astype(np.int32)
    assert len({a.tobytes() for a in out}) == n
    out.setflags(write=False)
    return out


def table_map(kind, T, stacks=STACKS):
    s, ch = np.arange(stacks)[:, None], np.arange(3)[None, :]
    if kind == "differ":
        m = (s + (3 if T % 3 else 1) * ch) % T
        assert all(len(set(row)) == 3 for row in m.tolist()), "the columns differ at every stack"
    elif kind == "const":
        m = np.broadcast_to(np.array([0, T // 2, T - 1]), (stacks, 3))
        assert len(set(m[0].tolist())) == 3
    elif kind == "fold":
        m = np.array([0, 3, 5])[(s + ch) % 3]
    elif kind == "runs3":
        m = ((s + ch) // 3) % T
    else:
        m = np.broadcast_to(s % T, (stacks, 3))
    return np.ascontiguousarray(m, np.uint8)


@contextlib.contextmanager
def _mode(ctx, pkg, mode):
    if mode != "planes":
        ctx.set_option(pkg.DCT3D_OPT_COLOUR, pkg.DCT3D_COLOUR_YCBCR)
    if mode == "420":
        ctx.set_chroma(pkg.DCT3D_CHROMA_420)
    try:
        yield ctx
    finally:
        ctx.set_chroma(pkg.DCT3D_CHROMA_444)
        ctx.set_option(pkg.DCT3D_OPT_COLOUR, 0)


@functools.lru_cache(maxsize=None)
def clip(depth, w, h, stacks=STACKS):
    return colour("uniform", depth, w, h, stacks) if (w, h) in FOLD_SHAPES else vq.frames(depth, w, h, 3, stacks)


@functools.lru_cache(maxsize=None)
def planes(mode, depth, w, h, stacks=STACKS):
    """plane k of the clip under the mode, k = 0, 1, 2 (contiguous, read-only)"""
    p, fr = qc.pkg(), clip(depth, w, h, stacks)
    if mode == "420":
        out = list(p.rgb_to_ycbcr420(fr))
    else:
        t = fr if mode == "planes" else p.rgb_to_ycbcr(fr)
        out = [t[..., k] for k in range(3)]
    out = [np.ascontiguousarray(a) for a in out]
    for a in out:
        a.setflags(write=False)
    return out


def compose(pkg, mode, outs):
    if mode == "420":
        return pkg.ycbcr420_to_rgb(*outs)
    t = np.stack(outs, axis=-1)
    return t if mode == "planes" else pkg.ycbcr_to_rgb(t)


def _sizes(pkg, mode, w, h):
    return [(w, h)] + [pkg.chroma_size(w, h) if mode == "420" else (w, h)] * 2


def _caps(pkg, mode, w, h, depth, stacks):
    """a capacity per stream that holds any content: 4 bytes per value of the padded plane (a code has 27 bits at most)"""
    return [(-(-pw // 8) * 8) * (-(-ph // 8) * 8) * depth * stacks * 4 + 64 for pw, ph in _sizes(pkg, mode, w, h)]


def _stats(ctx):
    st = ctx.stats()
    return st["n_units"], st["n_flagged"]


def _ragged(size):
    return bool(size[0] % 8 or size[1] % 8)


def encode_dev(ctx, fr, w, h, stacks, pal, m, carry, caps, call="encode_eg_frames_vqc_dev"):
    """the three-channel device encode into banded buffers (test_gpu_vq.encode_dev with the call to make):
    (streams, bands intact); an error is raised again after the bands are checked"""
    import torch
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    bufs = [qc.banded(torch, c, 0xC3, BAND) for c in caps]
    err = None
    try:
        tb = getattr(ctx, call)(d_fr, w, h, 3, stacks, pal, m, [b[1] for b in bufs], caps, carry)
    except qc.pkg().Dct3dError as e:
        err, tb = e, [0] * 3
    ctx.synchronize()
    checked = [qc.bands_intact(buf, c, 0xC3, BAND) for (buf, _), c in zip(bufs, caps)]
    if err is not None:
        assert all(ok for _, ok in checked), "wrote outside its outputs"
        raise err
    return [(mid[:(t + 7) // 8].tobytes(), t) for (mid, _), t in zip(checked, tb)], all(ok for _, ok in checked)


def _dev_streams(streams):
    import torch
    d_s = []
    for b, _ in streams:
        a = np.zeros((len(b) + 3) // 4 * 4 + 4, np.uint8)
        a[:len(b)] = np.frombuffer(b, np.uint8)
        d_s.append(torch.from_numpy(a).cuda())
    return d_s


def decode_dev(ctx, streams, start_bits, w, h, stacks, pal, m, call="decode_eg_frames_vqc_dev"):
    """the three-channel device decode into a banded buffer, twice with different fills: (frames, end bits, intact)"""
    import torch
    d_s = _dev_streams(streams)
    n = stacks * ctx.bd * h * w * 3
    outs, ok, eb = [], True, None
    for fill in (0xA5, 0x5A):
        buf, mid = qc.banded(torch, n, fill, BAND)
        eb = getattr(ctx, call)(d_s, [len(b) for b, _ in streams], start_bits, w, h, stacks, pal, m, mid)
        ctx.synchronize()
        host, intact = qc.bands_intact(buf, n, fill, BAND)
        ok &= intact
        outs.append(host.reshape(stacks * ctx.bd, h, w, 3))
    assert np.array_equal(outs[0], outs[1]), "a byte of the output was not written"
    return outs[0], eb, ok


def grey_encodes(ctx, pkg, mode, depth, w, h, stacks, pal, m, carry):
    """the grey _vq encode of plane k under col(k) and carry k, host and device entry points (mode off):
    (host streams, device streams, statistics of the device calls)"""
    pl, sz, caps = planes(mode, depth, w, h, stacks), _sizes(pkg, mode, w, h), _caps(pkg, mode, w, h, depth, stacks)
    host, dev, st = [], [], []
    for k in range(3):
        col = np.ascontiguousarray(m[:, k])
        host.append(ctx.encode_eg_frames_vq(pl[k], pal, col, [carry[k]])[0])
        got, ok = vq.encode_dev(ctx, pl[k], sz[k][0], sz[k][1], 1, stacks, pal, col, [carry[k]], caps=[caps[k]])
        st.append(_stats(ctx))
        assert ok
        dev.append(got[0])
    assert host == dev
    return host, dev, st


def grey_decodes(ctx, pkg, mode, streams, start_bits, w, h, stacks, pal, m):
    """the grey _vq decode of stream k under col(k) (mode off): (planes, end bits, statistics)"""
    outs, ebs, sts = [], [], []
    for k, ((b, _), (pw, ph)) in enumerate(zip(streams, _sizes(pkg, mode, w, h))):
        out, eb = ctx.decode_eg_frames_vq([b], pw, ph, stacks, pal, np.ascontiguousarray(m[:, k]), [start_bits[k]])
        outs.append(out)
        ebs.append(eb[0])
        sts.append(_stats(ctx))
    return outs, ebs, sts


def _check_encode_stats(pkg, mode, w, h, got, grey):
    print("encode statistics: packed", got, "grey", grey)
    assert got[0] == sum(u for u, _ in grey)
    if all(_ragged(s) for s in _sizes(pkg, mode, w, h)):
        assert got[1] == sum(f for _, f in grey)
    else:
        assert got[1] >= sum(f for _, f in grey)


def _check_decode(pkg, mode, got, grey):
    (on, eb, st), (outs, ebs, sts) = got, grey
    assert np.array_equal(on, compose(pkg, mode, outs)), f"{(on != compose(pkg, mode, outs)).sum()} bytes differ"
    assert eb == ebs
    assert st == (sum(u for u, _ in sts), sum(f for _, f in sts)), (st, sts)


def _cases():
    out = []
    for mode in MODES:
        for w, h in (SHAPES_420 if mode == "420" else SHAPES_444):
            for T, kind in COMBOS:
                out.append((mode, w, h, STACKS, T, kind))
    for w, h in FOLD_SHAPES:
        out.append(("420", w, h, 2, 8, "fold"))
    return out


# ---- 1, 3, 4, 8: the identities ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,w,h,stacks,T,kind", _cases())
@pytest.mark.parametrize("depth", [8, 4])
def test_identities(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h, stacks, T, kind):
    """host and device entry points, non-zero carries that differ per channel: streams, totals, guard bands and
    statistics of the encode; frames, end bits and statistics of the decode of those streams"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, pal, m = clip(depth, w, h, stacks), palette(depth, T), table_map(kind, T, stacks)
    caps = _caps(pkg, mode, w, h, depth, stacks)
    want_h, want_d, st_grey = grey_encodes(ctx, pkg, mode, depth, w, h, stacks, pal, m, CARRY)
    if kind == "fold":
        print("grey encodes' folds per plane:", [f for _, f in st_grey], "predicted", FOLD_OPEN[((w, h), depth)])
    if kind == "fold" and (w, h) == FOLD_SHAPES[0]:  # (all planes ragged: the grey runs count their exact folds)
        assert [f for _, f in st_grey] == FOLD_OPEN[((w, h), depth)], "the grey runs must take the predicted folds"
    start = [cn for _, cn in CARRY]
    grey = grey_decodes(ctx, pkg, mode, want_h, start, w, h, stacks, pal, m)
    assert grey[1] == [t for _, t in want_h]
    quant_before = ctx.quant().copy()
    with _mode(ctx, pkg, mode):
        got_h = ctx.encode_eg_frames_vqc(fr, pal, m, CARRY)
        st_h = _stats(ctx)
        got_d, intact = encode_dev(ctx, fr, w, h, stacks, pal, m, CARRY, caps)
        st_d = _stats(ctx)
        assert intact, "the encode wrote outside its outputs"
        assert got_h == want_h and got_d == want_d
        out_h, eb_h = ctx.decode_eg_frames_vqc([b for b, _ in want_h], w, h, stacks, pal, m, start)
        dst_h = _stats(ctx)
        out_d, eb_d, intact = decode_dev(ctx, want_h, start, w, h, stacks, pal, m)
        dst_d = _stats(ctx)
        assert intact, "the decode wrote outside its output"
        if kind == "equal":  # every output is the _vq call's with that column
            col = np.ascontiguousarray(m[:, 0])
            assert ctx.encode_eg_frames_vq(fr, pal, col, CARRY) == got_h
            assert encode_dev(ctx, fr, w, h, stacks, pal, col, CARRY, caps, call="encode_eg_frames_vq_dev") == (got_d, True)
            vq_h, vq_eb = ctx.decode_eg_frames_vq([b for b, _ in want_h], w, h, stacks, pal, col, start)
            assert np.array_equal(vq_h, out_h) and vq_eb == eb_h
            vq_d, vq_eb, _ = decode_dev(ctx, want_h, start, w, h, stacks, pal, col, call="decode_eg_frames_vq_dev")
            assert np.array_equal(vq_d, out_d) and vq_eb == eb_d
    assert [t for _, t in got_h] != [0, 0, 0]
    _check_encode_stats(pkg, mode, w, h, st_h, st_grey)
    _check_encode_stats(pkg, mode, w, h, st_d, st_grey)
    if kind == "fold":
        assert st_h[1] == st_d[1] == sum(FOLD_OPEN[((w, h), depth)])
    _check_decode(pkg, mode, (out_h, eb_h, dst_h), grey)
    _check_decode(pkg, mode, (out_d, eb_d, dst_d), grey)
    assert np.array_equal(ctx.quant(), quant_before), "a vqc call changed the context's quantiser"


def test_one_channel_is_the_vq_call(pkg, gpu_ctx8):
    ctx, depth, (w, h) = gpu_ctx8, 8, (61, 45)
    fr, pal = vq.frames(depth, w, h, 1), palette(depth, 8)
    col = vq.stack_map("cycle", 8)
    want = ctx.encode_eg_frames_vq(fr, pal, col, CARRY[:1])
    assert ctx.encode_eg_frames_vqc(fr, pal, col[:, None], CARRY[:1]) == want
    a, ea = ctx.decode_eg_frames_vq([want[0][0]], w, h, STACKS, pal, col, [CARRY[0][1]])
    b, eb = ctx.decode_eg_frames_vqc([want[0][0]], w, h, STACKS, pal, col[:, None], [CARRY[0][1]])
    assert np.array_equal(a, b) and ea == eb


# ---- 2: the numpy reference -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ref_plane(depth, w, h, s, ch, table_bytes):
    """(q [cube][cs], the decoded plane) of stack s of channel ch under one table: quant_common.ref_frames on that
    grey stack alone, as test_gpu_vq._ref_stack takes it of a whole stack"""
    fr = vq.frames(depth, w, h, 3)
    q, out = qc.ref_frames(np.ascontiguousarray(fr[s * depth:(s + 1) * depth, :, :, ch]), np.frombuffer(table_bytes, np.int32), depth)
    return q.reshape(-1, 64 * depth), out


@functools.lru_cache(maxsize=None)
def reference(depth, w, h, T, kind):
    """(per-stack q [channel][cube][cs], the decoded frames) of vq.frames(depth, w, h, 3) coded plane by plane, stack s
    of channel ch under palette(depth, T)[map[s, ch]]"""
    pal, m = palette(depth, T), table_map(kind, T)
    per_q, outs = [], []
    for s in range(STACKS):
        ref = [_ref_plane(depth, w, h, s, ch, pal[m[s, ch]].tobytes()) for ch in range(3)]
        per_q.append(np.stack([q for q, _ in ref]))
        outs.append(np.stack([o for _, o in ref], axis=-1))
    out = np.concatenate(outs)
    out.setflags(write=False)
    return per_q, out


@pytest.mark.parametrize("T,kind", [(3, "differ"), (8, "differ"), (32, "runs3")])
@pytest.mark.parametrize("depth", [8, 4])
def test_planes_mode_equals_the_numpy_reference(pkg, gpu_ctx8, gpu_ctx4, depth, T, kind):
    ctx, (w, h) = _ctx(depth, gpu_ctx8, gpu_ctx4), (61, 45)
    fr, pal, m = clip(depth, w, h), palette(depth, T), table_map(kind, T)
    per_q, out_ref = reference(depth, w, h, T, kind)
    want = vq.ref_streams(per_q, depth, 3, CARRY)
    got_h = ctx.encode_eg_frames_vqc(fr, pal, m, CARRY)
    got_d, intact = encode_dev(ctx, fr, w, h, STACKS, pal, m, CARRY, _caps(pkg, "planes", w, h, depth, STACKS))
    assert intact
    for ch in range(3):
        assert vq._same_stream(got_h[ch], want[ch]) and vq._same_stream(got_d[ch], want[ch]), (ch, got_h[ch][1], want[ch][1])
    start = [cn for _, cn in CARRY]
    out_h, eb_h = ctx.decode_eg_frames_vqc([b for b, _ in want], w, h, STACKS, pal, m, start)
    out_d, eb_d, intact = decode_dev(ctx, want, start, w, h, STACKS, pal, m)
    assert intact and eb_h == eb_d == [t for _, t in want]
    assert np.array_equal(out_h, out_ref), f"{(out_h != out_ref).sum()} bytes differ (host)"
    assert np.array_equal(out_d, out_ref), f"{(out_d != out_ref).sum()} bytes differ (device)"


# ---- 3: streams no encoder of this map wrote, and the decode's rare paths ----------------------------------------------

_UNRELATED = {}


def unrelated_streams(ctx, pkg, mode, depth, w, h, stacks, pal, m):
    """grey _vq encodes of uniform planes that have nothing to do with each other, under the map's columns rotated
    (plane k under col(k + 1)): made once per case"""
    key = (mode, depth, w, h, stacks, pal.shape[0], m.tobytes())
    if key not in _UNRELATED:
        sz = _sizes(pkg, mode, w, h)
        _UNRELATED[key] = tuple(
            ctx.encode_eg_frames_vq(pkg.synthetic.frames(sz[k][0], sz[k][1], stacks * depth, seed=SEED + 104729 * (k + 1),
                                                         frame0=5 * k, kind="uniform"),
                                    pal, np.ascontiguousarray(m[:, (k + 1) % 3]))[0] for k in range(3))
    return _UNRELATED[key]


@pytest.mark.parametrize("option,value", [(None, 0), ("DCT3D_OPT_DEC_MARGIN", 0.45), ("DCT3D_OPT_EG_FORCE_RETRY", 1),
                                          ("DCT3D_OPT_EG_NO_RESOLVE", 1)])
@pytest.mark.parametrize("mode,w,h,stacks", [("planes", 8, 8, STACKS), ("ycc", 24, 24, STACKS), ("ycc", 61, 45, STACKS),
                                             ("planes", 64, 64, STACKS), ("420", 16, 16, STACKS), ("420", 61, 27, STACKS),
                                             ("420", 32, 32, STACKS), ("420", 244, 54, 2), ("420", 208, 80, 2)])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_of_unrelated_streams_and_under_the_options(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h, stacks, option, value):
    """the differing-columns map; a margin that sends most lanes through the exact replay (a replay under another
    channel's table would change bytes), and the front's skip-and-rerun paths"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    pal, m = palette(depth, 8), table_map("differ", 8, stacks)
    streams = unrelated_streams(ctx, pkg, mode, depth, w, h, stacks, pal, m)
    with contextlib.ExitStack() as es:
        if option:
            es.enter_context(ctx_option(ctx, getattr(pkg, option), value))
        grey = grey_decodes(ctx, pkg, mode, streams, [0, 0, 0], w, h, stacks, pal, m)
        with _mode(ctx, pkg, mode):
            out_h, eb_h = ctx.decode_eg_frames_vqc([b for b, _ in streams], w, h, stacks, pal, m)
            st_h = _stats(ctx)
            out_d, eb_d, intact = decode_dev(ctx, streams, [0, 0, 0], w, h, stacks, pal, m)
            st_d = _stats(ctx)
    assert intact and grey[1] == [t for _, t in streams]
    if option == "DCT3D_OPT_DEC_MARGIN":
        print("grey decodes (n_units, n_flagged):", grey[2])
        assert all(2 * f > u for u, f in grey[2]), "the margin must flag most lanes on the reference side"
        # the columns matter: plane 0 decoded under column 1 is another plane
        other, _ = ctx.decode_eg_frames_vq([streams[0][0]], w, h, stacks, pal, np.ascontiguousarray(m[:, 1]))
        assert not np.array_equal(other, grey[0][0])
    _check_decode(pkg, mode, (out_h, eb_h, st_h), grey)
    _check_decode(pkg, mode, (out_d, eb_d, st_d), grey)


# ---- 5: DCT3D_ENOSPC ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,w,h", [("ycc", 61, 45), ("420", 61, 27)])
@pytest.mark.parametrize("depth", [8, 4])
def test_enospc_only_the_middle_capacity_suffices(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, pal, m = clip(depth, w, h), palette(depth, 8), table_map("differ", 8)
    pl, sz = planes(mode, depth, w, h), _sizes(pkg, mode, w, h)
    cols = [np.ascontiguousarray(m[:, k]) for k in range(3)]
    full = [ctx.encode_eg_frames_vq(pl[k], pal, cols[k])[0][1] for k in range(3)]
    caps = [64, ((full[1] + 31) // 32) * 4 + 64, 64]
    grey = []
    for k in range(3):
        try:
            got, _ = vq.encode_dev(ctx, pl[k], sz[k][0], sz[k][1], 1, STACKS, pal, cols[k], NO_CARRY[:1], caps=[caps[k]])
            grey.append((pkg.DCT3D_OK, got[0][1]))
        except pkg.Dct3dError as e:
            grey.append((e.code, e.total_bits[0]))
    assert [c for c, _ in grey] == [pkg.DCT3D_ENOSPC, pkg.DCT3D_OK, pkg.DCT3D_ENOSPC]
    with _mode(ctx, pkg, mode):
        with pytest.raises(pkg.Dct3dError) as e:
            encode_dev(ctx, fr, w, h, STACKS, pal, m, NO_CARRY, caps)
        assert e.value.code == pkg.DCT3D_ENOSPC and e.value.total_bits == [t for _, t in grey] == full
        got, ok = encode_dev(ctx, fr, w, h, STACKS, pal, m, NO_CARRY, _caps(pkg, mode, w, h, depth, STACKS))
    assert ok and [t for _, t in got] == full


# ---- 6: a truncated stream ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [0, 2])
@pytest.mark.parametrize("mode,w,h", [("ycc", 61, 45), ("420", 61, 27)])
@pytest.mark.parametrize("depth", [8, 4])
def test_truncated_stream(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h, bad):
    """the code and end bits of the _vq call for the same fault; a sentinel-filled raster stays untouched; the next
    call is good"""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, pal, m = clip(depth, w, h), palette(depth, 8), table_map("differ", 8)
    col = np.ascontiguousarray(m[:, 0])

    def run(call, ss, mm):
        d_s = _dev_streams(ss)
        d_out = torch.full((STACKS * depth * h * w * 3,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises(pkg.Dct3dError) as e:
            getattr(ctx, call)(d_s, [len(b) for b, _ in ss], [0, 0, 0], w, h, STACKS, pal, mm, d_out)
        ctx.synchronize()
        return e.value.code, e.value.end_bits, bool((d_out == 0xA5).all().item())

    def cut(ss):
        out = list(ss)
        out[bad] = (ss[bad][0][:-1], ss[bad][1])  # truncated by a byte
        return out

    with _mode(ctx, pkg, mode):
        streams = ctx.encode_eg_frames_vqc(fr, pal, m)
        vq_streams = ctx.encode_eg_frames_vq(fr, pal, col)
        good = decode_dev(ctx, streams, [0, 0, 0], w, h, STACKS, pal, m)
        code_vq, eb_vq, clean_vq = run("decode_eg_frames_vq_dev", cut(vq_streams), col)
        code, eb, clean = run("decode_eg_frames_vqc_dev", cut(streams), m)
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.decode_eg_frames_vqc([b for b, _ in cut(streams)], w, h, STACKS, pal, m)
        assert e.value.code == code
        again = decode_dev(ctx, streams, [0, 0, 0], w, h, STACKS, pal, m)
    assert code == code_vq == pkg.DCT3D_ENODATA and clean and clean_vq
    assert eb == [0 if k == bad else streams[k][1] for k in range(3)]
    assert eb_vq == [0 if k == bad else vq_streams[k][1] for k in range(3)]
    assert good[2] and again[2] and np.array_equal(again[0], good[0]) and again[1] == good[1] == [t for _, t in streams]


# ---- 7: DCT3D_EINVAL, and the call after -----------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_einval_and_the_call_after(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = (61, 27) if mode == "420" else (61, 45)
    fr, pal, m = clip(depth, w, h), palette(depth, 8), table_map("differ", 8)
    caps = _caps(pkg, mode, w, h, depth, STACKS)
    with _mode(ctx, pkg, mode):
        want = ctx.encode_eg_frames_vqc(fr, pal, m)
        out_ref, _ = ctx.decode_eg_frames_vqc([b for b, _ in want], w, h, STACKS, pal, m)

        def good():
            got, intact = encode_dev(ctx, fr, w, h, STACKS, pal, m, NO_CARRY, caps)
            assert intact and got == want
            out, eb, intact = decode_dev(ctx, want, [0, 0, 0], w, h, STACKS, pal, m)
            assert intact and np.array_equal(out, out_ref) and eb == [t for _, t in want]
            assert ctx.encode_eg_frames_vqc(fr, pal, m) == want

        def einval(tables, tmap):
            for call in (lambda: ctx.encode_eg_frames_vqc(fr, tables, tmap),
                         lambda: encode_dev(ctx, fr, w, h, STACKS, tables, tmap, NO_CARRY, caps),
                         lambda: ctx.decode_eg_frames_vqc([b for b, _ in want], w, h, STACKS, tables, tmap),
                         lambda: decode_dev(ctx, want, [0, 0, 0], w, h, STACKS, tables, tmap)):
                with pytest.raises(pkg.Dct3dError) as e:
                    call()
                assert e.value.code == pkg.DCT3D_EINVAL
            good()

        for s, ch in ((0, 0), (STACKS - 1, 2), (5, 1)):
            bad = m.copy()
            bad[s, ch] = 8
            einval(pal, bad)                                       # an entry == n_tables
        for step in (0, 256, -1):
            t = pal.copy()
            t[5, 3] = step
            einval(t, m)                                           # a step outside [1, 255]
        einval(np.concatenate([palette(depth, 32), pal[:1]]), m)   # 33 tables
        einval(None, m)
        einval(pal, None)
        einval(pal, m[:, 0])                                       # a map per stack
        einval(pal, m[:-1])                                        # a row too few
        einval(pal, np.ascontiguousarray(m.T))                     # [3, n_stacks]
        with ctx_option(ctx, pkg.DCT3D_OPT_EG_TWO_STEP, 1):        # refused, not ignored
            einval_two = []
            for call in (lambda: ctx.encode_eg_frames_vqc(fr, pal, m),
                         lambda: decode_dev(ctx, want, [0, 0, 0], w, h, STACKS, pal, m)):
                with pytest.raises(pkg.Dct3dError) as e:
                    call()
                einval_two.append(e.value.code)
            assert einval_two == [pkg.DCT3D_EINVAL] * 2
        good()
    if mode == "420":  # 4:2:0 on but the colour transform off: refused for three channels
        ctx.set_chroma(pkg.DCT3D_CHROMA_420)
        try:
            for call in (lambda: ctx.encode_eg_frames_vqc(fr, pal, m),
                         lambda: encode_dev(ctx, fr, w, h, STACKS, pal, m, NO_CARRY, caps),
                         lambda: ctx.decode_eg_frames_vqc([b for b, _ in want], w, h, STACKS, pal, m),
                         lambda: decode_dev(ctx, want, [0, 0, 0], w, h, STACKS, pal, m)):
                with pytest.raises(pkg.Dct3dError) as e:
                    call()
                assert e.value.code == pkg.DCT3D_EINVAL
        finally:
            ctx.set_chroma(pkg.DCT3D_CHROMA_444)
        with _mode(ctx, pkg, mode):
            good()


# ---- 9: a host-pointer decode of more than one pipeline chunk ------------------------------------------------------------

@pytest.mark.parametrize("mode,w,h,stacks", [("ycc", 64, 64, 3), ("420", 32, 32, 5)])
@pytest.mark.parametrize("depth", [8, 4])
def test_host_decode_in_several_chunks(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h, stacks):
    """The host-pointer decode moves the frames in chunks of whole stacks: at most ceil(n_stacks / 2) a chunk
    (chunk_stacks_for), rounded up to the stack count that puts a chunk's first cube on a group of 2,048 values in every
    plane (eg_stack_align: 1 for these planes' 64, 16 and 4 cubes a stack at 8x8x8; 2 for the 4-cube chroma plane at
    8x8x4).  So 3 stacks at 64 x 64 go as 2 + 1 and 5 stacks at 32 x 32 under 4:2:0 as 3 + 2 (8x8x8) or 4 + 1 (8x8x4):
    the smallest clips whose second chunk starts at a stack s0 > 1 in every case, where row s0 of the map, entry
    3 s0 + ch, must be the one in use.  The device-pointer decode takes one range: both must agree."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, pal, m = clip(depth, w, h, stacks), palette(depth, 8), table_map("differ", 8, stacks)
    want_h, _, _ = grey_encodes(ctx, pkg, mode, depth, w, h, stacks, pal, m, NO_CARRY)
    grey = grey_decodes(ctx, pkg, mode, want_h, [0, 0, 0], w, h, stacks, pal, m)
    with _mode(ctx, pkg, mode):
        assert ctx.encode_eg_frames_vqc(fr, pal, m) == want_h
        out_h, eb_h = ctx.decode_eg_frames_vqc([b for b, _ in want_h], w, h, stacks, pal, m)
        st_h = _stats(ctx)
        out_d, eb_d, intact = decode_dev(ctx, want_h, [0, 0, 0], w, h, stacks, pal, m)
    assert intact and np.array_equal(out_h, out_d) and eb_h == eb_d
    _check_decode(pkg, mode, (out_h, eb_h, st_h), grey)
    # the rows matter: the last stack decoded under the first stack's row is another stack
    m2 = m.copy()
    m2[stacks - 1] = m[0]
    with _mode(ctx, pkg, mode):
        other, _ = ctx.decode_eg_frames_vqc([b for b, _ in want_h], w, h, stacks, pal, m2)
    assert np.array_equal(other[:(stacks - 1) * depth], out_h[:(stacks - 1) * depth]) and not np.array_equal(other, out_h)


# ---- 10: the codec's qmap3= ---------------------------------------------------------------------------------------------

def _cli(pkg, *args, env=None):
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _files(tmp_path, name):
    return [(tmp_path / (name + s)).read_bytes() for s in (".red", ".green", ".blue")]


def test_cli_rate_with_a_three_column_map(pkg, gpu_ctx8, tmp_path):
    """encode_rgb ycc=1 chroma=420 rate= qmap3= cq=2: the written map is pick_stack_channel_qualities on rate_frames of
    the same frames, the printed bits are the summed total_bits of the Python encode under it, an encode that reads
    the map writes the same files, and decode_rgb with the map gives the Python decode's frames"""
    ctx, depth = gpu_ctx8, 8
    w, h, stacks, bpp = 64, 48, 6, 3.0
    fr = np.ascontiguousarray(vq.codec_clip(3)[:, :h])  # stacks alternate flat and noise
    raw, mapf = tmp_path / "in.rgb", tmp_path / "m.map"
    fr.tofile(raw)
    geo = (w, h, stacks * depth, 1, depth)
    tok = ("ycc=1", "chroma=420")
    env = dict(os.environ, DCT3D_CODEC_BATCH="4")  # batches of 4 and 2 stacks: each takes its own rows of the map
    out = _cli(pkg, "encode_rgb", raw, tmp_path / "m", *geo, *tok, f"rate={bpp}", f"qmap3={mapf}", "cq=2", env=env)
    got = re.search(r"^qmap3: stacks=(\d+) bits=(\d+)$", out, re.M)
    assert got and int(got.group(1)) == stacks, out
    pal = np.stack([pkg.quant_table(q, depth) for q in LADDER]).astype(np.int32)
    with _mode(ctx, pkg, "420"):
        bits = ctx.rate_frames(fr, list(pal))
    want_map = pkg.pick_stack_channel_qualities(bits, LADDER, bpp * w * h * depth, 2)
    assert len({t[0] for t in want_map}) >= 2 and any(t[0] != t[1] for t in want_map), want_map  # a condition on the content
    assert mapf.read_text() == "".join("%d %d %d\n" % t for t in want_map)
    idx = np.array([[LADDER.index(q) for q in t] for t in want_map], np.uint8)
    with _mode(ctx, pkg, "420"):
        streams = ctx.encode_eg_frames_vqc(fr, pal, idx)
        want, _ = ctx.decode_eg_frames_vqc([b for b, _ in streams], w, h, stacks, pal, idx)
    assert int(got.group(2)) == sum(t for _, t in streams) == sum(int(bits[idx[s, ch], s, ch]) for s in range(stacks) for ch in range(3))
    _cli(pkg, "encode_rgb", raw, tmp_path / "r", *geo, *tok, f"qmap3={mapf}", env=env)
    assert _files(tmp_path, "m") == _files(tmp_path, "r")
    _cli(pkg, "decode_rgb", tmp_path / "m", tmp_path / "dec.rgb", *geo, *tok, f"qmap3={mapf}", env=env)
    assert np.array_equal(np.fromfile(tmp_path / "dec.rgb", np.uint8).reshape(fr.shape), want)
    # the map through the environment: the same decode; three equal columns: the qmap= files
    _cli(pkg, "decode_rgb", tmp_path / "m", tmp_path / "env.rgb", *geo, *tok, env=dict(env, DCT3D_CODEC_QMAP3=f"qmap3={mapf}"))
    assert (tmp_path / "env.rgb").read_bytes() == (tmp_path / "dec.rgb").read_bytes()
    (tmp_path / "one.map").write_text("".join("%d\n" % t[0] for t in want_map))
    (tmp_path / "three.map").write_text("".join("%d %d %d\n" % ((t[0],) * 3) for t in want_map))
    _cli(pkg, "encode_rgb", raw, tmp_path / "a", *geo, *tok, f"qmap={tmp_path / 'one.map'}", env=env)
    _cli(pkg, "encode_rgb", raw, tmp_path / "b", *geo, *tok, f"qmap3={tmp_path / 'three.map'}", env=env)
    assert _files(tmp_path, "a") == _files(tmp_path, "b")
