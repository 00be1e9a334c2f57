"""GPU: the fused stream calls for frames of any size and packed RGB24 (dct3d_encode_eg_frames* /
dct3d_decode_eg_frames*): raster -> one Exp-Golomb stream per channel and back, no int32 intermediate.

Every expectation comes from the Java-semantics oracle: q = plan.encode_q of the edge-padded raster (planes via
test_gpu_rgb.planar for RGB), channel ch's blocks q.reshape(stacks, channels, C, -1)[:, ch] through
test_gpu_eg._expected for stream ch, and the cropped plan.decode_q for the frames (test_gpu_edge._oracle).
Bit-exact comparisons only.

Shapes (w, h, stacks): one cube per stack, w < 8 and h < 8, a partial segment and group | odd stride, 12 cubes = a
full segment + a ragged one | right edge only | bottom edge only | 18 cubes per stack: stacks begin inside a segment
and inside a decode group | 32 cubes per stack | 360 cubes: more than one decode block at both depths, so the
look-ahead groups run | aligned: grey hands over, RGB takes the (3, 0) kernels and the block stores | RGB only: a
full block inside one block-row."""
import filecmp
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ctx_option
from test_gpu_edge import GUARD, SHAPES as EDGE_SHAPES, _banded, _case, _ctx, _oracle, _pkg, _rare_case
from test_gpu_eg import _expected
from test_gpu_rgb import rgb_content

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3, 2), (13, 11, 3), (12, 16, 2), (16, 12, 2), (44, 20, 3), (61, 27, 2), (93, 45, 5), (64, 64, 2),
          (128, 16, 1)]
CASES = [(ch, s) for ch in (1, 3) for s in SHAPES if not (ch == 1 and s == (128, 16, 1))]
CARRY = [(0x00, 0), (0xA0, 3), (0xFE, 7)]  # per channel; as decode input: start bits 0 / 3 / 7


@functools.lru_cache(maxsize=None)
def _content(depth, channels, w, h, stacks):
    """(frames, oracle q of the padded raster, oracle's cropped decode): test_gpu_edge's case where it has one"""
    if channels == 3 or (w, h, stacks) in EDGE_SHAPES:
        return _case(depth, channels, w, h, stacks)
    fr = _pkg().synthetic.frames(w, h, stacks * depth, kind="ramp")
    q, out = _oracle(depth, fr)
    for a in (fr, q, out):
        a.setflags(write=False)
    return fr, q, out


def _streams_of(q, depth, channels, stacks, carry):
    import oracle
    blocks = q.reshape(stacks, channels, -1, 64 * depth)
    return tuple(_expected(oracle, _pkg(), np.ascontiguousarray(blocks[:, ch]), depth, *carry[ch]) for ch in range(channels))


@functools.lru_cache(maxsize=None)
def _streams(depth, channels, w, h, stacks):
    """the oracle's stream (bytes, total bits) of each channel, continuing CARRY[ch]"""
    _, q, _ = _content(depth, channels, w, h, stacks)
    return _streams_of(q, depth, channels, stacks, CARRY)


def _words(bits):
    return (bits + 31) // 32 * 4


def _encode_dev(ctx, fr, exp, junk, lead, torch, carry=CARRY, short=None, sync=True):
    """encode_eg_frames_dev with the input inside a larger tensor (`junk` around it, `lead` bytes before) and each
    channel's output (its words + 8 bytes, prefilled with 0x5A) between two 256-byte bands of 0xA5.  short: a
    channel whose capacity is one word short.  Returns (call, finish): finish() checks the bands and returns
    [(stream bytes, total bits, the region)] per channel."""
    channels = 1 if fr.ndim == 3 else 3
    f, h, w = fr.shape[:3]
    _, imid = _banded(fr.size, junk, torch, lead)  # (the view keeps the buffer alive)
    imid.copy_(torch.from_numpy(fr.reshape(-1).copy()))
    bufs, caps = [], []
    for ch in range(channels):
        cap = _words(exp[ch][1]) + 8 if ch != short else _words(exp[ch][1]) - 4
        obuf, omid = _banded(cap, 0xA5, torch)
        omid.fill_(0x5A)
        bufs.append((obuf, omid))
        caps.append(cap)
    torch.cuda.synchronize()

    def call():
        return ctx.encode_eg_frames_dev(imid.data_ptr(), w, h, channels, f // ctx.bd, [m.data_ptr() for _, m in bufs], caps,
                                        carry[:channels])

    def finish(tb):
        ctx.synchronize()
        res = []
        for ch in range(channels):
            host = bufs[ch][0].cpu().numpy()
            assert (host[:GUARD] == 0xA5).all() and (host[GUARD + caps[ch]:] == 0xA5).all(), f"channel {ch} wrote outside"
            region = host[GUARD:GUARD + caps[ch]]
            res.append((region[:(tb[ch] + 7) // 8].tobytes(), tb[ch], region))
        return res

    if not sync:
        return call, finish
    return finish(call())


def _check_streams(got, exp):
    for ch, ((g, tb, region), (e, ebits)) in enumerate(zip(got, exp)):
        assert tb == ebits, f"channel {ch}: {tb} bits, expected {ebits}"
        assert g == e, f"channel {ch}: the stream differs"
        assert not region[len(e):_words(ebits)].any(), f"channel {ch}: no zero padding to the word"


def _device_streams(exp, torch, cut=None, zero_run=None):
    """each channel's stream in a device tensor (4-byte aligned, a few spare bytes); cut: a channel truncated by a
    byte; zero_run: a channel with 48 zero bits from byte 10"""
    ts, nb = [], []
    for ch, (b, _) in enumerate(exp):
        a = np.frombuffer(b, np.uint8).copy()
        if ch == zero_run:
            a[10:16] = 0
        n = a.size - (1 if ch == cut else 0)
        pad = np.zeros((a.size + 11) // 4 * 4, np.uint8)
        pad[:n] = a[:n]
        ts.append(torch.from_numpy(pad).cuda())
        nb.append(n)
    return ts, nb


def _decode_dev(ctx, exp, shape, torch, lead=GUARD, sync=True):
    """decode_eg_frames_dev from the oracle's streams (start bits = CARRY's) into a byte buffer prefilled with 0xA5
    (and with 0x5A: a byte that kept its fill cannot equal both), 256-byte bands around it; checks the end bits
    and the bands, returns the frames"""
    channels = len(exp)
    f, h, w = shape[:3]
    n = int(np.prod(shape))
    ts, nb = _device_streams(exp, torch)
    sb = [CARRY[ch][1] for ch in range(channels)]
    outs = []
    for fill in (0xA5, 0x5A):
        obuf, omid = _banded(n, fill, torch, lead)
        eb = ctx.decode_eg_frames_dev(ts, nb, sb, w, h, f // ctx.bd, omid.data_ptr())
        ctx.synchronize()
        assert eb == [bits for _, bits in exp]
        host = obuf.cpu().numpy()
        assert (host[:lead] == fill).all() and (host[lead + n:] == fill).all(), "decode wrote outside its output"
        outs.append(host[lead:lead + n].reshape(shape))
    assert np.array_equal(outs[0], outs[1]), "a byte of the output was not written"
    return outs[0]


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("channels,shape", CASES)
@pytest.mark.parametrize("depth", [8, 4])
def test_streams_and_frames_match_oracle(pkg, gpu_ctx8, gpu_ctx4, depth, channels, shape, entry):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = shape
    fr, _, out_ref = _content(depth, channels, w, h, stacks)
    exp = _streams(depth, channels, w, h, stacks)
    if entry == "host":
        got = ctx.encode_eg_frames(fr, CARRY[:channels])
        for ch in range(channels):
            assert got[ch][1] == exp[ch][1], f"channel {ch}: {got[ch][1]} bits, expected {exp[ch][1]}"
            assert got[ch][0] == exp[ch][0], f"channel {ch}: the stream differs"
        out, eb = ctx.decode_eg_frames([b for b, _ in exp], w, h, stacks, [CARRY[ch][1] for ch in range(channels)])
        assert eb == [bits for _, bits in exp]
    else:
        import torch
        got = _encode_dev(ctx, fr, exp, 0x00, GUARD, torch)
        _check_streams(got, exp)
        # the same input at an odd address, other junk around it: the same bytes
        got2 = _encode_dev(ctx, fr, exp, 0xFF, GUARD - 3, torch)
        assert [g[0] for g in got2] == [g[0] for g in got], "the encode depends on bytes outside its input"
        out = _decode_dev(ctx, exp, fr.shape, torch)
        assert np.array_equal(out, _decode_dev(ctx, exp, fr.shape, torch, lead=GUARD - 3))
    assert out.shape == fr.shape and np.array_equal(out, out_ref), f"{(out != out_ref).sum()} bytes differ"
    assert ctx.stats()["n_units"] == channels * stacks * ((w + 7) // 8) * ((h + 7) // 8) * 64 * depth


@pytest.mark.parametrize("entry", ["host", "dev"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_encode_rare_path_reloads_padded_channel_rows(pkg, gpu_ctx8, gpu_ctx4, depth, channels, entry):
    """29 x 7, 48 stacks: the fp32 certificate leaves coefficients open at both depths, in every channel
    (tests/test_eg_frames_rare_content.py); the in-wave exact replay re-reads its rows through the edge and
    channel addressing."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, q_ref = _rare_case(depth, channels)
    exp = _streams_of(q_ref, depth, channels, 48, CARRY)
    if entry == "host":
        got = ctx.encode_eg_frames(fr, CARRY[:channels])
        st = ctx.stats()
        assert [(b, n) for b, n in got] == [(b, n) for b, n in exp]
    else:
        import torch
        got = _encode_dev(ctx, fr, exp, 0x33, GUARD - 1, torch)
        st = ctx.stats()
        _check_streams(got, exp)
    assert st["n_flagged"] > 0
    assert st["n_units"] == channels * 48 * 4 * 64 * depth


@pytest.mark.parametrize("w,h,stacks", [(61, 27, 2), (13, 11, 3)])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_forced_replay_reparses_its_stream(pkg, gpu_ctx8, gpu_ctx4, depth, channels, w, h, stacks):
    """A widened margin sends lanes to the in-wave exact replay, which re-parses its cube from stream ch at the
    cube's marks, ahead of the cropped stores."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr, _, out_ref = _content(depth, channels, w, h, stacks)
    exp = _streams(depth, channels, w, h, stacks)
    sb = [CARRY[ch][1] for ch in range(channels)]
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.45):
        out, eb = ctx.decode_eg_frames([b for b, _ in exp], w, h, stacks, sb)
        st = ctx.stats()
    assert st["n_flagged"] > 0
    assert eb == [bits for _, bits in exp]
    assert np.array_equal(out, out_ref)


@pytest.mark.parametrize("option", ["DCT3D_OPT_EG_FORCE_RETRY", "DCT3D_OPT_EG_TWO_STEP", "DCT3D_OPT_EG_NO_RESOLVE"])
@pytest.mark.parametrize("depth", [8, 4])
def test_options_give_the_same_results(pkg, gpu_ctx8, gpu_ctx4, depth, option):
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 44, 20, 3
    fr, _, out_ref = _content(depth, 3, w, h, stacks)
    exp = _streams(depth, 3, w, h, stacks)
    sb = [c[1] for c in CARRY]
    with ctx_option(ctx, getattr(pkg, option), 1):
        got = ctx.encode_eg_frames(fr, CARRY)
        out, eb = ctx.decode_eg_frames([b for b, _ in exp], w, h, stacks, sb)
        out_dev = _decode_dev(ctx, exp, fr.shape, torch)
    assert [(b, n) for b, n in got] == [(b, n) for b, n in exp]
    assert eb == [bits for _, bits in exp]
    assert np.array_equal(out, out_ref) and np.array_equal(out_dev, out_ref)


@pytest.mark.parametrize("depth", [8, 4])
def test_error_paths_and_the_call_after(pkg, gpu_ctx8, gpu_ctx4, depth):
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 44, 20, 3
    fr, _, out_ref = _content(depth, 3, w, h, stacks)
    exp = _streams(depth, 3, w, h, stacks)
    bits = [b for _, b in exp]
    sb = [c[1] for c in CARRY]

    def good():
        _check_streams(_encode_dev(ctx, fr, exp, 0x11, GUARD, torch), exp)
        assert np.array_equal(_decode_dev(ctx, exp, fr.shape, torch), out_ref)

    # channel 1's capacity one word short: ENOSPC, every total right, nothing outside any output
    call, finish = _encode_dev(ctx, fr, exp, 0x00, GUARD, torch, short=1, sync=False)
    with pytest.raises(pkg.Dct3dError) as e:
        call()
    assert e.value.code == pkg.DCT3D_ENOSPC and e.value.total_bits == bits
    finish(bits)  # (the bands)
    good()
    out = torch.zeros(fr.size, dtype=torch.uint8, device="cuda")
    # channel 1's stream truncated by a byte
    ts, nb = _device_streams(exp, torch, cut=1)
    with pytest.raises(pkg.Dct3dError) as e:
        ctx.decode_eg_frames_dev(ts, nb, sb, w, h, stacks, out)
    assert e.value.code == pkg.DCT3D_ENODATA
    assert e.value.end_bits == [bits[0], sb[1], bits[2]]
    good()
    with pytest.raises(pkg.Dct3dError) as e:
        ctx.decode_eg_frames([exp[0][0], exp[1][0][:-1], exp[2][0]], w, h, stacks, sb)
    assert e.value.code == pkg.DCT3D_ENODATA
    # a run of 40+ zero bits in channel 2: a corrupt stream
    ts, nb = _device_streams(exp, torch, zero_run=2)
    with pytest.raises(pkg.Dct3dError) as e:
        ctx.decode_eg_frames_dev(ts, nb, sb, w, h, stacks, out)
    assert e.value.code == pkg.DCT3D_EINVAL
    assert e.value.end_bits == [bits[0], bits[1], sb[2]]
    good()
    ctx.synchronize()


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("depth", [8, 4])
def test_back_to_back_calls_land_their_own_results(pkg, gpu_ctx8, gpu_ctx4, depth, side_stream):
    """two encodes, then two decodes, queued with no synchronisation between them: different content (the second
    is the first with its channels reversed, so the oracle's work is shared) and different outputs"""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = 93, 45, 5
    fr, q, out_ref = _content(depth, 3, w, h, stacks)
    exp = _streams(depth, 3, w, h, stacks)
    fr2 = np.ascontiguousarray(fr[..., ::-1])
    q2 = np.ascontiguousarray(q.reshape(stacks, 3, -1)[:, ::-1])
    exp2 = _streams_of(q2, depth, 3, stacks, CARRY)
    sb = [c[1] for c in CARRY]
    n = fr.size
    s = torch.cuda.Stream() if side_stream else None
    try:
        call1, fin1 = _encode_dev(ctx, fr, exp, 0x00, GUARD, torch, sync=False)
        call2, fin2 = _encode_dev(ctx, fr2, exp2, 0xFF, GUARD - 3, torch, sync=False)
        ts1, nb1 = _device_streams(exp, torch)
        ts2, nb2 = _device_streams(exp2, torch)
        o1 = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        o2 = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if s is not None:
            ctx.set_stream(s.cuda_stream)
        tb1 = call1()
        tb2 = call2()
        eb1 = ctx.decode_eg_frames_dev(ts1, nb1, sb, w, h, stacks, o1)
        eb2 = ctx.decode_eg_frames_dev(ts2, nb2, sb, w, h, stacks, o2)
        ctx.synchronize()
        _check_streams(fin1(tb1), exp)
        _check_streams(fin2(tb2), exp2)
        assert eb1 == [b for _, b in exp] and eb2 == [b for _, b in exp2]
        assert np.array_equal(o1.cpu().numpy().reshape(fr.shape), out_ref)
        assert np.array_equal(o2.cpu().numpy().reshape(fr.shape), out_ref[..., ::-1])
    finally:
        if s is not None:
            ctx.synchronize()
            ctx.set_stream(None)


def _run(args, env=None):
    r = subprocess.run(args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_cli_streams_equal_the_host_entropy_path(pkg, tmp_path, depth, channels):
    """20 frames of 29 x 13 through dct3d_codec: the files are byte for byte those written with
    DCT3D_CODEC_HOST_EG=1 (the int32 path, Exp-Golomb on the host), and either decode of them equals the
    oracle's (a short last stack zero-filled, as the codec does)."""
    w, h, frames = 29, 13, 20
    whole = (frames + depth - 1) // depth * depth
    fr = pkg.synthetic.frames(w, h, frames) if channels == 1 else rgb_content(pkg, w, h, frames)
    (tmp_path / "in.raw").write_bytes(fr.tobytes())
    enc, dec = ("encode", "decode") if channels == 1 else ("encode_rgb", "decode_rgb")
    tail = [str(w), str(h), str(frames), "1", str(depth)]
    host_env = dict(os.environ, DCT3D_CODEC_HOST_EG="1")
    dev_env = {k: v for k, v in os.environ.items() if k != "DCT3D_CODEC_HOST_EG"}
    _run([pkg.CLI_PATH, enc, str(tmp_path / "in.raw"), str(tmp_path / "a")] + tail, dev_env)
    _run([pkg.CLI_PATH, enc, str(tmp_path / "in.raw"), str(tmp_path / "b")] + tail, host_env)
    for sfx in ([""] if channels == 1 else [".red", ".green", ".blue"]):
        assert filecmp.cmp(str(tmp_path / "a") + sfx, str(tmp_path / "b") + sfx, shallow=False), sfx
    _run([pkg.CLI_PATH, dec, str(tmp_path / "a"), str(tmp_path / "a.out")] + tail, dev_env)
    _run([pkg.CLI_PATH, dec, str(tmp_path / "a"), str(tmp_path / "b.out")] + tail, host_env)
    cshape = () if channels == 1 else (3,)
    out = np.frombuffer((tmp_path / "a.out").read_bytes(), np.uint8).reshape((whole, h, w) + cshape)
    zfill = np.zeros((whole,) + fr.shape[1:], np.uint8)
    zfill[:frames] = fr
    _, out_ref = _oracle(depth, zfill)
    assert np.array_equal(out, out_ref)
    assert filecmp.cmp(str(tmp_path / "a.out"), str(tmp_path / "b.out"), shallow=False)
