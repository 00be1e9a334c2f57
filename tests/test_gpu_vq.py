"""GPU: per-stack quantiser tables in the fused stream calls (dct3d_*_eg_frames_vq*), exact equality
throughout.  The reference is quant_common's (ref_frames, code_bits, ref_decode_frames) applied stack by stack with
the stack's own table, the values in diagonal order, the Exp-Golomb bits written here in numpy.

Shapes, 11 stacks each: 8x8 (one cube per stack: every cube of an encode wave and of a decode wave has its own
table; the last wave is ragged), 24x24 (9 cubes per stack: the table changes inside a wave), 61x45 (edge) and 64x64
(aligned, whole waves per stack), the last two grey and packed RGB24.  Palettes of 1, 8, 11 and 32 tables from
quant_common.tables and quant_table(q) over the codec's ladder; maps cycling, constant and in runs of 3."""
import functools

import numpy as np
import pytest

import quant_common as qc
from conftest import ctx_option

pytestmark = pytest.mark.gpu

STACKS = 11
SHAPES = [(8, 8, 1), (24, 24, 1), (61, 45, 1), (61, 45, 3), (64, 64, 1), (64, 64, 3)]
LADDER = (1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 32, 40, 48, 64)
BAND = 4096


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


@functools.lru_cache(maxsize=None)
def palette(depth, n):
    """n tables: q1, all255, seeded, then the others of quant_common.tables, then quant_table(q) over the ladder and
    past it (distinct tables throughout)"""
    p = qc.pkg()
    t = qc.tables(depth)
    pool = [t[k] for k in ("q1", "all255", "seeded", "q2", "q12", "ones")]
    pool += [p.quant_table(q, depth) for q in LADDER if q not in (1, 2, 12)]
    pool += [p.quant_table(q, depth) for q in range(65, 65 + 32)]
    out = np.stack(pool[:n]).astype(np.int32)
    assert len({a.tobytes() for a in out}) == n
    out.setflags(write=False)
    return out


def stack_map(kind, n_tables, stacks=STACKS):
    s = np.arange(stacks)
    m = {"cycle": s % n_tables, "const": np.full(stacks, n_tables - 1), "runs3": (s // 3) % n_tables}[kind]
    return m.astype(np.uint8)


# (tables in the palette, map): every palette size, every map kind, the palette larger and smaller than the clip
COMBOS = [(1, "const"), (8, "cycle"), (8, "runs3"), (11, "cycle"), (11, "const"), (32, "cycle"), (32, "runs3")]


@functools.lru_cache(maxsize=None)
def frames(depth, w, h, channels, stacks=STACKS):
    """stacks in turn ramp, uniform noise and a flat grey level (read-only)"""
    p = qc.pkg()

    def plane(s, i):
        kind = ("ramp", "uniform", "flat")[s % 3]
        if kind == "flat":
            return np.full((depth, h, w), 37 + 11 * s + 50 * i, np.uint8)
        return p.synthetic.frames(w, h, depth, seed=0x5EED + 131 * s + 17 * i, frame0=2 * s + i, kind=kind)

    fr = np.concatenate([plane(s, 0) if channels == 1 else np.stack([plane(s, 0), plane(s, 1), plane(s, 2)], axis=-1)
                         for s in range(stacks)])
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def _ref_stack(depth, w, h, channels, s, table_bytes):
    """(q [channel][cube], decoded frames) of stack s under one table: quant_common.ref_frames on that stack alone"""
    T = np.frombuffer(table_bytes, np.int32)
    fr = frames(depth, w, h, channels)
    q, out = qc.ref_frames(np.ascontiguousarray(fr[s * depth:(s + 1) * depth]), T, depth)
    return q.reshape(channels, -1, 64 * depth), out


def eg_bits(vals):
    """the signed order-0 Exp-Golomb bits of vals, MSB first (uint8 0 / 1): n - 1 zeros, then the n bits of the code"""
    v = np.asarray(vals, np.int64).ravel()
    code = np.where(v <= 0, 1 - 2 * v, 2 * v)
    width = qc.code_bits(v)
    end = np.cumsum(width)
    bits = np.zeros(int(end[-1]) if v.size else 0, np.uint8)
    j = 0
    while (code >> j).any():
        on = ((code >> j) & 1) == 1
        bits[end[on] - 1 - j] = 1
        j += 1
    return bits


def ref_streams(per_stack_q, depth, channels, carry):
    """per_stack_q: [stack] of q [channel][cube][cs] -> per channel (stream bytes, total bits) under the carry"""
    order = qc.pkg().diagonal_order(8, 8, depth)
    res = []
    for ch in range(channels):
        vals = np.concatenate([q[ch][:, order].ravel() for q in per_stack_q])
        cb, cn = carry[ch]
        pre = np.unpackbits(np.array([cb], np.uint8))[:cn]
        b = np.concatenate([pre, eg_bits(vals)])
        res.append((np.packbits(b).tobytes(), int(b.size)))
    return res


@functools.lru_cache(maxsize=None)
def reference(depth, w, h, channels, n_tables, kind):
    """(per-stack q, the decoded frames) of the clip under palette(depth, n_tables) and stack_map(kind)"""
    pal, m = palette(depth, n_tables), stack_map(kind, n_tables)
    per = [_ref_stack(depth, w, h, channels, s, pal[m[s]].tobytes()) for s in range(STACKS)]
    out = np.concatenate([o for _, o in per])
    # the decode's definition on its own: ref_decode_frames of each stack's q under the stack's table
    for s in (0, STACKS - 1):
        q = np.ascontiguousarray(per[s][0]).reshape(-1, depth, 8, 8)
        assert np.array_equal(qc.ref_decode_frames(q, w, h, 1, channels, pal[m[s]], depth), per[s][1])
    out.setflags(write=False)
    return [q for q, _ in per], out


def _bytes_of(buf, tb):
    return buf[:(tb + 7) // 8].tobytes()


def _same_stream(got, want):
    """streams equal: total bits, and every bit of them (the last byte's unused bits are zero on both sides)"""
    (gb, gt), (wb, wt) = got, want
    return gt == wt and gb == wb


def encode_dev(ctx, fr, w, h, channels, stacks, pal, m, carry, caps=None, vq=True):
    """the device encode into banded buffers; (streams, bands intact)"""
    import torch
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    cap = ((fr.size // channels) * 2 + 64) // 4 * 4
    caps = caps or [cap] * channels
    bufs = [qc.banded(torch, c, 0xC3, BAND) for c in caps]
    err = None
    try:
        if vq:
            tb = ctx.encode_eg_frames_vq_dev(d_fr, w, h, channels, stacks, pal, m, [b[1] for b in bufs], caps, carry)
        else:
            tb = ctx.encode_eg_frames_dev(d_fr, w, h, channels, stacks, [b[1] for b in bufs], caps, carry)
    except qc.pkg().Dct3dError as e:
        err, tb = e, [0] * channels
    ctx.synchronize()
    if err is not None:  # an error: still nothing outside the outputs
        assert all(qc.bands_intact(buf, c, 0xC3, BAND)[1] for (buf, _), c in zip(bufs, caps)), "wrote outside its outputs"
        raise err
    res, ok = [], True
    for (buf, _), c, t in zip(bufs, caps, tb):
        mid, intact = qc.bands_intact(buf, c, 0xC3, BAND)
        ok &= intact
        res.append((_bytes_of(mid, t), t))
    return res, ok


def decode_dev(ctx, streams, start_bits, w, h, channels, stacks, pal, m, vq=True):
    """the device decode into a banded buffer, twice with different fills; (frames, end bits, bands intact)"""
    import torch
    d_s = []
    for b, _ in streams:
        a = np.zeros((len(b) + 3) // 4 * 4 + 4, np.uint8)
        a[:len(b)] = np.frombuffer(b, np.uint8)
        d_s.append(torch.from_numpy(a).cuda())
    n = stacks * ctx.bd * h * w * channels
    outs, ok, eb = [], True, None
    for fill in (0xA5, 0x5A):
        buf, mid = qc.banded(torch, n, fill, BAND)
        err = None
        try:
            if vq:
                eb = ctx.decode_eg_frames_vq_dev(d_s, [len(b) for b, _ in streams], start_bits, w, h, stacks, pal, m, mid)
            else:
                eb = ctx.decode_eg_frames_dev(d_s, [len(b) for b, _ in streams], start_bits, w, h, stacks, mid)
        except qc.pkg().Dct3dError as e:
            err = e
        ctx.synchronize()
        if err is not None:  # an error: the frames are unspecified, the bands are not
            assert qc.bands_intact(buf, n, fill, BAND)[1], "wrote outside its output"
            raise err
        host, intact = qc.bands_intact(buf, n, fill, BAND)
        ok &= intact
        outs.append(host.reshape((stacks * ctx.bd, h, w) + ((3,) if channels == 3 else ())))
    assert np.array_equal(outs[0], outs[1]), "a byte of the output was not written"
    return outs[0], eb, ok


@pytest.mark.parametrize("n_tables,kind", COMBOS)
@pytest.mark.parametrize("w,h,channels", SHAPES)
@pytest.mark.parametrize("depth", [8, 4])
def test_streams_and_frames_equal_the_per_stack_reference(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, channels, n_tables, kind):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    fr = frames(depth, w, h, channels)
    pal, m = palette(depth, n_tables), stack_map(kind, n_tables)
    per_q, out_ref = reference(depth, w, h, channels, n_tables, kind)
    quant_before = ctx.quant().copy()
    for carry in ([(0, 0)] * channels, [(0xB4, 3), (0x5F, 7), (0x80, 1)][:channels]):
        want = ref_streams(per_q, depth, channels, carry)
        got_d, intact = encode_dev(ctx, fr, w, h, channels, STACKS, pal, m, carry)
        assert intact, "the encode wrote outside its outputs"
        got_h = ctx.encode_eg_frames_vq(fr, pal, m, carry)
        for ch in range(channels):
            assert _same_stream(got_d[ch], want[ch]), (ch, got_d[ch][1], want[ch][1])
            assert _same_stream(got_h[ch], want[ch]), (ch, got_h[ch][1], want[ch][1])
        start = [cn for _, cn in carry]
        out_d, eb_d, intact = decode_dev(ctx, want, start, w, h, channels, STACKS, pal, m)
        assert intact, "the decode wrote outside its output"
        out_h, eb_h = ctx.decode_eg_frames_vq([b for b, _ in want], w, h, STACKS, pal, m, start)
        assert np.array_equal(out_d, out_ref), f"{(out_d != out_ref).sum()} bytes differ (device)"
        assert np.array_equal(out_h, out_ref), f"{(out_h != out_ref).sum()} bytes differ (host)"
        assert eb_d == [t for _, t in want] and eb_h == eb_d
    assert np.array_equal(ctx.quant(), quant_before), "a vq call changed the context's quantiser"


# ---- the chain of single-stack base calls ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain_ctx(pkg):
    """contexts of this module's own whose quantiser the chain sets stack by stack"""
    made = {}

    def get(depth):
        if depth not in made:
            try:
                made[depth] = pkg.Context(0, 8, 8, depth)
            except Exception as e:
                pytest.fail(f"HIP context for 8x8x{depth} could not be created: {e}")
        made[depth].set_option(pkg.DCT3D_OPT_DEC_MARGIN, 0)
        return made[depth]

    yield get
    for c in made.values():
        c.close()


def chain_encode(ctx, fr, w, h, channels, stacks, pal, m, carry):
    """`stacks` single-stack base calls, set_quant before each, the carry of each handed to the next:
    (streams, per-stack n_flagged, n_units summed)"""
    d = ctx.bd
    bits = [np.unpackbits(np.array([cb], np.uint8))[:cn] for cb, cn in carry]
    flagged, units = [], 0
    for s in range(stacks):
        ctx.set_quant(pal[m[s]])
        cur = []
        for b in bits:
            n = b.size % 8
            cur.append((int(np.packbits(b[b.size - n:])[0]) if n else 0, n))
        res, ok = encode_dev(ctx, np.ascontiguousarray(fr[s * d:(s + 1) * d]), w, h, channels, 1, None, None, cur, vq=False)
        assert ok
        st = ctx.stats()
        flagged.append(st["n_flagged"])
        units += st["n_units"]
        for ch, (by, tb) in enumerate(res):
            n = bits[ch].size % 8
            new = np.unpackbits(np.frombuffer(by, np.uint8))[:tb]
            bits[ch] = np.concatenate([bits[ch][:bits[ch].size - n], new])
    ctx.set_quant(None)
    return [(np.packbits(b).tobytes(), int(b.size)) for b in bits], flagged, units


def chain_decode(ctx, streams, start_bits, w, h, channels, stacks, pal, m):
    """the decode's chain: each single-stack base call starts where the one before ended.
    (frames, end bits, n_flagged summed, n_units summed)"""
    outs, pos, flagged, units = [], list(start_bits), 0, 0
    for s in range(stacks):
        ctx.set_quant(pal[m[s]])
        cut = [(b[p // 8:], t) for (b, t), p in zip(streams, pos)]
        out, eb, ok = decode_dev(ctx, cut, [p % 8 for p in pos], w, h, channels, 1, None, None, vq=False)
        assert ok
        st = ctx.stats()
        flagged += st["n_flagged"]
        units += st["n_units"]
        pos = [p // 8 * 8 + e for p, e in zip(pos, eb)]
        outs.append(out)
    ctx.set_quant(None)
    return np.concatenate(outs), pos, flagged, units


@pytest.mark.parametrize("w,h,channels", [(8, 8, 1), (24, 24, 1), (61, 45, 3), (64, 64, 1)])
@pytest.mark.parametrize("depth", [8, 4])
def test_one_call_equals_the_chain_of_base_calls(pkg, gpu_ctx8, gpu_ctx4, chain_ctx, depth, w, h, channels):
    ctx, cc = _ctx(depth, gpu_ctx8, gpu_ctx4), chain_ctx(depth)
    fr = frames(depth, w, h, channels)
    pal, m = palette(depth, 8), stack_map("cycle", 8)
    carry = [(0xB4, 3), (0x5F, 7), (0x80, 1)][:channels]
    want, flagged, units = chain_encode(cc, fr, w, h, channels, STACKS, pal, m, carry)
    got, intact = encode_dev(ctx, fr, w, h, channels, STACKS, pal, m, carry)
    st = ctx.stats()
    assert intact
    for ch in range(channels):
        assert _same_stream(got[ch], want[ch]), ch
    assert st["n_units"] == units and st["n_flagged"] == sum(flagged)
    start = [cn for _, cn in carry]
    out_c, eb_c, fl_c, un_c = chain_decode(cc, want, start, w, h, channels, STACKS, pal, m)
    out, eb, intact = decode_dev(ctx, want, start, w, h, channels, STACKS, pal, m)
    st = ctx.stats()
    assert intact and np.array_equal(out, out_c) and eb == eb_c
    assert st["n_units"] == un_c and st["n_flagged"] == fl_c


# ---- rare paths ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_encode_replays_under_the_source_cubes_table(pkg, gpu_ctx8, gpu_ctx4, chain_ctx, depth, channels):
    """test_gpu_edge's rare content (29 x 7, 48 stacks, every cube an edge cube) under a map alternating the
    reference table and q1: the whole-wave exact replay must divide by the step of the cube it replays"""
    from test_gpu_edge import _rare_content
    ctx, cc = _ctx(depth, gpu_ctx8, gpu_ctx4), chain_ctx(depth)
    fr = _rare_content(pkg, depth, channels)
    stacks = fr.shape[0] // depth
    pal = np.stack([pkg.quant_table(5, depth), qc.tables(depth)["q1"]]).astype(np.int32)
    m = (np.arange(stacks) % 2).astype(np.uint8)
    carry = [(0, 0)] * channels
    want, flagged, units = chain_encode(cc, fr, 29, 7, channels, stacks, pal, m, carry)
    # a condition on the input, asserted on the yardstick: replays in stacks of both tables
    assert any(f > 0 for f in flagged[0::2]) and any(f > 0 for f in flagged[1::2]), flagged
    got, intact = encode_dev(ctx, fr, 29, 7, channels, stacks, pal, m, carry)
    st = ctx.stats()
    assert intact
    for ch in range(channels):
        assert _same_stream(got[ch], want[ch]), ch
    assert st["n_flagged"] == sum(flagged) and st["n_units"] == units


@pytest.mark.parametrize("w,h,channels", [(8, 8, 1), (61, 45, 1), (61, 45, 3), (64, 64, 3)])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_forced_replay_under_a_cycling_map(pkg, gpu_ctx8, gpu_ctx4, depth, w, h, channels):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    pal, m = palette(depth, 8), stack_map("cycle", 8)
    per_q, out_ref = reference(depth, w, h, channels, 8, "cycle")
    want = ref_streams(per_q, depth, channels, [(0, 0)] * channels)
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.25):
        out, eb, intact = decode_dev(ctx, want, [0] * channels, w, h, channels, STACKS, pal, m)
        st = ctx.stats()
        out_h, _ = ctx.decode_eg_frames_vq([b for b, _ in want], w, h, STACKS, pal, m)
    assert intact and st["n_flagged"] > 0
    assert np.array_equal(out, out_ref) and np.array_equal(out_h, out_ref)


@pytest.mark.parametrize("option", ["DCT3D_OPT_EG_FORCE_RETRY", "DCT3D_OPT_EG_NO_RESOLVE"])
@pytest.mark.parametrize("channels", [1, 3])
def test_decode_options_act_as_on_the_base_calls(pkg, gpu_ctx8, option, channels):
    ctx, depth, (w, h) = gpu_ctx8, 8, (61, 45)
    pal, m = palette(depth, 11), stack_map("cycle", 11)
    per_q, out_ref = reference(depth, w, h, channels, 11, "cycle")
    want = ref_streams(per_q, depth, channels, [(0, 0)] * channels)
    with ctx_option(ctx, getattr(pkg, option), 1):
        out, eb, intact = decode_dev(ctx, want, [0] * channels, w, h, channels, STACKS, pal, m)
    assert intact and np.array_equal(out, out_ref) and eb == [t for _, t in want]


# ---- errors, and the call after ----------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_errors_and_the_call_after(pkg, gpu_ctx8, gpu_ctx4, depth, channels):
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = 61, 45
    fr = frames(depth, w, h, channels)
    pal, m = palette(depth, 8), stack_map("cycle", 8)
    per_q, out_ref = reference(depth, w, h, channels, 8, "cycle")
    carry = [(0, 0)] * channels
    want = ref_streams(per_q, depth, channels, carry)

    def good():
        got, intact = encode_dev(ctx, fr, w, h, channels, STACKS, pal, m, carry)
        assert intact and all(_same_stream(got[ch], want[ch]) for ch in range(channels))
        out, eb, intact = decode_dev(ctx, want, [0] * channels, w, h, channels, STACKS, pal, m)
        assert intact and np.array_equal(out, out_ref)
        assert all(_same_stream(a, b) for a, b in zip(ctx.encode_eg_frames_vq(fr, pal, m), want))
        assert np.array_equal(ctx.decode_eg_frames_vq([b for b, _ in want], w, h, STACKS, pal, m)[0], out_ref)

    def einval(tables, smap):
        for call in (lambda: ctx.encode_eg_frames_vq(fr, tables, smap),
                     lambda: encode_dev(ctx, fr, w, h, channels, STACKS, tables, smap, carry),
                     lambda: ctx.decode_eg_frames_vq([b for b, _ in want], w, h, STACKS, tables, smap),
                     lambda: decode_dev(ctx, want, [0] * channels, w, h, channels, STACKS, tables, smap)):
            with pytest.raises(pkg.Dct3dError) as e:
                call()
            assert e.value.code == pkg.DCT3D_EINVAL
        good()

    bad = m.copy()
    bad[STACKS - 1] = 8
    einval(pal, bad)                                      # an entry == n_tables
    for step in (0, 256, -1):
        t = pal.copy()
        t[5, 3] = step
        einval(t, m)                                      # a step outside [1, 255]
    einval(np.concatenate([palette(depth, 32), pal[:1]]), m)  # 33 tables
    einval(None, m)
    einval(pal, None)
    with ctx_option(ctx, pkg.DCT3D_OPT_EG_TWO_STEP, 1):   # refused, not ignored
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.encode_eg_frames_vq(fr, pal, m)
        assert e.value.code == pkg.DCT3D_EINVAL
    good()
    # a capacity too small: DCT3D_ENOSPC with every total set, nothing written past the capacity
    caps = [((want[ch][1] + 7) // 8 // 2) // 4 * 4 for ch in range(channels)]
    with pytest.raises(pkg.Dct3dError) as e:
        encode_dev(ctx, fr, w, h, channels, STACKS, pal, m, carry, caps=caps)
    assert e.value.code == pkg.DCT3D_ENOSPC and e.value.total_bits == [t for _, t in want]
    good()
    # a cut stream: DCT3D_ENODATA, the good streams' end bits
    cut = [(b[:len(b) // 2], t) if ch == channels - 1 else (b, t) for ch, (b, t) in enumerate(want)]
    with pytest.raises(pkg.Dct3dError) as e:
        decode_dev(ctx, cut, [0] * channels, w, h, channels, STACKS, pal, m)
    assert e.value.code == pkg.DCT3D_ENODATA
    if channels == 3:
        assert e.value.end_bits[:2] == [t for _, t in want[:2]]
    good()


def test_a_vq_call_between_two_base_encodes_on_a_framework_stream(pkg, gpu_ctx8):
    import torch
    ctx, depth, (w, h), channels = gpu_ctx8, 8, (61, 45), 3
    fr = frames(depth, w, h, channels)
    pal, m = palette(depth, 8), stack_map("cycle", 8)
    per_q, _ = reference(depth, w, h, channels, 8, "cycle")
    carry = [(0, 0)] * channels
    want = ref_streams(per_q, depth, channels, carry)
    per_ref = [_ref_stack(depth, w, h, channels, s, np.ascontiguousarray(ctx.quant()).tobytes())[0] for s in range(STACKS)]
    want_base = ref_streams(per_ref, depth, channels, carry)
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    cap = (fr.size // channels * 2 + 64) // 4 * 4
    s = torch.cuda.Stream()
    quant_before = ctx.quant().copy()
    ctx.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            bufs = [[torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(channels)] for _ in range(3)]
            t0 = ctx.encode_eg_frames_dev(d_fr, w, h, channels, STACKS, bufs[0], [cap] * channels)
            t1 = ctx.encode_eg_frames_vq_dev(d_fr, w, h, channels, STACKS, pal, m, bufs[1], [cap] * channels)
            t2 = ctx.encode_eg_frames_dev(d_fr, w, h, channels, STACKS, bufs[2], [cap] * channels)
        s.synchronize()
    finally:
        ctx.set_stream(None)
    for tb, bb, ref in ((t0, bufs[0], want_base), (t1, bufs[1], want), (t2, bufs[2], want_base)):
        for ch in range(channels):
            assert _same_stream((_bytes_of(bb[ch].cpu().numpy(), tb[ch]), tb[ch]), ref[ch]), ch
    assert np.array_equal(ctx.quant(), quant_before)


# ---- the codec's qmap= ---------------------------------------------------------------------------------------------

def _run_cli(pkg, args, env=None):
    import os
    import subprocess
    r = subprocess.run([pkg.CLI_PATH] + [str(a) for a in args], capture_output=True, text=True,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@functools.lru_cache(maxsize=None)
def codec_clip(channels, stacks=6, depth=8, w=64, h=64):
    """stacks alternate a flat level and uniform noise (read-only)"""
    p = qc.pkg()

    def plane(s, i):
        if s % 2 == 0:
            return np.full((depth, h, w), 90 + 7 * s + 30 * i, np.uint8)
        return p.synthetic.frames(w, h, depth, seed=0xC0DE + 31 * s + 5 * i, frame0=s + i, kind="uniform")

    fr = np.concatenate([plane(s, 0) if channels == 1 else np.stack([plane(s, 0), plane(s, 1), plane(s, 2)], axis=-1)
                         for s in range(stacks)])
    fr.setflags(write=False)
    return fr


@pytest.mark.parametrize("target", ["psnr=30", "rate=4"])  # (a flat RGB stack costs 3 bits a pixel: it fits, noise does not)
@pytest.mark.parametrize("channels", [1, 3])
def test_codec_writes_reads_and_decodes_a_quality_map(pkg, gpu_ctx8, tmp_path, channels, target):
    import zlib
    ctx, depth, w, h, stacks = gpu_ctx8, 8, 64, 64, 6
    fr = codec_clip(channels)
    frames_n = stacks * depth
    raw, binf, again, outf, mapf = (tmp_path / n for n in ("in.raw", "o.bin", "again.bin", "o.raw", "map.txt"))
    raw.write_bytes(fr.tobytes())
    enc, dec = ("encode", "decode") if channels == 1 else ("encode_rgb", "decode_rgb")
    env = {"DCT3D_CODEC_BATCH": "4"}  # batches of 4 and 2 stacks: each sees its own slice of the map
    r = _run_cli(pkg, [enc, raw, binf, w, h, frames_n, 1, depth, target, "qmap=" + str(mapf)], env)
    # the written map: the per-stack rule on the distortion probe's output
    ladder_tabs = np.stack([pkg.quant_table(q, depth) for q in LADDER])
    sse, bits = ctx.distortion_frames(fr, ladder_tabs, want_bits=True)
    if target.startswith("psnr="):
        want_map = pkg.pick_stack_qualities_psnr(sse, LADDER, w * h * depth * channels, float(target[5:]))
    else:
        want_map = pkg.pick_stack_qualities(bits, LADDER, float(target[5:]) * w * h * depth)
    assert len(set(want_map)) >= 2, want_map  # a condition on the content
    assert [int(x) for x in mapf.read_text().split()] == want_map and mapf.read_text().endswith("\n")
    total = sum(int(bits[LADDER.index(q), s].sum()) for s, q in enumerate(want_map))
    assert f"qmap: stacks={stacks} bits={total}\n" in r.stdout
    names = [str(binf)] if channels == 1 else [str(binf) + s for s in (".red", ".green", ".blue")]
    # the files: the per-stack reference's streams (each stack quantised with its own table), deflated
    m = np.array([LADDER.index(q) for q in want_map], np.uint8)
    per = [qc.ref_frames(np.ascontiguousarray(fr[s * depth:(s + 1) * depth]), ladder_tabs[m[s]], depth) for s in range(stacks)]
    want = ref_streams([q.reshape(channels, -1, 64 * depth) for q, _ in per], depth, channels, [(0, 0)] * channels)
    payload = [zlib.decompress(open(n, "rb").read()) for n in names]
    for ch in range(channels):  # (a stream that ends on a byte boundary is followed by the writer's empty next byte)
        nb = len(want[ch][0])
        assert payload[ch][:nb] == want[ch][0] and payload[ch][nb:] in (b"", b"\0"), names[ch]
    # re-encoding with the map alone: the same files
    _run_cli(pkg, [enc, raw, again, w, h, frames_n, 1, depth, "qmap=" + str(mapf)], env)
    for n in names:
        assert open(n, "rb").read() == open(n.replace("o.bin", "again.bin"), "rb").read()
    # the decode with the map: the Python decode of the same streams, and the per-stack reference
    _run_cli(pkg, [dec, binf, outf, w, h, frames_n, 1, depth, "qmap=" + str(mapf)], env)
    got = np.frombuffer(outf.read_bytes(), np.uint8).reshape(fr.shape)
    py, _ = ctx.decode_eg_frames_vq(payload, w, h, stacks, ladder_tabs, m)
    assert np.array_equal(got, py)
    assert np.array_equal(got, np.concatenate([o for _, o in per]))
    # the map through the environment: the same decode
    _run_cli(pkg, [dec, binf, tmp_path / "env.raw", w, h, frames_n, 1, depth], dict(env, DCT3D_CODEC_QMAP="qmap=" + str(mapf)))
    assert (tmp_path / "env.raw").read_bytes() == outf.read_bytes()


@pytest.mark.parametrize("channels", [1, 3])
def test_codec_constant_map_is_the_q_file(pkg, tmp_path, channels):
    depth, w, h, stacks = 8, 64, 64, 6
    fr = codec_clip(channels)
    raw, a, b, mapf = (tmp_path / n for n in ("in.raw", "a.bin", "b.bin", "map.txt"))
    raw.write_bytes(fr.tobytes())
    mapf.write_text("12\n" * stacks)
    enc, dec = ("encode", "decode") if channels == 1 else ("encode_rgb", "decode_rgb")
    env = {"DCT3D_CODEC_BATCH": "4"}
    _run_cli(pkg, [enc, raw, a, w, h, stacks * depth, 1, depth, "q=12"], env)
    _run_cli(pkg, [enc, raw, b, w, h, stacks * depth, 1, depth, "qmap=" + str(mapf)], env)
    for s in ([""] if channels == 1 else [".red", ".green", ".blue"]):
        assert open(str(a) + s, "rb").read() == open(str(b) + s, "rb").read()
    _run_cli(pkg, [dec, a, tmp_path / "a.raw", w, h, stacks * depth, 1, depth, "q=12"], env)
    _run_cli(pkg, [dec, a, tmp_path / "b.raw", w, h, stacks * depth, 1, depth, "qmap=" + str(mapf)], env)
    assert (tmp_path / "a.raw").read_bytes() == (tmp_path / "b.raw").read_bytes()
