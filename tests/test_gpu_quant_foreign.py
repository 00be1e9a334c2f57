"""GPU: the quantiser-table kernels (dct3d_quant.hip, dct3d_quant_eg.hip) on decode inputs that no
encoder of 8-bit frames writes -- a decoder's input is a file -- and the table as state between queued calls.

Every expectation is quant_common's reference: the numpy definition of the quantiser (dequantize_ref) around the
oracle's Java InverseDCT fold, RGB through qc.packed, ragged sizes cropped; streams are oracle.eg_write of the cubes
in diagonal order (test_gpu_eg._expected), the end bit = start bit + bit count.  np.array_equal only.

Tables (qc.tables): all255 (the upper range limit; the DC is divided too), ones (the lower), seeded (non-monotone,
step[0] = 3), and `forced`: the reference table through DCT3D_OPT_QUANT_FORCE_TABLE, whose expectation is
additionally Plan.decode_q.

Geometries (w, h): 168x8 (21 cubes per stack: a ragged last wave at both depths, an odd count of blocks per row:
per-lane stores), 48x32 (24: an even count, block stores through LDS), 163x13 (42) and 13x9 (4): the masked
stores of the EDGE kernels.  Both depths, grey and RGB, 1 and 2 stacks.  A block of 21 or more cubes holds every case
of section 1; the 4 cubes of 13x9 hold the guard cubes and one of the other cases, which moves with stack and channel.

What the inputs must reach is asserted in numpy before the GPU is called: the side of dec_l1_max a cube is on,
|q| = 2^15 - 1, the code widths."""
import functools

import numpy as np
import pytest

import quant_common as qc
from conftest import ctx_option
from foreign_common import STREAM_KINDS
from test_gpu_eg import _expected
from test_gpu_quant import _frames, tie_cube

pytestmark = pytest.mark.gpu

GEOMS = [(168, 8), (48, 32), (163, 13), (13, 9)]
TABLES = ("all255", "ones", "seeded", "forced")
CANARY = 0xC3


@pytest.fixture(scope="module")
def qctx(pkg):
    """contexts of this module's own (the session's shared ones keep the reference table whatever happens here)"""
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
        for opt in (pkg.DCT3D_OPT_QUANT_FORCE_TABLE, pkg.DCT3D_OPT_EG_TWO_STEP, pkg.DCT3D_OPT_ENC_NO_RECHECK,
                    pkg.DCT3D_OPT_DEC_MARGIN):
            ctx.set_option(opt, 0)
        return ctx

    yield get
    for c in made.values():
        c.close()


def _table(depth, name):
    return qc.pkg().quant_table(5, depth) if name == "forced" else qc.tables(depth)[name]


def _set_table(ctx, depth, name):
    """the context on the table kernels with table `name`; returns the table"""
    p = qc.pkg()
    T = _table(depth, name)
    ctx.set_quant(None if name == "forced" else T)
    ctx.set_option(p.DCT3D_OPT_QUANT_FORCE_TABLE, 1 if name == "forced" else 0)
    assert np.array_equal(ctx.quant(), T)
    return T


def _cps(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached arrays are read-only)


def _plan_decode(q, w, h, stacks, channels, depth):
    """Plan.decode_q of the same input: the reference table's second expectation"""
    wp, hp = qc.pkg().padded_size(w, h)
    out = qc.plan(depth).decode_q(np.ascontiguousarray(q, np.int32), wp, hp, channels * stacks * depth)
    if channels == 3:
        out = qc.packed(out, depth)
    return np.ascontiguousarray(out[:, :h, :w])


# ---- 1: int32 decode of arbitrary coefficients --------------------------------------------------------------------

def _guard_places(n):
    """(cubes over the guard: first, mid-wave, a neighbouring pair, last; cubes just under it) among n cubes"""
    if n >= 21:
        return [0, 5, 6, 13, n - 1], [2, 14]
    return [0, n - 1], [2]


def _block(name, depth, n, rot):
    """n cubes for table `name`: sections a to d of one clip.  Returns (q, over, under, ordinary): the index lists
    of the cubes built over the guard, just under it, and of the ordinary ones; the other cubes (the pool:
    saturation list, widest certified values, random dense cubes, rotated by `rot`) fall where they fall."""
    T = _table(depth, name)
    rng = np.random.default_rng(1000 * depth + 10 * TABLES.index(name) + rot)
    lmax = qc.l1_max(depth)
    over, under = _guard_places(n)
    q = np.zeros((n, depth, 8, 8), np.int32)
    for i in over:
        q[i] = qc.guard_cube(T, depth, rng, lmax * (1 + 2.0**-10) + 256)
    for i in under:
        q[i] = qc.guard_cube(T, depth, rng, lmax * (1 - 2.0**-10))
    pool = np.concatenate([qc.saturation_cubes(depth, rng), qc.widest_cubes(T, depth), qc.random_dense_cubes(depth, rng, 1)])
    pool = np.roll(pool, -rot, axis=0)
    rest = [i for i in range(n) if i not in over and i not in under]
    # ordinary cubes between the special ones: position 1 always, and every position the pool of 13 does not fill
    ordinary = [1] if n >= 21 else []
    free = [i for i in rest if i not in ordinary]
    ordinary += free[len(pool):]
    for i, c in zip(free, pool):
        q[i] = c
    if ordinary:
        q[ordinary] = qc.ordinary_cubes(T, depth, rng, len(ordinary))
    return q, over, under, ordinary


@functools.lru_cache(maxsize=None)
def _clip(name, depth, channels, w, h, stacks):
    """(q [stack][channel][cube], the count of cubes whose L1 reaches the guard under the table): the special cubes
    rotated by channel, so that a pixel's three channels meet different cases.  The sides are asserted here."""
    T = _table(depth, name)
    n = _cps(w, h)
    lmax = qc.l1_max(depth)
    blocks = []
    for s in range(stacks):
        for ch in range(channels):
            q, over, under, ordinary = _block(name, depth, n, 3 * ch + 7 * s)
            l1 = qc.l1(q, T, depth)
            assert (l1[over] >= lmax).all() and (l1[over] < lmax * 1.01).all(), "over the guard, and just"
            assert (l1[under] * (1 + 2.0**-12) < lmax).all() and (l1[under] > lmax * 0.99).all(), "under, and just"
            assert (l1[ordinary] < lmax / 8).all()
            if n >= 21:  # d: the widest values on the ordinary path are in the clip, below the guard
                wide = [i for i in range(n) if np.count_nonzero(q[i]) <= 2 and 0.97 * lmax < l1[i] < lmax]
                assert len(wide) == 4, wide
            blocks.append(np.roll(q, 3 * ch, axis=0))
    q = np.stack(blocks).reshape(stacks, channels, n, depth, 8, 8)
    q.setflags(write=False)
    return q, int((qc.l1(q, T, depth) >= lmax).sum())


@functools.lru_cache(maxsize=64)
def _clip_ref(name, depth, channels, w, h, stacks):
    q, _ = _clip(name, depth, channels, w, h, stacks)
    out = qc.ref_decode_frames(q, w, h, stacks, channels, _table(depth, name), depth)
    out.setflags(write=False)
    return out


def _decode_both(ctx, q, w, h, stacks, channels, depth, n_over):
    """decode_frames and decode_frames_dev of q: (host result, device result), the replays counted"""
    import torch
    out_h = ctx.decode_frames(q, w, h, stacks, channels)
    st = ctx.stats()
    assert st["n_flagged"] >= 64 * depth * n_over and st["n_flagged"] % 32 == 0, (st, n_over)
    d_o = torch.full(out_h.shape, 0x5A, dtype=torch.uint8, device="cuda")
    ctx.decode_frames_dev(_dev(q), w, h, channels, stacks, d_o)
    ctx.synchronize()
    st = ctx.stats()
    assert st["n_flagged"] >= 64 * depth * n_over and st["n_flagged"] % 32 == 0, (st, n_over)
    return out_h, d_o.cpu().numpy()


@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("stacks", [1, 2])
@pytest.mark.parametrize("w,h", GEOMS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("depth", [8, 4])
def test_int32_decode_arbitrary_coefficients(pkg, qctx, depth, channels, w, h, stacks, name):
    """1 a-d in one clip per table and geometry: random dense cubes, the saturation list (q = +-2^31 included), cubes
    just under and just over dec_l1_max under this very table (first, mid-wave, a pair, last; ordinary cubes
    between), and the widest values the ordinary path certifies (pixels near +-32000)."""
    q, n_over = _clip(name, depth, channels, w, h, stacks)
    assert n_over >= 2 * stacks * channels
    ref = _clip_ref(name, depth, channels, w, h, stacks)
    ctx = qctx(depth)
    _set_table(ctx, depth, name)
    out_h, out_d = _decode_both(ctx, q, w, h, stacks, channels, depth, n_over)
    assert np.array_equal(out_h, ref), f"{(out_h != ref).sum()} bytes differ"
    assert np.array_equal(out_d, ref), f"{(out_d != ref).sum()} bytes differ"
    if name == "forced":
        assert np.array_equal(ref, _plan_decode(q, w, h, stacks, channels, depth))


@pytest.mark.parametrize("built_for,other", [("all255", "seeded"), ("seeded", "ones"), ("ones", "all255")])
@pytest.mark.parametrize("w,h,channels", [(168, 8, 1), (163, 13, 3)])
@pytest.mark.parametrize("depth", [8, 4])
def test_int32_decode_same_q_two_sides_of_the_guard(pkg, qctx, depth, w, h, channels, built_for, other):
    """1c: one q array under two tables: the cubes built just over the guard for the first table are far under it
    with the finer second one, or every cube is over it with the coarser; each decode equals its own table's
    reference and counts its own replays"""
    q, n_over = _clip(built_for, depth, channels, w, h, 1)
    T1, T2 = _table(depth, built_for), _table(depth, other)
    lmax = qc.l1_max(depth)
    a, b = qc.l1(q, T1, depth), qc.l1(q, T2, depth)
    guard = (a >= lmax) & (a < lmax * 1.01)  # the cubes built for the guard of T1
    assert guard.sum() >= 5 * channels
    assert (b[guard] < 0.9 * lmax).all() or (b[guard] > 1.1 * lmax).all(), "the other side, and not in doubt"
    assert ((a >= lmax) != (b >= lmax)).sum() >= 5 * channels, "cubes that change sides"
    ctx = qctx(depth)
    for name, n in ((built_for, n_over), (other, int((b >= lmax).sum()))):
        T = _set_table(ctx, depth, name)
        ref = qc.ref_decode_frames(q, w, h, 1, channels, T, depth)
        out_h, out_d = _decode_both(ctx, q, w, h, 1, channels, depth, n)
        assert np.array_equal(out_h, ref) and np.array_equal(out_d, ref), name


# ---- streams no encoder wrote ---------------------------------------------------------------------------------------

# the cube kinds (3a: limit, 3b: long, 3c: all_long, and what an encoder writes: ordinary) live in foreign_common.py,
# which test_gpu_foreign_modes.py shares
@functools.lru_cache(maxsize=None)
def _stream_clip(kinds, depth, w, h, stacks):
    """q [stack][channel][cube]: channel ch's cubes (all stacks: one stream) of kind kinds[ch]"""
    n = _cps(w, h) * stacks
    chans = [STREAM_KINDS[k](depth, n, 77 + 13 * ch + depth) for ch, k in enumerate(kinds)]
    q = np.stack([c.reshape(stacks, -1, depth, 8, 8) for c in chans], axis=1)
    q = np.ascontiguousarray(q)
    q.setflags(write=False)
    return q


def _streams_of(q, depth, start_bits):
    """the oracle's stream of each channel of q [stack][channel][cube], from bit start_bits[ch] of a carried byte:
    [(bytes, end bit)]"""
    import oracle
    return [_expected(oracle, qc.pkg(), np.ascontiguousarray(q[:, ch]), depth, 0xFF, sb) for ch, sb in enumerate(start_bits)]


@functools.lru_cache(maxsize=64)
def _stream_case(kinds, depth, w, h, stacks, start_bits, name):
    """(q, streams [(bytes, end bit)], reference frames under table `name`)"""
    q = _stream_clip(kinds, depth, w, h, stacks)
    ref = qc.ref_decode_frames(q, w, h, stacks, len(kinds), _table(depth, name), depth)
    ref.setflags(write=False)
    return q, tuple(_streams_of(q, depth, start_bits)), ref


def _device_streams(exp):
    import torch
    ts = []
    for b, _ in exp:
        pad = np.zeros((len(b) + 11) // 4 * 4, np.uint8)
        pad[:len(b)] = np.frombuffer(b, np.uint8)
        ts.append(torch.from_numpy(pad).cuda())
    return ts, [len(b) for b, _ in exp]


def _decode_streams_every_way(ctx, exp, start_bits, shape, ref, want_replays):
    """decode_eg_frames and decode_eg_frames_dev, fused and under DCT3D_OPT_EG_TWO_STEP: frames, end bits, and the
    replays reported where the input has a cube over the guard or out of range"""
    import torch
    p = qc.pkg()
    f, h, w = shape[:3]
    stacks = f // ctx.bd
    ends = [e for _, e in exp]
    ts, nb = _device_streams(exp)
    for two_step in (0, 1):
        with ctx_option(ctx, p.DCT3D_OPT_EG_TWO_STEP, two_step):
            out, eb = ctx.decode_eg_frames([b for b, _ in exp], w, h, stacks, list(start_bits))
            st = ctx.stats()
            assert eb == ends, (two_step, eb, ends)
            assert np.array_equal(out, ref), f"two_step={two_step}: {(out != ref).sum()} bytes differ"
            if want_replays:
                assert st["n_flagged"] > 0, (two_step, st)
            d_o = torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda")
            eb = ctx.decode_eg_frames_dev(ts, nb, list(start_bits), w, h, stacks, d_o)
            ctx.synchronize()
            st = ctx.stats()
            assert eb == ends, (two_step, eb, ends)
            out = d_o.cpu().numpy()
            assert np.array_equal(out, ref), f"device form, two_step={two_step}: {(out != ref).sum()} bytes differ"
            if want_replays:
                assert st["n_flagged"] > 0, (two_step, st)


def _has_replay_cube(q, T, depth):
    return bool((qc.l1(q, T, depth) >= qc.l1_max(depth)).any() or (np.abs(q.astype(np.int64)) > qc.Q15).any())


@pytest.mark.parametrize("kind,name", [("limit", "all255"), ("long", "seeded"), ("long", "all255")])
@pytest.mark.parametrize("depth", [8, 4])
def test_stream_decode_multiply_limit_and_sparse_long_codes(pkg, qctx, depth, kind, name):
    """3a, 3b at 256 x 128, 2 stacks, grey.  limit: |q| = 2^15 - 1 times step 255, the integer product's and the
    lane's integer L1's largest values (32 (2^15 - 1) 255 < 2^28), and a whole cube of them, over the guard: the
    replay re-parses it from the stream (ReloadStreamQ).  long: a few 33- to 41-bit codes, the stream flagged."""
    w, h, stacks = 256, 128, 2
    q, exp, ref = _stream_case((kind,), depth, w, h, stacks, (0,), name)
    ctx = qctx(depth)
    T = _set_table(ctx, depth, name)
    if kind == "limit":
        n = q.shape[2] * stacks
        l1 = qc.l1(q, T, depth)
        assert (T == 255).all() and l1[2 * n // 3] == 64 * depth * qc.Q15 * 255 >= qc.l1_max(depth)
    assert _has_replay_cube(q, T, depth)
    _decode_streams_every_way(ctx, exp, (0,), (stacks * depth, h, w), ref, True)


@pytest.mark.parametrize("depth", [8, 4])
def test_stream_decode_every_value_a_long_code(pkg, qctx, depth):
    """3c: 64 x 48, 2 stacks, seeded: 33-bit codes only, the marks wrap inside a group and every cube is replayed
    from the stream"""
    w, h, stacks = 64, 48, 2
    q, exp, ref = _stream_case(("all_long",), depth, w, h, stacks, (0,), "seeded")
    ctx = qctx(depth)
    _set_table(ctx, depth, "seeded")
    assert 2048 * 33 > 2**16, "a consumer group's values span more bits than a 16-bit mark holds"
    _decode_streams_every_way(ctx, exp, (0,), (stacks * depth, h, w), ref, True)
    # every cube, whole: the replays of the last (device) call
    assert ctx.stats()["n_flagged"] >= q.size


@pytest.mark.parametrize("name", ["all255", "seeded"])
@pytest.mark.parametrize("w,h", [(48, 32), (168, 8), (50, 21), (13, 9)])
@pytest.mark.parametrize("depth", [8, 4])
def test_stream_decode_rgb_three_different_streams(pkg, qctx, depth, w, h, name):
    """3d, 3e: one ordinary stream, one with sparse long codes, one of case 3a, from start bits (3, 0, 5): the
    per-channel status and the per-channel replays must not mix"""
    stacks, sb = 2, (3, 0, 5)
    q, exp, ref = _stream_case(("ordinary", "long", "limit"), depth, w, h, stacks, sb, name)
    ctx = qctx(depth)
    T = _set_table(ctx, depth, name)
    assert not _has_replay_cube(q[:, 0], T, depth) and _has_replay_cube(q[:, 1], T, depth)
    _decode_streams_every_way(ctx, exp, sb, (stacks * depth, h, w, 3), ref, True)


@pytest.mark.parametrize("start_bit", range(1, 8))
@pytest.mark.parametrize("depth", [8, 4])
def test_stream_decode_grey_start_bits(pkg, qctx, depth, start_bit):
    """3e: the stream begins at bit 1 .. 7 of its first byte (163 x 13 and 48 x 32 in turn, seeded and all255 in
    turn); the end bits are compared"""
    w, h = (163, 13) if start_bit % 2 else (48, 32)
    name = ("seeded", "all255")[(start_bit // 2) % 2]
    q, exp, ref = _stream_case(("limit",), depth, w, h, 2, (start_bit,), name)
    ctx = qctx(depth)
    T = _set_table(ctx, depth, name)
    assert exp[0][1] == start_bit + int(qc.code_bits(q).sum())
    _decode_streams_every_way(ctx, exp, (start_bit,), (2 * depth, h, w), ref, _has_replay_cube(q, T, depth))


# ---- 3f: the encode side --------------------------------------------------------------------------------------------

def _encode_content(depth, channels, w, h):
    """5 stacks: the 0 / 255 checkerboard, then constant frames 0, 1, 128, 255"""
    z, y, x = np.meshgrid(np.arange(depth), np.arange(h), np.arange(w), indexing="ij")
    planes = [(((x + y + z) % 2) * 255).astype(np.uint8)] + [np.full((depth, h, w), c, np.uint8) for c in (0, 1, 128, 255)]
    fr = np.concatenate(planes)
    return fr if channels == 1 else np.ascontiguousarray(np.stack([fr, fr[::-1], np.roll(fr, depth, axis=0)], axis=-1))


@functools.lru_cache(maxsize=None)
def _encode_case(depth, channels, w, h, name):
    fr = _encode_content(depth, channels, w, h)
    q, out = qc.ref_frames(fr, _table(depth, name), depth)
    for a in (fr, q, out):
        a.setflags(write=False)
    return fr, q, out


@pytest.mark.parametrize("bits", [0, 3, 7])
@pytest.mark.parametrize("name", ["ones", "all255"])
@pytest.mark.parametrize("w,h,channels", [(48, 32, 1), (163, 13, 1), (13, 9, 3), (48, 32, 3)])
@pytest.mark.parametrize("depth", [8, 4])
def test_stream_encode_with_a_carry(pkg, qctx, depth, w, h, channels, name, bits):
    """3f: encode_eg_frames continuing a carried partial byte under ones (the longest codes the encoder emits) and
    all255, fused and two-step, on the checkerboard and constant frames: the oracle's stream with the same carry"""
    import oracle
    stacks = 5
    fr, q_ref, _ = _encode_case(depth, channels, w, h, name)
    carry = [(0xB4, bits), (0x6D, (bits + 3) % 8), (0x00, 0)][:channels]
    blocks = q_ref.reshape(stacks, channels, -1, 64 * depth)
    exp = [_expected(oracle, pkg, np.ascontiguousarray(blocks[:, ch]), depth, *carry[ch]) for ch in range(channels)]
    ctx = qctx(depth)
    _set_table(ctx, depth, name)
    assert ctx.encode_eg_frames(fr, carry) == exp, "fused"
    with ctx_option(ctx, pkg.DCT3D_OPT_EG_TWO_STEP, 1):
        assert ctx.encode_eg_frames(fr, carry) == exp, "two-step"


# ---- 2: nothing written outside the frames ----------------------------------------------------------------------------

def _words(bits):
    return (bits + 31) // 32 * 4


# all255 on half of the cases and seeded on the others: either reaches the same instantiation and store path
BAND_CASES = [(d, ch, w, h, st, "all255" if (d == 8) == (ch == 1) else "seeded")
              for d in (8, 4) for ch in (1, 3) for (w, h) in [(163, 13), (13, 9), (168, 8)] for st in (1, 2)]


@pytest.mark.parametrize("depth,channels,w,h,stacks,name", BAND_CASES)
def test_device_calls_write_nothing_outside_their_outputs(pkg, qctx, depth, channels, w, h, stacks, name):
    """2: the masked and the per-lane stores of the table kernels, device forms: every output lies between two
    4 KiB bands of a canary byte, which stay as they were; the outputs equal the reference.  Stream buffers have
    exactly the capacity the call was told (the stream's words)."""
    import torch
    ctx = qctx(depth)
    T = _set_table(ctx, depth, name)
    shape = (stacks * depth, h, w) + ((3,) if channels == 3 else ())
    nbytes = int(np.prod(shape))
    # decode_frames_dev: the clip of section 1
    q, _ = _clip(name, depth, channels, w, h, stacks)
    ref = _clip_ref(name, depth, channels, w, h, stacks)
    buf, mid = qc.banded(torch, nbytes, CANARY)
    ctx.decode_frames_dev(_dev(q), w, h, channels, stacks, mid.data_ptr())
    ctx.synchronize()
    got, intact = qc.bands_intact(buf, nbytes, CANARY)
    assert intact, "decode_frames_dev wrote outside its output"
    assert np.array_equal(got.reshape(shape), ref)
    # decode_eg_frames_dev: foreign streams
    kinds = ("limit",) if channels == 1 else ("ordinary", "long", "limit")
    sb = (5,) if channels == 1 else (3, 0, 5)
    qs, exp, sref = _stream_case(kinds, depth, w, h, stacks, sb, name)
    ts, nb = _device_streams(exp)
    buf, mid = qc.banded(torch, nbytes, CANARY)
    eb = ctx.decode_eg_frames_dev(ts, nb, list(sb), w, h, stacks, mid.data_ptr())
    ctx.synchronize()
    got, intact = qc.bands_intact(buf, nbytes, CANARY)
    assert intact, "decode_eg_frames_dev wrote outside its output"
    assert eb == [e for _, e in exp] and np.array_equal(got.reshape(shape), sref)
    # encode_frames_dev: the int32 output between the bands
    fr = _frames(depth, channels, w, h, stacks, 2)  # a checkerboard stack first
    q_ref, _ = qc.ref_frames(fr, T, depth)
    buf, mid = qc.banded(torch, q_ref.size * 4, CANARY)
    ctx.encode_frames_dev(_dev(fr), w, h, channels, stacks, mid.data_ptr())
    ctx.synchronize()
    got, intact = qc.bands_intact(buf, q_ref.size * 4, CANARY)
    assert intact, "encode_frames_dev wrote outside its output"
    assert np.array_equal(got.view(np.int32), q_ref.reshape(-1))
    # encode_eg_frames_dev: each channel's capacity is its stream's words, the bands begin right there
    blocks = q_ref.reshape(stacks, channels, -1, 64 * depth)
    carry = [(0xB4, 3), (0x6D, 0), (0xFE, 7)][:channels]
    import oracle
    sexp = [_expected(oracle, pkg, np.ascontiguousarray(blocks[:, ch]), depth, *carry[ch]) for ch in range(channels)]
    caps = [_words(bits) for _, bits in sexp]
    bufs = [qc.banded(torch, cap, CANARY) for cap in caps]
    tb = ctx.encode_eg_frames_dev(_dev(fr), w, h, channels, stacks, [m.data_ptr() for _, m in bufs], caps, carry)
    ctx.synchronize()
    assert tb == [bits for _, bits in sexp]
    for ch, ((b, _), cap) in enumerate(zip(bufs, caps)):
        got, intact = qc.bands_intact(b, cap, CANARY)
        assert intact, f"encode_eg_frames_dev wrote outside channel {ch}'s {cap} bytes"
        assert got[:len(sexp[ch][0])].tobytes() == sexp[ch][0] and not got[len(sexp[ch][0]):].any()


# ---- 4: errors leave the context usable ---------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,channels", [(128, 64, 1), (50, 21, 3)])
@pytest.mark.parametrize("depth", [8, 4])
def test_errors_leave_the_table_and_the_context_usable(pkg, qctx, depth, w, h, channels):
    """4: with the seeded table set, a stream cut to half its length is DCT3D_ENODATA (RGB: only the second channel
    is cut, and the device form's .end_bits holds the first channel's true end bit); six zero bytes in the middle
    are DCT3D_EINVAL or DCT3D_ENODATA.  After each failure the table is still set and the same context decodes the
    intact streams to the reference.  (test_fused_decode_truncated_and_corrupt's two corruptions.)"""
    import torch
    stacks = 2
    kinds, sb = (("limit",), (0,)) if channels == 1 else (("ordinary", "limit", "long"), (3, 0, 5))
    q, exp, ref = _stream_case(kinds, depth, w, h, stacks, sb, "seeded")
    ctx = qctx(depth)
    T = _set_table(ctx, depth, "seeded")
    shape = ref.shape
    bad_ch = channels // 2  # grey: the stream; RGB: the second channel
    good = [b for b, _ in exp]
    ends = [e for _, e in exp]

    def intact():
        assert np.array_equal(ctx.quant(), T)
        _decode_streams_every_way(ctx, exp, sb, shape, ref, True)

    def both_forms(streams, codes):
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.decode_eg_frames(streams, w, h, stacks, list(sb))
        assert e.value.code in codes
        ts, nb = _device_streams([(b, 0) for b in streams])
        out = torch.zeros(int(np.prod(shape)), dtype=torch.uint8, device="cuda")
        with pytest.raises(pkg.Dct3dError) as e:
            ctx.decode_eg_frames_dev(ts, nb, list(sb), w, h, stacks, out)
        ctx.synchronize()
        assert e.value.code in codes
        return e.value.end_bits

    intact()
    cut = list(good)
    cut[bad_ch] = good[bad_ch][:len(good[bad_ch]) // 2]
    end_bits = both_forms(cut, (pkg.DCT3D_ENODATA,))
    if channels == 3:
        assert end_bits[0] == ends[0]
    intact()
    zeroed = list(good)
    b = bytearray(good[bad_ch])
    b[len(b) // 3: len(b) // 3 + 6] = bytes(6)  # 48 zero bits: no valid code
    zeroed[bad_ch] = bytes(b)
    both_forms(zeroed, (pkg.DCT3D_EINVAL, pkg.DCT3D_ENODATA))
    intact()


# ---- 5: the table as state between queued calls -------------------------------------------------------------------------

QUEUED = (136, 72, 3)  # w, h, stacks: the first call's kernels are still running when set_quant arrives


QUEUED_TABLES = ("seeded", "all255")


@functools.lru_cache(maxsize=None)
def _queued_case(depth, channels, name):
    """what each of the four device calls gives for its input alone under table `name`: (q of the frames, the frames'
    streams, the decode of the foreign q -- the first table's clip of section 1 under either table --, the foreign
    streams, their decode)"""
    import oracle
    w, h, stacks = QUEUED
    T = _table(depth, name)
    fr = _frames(depth, channels, w, h, stacks, 0)
    q_enc, _ = qc.ref_frames(fr, T, depth)
    blocks = q_enc.reshape(stacks, channels, -1, 64 * depth)
    s_enc = [_expected(oracle, qc.pkg(), np.ascontiguousarray(blocks[:, ch]), depth) for ch in range(channels)]
    kinds = ("limit",) if channels == 1 else ("ordinary", "long", "limit")
    _, exp, s_dec = _stream_case(kinds, depth, w, h, stacks, (0,) * channels, name)
    q_in, _ = _clip(QUEUED_TABLES[0], depth, channels, w, h, stacks)
    q_dec = qc.ref_decode_frames(q_in, w, h, stacks, channels, T, depth)
    return q_enc, s_enc, q_dec, exp, s_dec


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("depth,channels", [(8, 1), (4, 1), (4, 3)])
def test_set_quant_between_queued_calls(pkg, qctx, depth, channels, side_stream):
    """5: a device call queued under T1, then -- with no synchronisation by the test -- set_quant(T2) and the same
    call queued under T2 into a second output: each output is its own table's reference, for the stream decode
    (it returns while its consumer runs), the stream encode, the int32 encode and the int32 decode; on the
    context's own stream and on a torch side stream.  The int32 decode's input is T1's clip of section 1 both
    times (one q array, two tables)."""
    import torch
    w, h, stacks = QUEUED
    names = QUEUED_TABLES
    ctx = qctx(depth)
    fr = _frames(depth, channels, w, h, stacks, 0)
    cases = [_queued_case(depth, channels, n) for n in names]
    q_in, _ = _clip(names[0], depth, channels, w, h, stacks)
    dec_refs = [cases[0][2], cases[1][2]]
    assert not np.array_equal(dec_refs[0], dec_refs[1]) and not np.array_equal(cases[0][0], cases[1][0])
    exp = cases[0][3]
    assert [b for b, _ in exp] == [b for b, _ in cases[1][3]], "the same streams under both tables"
    ts, nb = _device_streams(exp)
    d_fr, d_q = _dev(fr), _dev(q_in)
    s = torch.cuda.Stream() if side_stream else None
    _set_table(ctx, depth, names[0])
    torch.cuda.synchronize()
    try:
        if s is not None:
            ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s) if s is not None else torch.cuda.stream(torch.cuda.current_stream()):
            # stream decode
            outs = [torch.full(fr.shape, 0x5A, dtype=torch.uint8, device="cuda") for _ in names]
            ctx.synchronize()
            ebs = []
            for k, name in enumerate(names):
                ctx.set_quant(_table(depth, name))
                ebs.append(ctx.decode_eg_frames_dev(ts, nb, [0] * channels, w, h, stacks, outs[k]))
            ctx.synchronize()
            for k, name in enumerate(names):
                assert ebs[k] == [e for _, e in exp]
                assert np.array_equal(outs[k].cpu().numpy(), cases[k][4]), f"stream decode under {name}"
            # int32 decode
            outs = [torch.full(fr.shape, 0x5A, dtype=torch.uint8, device="cuda") for _ in names]
            ctx.synchronize()
            for k, name in enumerate(names):
                ctx.set_quant(_table(depth, name))
                ctx.decode_frames_dev(d_q, w, h, channels, stacks, outs[k])
            ctx.synchronize()
            for k, name in enumerate(names):
                assert np.array_equal(outs[k].cpu().numpy(), dec_refs[k]), f"int32 decode under {name}"
            # int32 encode
            outs = [torch.full((cases[0][0].size,), -7, dtype=torch.int32, device="cuda") for _ in names]
            ctx.synchronize()
            for k, name in enumerate(names):
                ctx.set_quant(_table(depth, name))
                ctx.encode_frames_dev(d_fr, w, h, channels, stacks, outs[k])
            ctx.synchronize()
            for k, name in enumerate(names):
                assert np.array_equal(outs[k].cpu().numpy(), cases[k][0].reshape(-1)), f"int32 encode under {name}"
            # stream encode
            caps = [[_words(bits) + 8 for _, bits in cases[k][1]] for k in range(2)]
            outs = [[torch.zeros(cap, dtype=torch.uint8, device="cuda") for cap in caps[k]] for k in range(2)]
            ctx.synchronize()
            tbs = []
            for k, name in enumerate(names):
                ctx.set_quant(_table(depth, name))
                tbs.append(ctx.encode_eg_frames_dev(d_fr, w, h, channels, stacks, outs[k], caps[k]))
            ctx.synchronize()
            for k, name in enumerate(names):
                assert tbs[k] == [bits for _, bits in cases[k][1]], f"stream encode under {name}"
                for ch, (b, _) in enumerate(cases[k][1]):
                    assert outs[k][ch].cpu().numpy()[:len(b)].tobytes() == b, f"stream encode under {name}, channel {ch}"
    finally:
        ctx.synchronize()
        ctx.set_stream(None)




def _counts(st):
    return {k: st[k] for k in ("n_units", "n_flagged", "n_rechecked")}


@functools.lru_cache(maxsize=None)
def _alternating_case(depth, channels, w, h, stacks):
    """two clips under the reference table, the first with tie_cube at 12 cubes of its first stack (every channel:
    open coefficients for certain), the second without: [(frames, q, decoded frames, streams)]"""
    import oracle
    T = _table(depth, "forced")
    tie = _frames(depth, channels, w, h, stacks, 0).copy()
    cube = np.tile(tie_cube(depth, T), (1, 2, 6))  # 12 cubes of the first stack
    tie[:depth, :16, :48] = cube if channels == 1 else cube[..., None]
    res = []
    for fr in (tie, _frames(depth, channels, w, h, stacks, 1)):
        q, out = qc.ref_frames(fr, T, depth)  # (Plan.encode_q / decode_q for this table: test_quant_plan.py)
        blocks = q.reshape(stacks, channels, -1, 64 * depth)
        streams = [_expected(oracle, qc.pkg(), np.ascontiguousarray(blocks[:, ch]), depth) for ch in range(channels)]
        res.append((fr, q, out, streams))
    return res


@pytest.mark.parametrize("call", ["decode_eg", "encode_eg", "encode", "decode"])
@pytest.mark.parametrize("depth,channels", [(8, 1), (4, 3)])
def test_product_and_table_kernels_alternate(pkg, qctx, depth, channels, call):
    """5: eight calls back to back on one context with the reference table, DCT3D_OPT_QUANT_FORCE_TABLE toggled
    before each, a clip with a tie cube and one without in turn (0 1 1 0 1 0 0 1: each clip meets each family): the
    two kernel families share the alternating counter and status slots.  Every output is the single call's, and
    stats() after the last synchronise is the last call's alone.  The rare paths run: the second certificate is off
    for the encodes; the decodes' margin is widened by 0.01, which sends about half of the lanes to the replay, so
    that the two clips count differently."""
    import torch
    w, h, stacks = 50, 21, 3
    ctx = qctx(depth)
    clips = _alternating_case(depth, channels, w, h, stacks)
    d_frs = [_dev(c[0]) for c in clips]
    d_qs = [_dev(c[1]) for c in clips]
    d_ss = [_device_streams(c[3]) for c in clips]

    def queue(k, force):
        """clip k through the table kernels (force) or the product kernels: (output tensors, the value returned)"""
        ctx.set_option(pkg.DCT3D_OPT_QUANT_FORCE_TABLE, force)
        fr, q, _, streams = clips[k]
        if call == "decode_eg":
            o = torch.full(fr.shape, 0x5A, dtype=torch.uint8, device="cuda")
            return [o], ctx.decode_eg_frames_dev(d_ss[k][0], d_ss[k][1], [0] * channels, w, h, stacks, o)
        if call == "decode":
            o = torch.full(fr.shape, 0x5A, dtype=torch.uint8, device="cuda")
            return [o], ctx.decode_frames_dev(d_qs[k], w, h, channels, stacks, o)
        if call == "encode":
            o = torch.full((q.size,), -7, dtype=torch.int32, device="cuda")
            return [o], ctx.encode_frames_dev(d_frs[k], w, h, channels, stacks, o)
        caps = [_words(bits) + 8 for _, bits in streams]
        o = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for cap in caps]
        return o, ctx.encode_eg_frames_dev(d_frs[k], w, h, channels, stacks, o, caps)

    def check(k, outs, ret, what):
        _, q, out, streams = clips[k]
        if call in ("decode_eg", "decode"):
            assert np.array_equal(outs[0].cpu().numpy(), out), what
            if call == "decode_eg":
                assert ret == [bits for _, bits in streams], what
        elif call == "encode":
            assert np.array_equal(outs[0].cpu().numpy(), q.reshape(-1)), what
        else:
            assert ret == [bits for _, bits in streams], what
            for ch, (b, _) in enumerate(streams):
                assert outs[ch].cpu().numpy()[:len(b)].tobytes() == b, (what, ch)

    ctx.set_quant(None)
    ctx.set_option(pkg.DCT3D_OPT_DEC_MARGIN, 0.01 if call in ("decode_eg", "decode") else 0)
    ctx.set_option(pkg.DCT3D_OPT_ENC_NO_RECHECK, 1)
    try:
        alone = {}
        for k in (0, 1):
            for force in (0, 1):
                outs, ret = queue(k, force)
                ctx.synchronize()
                alone[k, force] = _counts(ctx.stats())
                check(k, outs, ret, f"alone: clip {k}, force {force}")
        assert alone[0, 0]["n_flagged"] > 0 and alone[0, 1]["n_flagged"] > 0, alone
        assert alone[0, 0] != alone[1, 0] and alone[0, 1] != alone[1, 1], "a mixture of the two clips' counts would show"
        torch.cuda.synchronize()
        order = [(k, (i + 1) % 2) for i, k in enumerate((0, 1, 1, 0, 1, 0, 0, 1))]  # (clip, force)
        assert set(order) == {(0, 0), (0, 1), (1, 0), (1, 1)}
        queued = [queue(k, force) for k, force in order]
        ctx.synchronize()
        st = _counts(ctx.stats())
        for i, ((k, force), (outs, ret)) in enumerate(zip(order, queued)):
            check(k, outs, ret, f"queued call {i}: clip {k}, force {force}")
        assert st == alone[order[-1]], (st, order[-1], alone)
    finally:
        ctx.synchronize()
        for opt in (pkg.DCT3D_OPT_QUANT_FORCE_TABLE, pkg.DCT3D_OPT_DEC_MARGIN, pkg.DCT3D_OPT_ENC_NO_RECHECK):
            ctx.set_option(opt, 0)
