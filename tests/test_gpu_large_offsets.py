"""GPU: streams past 2^32 bits, rasters past 4 GiB, 2^32 values and more.

Every other GPU test runs at sizes where a 32-bit counter and a 64-bit counter give the same answer.  Each case here
crosses one threshold well inside its work -- thousands of cubes and many blocks of every kernel on both sides -- and
compares every output bit with the reference.  The reference is large_common's cube pool: the oracle runs once on a
few hundred cubes, an id per cube is drawn from a seeded generator, and the raster, the coefficients, the decoded
raster, the stream offsets and the stream are indexings of the pool on the device (test_large_common.py compares
that construction with the oracle on a whole small clip).  Streams are read completely by large_common.check_stream,
which knows nothing of the library.  Every device output lies between two 4 KiB canary bands.

A case skips only when the device has less free memory than the peak its docstring states."""
import ctypes as C
import time

import numpy as np
import pytest

import large_common as lc
import quant_common as qc
from conftest import ctx_option

pytestmark = pytest.mark.gpu

B32 = 1 << 32
GIB = 1 << 30


@pytest.fixture
def lctx(pkg):
    """contexts of the test's own, closed at its end: a context keeps the work buffers of its largest call"""
    import torch
    made = []

    def get(depth):
        try:
            made.append(pkg.Context(0, 8, 8, depth))
        except Exception as e:
            pytest.fail(f"HIP context for 8x8x{depth} could not be created: {e}")
        return made[-1]

    yield get
    for c in made:
        c.close()
    torch.cuda.empty_cache()


def _need(gib):
    """skip when the device has less free memory than the case's stated peak"""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < gib * GIB:
        pytest.skip(f"needs {gib} GiB of device memory at its peak, {free / GIB:.1f} GiB are free")


def _report(name, t0, **figures):
    """the case's wall time and figures, for DESIGN 4h (shown with pytest -s)"""
    import torch
    torch.cuda.synchronize()
    print(f"\n[large] {name}: {time.time() - t0:.2f} s " + " ".join(f"{k}={v}" for k, v in figures.items()))


def _dev_ids(ids):
    import torch
    return torch.from_numpy(ids).cuda()


def _words_cap(total_bits):
    return (total_bits + 31) // 32 * 4


def _assert_stream(words, dp, t_ids, carry, total):
    import torch
    bad, first, tot, ends = lc.check_stream(torch, words, dp, t_ids, *carry)
    assert tot == total
    assert bad == 0, f"{bad} cubes of the stream differ from the pool's, the first is cube {first}"
    assert ends, "the carried bits or the zero padding after the last bit"


def _past(off, threshold):
    """cubes that start at or past a bit threshold"""
    return int((off >= threshold).sum())


def _raw_eg_decode(pkg, ctx, d_bytes, nbytes, start_bit, n_cubes, d_q):
    """dct3d_eg_decode_dev itself: (return code, end bit) -- the binding raises and drops the end bit"""
    eb = C.c_uint64(0xDEAD)
    rc = pkg.lib().dct3d_eg_decode_dev(ctx._h, d_bytes, nbytes, start_bit, n_cubes, d_q, C.byref(eb))
    return rc, eb.value


# ---- A1, A2: the entropy stage on int32 cubes, bit positions >= 2^32 -------------------------------------------------

A_CARRY = (0xA8, 5)


def _a1_inputs(depth):
    """(device pool, ids, device ids, offsets, total bits): synthetic coefficient cubes whose stream is about
    2^32 + 2^27 bits long"""
    import torch
    pool = lc.synthetic_q_pool(depth)
    n = int((B32 + (1 << 27)) / pool.bits.mean())
    ids = lc.draw_ids(n, pool.k, 510 + depth, pool.cs)
    dp = pool.dev(torch, "cuda")
    t_ids = _dev_ids(ids)
    off, total = lc.offsets(torch, dp.bits, t_ids, A_CARRY[1])
    assert total > B32 + (1 << 26) and _past(off, B32) >= 3000 and _past(off, B32) <= n - 3000
    return dp, ids, t_ids, off, total


def _a1_encode(ctx, dp, t_ids, total):
    """eg_encode_dev of the pool's cubes into a banded buffer of exactly the stream's words: (buffer, its words)"""
    import torch
    q = dp.q[t_ids]
    cap = _words_cap(total)
    buf, mid = lc.banded(torch, cap)
    tb = ctx.eg_encode_dev(q, len(t_ids), mid.data_ptr(), cap, *A_CARRY)
    ctx.synchronize()
    assert tb == total, (tb, total)
    assert lc.bands_intact(buf, cap), "eg_encode_dev wrote outside its output"
    return buf, mid.view(torch.int32)


@pytest.mark.parametrize("depth", [8, 4])
def test_a1_entropy_encode_past_2_32_bits(pkg, lctx, depth):
    """A1: dct3d_eg_encode_dev writes a stream of 2^32 + 2^27 bits (about 250 k cubes at depth 8, 500 k at depth 4) of
    synthetic coefficients: zero cubes, short codes, dense 33- to 61-bit codes, cube lengths of every residue mod 32,
    carry 5 bits.  The whole stream is read back and compared; total_bits = carry + the sum of the cubes' bits.
    Peak device memory 3 GiB (0.55 GiB of cubes, 0.55 GiB of stream, the check's slices)."""
    _need(3)
    t0 = time.time()
    dp, ids, t_ids, off, total = _a1_inputs(depth)
    buf, words = _a1_encode(lctx(depth), dp, t_ids, total)
    _assert_stream(words, dp, t_ids, A_CARRY, total)
    _report(f"A1 depth {depth}", t0, cubes=len(ids), bits=total, cubes_past_2_32=_past(off, B32))


@pytest.mark.parametrize("depth", [8, 4])
def test_a2_entropy_decode_past_2_32_bits(pkg, lctx, depth):
    """A2: dct3d_eg_decode_dev on A1's stream (encoded again here; A1 is where its content is checked): all cubes
    from start bit 5, and the cubes from the first one that starts past bit 2^32, each with the default front, with
    DCT3D_OPT_EG_FUSED_FRONT and with DCT3D_OPT_EG_NO_RESOLVE; q equals the pool's, end_bit the total.  The buffer
    cut inside a cube past 2^32 is DCT3D_ENODATA, a copy with 64 zero bits at a cube boundary past 2^32 is
    DCT3D_EINVAL, and both leave end_bit = start_bit.  Peak device memory 4 GiB."""
    import torch
    _need(4)
    t0 = time.time()
    dp, ids, t_ids, off, total = _a1_inputs(depth)
    ctx = lctx(depth)
    n, cs = len(ids), dp.cs
    buf, words = _a1_encode(ctx, dp, t_ids, total)
    cap = _words_cap(total)
    g0 = int(torch.searchsorted(off, torch.tensor([B32 + 1], device="cuda"))[0])
    assert int(off[g0]) > B32 and 3000 <= n - g0 <= n - 3000
    obuf, omid = lc.banded(torch, n * cs * 4)
    out = omid.view(torch.int32).view(n, cs)
    for name, opts in (("default", {}), ("fused front", {pkg.DCT3D_OPT_EG_FUSED_FRONT: 1}),
                       ("no resolve", {pkg.DCT3D_OPT_EG_NO_RESOLVE: 1})):
        for o, v in opts.items():
            ctx.set_option(o, v)
        try:
            for first in (0, g0):
                out.fill_(-7)
                start = int(off[first])
                eb = ctx.eg_decode_dev(words.data_ptr(), cap, start, n - first, out.data_ptr())
                ctx.synchronize()
                assert eb == total, (name, first, eb, total)
                assert lc.cube_mismatches(out[:n - first], dp.q, t_ids[first:]) == 0, (name, first)
                assert bool((out[n - first:] == -7).all()) and lc.bands_intact(obuf, n * cs * 4), (name, first)
        finally:
            for o in opts:
                ctx.set_option(o, 0)
    # errors past 2^32, decoding from cube g0
    g1 = g0 + (n - g0) // 2
    start = int(off[g0])
    cut = (int(off[g1]) + int(dp.bits[t_ids[g1]]) // 2) // 32 * 4  # bytes: inside cube g1
    assert int(off[g1]) < 8 * cut < int(off[g1 + 1])
    rc, eb = _raw_eg_decode(pkg, ctx, words.data_ptr(), cut, start, n - g0, out.data_ptr())
    assert (rc, eb) == (pkg.DCT3D_ENODATA, start)
    bad = words.clone()
    z0 = (int(off[g1]) + 7) // 8
    bad.view(torch.uint8)[z0:z0 + 8] = 0  # 64 zero bits from the first byte boundary of cube g1
    rc, eb = _raw_eg_decode(pkg, ctx, bad.data_ptr(), cap, start, n - g0, out.data_ptr())
    assert (rc, eb) == (pkg.DCT3D_EINVAL, start)
    # and the context still decodes
    out.fill_(-7)
    assert ctx.eg_decode_dev(words.data_ptr(), cap, start, n - g0, out.data_ptr()) == total
    ctx.synchronize()
    assert lc.cube_mismatches(out[:n - g0], dp.q, t_ids[g0:]) == 0
    _report(f"A2 depth {depth}", t0, cubes=n, first_cube_past_2_32=g0)


# ---- A3: small real streams placed across bit 2^32 ----------------------------------------------------------------------

A3_BUF = 513 << 20
A3_CASES = {"grey64": (64, 64, 1), "grey_edge": (61, 45, 1), "rgb_edge": (61, 45, 3)}


def _a3_reference(pool, ids, w, h, channels, stacks, depth):
    """the decode of the cubes ids [stack][channel][cube] of the padded raster, cropped: frames [F, h, w(, 3)]"""
    import oracle
    wp, hp = qc.pkg().padded_size(w, h)
    planes = oracle.from_cubes(pool.px_out[ids.reshape(-1)].reshape(-1, depth, 8, 8), wp, hp, channels * stacks * depth)
    if channels == 3:
        planes = qc.packed(planes, depth)
    return np.ascontiguousarray(planes[:, :h, :w])


@pytest.mark.parametrize("table", [None, "q1"])
@pytest.mark.parametrize("case", list(A3_CASES))
def test_a3_small_streams_across_bit_2_32(pkg, lctx, case, table):
    """A3: 2 stacks of pool-built cubes (64 x 64 grey; 61 x 45 grey; 61 x 45 packed RGB24), their oracle streams copied
    into zeroed 513 MiB device buffers so that they begin at bit 2^32 - 4099 and at bit 2^32 - 7 (RGB: the channels at
    2^32 - 4099 or 2^32 - 7, at 3 in a small buffer, at 2^32 + 12345), decoded by dct3d_decode_eg_frames_dev (64 x 64
    also by dct3d_decode_eg_dev), with the margin of DCT3D_OPT_DEC_MARGIN 0 and 0.45 (the in-wave exact replay re-reads
    the stream), under the reference quantiser and quant_table(1).  Frames and end bits are exact.  Peak 1.1 GiB."""
    import torch
    _need(2)
    t0 = time.time()
    depth, stacks = 8, 2
    w, h, channels = A3_CASES[case]
    wp, hp = pkg.padded_size(w, h)
    cps = (wp // 8) * (hp // 8)
    pool = lc.general_pool(depth, table)
    ids = np.random.default_rng(31 + channels + w).integers(0, pool.k, size=(stacks, channels, cps))
    ref = _a3_reference(pool, ids, w, h, channels, stacks, depth)
    streams = [lc.build_stream(pool, ids[:, ch].reshape(-1)) for ch in range(channels)]
    ctx = lctx(depth)
    ctx.set_quant(None if table is None else qc.tables(depth)[table])
    big = [torch.zeros(A3_BUF, dtype=torch.uint8, device="cuda") for _ in range(2 if channels == 3 else 1)]
    small = torch.zeros(1 << 18, dtype=torch.uint8, device="cuda")
    nbytes = int(np.prod(ref.shape))
    for first_at in (B32 - 4099, B32 - 7):
        ats = [first_at] if channels == 1 else [first_at, 3, B32 + 12345]
        bufs = big[:1] if channels == 1 else [big[0], small, big[1]]
        nb, ends = [], []
        for ch in range(channels):
            data, byte0, start, end = lc.place_stream(*streams[ch], ats[ch])
            bufs[ch].zero_()
            bufs[ch][byte0:byte0 + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
            nb.append((byte0 + len(data) + 3) // 4 * 4)
            ends.append(end)
        assert ats[0] < B32 < ends[0] and nb[0] <= A3_BUF
        for margin in (0, 0.45):
            with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, margin):
                obuf, omid = lc.banded(torch, nbytes)
                eb = ctx.decode_eg_frames_dev(bufs, nb, ats, w, h, stacks, omid.data_ptr())
                ctx.synchronize()
                st = ctx.stats()
                assert eb == ends, (first_at, margin, eb, ends)
                assert lc.bands_intact(obuf, nbytes)
                got = omid.cpu().numpy().reshape(ref.shape)
                assert np.array_equal(got, ref), f"at {first_at}, margin {margin}: {(got != ref).sum()} bytes differ"
                if margin:
                    assert st["n_flagged"] > 0, "the exact replay ran"
                if case == "grey64":
                    obuf, omid = lc.banded(torch, nbytes)
                    eb = ctx.decode_eg_dev(bufs[0], nb[0], ats[0], w, h, stacks, omid.data_ptr())
                    ctx.synchronize()
                    assert eb == ends[0] and lc.bands_intact(obuf, nbytes)
                    assert np.array_equal(omid.cpu().numpy().reshape(ref.shape), ref), (first_at, margin)
    _report(f"A3 {case} {table}", t0)


# ---- A4, B2, B3: the fused stream calls ---------------------------------------------------------------------------------

def _fused_round_trip(pkg, ctx, dp, ids, w, h, stacks, carry, name, small_rate=None):
    """dct3d_encode_eg_dev of the pool-built raster (the whole stream checked), then dct3d_decode_eg_dev of that
    stream from its carry (the raster compared with the pool's decode); returns (total bits, offsets, n_flagged)"""
    import torch
    depth = dp.depth
    nby, nbx = h // 8, w // 8
    t_ids = _dev_ids(ids)
    off, total = lc.offsets(torch, dp.bits, t_ids, carry[1])
    raster = lc.fill_raster(torch.empty((stacks * depth, h, w), dtype=torch.uint8, device="cuda"), dp.px_in, t_ids,
                            stacks, nby, nbx, depth)
    cap = _words_cap(total)
    sbuf, smid = lc.banded(torch, cap)
    tb = ctx.encode_eg_dev(raster, w, h, stacks, smid.data_ptr(), cap, *carry)
    ctx.synchronize()
    assert tb == total, (name, tb, total)
    assert lc.bands_intact(sbuf, cap), "encode_eg_dev wrote outside its output"
    _assert_stream(smid.view(torch.int32), dp, t_ids, carry, total)
    del raster
    nbytes = stacks * depth * h * w
    obuf, omid = lc.banded(torch, nbytes)
    eb = ctx.decode_eg_dev(smid.data_ptr(), cap, carry[1], w, h, stacks, omid.data_ptr())
    ctx.synchronize()
    flagged = ctx.stats()["n_flagged"]
    assert eb == total, (name, eb, total)
    assert lc.bands_intact(obuf, nbytes), "decode_eg_dev wrote outside its output"
    bad = lc.raster_mismatches(omid.view(stacks * depth, h, w), dp.px_out, t_ids, stacks, nby, nbx, depth)
    assert bad == 0, f"{name}: {bad} bytes of the decoded raster differ"
    return total, off, flagged


@pytest.mark.parametrize("table", ["ones", "forced"])
def test_a4_fused_stream_past_2_32_bits(pkg, lctx, table):
    """A4: dct3d_encode_eg_dev writes more than 2^32 bits of pool-built 1920 x 1080 grey frames, dct3d_decode_eg_dev
    reads them back.  `ones`: the all-ones table, the most bits per pixel a quantiser gives: the general pool's mean is
    3,623.7 bits per cube, so 38 stacks (1.23 M cubes) give 2^32 x 1.03 bits (computed from the pool below, and
    printed).  `forced`: the reference table through DCT3D_OPT_QUANT_FORCE_TABLE: 1,002.9 bits per cube, 137 stacks
    (4.44 M cubes).  The whole stream is checked, the decoded raster equals the pool's decode, and the decode's
    replayed pixels per cube are those of a one-stack run within a half and the sampling noise (a sanity check).
    Peak device memory: ones 4 GiB, forced 14 GiB (the raster, the encoder's slots of 13.5 KiB per 8 cubes, the
    stream, the decoded raster)."""
    import torch
    _need(4 if table == "ones" else 14)
    t0 = time.time()
    depth, w, h = 8, 1920, 1080
    cps = (w // 8) * (h // 8)
    pool = lc.general_pool(depth, "ones" if table == "ones" else None)
    mean = float(pool.bits.mean())
    stacks = int(np.ceil(B32 * 1.03 / (mean * cps)))
    ids = lc.draw_ids(stacks * cps, pool.k, 77, pool.cs)
    dp = pool.dev(torch, "cuda")
    ctx = lctx(depth)
    if table == "ones":
        ctx.set_quant(qc.tables(depth)["ones"])
    else:
        ctx.set_option(pkg.DCT3D_OPT_QUANT_FORCE_TABLE, 1)
    _, _, small = _fused_round_trip(pkg, ctx, dp, ids[:cps], w, h, 1, (0x5C, 3), "one stack")
    total, off, flagged = _fused_round_trip(pkg, ctx, dp, ids, w, h, stacks, (0x5C, 3), "A4")
    assert total > B32 * 1.01 and 3000 <= _past(off, B32) <= len(ids) - 3000
    rate, small_rate = flagged / (stacks * cps), small / cps
    noise = 160 * (np.sqrt(small / 32) + 1) / cps  # five deviations of the one-stack run's count of replayed lanes
    assert abs(rate - small_rate) <= 0.5 * small_rate + noise, (rate, small_rate)
    _report(f"A4 {table}", t0, mean_bits_per_cube=round(mean, 1), stacks=stacks, bits=total,
            cubes_past_2_32=_past(off, B32), replay_rate=round(rate, 4), small_rate=round(small_rate, 4))


def _constant_heavy_ids(pool, n, seed):
    return lc.draw_ids(n, pool.k, seed, pool.cs, lc.constant_heavy_weights(pool.k))


def test_b2_fused_calls_past_2_32_values(pkg, lctx):
    """B2: dct3d_encode_eg_dev and dct3d_decode_eg_dev at 2048 x 2048, 129 stacks: 2^23 + 2^16 cubes, 4.33 G values, a
    4.03 GiB raster, and -- from the constant-heavy pool, 540.7 bits per cube -- a stream of 2^32 x 1.064 bits (545 MiB),
    past 2^32 bits too.  Separate from A4 so that a failure names its threshold.  The whole stream is checked and the
    decoded raster compared with the pool's decode.  Peak device memory 20 GiB (the raster 4.03, the encoder's slots
    14.6, the stream 0.6; the input raster is freed before the decoded one is made)."""
    import torch
    _need(20)
    t0 = time.time()
    depth, w, h, stacks = 8, 2048, 2048, 129
    pool = lc.constant_heavy_pool(depth)
    n = stacks * (w // 8) * (h // 8)
    assert n == (1 << 23) + (1 << 16) and n * pool.cs > B32 and stacks * depth * w * h > B32
    ids = _constant_heavy_ids(pool, n, 88)
    total, off, _ = _fused_round_trip(pkg, lctx(depth), pool.dev(torch, "cuda"), ids, w, h, stacks, (0x00, 0), "B2")
    assert total > B32 and 3000 <= _past(off, B32) <= n - 3000
    _report("B2", t0, cubes=n, bits=total, cubes_past_2_32_bits=_past(off, B32))


def test_b3_one_stack_past_4_gib(pkg, lctx):
    """B3: one stack of 23176 x 23176 frames at depth 8: plane * depth = 4.0005 GiB >= 2^32, so blk_store is 0 and the
    byte offsets inside the stack need 64 bits.  2897^2 = 8,392,609 cubes: under the cube limit 2^28 and under the
    FastDiv bound 2^31 (asserted).  Through the fused calls only (the int32 side of this size is B1's): the stream of
    the constant-heavy pool's raster, checked whole, decoded by dct3d_decode_eg_dev and compared with the pool's
    decode.  Peak device memory 20 GiB (as B2)."""
    import torch
    _need(20)
    t0 = time.time()
    depth, w, stacks = 8, 23176, 1
    n = (w // 8) ** 2
    assert w % 8 == 0 and w * w * depth >= B32 and (w - 8) * (w - 8) * depth < B32 and n == 2897**2 < (1 << 28) < (1 << 31)
    pool = lc.constant_heavy_pool(depth)
    ids = _constant_heavy_ids(pool, n, 89)
    total, off, _ = _fused_round_trip(pkg, lctx(depth), pool.dev(torch, "cuda"), ids, w, w, stacks, (0xE0, 3), "B3")
    _report("B3", t0, cubes=n, bits=total)


# ---- B1: the int32 calls, value indices >= 2^32 ---------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [8, 4])
def test_b1_int32_calls_past_2_32_values(pkg, lctx, depth):
    """B1: dct3d_encode_stacks_dev and dct3d_decode_stacks_dev at 2048 x 2048, 129 stacks = 2^23 + 2^16 cubes.  Depth 8:
    a 4.03 GiB raster and 16.1 GiB of int32; element 2^31 is in cube 2^22, element 2^32 in cube 2^23, byte 2^32 of the
    raster in stack 128.  Depth 4, the twin at the smallest size that crosses 2^31 elements (cube 2^23 of 256 values):
    2.02 GiB and 8.06 GiB.  Both directions against the pool, in slices on the device; the decode's input is the
    pool's coefficients, written over the encode's output.  Peak device memory 21 GiB at depth 8 (int32 16.1, one
    raster 4.03, slices), 11 GiB at depth 4."""
    import torch
    _need(21 if depth == 8 else 11)
    t0 = time.time()
    w, h, stacks = 2048, 2048, 129
    nby, nbx = h // 8, w // 8
    n = stacks * nby * nbx
    pool = lc.general_pool(depth)
    cs = pool.cs
    assert n == (1 << 23) + (1 << 16) and n * cs > (B32 if depth == 8 else 1 << 31)
    ids = lc.draw_ids(n, pool.k, 66 + depth, cs)
    dp, t_ids, ctx = pool.dev(torch, "cuda"), _dev_ids(ids), lctx(depth)
    raster = lc.fill_raster(torch.empty((stacks * depth, h, w), dtype=torch.uint8, device="cuda"), dp.px_in, t_ids,
                            stacks, nby, nbx, depth)
    qbuf, qmid = lc.banded(torch, n * cs * 4)
    ctx.encode_stacks_dev(raster, w, h, stacks, qmid.data_ptr())
    ctx.synchronize()
    assert lc.bands_intact(qbuf, n * cs * 4), "encode_stacks_dev wrote outside its output"
    q = qmid.view(torch.int32).view(n, cs)
    bad = lc.cube_mismatches(q, dp.q, t_ids)
    assert bad == 0, f"{bad} cubes of the encode differ from the pool's"
    del raster
    for g0 in range(0, n, 1 << 18):
        q[g0:g0 + (1 << 18)] = dp.q[t_ids[g0:g0 + (1 << 18)]]
    nbytes = stacks * depth * h * w
    obuf, omid = lc.banded(torch, nbytes)
    ctx.decode_stacks_dev(q, w, h, stacks, omid.data_ptr())
    ctx.synchronize()
    assert lc.bands_intact(obuf, nbytes), "decode_stacks_dev wrote outside its output"
    bad = lc.raster_mismatches(omid.view(stacks * depth, h, w), dp.px_out, t_ids, stacks, nby, nbx, depth)
    assert bad == 0, f"{bad} bytes of the decoded raster differ"
    _report(f"B1 depth {depth}", t0, cubes=n, int32_gib=round(n * cs * 4 / GIB, 2))


# ---- B4, C: frames of any size and packed RGB24 past 4 GiB; the host-pointer calls past 2^31 bytes ----------------------

def _edge_ids(pool, stacks, channels, nby, nbx, seed):
    """ids [stacks, channels, nby, nbx]: interior cubes from the whole constant-heavy pool, the last block column and
    the last block row constant cubes (ids < 256): their edge-padded reference is the constant cube's own, while a
    load clamped to the wrong column or row would read a neighbour that differs.  Not periodic (asserted)."""
    ids = lc.draw_ids(stacks * channels * nby * nbx, pool.k, seed, pool.cs).reshape(stacks, channels, nby, nbx)
    rng = np.random.default_rng(seed + 1)
    ids[:, :, -1, :] = rng.integers(0, 256, size=(stacks, channels, nbx))
    ids[:, :, :, -1] = rng.integers(0, 256, size=(stacks, channels, nby))
    assert lc.alias_share(ids.reshape(-1), pool.cs) >= lc.ALIAS_SHARE
    return ids


def _stack_frames(cubes, ids_s, depth, h, w):
    """one stack's frames, cropped to h x w, from cubes[ids_s] (ids_s [channels, nby, nbx] on the device): a view
    [depth, h, w] (one channel) or [depth, h, w, 3] (packed RGB24)"""
    ch, nby, nbx = ids_s.shape
    c = cubes[ids_s.reshape(-1)].view(ch, nby, nbx, depth, 8, 8)
    planes = c.permute(0, 3, 1, 4, 2, 5).reshape(ch, depth, nby * 8, nbx * 8)[:, :, :h, :w]
    return planes[0] if ch == 1 else planes.permute(1, 2, 3, 0)


def _fill_frames(torch, cubes, t_ids, depth, h, w):
    stacks, ch = t_ids.shape[:2]
    out = torch.empty((stacks * depth, h, w) + ((3,) if ch == 3 else ()), dtype=torch.uint8, device="cuda")
    for s in range(stacks):
        out[s * depth:(s + 1) * depth] = _stack_frames(cubes, t_ids[s], depth, h, w)
    return out


def _frames_mismatches(got, cubes, t_ids, depth, h, w):
    return sum(int((got[s * depth:(s + 1) * depth] != _stack_frames(cubes, t_ids[s], depth, h, w)).sum())
               for s in range(t_ids.shape[0]))


def test_b4_rgb_frames_of_any_size_past_4_gib(pkg, lctx):
    """B4: packed RGB24 frames of 2045 x 2043 (padded 2048 x 2048), 44 stacks: a raster of 4.11 GiB -- byte 2^32 lies in
    stack 42, 1.2 stacks or 230 k int32 cubes before the end -- and 8.65 M int32 cubes (16.5 GiB: past 2^32 elements).
    (More stacks do not fit the 24 GiB a case may hold: the int32 side of 115 stacks is 43 GiB.)  Through
    dct3d_encode_frames_dev, dct3d_decode_frames_dev and the _eg_frames_dev pair (the three streams checked whole).
    The cubes of the last block column and row are constant, so their edge-padded reference is the pool's.  The
    decodes' crop is checked by the canary bands and by equality of the dense frames.  Peak device memory 21 GiB
    (int32 16.5, one raster 4.11, slices)."""
    import torch
    _need(21)
    t0 = time.time()
    depth, w, h, stacks = 8, 2045, 2043, 44
    nby = nbx = 256
    pool = lc.constant_heavy_pool(depth)
    cs = pool.cs
    nbytes = stacks * depth * h * w * 3
    assert nbytes > B32 + 1000 * 8 * 8 * 8 * 3 and 3 * stacks * nby * nbx * cs > B32
    ids = _edge_ids(pool, stacks, 3, nby, nbx, 91)
    dp, t_ids, ctx = pool.dev(torch, "cuda"), _dev_ids(ids), lctx(depth)
    flat = t_ids.reshape(-1)
    n = flat.numel()
    frames = _fill_frames(torch, dp.px_in, t_ids, depth, h, w)
    qbuf, qmid = lc.banded(torch, n * cs * 4)
    ctx.encode_frames_dev(frames, w, h, 3, stacks, qmid.data_ptr())
    ctx.synchronize()
    assert lc.bands_intact(qbuf, n * cs * 4), "encode_frames_dev wrote outside its output"
    q = qmid.view(torch.int32).view(n, cs)
    bad = lc.cube_mismatches(q, dp.q, flat)
    assert bad == 0, f"{bad} cubes of the encode differ from the pool's"
    del frames
    for g0 in range(0, n, 1 << 18):
        q[g0:g0 + (1 << 18)] = dp.q[flat[g0:g0 + (1 << 18)]]
    obuf, omid = lc.banded(torch, nbytes)
    ctx.decode_frames_dev(q, w, h, 3, stacks, omid.data_ptr())
    ctx.synchronize()
    assert lc.bands_intact(obuf, nbytes), "decode_frames_dev wrote outside its output"
    bad = _frames_mismatches(omid.view(stacks * depth, h, w, 3), dp.px_out, t_ids, depth, h, w)
    assert bad == 0, f"{bad} bytes of the decoded frames differ"
    del q, qmid, qbuf, omid, obuf
    # the stream pair: one stream per channel
    frames = _fill_frames(torch, dp.px_in, t_ids, depth, h, w)
    carry = [(0xB4, 3), (0x6D, 0), (0xFE, 7)]
    ch_ids = [t_ids[:, ch].reshape(-1).contiguous() for ch in range(3)]
    totals = [lc.offsets(torch, dp.bits, ch_ids[ch], carry[ch][1])[1] for ch in range(3)]
    caps = [_words_cap(t) for t in totals]
    sb = [lc.banded(torch, cap) for cap in caps]
    tb = ctx.encode_eg_frames_dev(frames, w, h, 3, stacks, [m.data_ptr() for _, m in sb], caps, carry)
    ctx.synchronize()
    assert tb == totals
    for ch in range(3):
        assert lc.bands_intact(sb[ch][0], caps[ch]), f"encode_eg_frames_dev wrote outside channel {ch}'s output"
        _assert_stream(sb[ch][1].view(torch.int32), dp, ch_ids[ch], carry[ch], totals[ch])
    del frames
    obuf, omid = lc.banded(torch, nbytes)
    eb = ctx.decode_eg_frames_dev([m.data_ptr() for _, m in sb], caps, [c[1] for c in carry], w, h, stacks, omid.data_ptr())
    ctx.synchronize()
    assert eb == totals and lc.bands_intact(obuf, nbytes), "decode_eg_frames_dev: end bits, or a write outside its output"
    bad = _frames_mismatches(omid.view(stacks * depth, h, w, 3), dp.px_out, t_ids, depth, h, w)
    assert bad == 0, f"{bad} bytes of the frames decoded from the streams differ"
    _report("B4", t0, cubes=n, raster_gib=round(nbytes / GIB, 2), stream_bits=totals)


C_BYTES = (1 << 31) + (1 << 25)


@pytest.mark.parametrize("w,h,stacks", [(2048, 1024, 130), (2045, 1021, 131), (2048, 1024, 258)])
def test_c_host_calls_past_2_31_bytes(pkg, lctx, w, h, stacks):
    """C: the host-pointer stream calls on a host raster of at least 2^31 + 2^25 bytes, where an int product in the chunk
    pipeline would be negative: 2048 x 1024, 130 stacks (exactly 2^31 + 2^25 bytes) through dct3d_encode_eg and
    dct3d_decode_eg; 2045 x 1021, 131 stacks through the any-size stream calls dct3d_encode_eg_frames and
    dct3d_decode_eg_frames with channels = 1 (the stream calls, not the int32 ones: their host array would be 9 GiB);
    2048 x 1024, 258 stacks: 4.03 GiB, past 2^32 bytes.  The streams equal the _dev call's for the same frames byte for
    byte (and are checked whole against the pool); the decoded frames equal the _dev call's and the pool's decode.
    Peak device memory 6 GiB at 130 stacks, 11 GiB at 258 (two rasters, the encoder's slots); the same in host memory."""
    import torch
    _need(6 if stacks < 200 else 11)
    t0 = time.time()
    depth = 8
    wp, hp = pkg.padded_size(w, h)
    nby, nbx = hp // 8, wp // 8
    edge = (wp, hp) != (w, h)
    pool = lc.constant_heavy_pool(depth)
    nbytes = stacks * depth * h * w
    limit = C_BYTES if stacks < 200 else B32
    assert limit <= nbytes < limit + 3 * depth * h * w, "the smallest count of stacks that reaches the size"
    ids = _edge_ids(pool, stacks, 1, nby, nbx, 93 + stacks)
    dp, t_ids, ctx = pool.dev(torch, "cuda"), _dev_ids(ids), lctx(depth)
    flat = t_ids.reshape(-1)
    carry = (0xD2, 6)
    d_frames = _fill_frames(torch, dp.px_in, t_ids, depth, h, w)
    h_frames = d_frames.cpu().numpy()
    total = lc.offsets(torch, dp.bits, flat, carry[1])[1]
    cap = _words_cap(total)
    # encode: the device call (checked against the pool), then the host call against it
    sbuf, smid = lc.banded(torch, cap)
    if edge:
        tb = ctx.encode_eg_frames_dev(d_frames, w, h, 1, stacks, [smid.data_ptr()], [cap], [carry])[0]
    else:
        tb = ctx.encode_eg_dev(d_frames, w, h, stacks, smid.data_ptr(), cap, *carry)
    ctx.synchronize()
    assert tb == total and lc.bands_intact(sbuf, cap)
    _assert_stream(smid.view(torch.int32), dp, flat, carry, total)
    dev_stream = smid[:(total + 7) // 8].cpu().numpy().tobytes()
    del d_frames
    t1 = time.time()
    if edge:
        (host_stream, tb), = ctx.encode_eg_frames(h_frames, [carry])
    else:
        host_stream, tb = ctx.encode_eg(h_frames, *carry)
    t_enc = time.time() - t1
    assert tb == total and host_stream == dev_stream, "the host call's stream differs from the device call's"
    del h_frames
    # decode
    obuf, omid = lc.banded(torch, nbytes)
    if edge:
        eb = ctx.decode_eg_frames_dev([smid.data_ptr()], [cap], [carry[1]], w, h, stacks, omid.data_ptr())[0]
    else:
        eb = ctx.decode_eg_dev(smid.data_ptr(), cap, carry[1], w, h, stacks, omid.data_ptr())
    ctx.synchronize()
    assert eb == total and lc.bands_intact(obuf, nbytes)
    d_out = omid.view(stacks * depth, h, w)
    assert _frames_mismatches(d_out, dp.px_out, t_ids, depth, h, w) == 0, "the device decode differs from the pool's"
    t1 = time.time()
    if edge:
        h_out, (eb,) = ctx.decode_eg_frames([host_stream], w, h, stacks, [carry[1]])
    else:
        h_out, eb = ctx.decode_eg(host_stream, w, h, stacks, carry[1])
    t_dec = time.time() - t1
    assert eb == total
    assert bool((torch.from_numpy(h_out).cuda() == d_out).all()), "the host decode differs from the device decode"
    _report(f"C {w}x{h}x{stacks}", t0, host_bytes=nbytes, host_encode_s=round(t_enc, 2), host_decode_s=round(t_dec, 2))


def test_c_host_int32_frames_calls_past_2_31_bytes(pkg, lctx):
    """C: dct3d_encode_frames and dct3d_decode_frames, channels = 1, 2045 x 1021 (no multiple of 8), 131 stacks: a host
    raster of 2^31 + 2^25 bytes and more, and 8.2 GiB of int32 in host memory, through the chunk pipeline.  The
    coefficients equal the pool's (which B4 shows the _dev call to write), the decoded frames the pool's decode.
    Peak device memory 3 GiB (the pipeline's chunks, the comparison's slices); 13 GiB of host memory."""
    import torch
    _need(3)
    t0 = time.time()
    depth, w, h, stacks = 8, 2045, 1021, 131
    nby, nbx = 128, 256
    pool = lc.constant_heavy_pool(depth)
    assert stacks * depth * h * w >= C_BYTES
    ids = _edge_ids(pool, stacks, 1, nby, nbx, 97)
    dp, t_ids, ctx = pool.dev(torch, "cuda"), _dev_ids(ids), lctx(depth)
    flat = t_ids.reshape(-1)
    n = flat.numel()
    h_frames = _fill_frames(torch, dp.px_in, t_ids, depth, h, w).cpu().numpy()
    t1 = time.time()
    h_q = ctx.encode_frames(h_frames)
    t_enc = time.time() - t1
    del h_frames
    bad = 0
    for g0 in range(0, n, 1 << 18):
        got = torch.from_numpy(h_q[g0:g0 + (1 << 18)].reshape(-1, pool.cs)).cuda()
        bad += int((got != dp.q[flat[g0:g0 + (1 << 18)]]).any(dim=1).sum())
    assert bad == 0, f"{bad} cubes of the host encode differ from the pool's"
    t1 = time.time()
    h_out = ctx.decode_frames(h_q, w, h, stacks, 1)
    t_dec = time.time() - t1
    del h_q
    assert _frames_mismatches(torch.from_numpy(h_out).cuda(), dp.px_out, t_ids, depth, h, w) == 0
    _report("C int32 2045x1021x131", t0, host_encode_s=round(t_enc, 2), host_decode_s=round(t_dec, 2))
