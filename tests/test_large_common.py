"""CPU: the builders of the large-offset tests (large_common.py) against the oracle.  The GPU cases trust the pool
construction -- a raster, its coefficients, its stream and the stream's offsets, all indexed out of a pool -- and the
stream extraction helper; this is where both are compared with Plan.encode_q / Plan.decode_q and the oracle's
Exp-Golomb writer on a whole small clip, and where the helper is shown to see a single wrong bit."""
import numpy as np
import pytest

import large_common as lc
import quant_common as qc

W, H, STACKS = 64, 48, 3
CARRY = (0xB4, 5)


def _oracle_stream(oracle, q, depth, carry_byte, carry_bits):
    """the oracle's writer on the whole clip (test_gpu_eg._expected): (bytes, total bits)"""
    vals = q.reshape(-1, 64 * depth)[:, lc.diag_order(depth)].ravel()
    nbits = int(qc.code_bits(vals).sum())
    body = np.unpackbits(np.frombuffer(oracle.eg_write(vals), np.uint8))[:nbits]
    bits = np.concatenate([np.unpackbits(np.array([carry_byte], np.uint8))[:carry_bits], body])
    return np.packbits(bits).tobytes(), carry_bits + nbits


def _words(torch, stream, extra=2):
    """stream bytes -> the int32 memory-order words a device buffer holds (zero padded, `extra` words more)"""
    pad = np.zeros((len(stream) + 3) // 4 * 4 + 4 * extra, np.uint8)
    pad[:len(stream)] = np.frombuffer(stream, np.uint8)
    return torch.from_numpy(pad.view(np.int32))


@pytest.mark.parametrize("kind", ["general", "constant_heavy"])
@pytest.mark.parametrize("depth", [8, 4])
def test_pool_built_clip_equals_the_oracle(pkg, oracle, depth, kind):
    """a 3-stack 64 x 48 clip out of the pool: its raster, coefficients, decoded raster, stream (carry 5 bits) and
    offsets equal the oracle's for that raster; the extraction helper recovers every cube from the oracle's stream"""
    import torch
    nby, nbx = H // 8, W // 8
    n = STACKS * nby * nbx
    if kind == "general":
        pool, weights = lc.general_pool(depth), None
    else:
        pool = lc.constant_heavy_pool(depth)
        weights = np.full(pool.k, 1.0 / pool.k)  # (every pool cube in so small a clip)
    assert np.array_equal(lc.diag_order(depth), pkg.diagonal_order(8, 8, depth))
    ids = lc.draw_ids(n, pool.k, 99 + depth, pool.cs, weights)
    dp = pool.dev(torch, "cpu")
    t_ids = torch.from_numpy(ids)
    raster = lc.fill_raster(torch.zeros((STACKS * depth, H, W), dtype=torch.uint8), dp.px_in, t_ids, STACKS, nby, nbx,
                            depth, slice_cubes=20).numpy()
    plan = qc.plan(depth)
    q_ref = plan.encode_q(raster)
    assert np.array_equal(pool.q[ids], q_ref.reshape(n, -1)), "the coefficients of the clip are the pool's"
    out_ref = plan.decode_q(q_ref, W, H, STACKS * depth)
    assert lc.raster_mismatches(torch.from_numpy(out_ref), dp.px_out, t_ids, STACKS, nby, nbx, depth, 20) == 0
    assert lc.cube_mismatches(torch.from_numpy(q_ref.reshape(n, -1)), dp.q, t_ids, slice_cubes=50) == 0
    # the stream and its offsets
    stream, total = _oracle_stream(oracle, q_ref, depth, *CARRY)
    assert lc.build_stream(pool, ids, *CARRY) == (stream, total)
    off, tot = lc.offsets(torch, dp.bits, t_ids, CARRY[1])
    per_cube = qc.code_bits(q_ref.reshape(n, -1)).sum(axis=1)
    assert tot == total and np.array_equal(off.numpy(), CARRY[1] + np.cumsum(per_cube) - per_cube)
    words = _words(torch, stream)
    assert lc.check_stream(torch, words, dp, t_ids, *CARRY, slice_words=4096) == (0, -1, total, True)
    # the helper against the oracle's reader, cube by cube: its words re-read as values
    g = n // 2
    got = lc.extract(torch, words, off[g:g + 1], dp.bits[t_ids[g:g + 1]], dp.n_words).numpy()[0]
    vals = oracle.eg_read(got.astype(">u4").tobytes(), pool.cs)
    assert np.array_equal(vals, q_ref.reshape(n, -1)[g, lc.diag_order(depth)])


def test_the_stream_check_sees_one_wrong_bit(oracle):
    """a single flipped bit is one bad cube, named; a flipped carry bit or padding bit fails the ends; a stream
    shifted by one cube or built from rotated ids fails nearly everywhere"""
    import torch
    depth = 8
    pool = lc.general_pool(depth)
    ids = lc.draw_ids(144, pool.k, 7, pool.cs)
    dp = pool.dev(torch, "cpu")
    t_ids = torch.from_numpy(ids)
    stream, total = lc.build_stream(pool, ids, *CARRY)
    off, _ = lc.offsets(torch, dp.bits, t_ids, CARRY[1])
    for g, where in ((0, 0), (77, 0), (77, -1), (143, -1)):  # the first and the last bit of a cube
        bit = int(off[g]) + (int(pool.bits[ids[g]]) - 1 if where else 0)
        b = bytearray(stream)
        b[bit // 8] ^= 0x80 >> (bit % 8)
        assert lc.check_stream(torch, _words(torch, bytes(b)), dp, t_ids, *CARRY) == (1, g, total, True), (g, where)
    b = bytearray(stream)
    b[0] ^= 0x80  # a carried bit
    assert lc.check_stream(torch, _words(torch, bytes(b)), dp, t_ids, *CARRY) == (0, -1, total, False)
    if total % 32:
        b = bytearray(stream) + bytes(4)
        b[total // 8] |= 0x80 >> (total % 8)  # the first padding bit
        assert lc.check_stream(torch, _words(torch, bytes(b)), dp, t_ids, *CARRY) == (0, -1, total, False)
    rolled, _ = lc.build_stream(pool, np.roll(ids, 1), *CARRY)
    bad = lc.check_stream(torch, _words(torch, rolled, extra=400), dp, t_ids, *CARRY)[0]
    assert bad >= 140, bad


def test_pool_perturbations_are_seen(oracle):
    """the comparisons the GPU cases make do fail on a wrong pool: one changed pixel of one pool cube changes its
    coefficients, and the clip's comparison with the oracle then counts exactly the cubes that drew it"""
    import torch
    depth = 8
    pool = lc.general_pool(depth)
    ids = lc.draw_ids(4000, pool.k, 11, pool.cs)
    victim = int(ids[5])
    px = pool.px_in.copy()
    px[victim, 3] ^= 0x40
    q_ref = qc.plan(depth).encode_q(oracle.from_cubes(px[ids[:48]].reshape(48, depth, 8, 8), 64, 48, depth))
    wrong = (pool.q[ids[:48]] != q_ref.reshape(48, -1)).any(axis=1)
    assert np.array_equal(wrong, ids[:48] == victim) and wrong[5]


def test_ids_are_not_periodic():
    """alias_share: random ids pass, ids periodic in a power of two (or in the cubes of 2^32 values) do not"""
    cs = 512
    ids = lc.draw_ids(1 << 16, 256, 3, cs)
    assert lc.alias_share(ids, cs) >= lc.ALIAS_SHARE
    assert (1 << 23) in lc.alias_distances((1 << 23) + (1 << 16), cs), "2^32 values of 8x8x8 cubes"
    assert (1 << 22) in lc.alias_distances((1 << 23) + (1 << 16), cs), "2^31 int32 elements"
    for period in (1 << 10, 1 << 14):
        assert lc.alias_share(np.resize(ids[:period], 1 << 16), cs) == 0.0
    with pytest.raises(AssertionError):
        lc.draw_ids(1 << 16, 1, 3, cs)
    w = lc.constant_heavy_weights(288)
    assert abs(w.sum() - 1) < 1e-12 and lc.alias_share(lc.draw_ids(1 << 16, 288, 5, cs, w), cs) >= lc.ALIAS_SHARE


def test_synthetic_q_pool_and_placement(oracle):
    """the pool of coefficients of the entropy-stage case: long codes read back by the oracle's reader; place_stream
    moves a stream to a bit position bit for bit"""
    for depth in (8, 4):
        pool = lc.synthetic_q_pool(depth)
        assert 30 * pool.cs < pool.bits.mean() < 45 * pool.cs, "about 2^32 bits in a few hundred thousand cubes"
        i = int(np.argmax(pool.bits))
        vals = oracle.eg_read(pool.words[i].astype(">u4").tobytes(), pool.cs)
        assert np.array_equal(vals, pool.q[i][lc.diag_order(depth)])
    pool = lc.general_pool(8)
    stream, total = lc.build_stream(pool, [3, 9, 200])
    for at in ((1 << 32) - 4099, (1 << 32) - 7, 3, (1 << 32) + 12345):
        data, byte0, start, end = lc.place_stream(stream, total, at)
        assert (byte0, start, end) == (at // 8, at, at + total)
        bits = np.unpackbits(np.frombuffer(data, np.uint8))
        assert not bits[:at % 8].any() and not bits[at % 8 + total:].any()
        assert np.array_equal(bits[at % 8:at % 8 + total], np.unpackbits(np.frombuffer(stream, np.uint8))[:total])
