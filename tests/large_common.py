"""Builders of the large-offset tests (test_gpu_large_offsets.py; checked on the CPU against the oracle
by test_large_common.py): inputs of several GiB and their exact expectations in seconds, from a pool of cubes.

A cube's coefficients depend on its own 8 x 8 x D pixels only, and its code on its own coefficients.  So the oracle
runs once on a pool of K cubes (Pool), an id per cube is drawn from a seeded generator (draw_ids), and everything a
case needs is an indexing of the pool by the ids, with torch on either device:

    raster            pool.px_in[ids]   as (S, nby, nbx, D, 8, 8) -> (S, D, nby, 8, nbx, 8)       fill_raster
    int32 cubes       pool.q[ids]
    decoded raster    pool.px_out[ids]  permuted the same way
    stream offsets    carry_bits + the exclusive int64 sum of pool.bits[ids]                       offsets
    stream            cube g's bits at its offset are pool.words[ids[g]]                           check_stream

check_stream reads a stream completely and knows nothing of the library: for every cube it gathers the words at its
offset, swaps them to stream order, funnel-shifts them by the offset's low 5 bits in int64, masks them to the
cube's length and compares them with the pool cube's own stream, which the oracle's writer coded from bit 0.

The ids must not repeat with a power-of-two period: a cube written at index g mod 2^k would otherwise still carry
the right content.  alias_share measures that, draw_ids asserts it."""
import functools

import numpy as np

import quant_common as qc

M32 = 0xFFFFFFFF
ALIAS_SHARE = 0.99  # of the cubes g, ids[g] != ids[g - A] for every alias distance A; random ids give 255/256


# ---- the pools (numpy, built once) ---------------------------------------------------------------------------------

def _extreme_patterns(depth):
    """test_encode_extreme_patterns' four, one cube each"""
    z, y, x = np.meshgrid(np.arange(depth), np.arange(8), np.arange(8), indexing="ij")
    return [((x + y + z) % 2) * 255, ((x // 4 + y // 4) % 2) * 255, (x * 37 + y * 11 + z * 5) % 256,
            np.where(z % depth < depth // 2, 0, 255)]


def general_cubes(depth, k=256, seed=4100):
    """uint8 [k, depth, 8, 8]: uniform noise, ramps, the "ties" kind (frame 0 of each four carries a step over a flat
    block: values on x.5 exactly), constants 0, 128 and 255, the extreme patterns, low-amplitude noise"""
    rng = np.random.default_rng(seed + depth)
    z, y, x = np.meshgrid(np.arange(depth), np.arange(8), np.arange(8), indexing="ij")
    cubes = [np.full((depth, 8, 8), c) for c in (0, 128, 255)] + _extreme_patterns(depth)
    n_rest = k - len(cubes)
    n_noise, n_ramp, n_ties = (3 * n_rest) // 8, n_rest // 5, n_rest // 5
    cubes += list(rng.integers(0, 256, size=(n_noise, depth, 8, 8)))
    for _ in range(n_ramp):
        a, b, c, d = rng.integers(0, 12, 3).tolist() + [int(rng.integers(0, 256))]
        cubes.append((a * x + b * y + c * z + d) % 256)
    for i in range(n_ties):
        v = 60 + 2 * i + 8 * ((z % 4 == 0) & ((y == 0) | ((y == 1) & (x < 2))))
        cubes.append(v + 16 * ((z % 4 == 3) & (x == 4) & (y < 5) & (i % 2 == 1)))
    n_low = k - len(cubes)
    cubes += list(128 + rng.integers(-6, 7, size=(n_low, depth, 8, 8)))
    out = np.stack(cubes).astype(np.uint8)
    assert out.shape == (k, depth, 8, 8)
    return out[rng.permutation(k)]


def constant_heavy_cubes(depth, n_other=32, seed=4200):
    """uint8 [256 + n_other, depth, 8, 8]: the 256 constant cubes (distinct ids stay distinct contents), then noise and
    ramps from general_cubes; CONSTANT_WEIGHT of the draws go to the constants"""
    other = general_cubes(depth, 256, seed)[:n_other]
    const = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, depth, 8, 8))
    return np.concatenate([const, other])


CONSTANT_WEIGHT = 0.985


def constant_heavy_weights(k, n_const=256):
    w = np.full(k, (1.0 - CONSTANT_WEIGHT) / (k - n_const))
    w[:n_const] = CONSTANT_WEIGHT / n_const
    return w


def synthetic_q_cubes(depth, k=256, seed=4300):
    """int32 [k, depth, 8, 8], no pixels behind them (the entropy stage alone): 10 % all-zero cubes (512 or 256 one-bit
    codes), 20 % sparse small values, 70 % dense values of 2^15 <= |v| < 2^30 (33- to 61-bit codes, every width as
    likely).  Per-cube lengths of every residue mod 32 (asserted)."""
    rng = np.random.default_rng(seed + depth)
    q = np.zeros((k, depth, 8, 8), np.int64)
    kind = rng.permutation(k) % 10  # 0: zeros, 1-2: short, 3-9: long
    short = np.isin(kind, (1, 2))
    long_ = kind >= 3
    s = rng.integers(-20, 21, size=q.shape)
    s[rng.random(q.shape) < 0.5] = 0
    q[short] = s[short]
    e = rng.integers(15, 30, size=q.shape)
    v = (1 << e) + (rng.integers(0, 1 << 30, size=q.shape) & ((1 << e) - 1))
    v *= rng.choice([-1, 1], size=q.shape)
    q[long_] = v[long_]
    assert np.abs(q).max() < 2**30
    bits = qc.code_bits(q).reshape(k, -1)
    assert bits[long_].min() == 33 and bits[long_].max() == 61 and (bits[kind == 0] == 1).all()
    assert len(set((bits.sum(1) % 32).tolist())) >= 16, "cube lengths of many residues mod 32"
    return q.astype(np.int32)


def diag_order(depth):
    """stream position -> cube index x + 8 y + 64 z (cubeUtils_diagonalSlices), from the oracle"""
    import oracle
    d = oracle.diagonal_slices(8, 8, depth).astype(np.int64)
    return d[:, 0] + 8 * d[:, 1] + 64 * d[:, 2]


def cube_stream_words(q, depth):
    """(bits int64 [k], words int64 [k, W]): each cube's own Exp-Golomb stream from bit 0 -- the oracle's writer on its
    values in diagonal order -- as MSB-first 32-bit words, zero past its bits; W = the longest cube's words + 1"""
    import oracle
    vals = np.asarray(q).reshape(len(q), 64 * depth)[:, diag_order(depth)]
    bits = qc.code_bits(vals).sum(axis=1)
    n_words = int((bits.max() + 31) // 32) + 1
    words = np.zeros((len(q), n_words), np.int64)
    for i, v in enumerate(vals):
        b = np.frombuffer(oracle.eg_write(v), np.uint8)
        assert 8 * (len(b) - 1) <= bits[i] < 8 * len(b), "the writer's length and code_bits agree"
        pad = np.zeros(4 * n_words, np.uint8)
        pad[:(bits[i] + 7) // 8] = b[:(bits[i] + 7) // 8]
        words[i] = pad.view(">u4").astype(np.int64)
        tail = int(bits[i] % 32)
        if tail:
            words[i, bits[i] // 32] &= (M32 << (32 - tail)) & M32
    return bits.astype(np.int64), words


class Pool:
    """K cubes and what the reference makes of each: px_in uint8 [K, cs] (None for a pool of coefficients), q int32
    [K, cs], px_out uint8 [K, cs] (the decode of q; None likewise), bits int64 [K], words int64 [K, W].  numpy; dev()
    gives the same as torch tensors."""

    def __init__(self, depth, px_in, q, px_out):
        self.depth, self.cs, self.k = depth, 64 * depth, len(q)
        self.px_in = None if px_in is None else np.ascontiguousarray(px_in.reshape(self.k, -1))
        self.q = np.ascontiguousarray(q.reshape(self.k, -1))
        self.px_out = None if px_out is None else np.ascontiguousarray(px_out.reshape(self.k, -1))
        self.bits, self.words = cube_stream_words(q, depth)
        self.n_words = self.words.shape[1]

    def dev(self, torch, device):
        t = lambda a: None if a is None else torch.from_numpy(a).to(device)
        return DevPool(self, t(self.px_in), t(self.q), t(self.px_out), t(self.bits), t(self.words))


class DevPool:
    def __init__(self, pool, px_in, q, px_out, bits, words):
        self.pool, self.depth, self.cs, self.k, self.n_words = pool, pool.depth, pool.cs, pool.k, pool.n_words
        self.px_in, self.q, self.px_out, self.bits, self.words = px_in, q, px_out, bits, words


def pixel_pool(cubes, depth, steps=None):
    """the reference on pixel cubes [K, depth, 8, 8]: the K cubes side by side as one stack of 8 K x 8 frames through
    Plan.encode_q / Plan.decode_q (steps None: the reference quantiser) or quant_common's table reference"""
    import oracle
    k = len(cubes)
    frames = oracle.from_cubes(np.ascontiguousarray(cubes), 8 * k, 8, depth)
    if steps is None:
        q = qc.plan(depth).encode_q(frames)
        out = qc.plan(depth).decode_q(q, 8 * k, 8, depth)
    else:
        q = qc.ref_encode(frames, steps, depth)
        out = qc.ref_decode(q, 8 * k, 8, depth, steps, depth)
    return Pool(depth, cubes, q, oracle.to_cubes(out, 8, 8, depth))


@functools.lru_cache(maxsize=None)
def general_pool(depth, table=None):
    """table: None (the reference quantiser) or a name of quant_common.tables"""
    return pixel_pool(general_cubes(depth), depth, None if table is None else qc.tables(depth)[table])


@functools.lru_cache(maxsize=None)
def constant_heavy_pool(depth):
    return pixel_pool(constant_heavy_cubes(depth), depth)


@functools.lru_cache(maxsize=None)
def synthetic_q_pool(depth):
    return Pool(depth, None, synthetic_q_cubes(depth), None)


# ---- ids ---------------------------------------------------------------------------------------------------------------

def alias_distances(n, cs):
    """the distances a narrow index could fold cubes by: every power of two of cubes, and the cubes of 2^31 and 2^32
    values or bytes of int32; only those that leave 1,000 cubes to compare"""
    d = {1 << k for k in range(0, 40)} | {(1 << 31) // cs, (1 << 32) // cs, (1 << 31) // (4 * cs), (1 << 32) // (4 * cs)}
    return sorted(a for a in d if 0 < a and n - a >= 1000)


def alias_share(ids, cs):
    """the smallest share, over alias_distances, of the cubes g whose id differs from cube g - A's"""
    ids = np.asarray(ids)
    return min([float(np.mean(ids[a:] != ids[:-a])) for a in alias_distances(len(ids), cs)] or [1.0])


def draw_ids(n, k, seed, cs, weights=None):
    """int64 [n] pool ids from a seeded generator (weights: the probability of each pool cube), never periodic in a
    power of two: alias_share >= ALIAS_SHARE is asserted here, on the CPU"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, k, size=n) if weights is None else rng.choice(k, size=n, p=weights)
    share = alias_share(ids, cs)
    assert share >= ALIAS_SHARE, f"ids alias: only {share:.4f} of the cubes differ from their alias"
    return ids.astype(np.int64)


# ---- rasters -----------------------------------------------------------------------------------------------------------

def _raster_slices(cubes, ids, stacks, nby, nbx, depth, slice_cubes):
    """(stack, first block-row, end block-row, the cubes of those rows as [depth, rows, 8, nbx, 8]): a raster in
    slices of about slice_cubes cubes, whole block-rows of one stack each (the gather is a slice's only temporary)"""
    rows = max(1, min(nby, slice_cubes // nbx))
    for s in range(stacks):
        for by0 in range(0, nby, rows):
            by1 = min(nby, by0 + rows)
            g0 = (s * nby + by0) * nbx
            c = cubes[ids[g0:g0 + (by1 - by0) * nbx]].view(by1 - by0, nbx, depth, 8, 8)
            yield s, by0, by1, c.permute(2, 0, 3, 1, 4)


def fill_raster(dst, cubes, ids, stacks, nby, nbx, depth, slice_cubes=1 << 18):
    """dst uint8 [stacks * depth, 8 nby, 8 nbx] (torch) <- the cubes [K, cs] of ids [stacks * nby * nbx]"""
    view = dst.view(stacks, depth, nby, 8, nbx, 8)
    for s, by0, by1, c in _raster_slices(cubes, ids, stacks, nby, nbx, depth, slice_cubes):
        view[s, :, by0:by1] = c
    return dst


def raster_mismatches(got, cubes, ids, stacks, nby, nbx, depth, slice_cubes=1 << 18):
    """the bytes of got [stacks * depth, 8 nby, 8 nbx] that differ from the raster of cubes[ids]"""
    view = got.view(stacks, depth, nby, 8, nbx, 8)
    bad = 0
    for s, by0, by1, c in _raster_slices(cubes, ids, stacks, nby, nbx, depth, slice_cubes):
        bad += int((view[s, :, by0:by1] != c).sum())
    return bad


def cube_mismatches(got, cubes, ids, slice_cubes=1 << 18):
    """the cubes of got [n, cs] that differ from cubes[ids]"""
    bad = 0
    for g0 in range(0, len(ids), slice_cubes):
        g1 = min(len(ids), g0 + slice_cubes)
        bad += int((got[g0:g1] != cubes[ids[g0:g1]]).any(dim=1).sum())
    return bad


# ---- streams -----------------------------------------------------------------------------------------------------------

def offsets(torch, bits, ids, carry_bits):
    """(off int64 [n]: the stream bit each cube starts at; the total bits, carry included)"""
    b = bits[ids]
    incl = torch.cumsum(b, dim=0)
    return incl - b + carry_bits, int(incl[-1]) + carry_bits


def bswap32(u):
    """int64 tensor of 32-bit memory-order (little-endian) words -> stream-order (MSB-first) words"""
    return ((u & 0xFF) << 24) | ((u & 0xFF00) << 8) | ((u >> 8) & 0xFF00) | ((u >> 24) & 0xFF)


def extract(torch, words, off, nbits, n_words):
    """int64 [m, n_words]: for each of m cubes the stream bits [off, off + nbits) as MSB-first 32-bit words from bit 0,
    zero past nbits.  words: the stream as an int32 tensor in memory order.  Independent of the library."""
    j = torch.arange(n_words + 1, device=words.device, dtype=torch.int64)
    idx = ((off >> 5)[:, None] + j[None, :]).clamp_(max=words.numel() - 1)  # (a word past the buffer: masked below)
    w = bswap32(words[idx].to(torch.int64) & M32)
    sh = (off & 31)[:, None]
    v = ((w[:, :-1] << sh) | (w[:, 1:] >> (32 - sh))) & M32
    valid = (nbits[:, None] - 32 * j[None, :n_words]).clamp_(0, 32)
    return v & ((1 << 32) - (torch.ones_like(valid) << (32 - valid)))  # the top `valid` bits of a word


def check_stream(torch, words, dp, ids, carry_byte, carry_bits, slice_words=1 << 24):
    """The whole stream against the pool: (cubes whose bits differ, the first such cube or -1, the expected total
    bits, whether the carried bits and the zero padding after the last bit are right).  words: int32 tensor of at
    least ceil(total / 32) words; ids: int64 tensor on the same device."""
    off, total = offsets(torch, dp.bits, ids, carry_bits)
    assert words.numel() * 32 >= total, "the buffer holds the stream"
    step = max(1, slice_words // (dp.n_words + 1))
    bad, first = 0, -1
    for g0 in range(0, len(ids), step):
        sl = slice(g0, min(len(ids), g0 + step))
        got = extract(torch, words, off[sl], dp.bits[ids[sl]], dp.n_words)
        diff = (got != dp.words[ids[sl]]).any(dim=1)
        n = int(diff.sum())
        if n and first < 0:
            first = g0 + int(torch.nonzero(diff)[0])
        bad += n
    w_first = int(bswap32(words[:1].to(torch.int64) & M32))
    w_last = int(bswap32(words[(total - 1) >> 5:((total - 1) >> 5) + 1].to(torch.int64) & M32))
    ends_ok = (w_first >> (32 - carry_bits) if carry_bits else 0) == (carry_byte >> (8 - carry_bits) if carry_bits else 0)
    ends_ok = ends_ok and (w_last & (M32 >> (total % 32) if total % 32 else 0)) == 0
    return bad, first, total, ends_ok


def build_stream(pool, ids, carry_byte=0, carry_bits=0):
    """numpy, for small cases: (the stream bytes of the cubes ids continuing the carried partial byte, total bits), the
    pool cubes' own streams laid end to end"""
    pieces = [np.unpackbits(np.array([carry_byte], np.uint8))[:carry_bits]]
    for i in ids:
        w = pool.words[i].astype(">u4").view(np.uint8)
        pieces.append(np.unpackbits(w)[:pool.bits[i]])
    bits = np.concatenate(pieces)
    return np.packbits(bits).tobytes(), int(bits.size)


def place_stream(stream, total_bits, at_bit):
    """(bytes, first byte, start bit, end bit): the stream's bits moved to begin at absolute bit `at_bit` of a zeroed
    buffer: the bytes to copy to byte at_bit // 8 of it"""
    bits = np.unpackbits(np.frombuffer(stream, np.uint8))[:total_bits]
    moved = np.concatenate([np.zeros(at_bit % 8, np.uint8), bits])
    return np.packbits(moved).tobytes(), at_bit // 8, at_bit, at_bit + total_bits


# ---- canary bands --------------------------------------------------------------------------------------------------------

BAND = 4096
CANARY = 0xC3


def banded(torch, nbytes, fill=CANARY, device="cuda"):
    """(buffer, middle view): nbytes between two 4 KiB bands, every byte `fill` (the bands must stay so)"""
    buf = torch.full((BAND + nbytes + BAND,), fill, dtype=torch.uint8, device=device)
    return buf, buf[BAND:BAND + nbytes]


def bands_intact(buf, nbytes, fill=CANARY):
    return bool((buf[:BAND] == fill).all()) and bool((buf[BAND + nbytes:] == fill).all())
