"""Host model of the stream decode's front (csrc/dct3d_eg.hip), pure numpy, no device.

The device cuts the stream into 512-bit chunks from start_bit.  Pass 0 parses every chunk from its nominal first
bit; a plain confirming pass parses chunk t from the exit the previous pass gave chunk t - 1 (chunk 0: the
stream's first bit; after an invalid parse: the nominal start again).  A parse reads codes until it stands at or
past min(chunk end, data end): that position is the chunk's exit.  A code with 32 or more leading zeros, or one
that runs past the data end, ends the parse invalid (no exit).  Bits past the data end read as zero.

FrontModel restates exactly that on a bit array, so that a test can say of its input what the device will meet:
how many chunks are out of step after pass 0, how many confirming passes a plain scheme needs, and where inside
a chunk the pass-0 parse and the true parse first stand on the same bit."""
import numpy as np

CHUNK_BITS = 512
CHAIN_BLOCK = 256     # chunks per block of the chained confirming pass (eg_chain_kernel)
MEET_BITS = 128       # the resolve walk gives up once both parses stand at or past this bit (kMeetBits)
NO_EXIT = -1


def code_bits(vals) -> np.ndarray:
    """The bits (uint8, one per element) exp_golomb.c writes for the values, in order: v <= 0 -> -2v, v > 0 ->
    2v - 1, plus one, as n - 1 zero bits and the n-bit value, MSB first."""
    v = np.asarray(vals, np.int64).ravel()
    code = np.where(v <= 0, -2 * v, 2 * v - 1) + 1
    n = np.zeros(v.size, np.int64)
    c = code.copy()
    while (c > 0).any():          # bit length, exactly (no floating-point log)
        n += c > 0
        c >>= 1
    width = 2 * n - 1
    end = np.cumsum(width)
    bits = np.zeros(int(end[-1]) if v.size else 0, np.uint8)
    for k in range(int(n.max()) if v.size else 0):   # bit k of the value sits k + 1 bits before the code's end
        m = n > k
        bits[end[m] - 1 - k] = (code[m] >> k) & 1
    return bits


def stream_bytes(vals, carry_byte=0, carry_bits=0):
    """(bytes, total bits) of the values' stream behind carry_bits carried bits: what the encoder hands a decoder."""
    pre = np.unpackbits(np.array([carry_byte], np.uint8))[:carry_bits]
    bits = np.concatenate([pre, code_bits(vals)])
    return np.packbits(bits).tobytes(), int(bits.size)


def code_widths(vals) -> np.ndarray:
    v = np.asarray(vals, np.int64).ravel()
    c = np.where(v <= 0, -2 * v, 2 * v - 1) + 1
    n = np.zeros(v.size, np.int64)
    while (c > 0).any():
        n += c > 0
        c >>= 1
    return 2 * n - 1


def lay_ones(vals, a, b, off_step_at=None):
    """vals with a run of the value 1 (code `010`) from the code that holds stream bit a until the run's codes reach
    bit b, both counted in the RESULT's stream (what lies before the run is unchanged).  off_step_at: a bit inside
    the run that must not be one of its code boundaries; the run then begins up to two codes later.  A parse
    entering `010010...` off a boundary reads `1`, `00100`, `1`, ... and never stands on one."""
    v = np.array(vals, np.int64).ravel()
    start = np.concatenate([[0], np.cumsum(code_widths(v))[:-1]])
    i = max(int(np.searchsorted(start, a, side="right")) - 1, 0)
    while off_step_at is not None and (off_step_at - int(start[i])) % 3 == 0:
        i += 1
    k = -(-(b - int(start[i])) // 3)
    v[i:i + k] = 1
    return v


def periodic_values(pattern, n) -> np.ndarray:
    """n values repeating `pattern`."""
    pat = np.atleast_1d(np.asarray(pattern, np.int64))
    return np.tile(pat, -(-n // pat.size))[:n]


def random_values(n, seed) -> np.ndarray:
    return np.random.default_rng(seed).integers(-20, 21, n)


def chain_values(n, seed, first_chunk, run_chunks) -> np.ndarray:
    """Random values with one run of 1s from 60 bits before the first bit of chunk first_chunk to the end of chunk
    first_chunk + run_chunks - 1, the run out of step at its first chunk boundary: a plain scheme corrects one chunk
    of the run per confirming pass."""
    return lay_ones(random_values(n, seed), CHUNK_BITS * first_chunk - 60, CHUNK_BITS * (first_chunk + run_chunks),
                    off_step_at=CHUNK_BITS * first_chunk)


def late_meeting_values(n, seed) -> np.ndarray:
    """Random values with a run of 1s from 60 bits before to 200 bits after the first bit of chunks 1, 5, 9, ...,
    each out of step there: that chunk's pass-0 parse cannot meet the true one before the run ends, past the
    resolve walk's 128 bits, and does meet it soon after, inside the chunk.  Behind the last run the values are 0
    (one bit each, every bit a boundary), so that the runs' chunks are a quarter of all chunks."""
    v = random_values(n, seed)
    k = 1
    while CHUNK_BITS * k + 200 + 64 < int(code_widths(v).sum()):
        v = lay_ones(v, CHUNK_BITS * k - 60, CHUNK_BITS * k + 200, off_step_at=CHUNK_BITS * k)
        k += 4
    start = np.concatenate([[0], np.cumsum(code_widths(v))[:-1]])
    v[start >= CHUNK_BITS * (k - 4) + 200 + 64] = 0
    return v


# the GPU tests' streams of 64 x 40 x 1 stack (40 cubes), made here so that the CPU tests speak of the same values
# (depth, chunks of the run, its first chunk; 253: the run crosses a block of the chained pass)
CHAINS = [(8, 1, 17), (8, 2, 17), (8, 5, 17), (8, 5, 253), (4, 1, 17), (4, 2, 17), (4, 5, 17)]


def chain_case(depth, run, first) -> np.ndarray:
    return chain_values(40 * 64 * depth, 100 * depth + run, first, run)


def late_case(depth) -> np.ndarray:
    return late_meeting_values(40 * 64 * depth, 7 + depth)


def cubes_of(vals, diag, depth) -> np.ndarray:
    """Cube-major q [n, depth, 8, 8] (int32) whose stream, in diagonal order `diag`, holds vals in order."""
    cs = 64 * depth
    q = np.empty((len(vals) // cs, cs), np.int32)
    q[:, np.asarray(diag)] = np.asarray(vals, np.int32).reshape(-1, cs)
    return q.reshape(-1, depth, 8, 8)


class FrontModel:
    def __init__(self, data: bytes, start_bit: int = 0):
        bits = np.unpackbits(np.frombuffer(data, np.uint8))
        self.limit = L = int(bits.size)
        self.start = int(start_bit)
        self.n_chunks = -(-(L - self.start) // CHUNK_BITS)
        t = np.arange(self.n_chunks, dtype=np.int64)
        self.begin = self.start + t * CHUNK_BITS
        self.stop = np.minimum(self.begin + CHUNK_BITS, L)
        # nxt[p]: the boundary after the code at p; INV (absorbing, above every stop) when that code is invalid
        self.INV = INV = L + 1
        ones = np.flatnonzero(bits)
        nxt_one = np.full(L + 1, L + 64, np.int64)               # no 1 before the data end: zeros for ever
        if ones.size:
            idx = np.searchsorted(ones, np.arange(L), side="left")
            ok = idx < ones.size
            nxt_one[:L][ok] = ones[idx[ok]]
        p = np.arange(L + 1, dtype=np.int64)
        z = nxt_one - p
        e = p + 2 * z + 1
        nxt = np.where((z < 32) & (e <= L), e, INV)
        nxt[L] = INV
        self.nxt = np.concatenate([nxt, [INV]])                   # index INV itself
        # jump[k][p] = nxt applied 2^k times; a chunk holds at most 512 codes (+ the one that leaves it)
        self.jump = [self.nxt]
        for _ in range(10):
            j = self.jump[-1]
            self.jump.append(j[j])

    def parse(self, p, stop):
        """Vectorised: from positions p, codes until at or past stop.  Returns (exit or NO_EXIT, codes read)."""
        p = np.array(p, np.int64)
        stop = np.asarray(stop, np.int64)
        n = np.zeros(p.shape, np.int64)
        for k in range(len(self.jump) - 1, -1, -1):              # greedy descent: every code that ends before stop
            q = self.jump[k][p]
            take = (p < stop) & (q < stop)
            p = np.where(take, q, p)
            n += take * (1 << k)
        last = p < stop                                           # one more code crosses the stop (or is invalid)
        q = self.nxt[p]
        p = np.where(last, q, p)
        n += last & (q != self.INV)
        return np.where(p == self.INV, NO_EXIT, p), n

    def pass0(self):
        return self.parse(self.begin, self.stop)

    def confirm(self, exits):
        """One plain confirming pass over the exits of the pass before."""
        s = self.begin.copy()
        prev = np.asarray(exits[:-1])
        s[1:] = np.where(prev == NO_EXIT, self.begin[1:], prev)
        return self.parse(s, self.stop)

    def true_parse(self):
        """(exits, counts) of the one parse from the stream's first bit, chunk by chunk."""
        ex = np.empty(self.n_chunks, np.int64)
        cn = np.empty(self.n_chunks, np.int64)
        p = self.start
        for t in range(self.n_chunks):
            e, n = self.parse([p], [self.stop[t]])
            ex[t], cn[t] = e[0], n[0]
            p = self.begin[t] + CHUNK_BITS if e[0] == NO_EXIT else int(e[0])   # (as a confirming pass restarts)
        return ex, cn

    def plain_passes(self):
        """(confirming passes until one changes no exit, that one included; chunks whose pass-0 exit is already
        the fixed point's)."""
        ex, _ = self.pass0()
        first = ex
        k = 0
        while True:
            new, _ = self.confirm(ex)
            k += 1
            if np.array_equal(new, ex):
                break
            ex = new
            assert k <= self.n_chunks + 1
        return k, int((first == ex).sum())

    def meeting_bits(self):
        """Per chunk, the chunk-relative bit at which the pass-0 parse (from the chunk's first bit) first stands on
        a boundary of the true parse, or -1 when it does not inside the chunk (or ends invalid first)."""
        L = self.limit
        is_true = np.zeros(L + 2, bool)
        p = self.start
        while p != self.INV and p <= L:
            is_true[p] = True
            if p == L:
                break
            p = int(self.nxt[p])
        p = self.begin.copy()
        end = self.begin + CHUNK_BITS
        for _ in range(CHUNK_BITS + 1):
            go = (p < np.minimum(end, L)) & ~is_true[np.minimum(p, L + 1)]
            if not go.any():
                break
            p = np.where(go, self.nxt[np.minimum(p, L + 1)], p)
        met = (p < end) & (p <= L) & is_true[np.minimum(p, L + 1)]
        return np.where(met, p - self.begin, -1)


def launch_bound(nbytes: int, start_bit: int = 0) -> int:
    """The sync launches a front may issue on ANY stream: one chained confirming pass per block of 256 chunks,
    pass 0, the pass that sees no change, and the speculative attempt's pass 0 before the rerun."""
    n_chunks = -(-(8 * nbytes - start_bit) // CHUNK_BITS)
    return -(-n_chunks // CHAIN_BLOCK) + 3
