"""CPU: the host model of the stream decode's front (eg_sync_common.py) and the streams test_gpu_eg_periodic.py
feeds the device.  Here the inputs prove that they are what the GPU tests say they are: the model writes the
oracle's bytes, its parses are a one-code-at-a-time reader's, periodic streams need one plain confirming pass per
chunk, and the laid runs put the meeting points where the GPU tests need them."""
import numpy as np
import pytest

import eg_sync_common as m

N48 = 48 * 512        # the table's clips: 48 cubes of 8x8x8
PATTERNS = {"all 0": 0, "all -1": -1, "all 1": 1, "1, -1": (1, -1), "all 2": 2, "all 3": 3, "all 7": 7}


def _values(name, n=N48):
    return m.random_values(n, 0) if name == "random" else m.periodic_values(PATTERNS[name], n)


def _model(vals, carry_byte=0, carry_bits=0):
    data, nbits = m.stream_bytes(vals, carry_byte, carry_bits)
    return m.FrontModel(data, carry_bits), nbits


def _slow_parse(bits, p, stop, limit):
    """one code at a time, as expGolomb_readValue reads: (exit or NO_EXIT, codes)"""
    n = 0
    while p < stop:
        z = 0
        while p + z < limit and not bits[p + z]:
            z += 1
        if p + z >= limit or z >= 32 or p + 2 * z + 1 > limit:
            return m.NO_EXIT, n
        p += 2 * z + 1
        n += 1
    return p, n


@pytest.mark.parametrize("name", list(PATTERNS) + ["random", "chain", "late"])
def test_model_bits_are_the_oracle_s_stream(oracle, name):
    if name == "chain":
        vals = m.chain_values(40 * 512, 805, 17, 5)
    elif name == "late":
        vals = m.late_meeting_values(40 * 512, 15)
    else:
        vals = _values(name, 40 * 512)
    bits = m.code_bits(vals)
    assert bits.size == int(m.code_widths(vals).sum())
    ref = np.unpackbits(np.frombuffer(oracle.eg_write(vals.astype(np.int32)), np.uint8))
    assert np.array_equal(bits, ref[:bits.size]) and not ref[bits.size:].any()
    data, nbits = m.stream_bytes(vals, 0xA5, 3)       # behind a carried partial byte
    got = np.unpackbits(np.frombuffer(data, np.uint8))
    assert nbits == bits.size + 3 and np.array_equal(got[:3], [1, 0, 1]) and np.array_equal(got[3:nbits], bits)


def test_model_bits_of_long_codes(oracle):
    vals = np.array([0, 1, -1, 2**15 - 1, -(2**15), 2**30 - 1, -(2**30) + 1, 5, 0], np.int64)
    ref = np.unpackbits(np.frombuffer(oracle.eg_write(vals.astype(np.int32)), np.uint8))
    bits = m.code_bits(vals)
    assert np.array_equal(bits, ref[:bits.size])
    assert list(m.code_widths(vals)) == [1, 3, 3, 31, 33, 61, 61, 7, 1]


@pytest.mark.parametrize("name,carry_bits", [("all 1", 0), ("1, -1", 3), ("all 7", 0), ("random", 0), ("random", 3)])
def test_true_parse_is_a_one_at_a_time_reader_s(name, carry_bits):
    vals = _values(name, 6 * 512)
    f, nbits = _model(vals, 0x5A, carry_bits)
    bounds = carry_bits + np.concatenate([[0], np.cumsum(m.code_widths(vals))])   # every code's first bit, and the end
    exits, counts = f.true_parse()
    assert f.n_chunks == -(-(f.limit - carry_bits) // 512)
    prev = carry_bits
    for t in range(f.n_chunks):
        end = carry_bits + 512 * (t + 1)
        if end > nbits:       # the chunk holding the padding: its parse runs into the byte's zero bits
            break
        e = int(bounds[np.searchsorted(bounds, end, side="left")])
        assert exits[t] == e
        assert counts[t] == np.searchsorted(bounds, e) - np.searchsorted(bounds, prev)
        prev = e
    assert t >= f.n_chunks - 1
    # and the fixed point of the confirming passes is that parse
    ex, cn = f.pass0()
    for _ in range(f.n_chunks + 1):
        ex, cn = f.confirm(ex)
    assert np.array_equal(ex, exits) and np.array_equal(cn, counts)


@pytest.mark.parametrize("name", ["all 1", "all 7", "random"])
def test_vectorised_parse_is_the_slow_one(name):
    vals = _values(name, 4 * 512)
    if name == "random":
        vals[100:104] = [2**20, -(2**29), 2**30 - 1, 3]     # long codes, one of them across a chunk end
    data, _ = m.stream_bytes(vals)
    data = data[:-3]                                          # a data end inside a code
    f = m.FrontModel(data)
    bits = np.unpackbits(np.frombuffer(data, np.uint8))
    ex, cn = f.pass0()
    for t in range(f.n_chunks):
        assert (ex[t], cn[t]) == _slow_parse(bits, int(f.begin[t]), int(f.stop[t]), f.limit), t
    for s in (1, 2, 5, 63):
        e2, c2 = f.parse(f.begin + s, f.stop)
        for t in range(f.n_chunks):
            assert (e2[t], c2[t]) == _slow_parse(bits, int(f.begin[t]) + s, int(f.stop[t]), f.limit), (s, t)
    zero = m.FrontModel(bytes(200))                           # 32 zero bits: invalid everywhere
    assert (zero.pass0()[0] == m.NO_EXIT).all()


# values | bits | chunks | chunks whose pass-0 exit is already the true exit | plain confirming passes
TABLE = [("all 0", 24576, 48, 48, 1), ("all -1", 73728, 144, 144, 1), ("all 1", 73728, 144, 48, 144),
         ("1, -1", 73728, 144, 96, 144), ("all 2", 122880, 240, 48, 240), ("all 3", 122880, 240, 48, 240),
         ("all 7", 172032, 336, 48, 336), ("random", 201942, 395, 395, 1)]


@pytest.mark.parametrize("name,bits,chunks,in_step,passes", TABLE)
def test_periodic_streams_take_one_plain_pass_per_chunk(name, bits, chunks, in_step, passes):
    f, nbits = _model(_values(name))
    assert (nbits, f.n_chunks) == (bits, chunks)
    assert f.plain_passes() == (passes, in_step)
    meet = f.meeting_bits()
    if passes == 1:
        assert (meet >= 0).all() and meet.max() < m.MEET_BITS      # every chunk falls into step, within the walk
    else:
        assert passes == chunks                                    # ... and here never: a cycle of valid codes
        assert (meet < 0).sum() == chunks - in_step and (meet[meet >= 0] <= 2).all()


@pytest.mark.parametrize("depth,name,chunks", [(8, "all 1", 120), (8, "1, -1", 120), (8, "all 2", 200), (8, "all 7", 280),
                                               (4, "all 1", 60), (4, "1, -1", 60), (4, "all 2", 100), (4, "all 7", 140)])
def test_never_meeting_streams_of_the_gpu_tests(depth, name, chunks):
    """64 x 40 x 1 stack: all 7 at 8x8x8 is more than one block of 256 chunks; behind a carried byte too"""
    vals = _values(name, 40 * 64 * depth)
    for carry_bits in (0, 3):
        f, _ = _model(vals, 0xA5, carry_bits)
        assert f.n_chunks in (chunks, chunks + 1) and (carry_bits or f.n_chunks == chunks)
        passes, in_step = f.plain_passes()
        assert passes >= chunks
        assert m.launch_bound(len(m.stream_bytes(vals, 0xA5, carry_bits)[0]), carry_bits) == -(-f.n_chunks // 256) + 3 < passes


@pytest.mark.parametrize("depth,values,chunks", [(8, 0, 280), (8, -1, 288), (4, 0, 280), (4, -1, 288)])
def test_in_step_streams_of_the_gpu_tests(depth, values, chunks):
    """all 0 (64 x 40 x 7 stacks; 14 at 8x8x4) and all -1 (64 x 24 x 4; 8): two blocks of chunks, every chunk in step"""
    n = 64 * 40 * 7 * 8 if values == 0 else 64 * 24 * 4 * 8
    f, _ = _model(m.periodic_values(values, n))
    assert f.n_chunks == chunks > m.CHAIN_BLOCK
    assert f.plain_passes() == (1, chunks)
    assert f.meeting_bits().max() <= 2


@pytest.mark.parametrize("depth,run,first", m.CHAINS)
def test_chain_of_known_length(depth, run, first):
    """a run of 1s over `run` whole chunks in random values: out of step at its first chunk, a plain scheme
    corrects one chunk per confirming pass and then sees no change: run + 1 passes"""
    f, _ = _model(m.chain_case(depth, run, first))
    meet = f.meeting_bits()
    assert meet[first] < 0 and (meet[:first] >= 0).all() and (meet[first + run:-1] >= 0).all()
    assert f.plain_passes()[0] == run + 1
    if first > 100:
        assert first < m.CHAIN_BLOCK <= first + run - 1     # the run crosses a block of the chained pass


@pytest.mark.parametrize("depth", [8, 4])
def test_late_meeting_without_a_changed_exit(depth):
    """runs of 1s across the first bit of chunks 1, 5, 9, ...: those chunks meet the true parse past the walk's 128
    bits (past the run's 200) and inside the chunk, so every pass-0 exit is already true: one plain pass, no change"""
    f, _ = _model(m.late_case(depth))
    meet = f.meeting_bits()
    assert f.plain_passes() == (1, f.n_chunks)
    assert (meet >= 0).all()
    late = meet > m.MEET_BITS
    laid = np.arange(1, f.n_chunks - 1, 4)
    assert (meet[laid] >= 200).all() and (meet[laid] < 512).all()
    assert 4 * int(late.sum()) >= f.n_chunks
