"""Builders of decode inputs that no encoder of 8-bit frames writes, shared by test_gpu_quant_foreign.py,
test_gpu_foreign_modes.py and test_foreign_common.py (which asserts on the CPU every condition the GPU cases rely on).
numpy only: nothing here calls the library's kernels.

The stream decode kernels parse a wave's group of CPW = 2048 / CS cubes (2,048 values) from an LDS window of WIN words
when the group's `span` of stream words is at most WIN, and from global memory otherwise (decode_eg_kernel's
open_window, the channel loop of decode_eg_rgb_kernel, decode_eg_y420_kernel):

    span = (last >> 5) + 5 - (gb >> 5)      gb: the bit of the group's first value, last: the next group's (or the end bit)

boundary_cubes builds content whose spans sit on WIN - 1, WIN, WIN + 1 and around them; split_guard_cubes builds content
whose cubes change sides of the decode's L1 guard with the table of their stack; ref_modes is the reference of every
stream decode (grey, planes, YCbCr, 4:2:0) under a table per (stack, channel)."""
import functools
import os
import re

import numpy as np

import quant_common as qc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "3ddctvideoencoding_amd", "csrc")


# ---- the cube kinds of test_gpu_quant_foreign.py (section 3) --------------------------------------------------------

def sparse(rng, n, depth):
    q = rng.integers(-20, 21, size=(n, depth, 8, 8))
    q[rng.random(q.shape) < 0.5] = 0
    return q


def limit_cubes(depth, n, seed):
    """3a: sparse small values with +-(2^15 - 1) among them (31-bit codes, the widest the unchecked parse steps take);
    cube n // 3: all 32 values of one lane's part (kz = depth - 1, every ky, kx = 4 .. 7) are +-(2^15 - 1); cube
    2n // 3: entirely +-(2^15 - 1)"""
    rng = np.random.default_rng(seed)
    q = sparse(rng, n, depth)
    sgn = rng.choice([-1, 1], size=q.shape)
    edge = rng.random(q.shape) < 0.002
    edge[0, 0, 0, 1] = True
    q[edge] = qc.Q15 * sgn[edge]
    q[n // 3, depth - 1, :, 4:] = qc.Q15 * sgn[n // 3, depth - 1, :, 4:]
    q[2 * n // 3] = qc.Q15 * sgn[2 * n // 3]
    q = q.astype(np.int32)
    assert np.abs(q).max() == qc.Q15 and qc.code_bits(q).max() == 31
    assert np.abs(q[n // 3, depth - 1, :, 4:]).min() == qc.Q15 and 32 * qc.Q15 * 255 < 2**28
    return q


def long_cubes(depth, n, seed):
    """3b: a few values in [2^15, 2^20) (33- to 41-bit codes) among sparse small ones and +-(2^15 - 1); the first
    value of the stream is 2^15, the narrowest long code"""
    rng = np.random.default_rng(seed)
    q = sparse(rng, n, depth)
    sgn = rng.choice([-1, 1], size=q.shape)
    edge = rng.random(q.shape) < 0.002
    q[edge] = qc.Q15 * sgn[edge]
    big = rng.random(q.shape) < 0.001
    big[n - 1, 1, 2, 3] = True
    q[big] = rng.integers(2**15, 2**20, size=int(big.sum())) * sgn[big]
    q[0, 0, 0, 0] = 2**15
    q = q.astype(np.int32)
    bits = qc.code_bits(q)
    assert bits[0, 0, 0, 0] == 33 and 33 <= bits.max() <= 41 and (bits > 31).sum() >= 2
    return q


def all_long_cubes(depth, n, seed):
    """3c: every |q| in [2^15, 2^16): 33-bit codes only"""
    rng = np.random.default_rng(seed)
    q = (rng.integers(2**15, 2**16, size=(n, depth, 8, 8)) * rng.choice([-1, 1], size=(n, depth, 8, 8))).astype(np.int32)
    assert (qc.code_bits(q) == 33).all()
    return q


def ordinary_stream_cubes(depth, n, seed):
    """what an encoder writes even under all255: a DC of at most 11 (255 sqrt(512) / 255), one AC value in ten +-1:
    L1 under the guard with every table"""
    rng = np.random.default_rng(seed)
    q = rng.choice([-1, 1], size=(n, depth, 8, 8)) * (rng.random((n, depth, 8, 8)) < 0.1)
    q[:, 0, 0, 0] = rng.integers(0, 12, size=n)
    assert (qc.l1(q, np.full(qc.n_steps(depth), 255), depth) < qc.l1_max(depth) / 4).all()
    return q.astype(np.int32)


STREAM_KINDS = {"limit": limit_cubes, "long": long_cubes, "all_long": all_long_cubes, "ordinary": ordinary_stream_cubes}


# ---- the window ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def window_geometry(depth):
    """(WIN, CPW): the words of a wave's LDS window, WIN = kDecWaveLds / 4 - 1 with kDecWaveLds read from the text of
    dct3d_decode_dev.h, and the cubes of a wave's group, 2048 / (64 depth).  Every copy of the window logic is held to
    that expression of WIN here, so that a copy changed on its own fails on the CPU."""
    text = open(os.path.join(CSRC, "dct3d_decode_dev.h")).read()
    m = re.findall(r"constexpr\s+int\s+kDecWaveLds\s*=\s*(\d+)\s*;", text)
    assert len(m) == 1, "kDecWaveLds is defined once, as a literal"
    copies = 0
    for name in ("dct3d_eg_fused_dev.h", "dct3d_c420.hip"):
        src = open(os.path.join(CSRC, name)).read()
        copies += len(re.findall(r"constexpr\s+uint32_t\s+WIN\s*=\s*kDecWaveLds\s*/\s*4\s*-\s*1\s*;", src))
        assert len(re.findall(r"\bWIN\s*=", src)) == len(re.findall(r"WIN\s*=\s*kDecWaveLds\s*/\s*4\s*-\s*1\s*;", src)), name
    assert copies == 3, "decode_eg_kernel, decode_eg_rgb_kernel and decode_eg_y420_kernel"
    return int(m[0]) // 4 - 1, 2048 // (64 * depth)


def stream_values(q, depth):
    """one channel's cubes [.., depth, 8, 8] in stream order: [cube][CS] values in diagonal order"""
    order = qc.pkg().diagonal_order(8, 8, depth)
    return np.asarray(q).reshape(-1, 64 * depth)[:, order]


def group_spans(q, depth, start_bit):
    """the kernels' span of each group of CPW cubes of one channel's stream that starts at bit start_bit: int64 [groups]
    (a last group of fewer cubes included; its `last` is the end bit, as the first group's gb is the start bit)"""
    _, cpw = window_geometry(depth)
    per_cube = qc.code_bits(stream_values(q, depth)).sum(axis=1)
    pos = start_bit + np.concatenate([[0], np.cumsum(per_cube)])
    gb = pos[:-1:cpw]
    last = np.concatenate([gb[1:], pos[-1:]])
    return (last >> 5) + 5 - (gb >> 5)


WIDTHS = (39, 41, 43, 45, 47, 49)  # the long cubes' code widths: |q| in [2^18, 2^24)
FIT_PATTERN = (True, True, False, False, True, False, True, False)  # (g, g + 4): fit/fit, fit/no, no/fit, no/no


def boundary_plan(depth, n_groups, seed):
    """(span - WIN of each group, the ordinary cube's place in each group).  Fitting and non-fitting groups follow
    FIT_PATTERN, inverted for an odd seed, and the last group is the opposite of the first: across two seeds of
    different parity the first and the last group take both kinds.  The first fitting groups are at WIN, WIN - 1, WIN,
    WIN - 1 and the first two others at WIN + 1; the rest are drawn from [-200, -2] and [2, 200], as far as the widths
    reach: at 8x8x8 a group's 1,536 long values end at WIN + 60 with 49 bits each, at 8x8x4 its 1,792 begin at WIN - 100
    with 39 bits each.  The ordinary cube is first, in the middle, last in turn,
    and last in the last group."""
    assert n_groups >= 8, "all four combinations of (g, g + 4)"
    _, cpw = window_geometry(depth)
    rng = np.random.default_rng(4099 * seed + depth)
    fit = [FIT_PATTERN[g % 8] != bool(seed % 2) for g in range(n_groups)]
    fit[-1] = not fit[0]
    lo, hi = (200, 60) if depth == 8 else (100, 200)
    near_fit, near_no = [0, -1, 0, -1], [1, 1]
    delta = [(near_fit.pop(0) if near_fit else -int(rng.integers(2, lo + 1))) if f else
             (near_no.pop(0) if near_no else int(rng.integers(2, hi + 1))) for f in fit]
    place = [(0, cpw // 2, cpw - 1)[(g + 2) % 3] for g in range(n_groups)]  # (group 0: last)
    place[-1] = cpw - 1
    return np.array(delta), np.array(place)


def dense_ordinary_cube(depth, rng):
    """ordinary_stream_cubes' kind, denser: one AC value in three is +-1 (mostly), +-2 or +-3, the DC at most 11.  In
    range, its L1 under l1_max / 4 with every table (asserted with all255), and no 32-bit word of its codes without a
    non-zero value, so that any missing window word changes its pixels."""
    mag = rng.choice([1, 2, 3], p=[0.8, 0.15, 0.05], size=(depth, 8, 8))
    q = rng.choice([-1, 1], size=(depth, 8, 8)) * mag * (rng.random((depth, 8, 8)) < 1 / 3)
    q[0, 0, 0] = rng.integers(0, 12)
    assert qc.l1(q, np.full(qc.n_steps(depth), 255), depth)[0] < qc.l1_max(depth) / 4
    return q.astype(np.int32)


@functools.lru_cache(maxsize=None)
def boundary_cubes(depth, n_groups, seed, start_bit):
    """int32 [n_groups * CPW, depth, 8, 8] (read-only): in every group CPW - 1 long cubes (every |q| >= 2^18: out of
    range, replayed whole from the stream) and one dense ordinary cube (in range, under the guard: its bytes come
    straight from the one-pass parse), the long cubes' code widths chosen per value from WIDTHS and tuned, two bits at
    a time, so that the group's span from start_bit is WIN + boundary_plan's delta exactly."""
    win, cpw = window_geometry(depth)
    cs = 64 * depth
    order = qc.pkg().diagonal_order(8, 8, depth)
    rng = np.random.default_rng(7919 * seed + 31 * depth + start_bit)
    delta, place = boundary_plan(depth, n_groups, seed)
    out = np.zeros((n_groups * cpw, cs), np.int64)  # in stream order
    n_long = (cpw - 1) * cs
    pos = start_bit
    for g in range(n_groups):
        o = dense_ordinary_cube(depth, rng).reshape(cs)[order]
        ob = int(qc.code_bits(o).sum())
        # last >> 5 = (gb >> 5) + span - 5: the long widths' sum s is even (an even count of odd widths)
        lo = 32 * ((pos >> 5) + win + int(delta[g]) - 5) - pos - ob
        s = lo + int(rng.integers(0, 32))
        s += s % 2 if s + 1 < lo + 32 else -(s % 2)
        k_sum = (s - WIDTHS[0] * n_long) // 2
        assert (s - WIDTHS[0] * n_long) % 2 == 0 and 0 <= k_sum <= 5 * n_long, (g, s)
        k = np.clip(np.rint(k_sum / n_long + rng.normal(0, 1.2, n_long)), 0, 5).astype(np.int64)
        diff = k_sum - int(k.sum())
        while diff:  # one step on |diff| values that have room, chosen at random
            room = np.flatnonzero(k < 5) if diff > 0 else np.flatnonzero(k > 0)
            pick = rng.choice(room, size=min(abs(diff), room.size), replace=False)
            k[pick] += 1 if diff > 0 else -1
            diff = k_sum - int(k.sum())
        nbits = 20 + k  # the code's bits: width = 2 nbits - 1; |q| in [2^(nbits - 2), 2^(nbits - 1))
        mag = (1 << (nbits - 2)) + (rng.random(n_long) * (1 << (nbits - 2))).astype(np.int64)
        longs = (mag * rng.choice([-1, 1], size=n_long)).reshape(cpw - 1, cs)
        grp = out[g * cpw:(g + 1) * cpw]
        grp[np.arange(cpw) != place[g]] = longs
        grp[place[g]] = o
        pos += s + ob
    q = np.zeros_like(out)
    q[:, order] = out
    q = q.reshape(-1, depth, 8, 8).astype(np.int32)
    q.setflags(write=False)
    return q


# What test_gpu_foreign_modes.py decodes, asserted on the CPU by test_foreign_common.py: a boundary stream is 96 cubes
# (2 stacks of 48: 64 x 48, 61 x 45, or the chroma planes of 128 x 96), 24 groups at 8x8x8 and 12 at 8x8x4; name ->
# (seed, start bit): the grey cases' two start bits, and channel k of an RGB or 4:2:0 call from start bits (3, 0, 5)
BOUNDARY_CUBES = 96
BOUNDARY_USES = {"grey0": (0, 0), "grey5": (1, 5), "ch0": (0, 3), "ch1": (1, 0), "ch2": (0, 5)}


def boundary_use(depth, name):
    """(cubes [96, depth, 8, 8], bool [96]: the ordinary ones, start bit) of BOUNDARY_USES[name]"""
    seed, sb = BOUNDARY_USES[name]
    n_groups = BOUNDARY_CUBES // window_geometry(depth)[1]
    return boundary_cubes(depth, n_groups, seed, sb), ordinary_mask(depth, n_groups, seed), sb


@functools.lru_cache(maxsize=None)
def guard_palette(depth):
    """ones, seeded, all255 (read-only): split_guard_cubes' fine, middle and coarse table"""
    t = qc.tables(depth)
    pal = np.stack([t["ones"], t["seeded"], t["all255"]]).astype(np.int32)
    pal.setflags(write=False)
    return pal


def guard_map(stacks):
    """uint8 [stacks, 3] over guard_palette: column 0 alternates ones / all255, column 1 all255 / ones, column 2
    seeded / all255 -- at an even stack a guard cube is over the guard in channel 1 alone, at an odd one in 0 and 2"""
    s = np.arange(stacks) % 2
    return np.ascontiguousarray(np.stack([2 * s, 2 - 2 * s, 1 + s], axis=1), np.uint8)


def ordinary_mask(depth, n_groups, seed):
    """bool [n_groups * CPW]: the ordinary cube of each group of boundary_cubes"""
    _, cpw = window_geometry(depth)
    _, place = boundary_plan(depth, n_groups, seed)
    m = np.zeros(n_groups * cpw, bool)
    m[np.arange(n_groups) * cpw + place] = True
    return m


# ---- the guard under two tables ------------------------------------------------------------------------------------

GUARD_SIZES = [(8, 8, 12), (24, 24, 12), (29, 13, 4)]  # (w, h, stacks) of the split-guard cases


def guard_places(stacks, cps):
    """[(stack, cube)] of split_guard_cubes' guard cubes: pair j of stacks (2 j, 2 j + 1) at cube j % cps; with one cube
    per stack only every other pair, so that other kinds stand between them"""
    return [(2 * j + i, j % cps) for j in range(stacks // 2) if cps > 1 or j % 2 == 0 for i in (0, 1)]


def split_guard_cubes(depth, pal, m, cps, seed, channel=0):
    """int32 [stacks, cps, depth, 8, 8] for a map column m (one palette entry per stack) that alternates a fine and a
    coarse table: both stacks of a pair of guard_places hold the same guard_cube, built with the coarser of the pair's
    two tables just over l1_max (by more than its largest step) -- under the finer one it is far under the guard: one cube, under the guard with its
    stack's table and over it with the next stack's (or the other way round).  Around it: limit, long and ordinary
    cubes in turn.  channel: varies the seed."""
    m = np.asarray(m)
    stacks = m.size
    assert stacks % 2 == 0
    rng = np.random.default_rng(104729 * seed + 17 * depth + channel)
    lmax = qc.l1_max(depth)
    n = stacks * cps
    fill = [STREAM_KINDS[k](depth, max(n, 3), 1000 * seed + 7 * i + depth + channel) for i, k in enumerate(("limit", "long", "ordinary"))]
    q = np.stack([fill[i % 3][i] for i in range(n)]).reshape(stacks, cps, depth, 8, 8)
    places = guard_places(stacks, cps)
    for (s0, c), (s1, _) in zip(places[0::2], places[1::2]):
        ta, tb = pal[m[s0]], pal[m[s1]]
        g = qc.guard_cube(ta if ta.sum() > tb.sum() else tb, depth, rng, lmax * (1 + 2.0**-10) + 512)
        q[s0, c] = g
        q[s1, c] = g
    return np.ascontiguousarray(q, np.int32)


# ---- the reference ---------------------------------------------------------------------------------------------------

def channels_of(q):
    """q [stack][channel][cube] as an array, or a sequence over the channels of [stack][cube] arrays (4:2:0: the
    channels differ in size) -> the list over the channels"""
    if isinstance(q, np.ndarray):
        return [q[:, k] for k in range(q.shape[1])]
    return list(q)


def ref_modes(q, w, h, stacks, depth, pal, table_map, mode):
    """The stream decodes' definition with a table per (stack, channel), no call into the library's kernels: channel
    k of stack s is qc.ref_decode_frames (dequantize_ref, the oracle's Java fold, the byte clamp, the crop) under
    pal[table_map[s][k]] at the channel's size; then mode "planes": the channels packed (one channel: the grey frames);
    "ycc": ycbcr_to_rgb of them; "c420": ycbcr420_to_rgb(y, cb, cr), cb and cr at chroma_size(w, h)."""
    p = qc.pkg()
    chans = channels_of(q)
    table_map = np.asarray(table_map).reshape(stacks, len(chans))
    sizes = [(w, h)] + [p.chroma_size(w, h) if mode == "c420" else (w, h)] * (len(chans) - 1)
    planes = []
    for k, (qk, (wk, hk)) in enumerate(zip(chans, sizes)):
        planes.append(np.concatenate([qc.ref_decode_frames(np.ascontiguousarray(qk[s]), wk, hk, 1, 1, pal[table_map[s][k]], depth)
                                      for s in range(stacks)]))
    if len(chans) == 1:
        assert mode == "planes"
        return planes[0]
    if mode == "c420":
        return p.ycbcr420_to_rgb(*planes)
    out = np.ascontiguousarray(np.stack(planes, axis=-1))
    return out if mode == "planes" else p.ycbcr_to_rgb(out)


def streams_of(q, depth, start_bits):
    """test_gpu_vq.ref_streams of q (channels_of) from bit start_bits[k] of a carried byte of ones: [(bytes, end bit)]"""
    from test_gpu_vq import ref_streams
    res = []
    for qk, sb in zip(channels_of(q), start_bits):
        per = [np.asarray(qs).reshape(1, -1, 64 * depth) for qs in qk]
        res.append(ref_streams(per, depth, 1, [(0xFF, sb)])[0])
    return res
