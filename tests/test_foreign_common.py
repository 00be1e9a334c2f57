"""CPU: every condition on its inputs that test_gpu_foreign_modes.py relies on, asserted before any GPU exists
(foreign_common.py's builders): the window spans on and around WIN, the ordinary and the long cubes' kinds, the sides of
the guard under two tables, the reference of the modes against the references the suite already trusts, and the numpy
stream writer against the oracle's on foreign values."""
import numpy as np
import pytest

import foreign_common as fc
import quant_common as qc

DEPTHS = [8, 4]


def _tables_used(depth):
    """every table a GPU case decodes under: the reference table, the set table, the guard palette"""
    t = qc.tables(depth)
    return [qc.pkg().quant_table(5, depth), t["seeded"]] + list(fc.guard_palette(depth))


def test_window_geometry_is_read_from_the_header():
    for depth in DEPTHS:
        win, cpw = fc.window_geometry(depth)
        assert cpw * 64 * depth == 2048
        assert win % 4 == 3 and win > 2048 * 27 // 32, "a multiple of 16 bytes less one word; an encoder's group always fits"


def test_group_spans_counts_as_the_kernel_does():
    """span = (last >> 5) + 5 - (gb >> 5) by hand on all-zero cubes (one bit a value: 2,048 bits a group)"""
    for depth in DEPTHS:
        _, cpw = fc.window_geometry(depth)
        q = np.zeros((2 * cpw + 1, depth, 8, 8), np.int32)  # two groups and a last one of a single cube
        assert fc.group_spans(q, depth, 0).tolist() == [64 + 5, 64 + 5, (64 * depth) // 32 + 5]
        # from bit 5 the first group ends at bit 2053 of word 64, and so on; the last one at bit 4101 + 64 depth
        assert fc.group_spans(q, depth, 5).tolist() == [64 + 5, 64 + 5, (4101 + 64 * depth) // 32 - 128 + 5]
        q[0, 0, 0, 0] = 2**15  # 33 bits in place of 1: every later mark moves by one word
        assert fc.group_spans(q, depth, 0).tolist() == [65 + 5, 64 + 5, (64 * depth) // 32 + 5]


@pytest.mark.parametrize("name", sorted(fc.BOUNDARY_USES))
@pytest.mark.parametrize("depth", DEPTHS)
def test_boundary_spans(depth, name):
    win, cpw = fc.window_geometry(depth)
    q, ordinary, sb = fc.boundary_use(depth, name)
    seed = fc.BOUNDARY_USES[name][0]
    n_groups = fc.BOUNDARY_CUBES // cpw
    assert q.shape == (fc.BOUNDARY_CUBES, depth, 8, 8) and q.dtype == np.int32
    span = fc.group_spans(q, depth, sb)
    delta, place = fc.boundary_plan(depth, n_groups, seed)
    assert np.array_equal(span, win + delta), "the spans are the planned ones exactly"
    for at in (win - 1, win, win + 1):
        assert (span == at).sum() >= 2, at
    assert ((span >= win - 200) & (span <= win + 200)).all()
    assert (span < win - 1).sum() >= 2 and (span > win + 1).sum() >= 2, "other spans on both sides"
    fits = span <= win
    pairs = {(bool(fits[g]), bool(fits[g + 4])) for g in range(n_groups - 4)}
    assert pairs == {(True, True), (True, False), (False, True), (False, False)}, "successive rounds of one wave"
    assert fits[0] != fits[-1] and fits[0] == (seed % 2 == 0)
    # the ordinary cube: one a group, first, in the middle and last in turn; last in a group that fits with no word
    # to spare and in one that does not fit
    assert ordinary.reshape(n_groups, cpw).sum(axis=1).tolist() == [1] * n_groups
    assert {int(p) for p in place} == {0, cpw // 2, cpw - 1}
    last = place == cpw - 1
    assert (last & (span >= win - 1) & fits).any() and (last & ~fits).any()
    assert place[0] == cpw - 1 and place[-1] == cpw - 1


@pytest.mark.parametrize("depth", DEPTHS)
def test_first_and_last_group_take_both_kinds_across_the_uses(depth):
    win, _ = fc.window_geometry(depth)
    first, last = set(), set()
    for name in fc.BOUNDARY_USES:
        q, _, sb = fc.boundary_use(depth, name)
        span = fc.group_spans(q, depth, sb)
        first.add(bool(span[0] <= win))
        last.add(bool(span[-1] <= win))
    assert first == {True, False} and last == {True, False}


@pytest.mark.parametrize("name", sorted(fc.BOUNDARY_USES))
@pytest.mark.parametrize("depth", DEPTHS)
def test_boundary_cube_kinds(depth, name):
    q, ordinary, _ = fc.boundary_use(depth, name)
    lmax = qc.l1_max(depth)
    longs, ords = q[~ordinary], q[ordinary]
    assert np.abs(longs.astype(np.int64)).min() > qc.Q15, "every value of a long cube is out of range: replayed whole"
    bits = qc.code_bits(longs)
    assert set(np.unique(bits).tolist()) == set(fc.WIDTHS), "39- to 49-bit codes, each width in use"
    assert np.abs(ords).max() <= 11 and np.abs(ords.reshape(len(ords), -1)[:, 1:]).max() <= 3
    for T in _tables_used(depth):
        assert (qc.l1(ords, T, depth) < lmax / 4).all()
    # dense: one AC value in three, and no 32 bits of its codes without a non-zero value
    vals = fc.stream_values(ords, depth)
    assert 0.25 < np.count_nonzero(vals) / vals.size < 0.42
    for row in vals:
        pos = np.concatenate([[0], np.cumsum(qc.code_bits(row))])
        nz = pos[:-1][row != 0]
        assert np.diff(np.concatenate([[0], nz, pos[-1:]])).max() <= 32


def _guard_cases(depth):
    p = qc.pkg()
    pal = fc.guard_palette(depth)
    for w, h, stacks in fc.GUARD_SIZES:
        m = fc.guard_map(stacks)
        for size in ((w, h), p.chroma_size(w, h)):
            wp, hp = p.padded_size(*size)
            cps = (wp // 8) * (hp // 8)
            for k in range(3):
                yield pal, m[:, k], stacks, cps, k


@pytest.mark.parametrize("depth", DEPTHS)
def test_split_guard_cubes_are_on_the_stated_sides(depth):
    lmax = qc.l1_max(depth)
    n = 0
    for pal, col, stacks, cps, k in _guard_cases(depth):
        q = fc.split_guard_cubes(depth, pal, col, cps, 5, k)
        assert q.shape == (stacks, cps, depth, 8, 8)
        places = fc.guard_places(stacks, cps)
        assert len(places) >= 2 and len(places) < stacks * cps, "guard cubes, and other kinds around them"
        for (s0, c), (s1, c1) in zip(places[0::2], places[1::2]):
            assert s1 == s0 + 1 and c1 == c and np.array_equal(q[s0, c], q[s1, c]), "one cube in two consecutive stacks"
            l1 = [int(qc.l1(q[s, c], pal[col[s]], depth)[0]) for s in (s0, s1)]
            hi, lo = max(l1), min(l1)
            assert hi - 255 >= lmax and hi < lmax * 1.01, "over the guard with the coarser table, and just"
            assert lo + 255 < lmax * 0.75, "far under it with the finer one (ones: 1 / 255 of it; seeded: its mean step / 255)"
            assert np.abs(q[s0, c]).max() <= qc.Q15, "in range: the guard alone sends it to the replay"
            n += 1
    assert n >= 6
    # at an even stack a guard cube is over the guard in channel 1 alone
    m = fc.guard_map(4)
    pal = fc.guard_palette(depth)
    coarse = [[int(pal[m[s, k]].sum()) == 255 * qc.n_steps(depth) for k in range(3)] for s in range(4)]
    assert coarse == [[False, True, False], [True, False, True]] * 2


@pytest.mark.parametrize("depth", DEPTHS)
def test_ref_modes_is_the_vq_reference(depth):
    """encoder-written values of 24 x 24 grey, 11 stacks, 8 tables cycling: test_gpu_vq.reference"""
    import test_gpu_vq as vq
    w, h = 24, 24
    per_q, out = vq.reference(depth, w, h, 1, 8, "cycle")
    pal, m = vq.palette(depth, 8), vq.stack_map("cycle", 8)
    q = np.stack(per_q).reshape(vq.STACKS, 1, -1, depth, 8, 8)
    assert np.array_equal(fc.ref_modes(q, w, h, vq.STACKS, depth, pal, m[:, None], "planes"), out)
    # and the streams of those values
    assert fc.streams_of(q, depth, [3]) == vq.ref_streams(per_q, depth, 1, [(0xFF, 3)])


@pytest.mark.parametrize("depth", DEPTHS)
def test_ref_modes_is_the_colour_composition_of_ref_frames(depth):
    """one ycc shape and one c420 shape: ycbcr_to_rgb / ycbcr420_to_rgb of quant_common.ref_frames' planes"""
    from test_gpu_ycc import colour
    p = qc.pkg()
    T = qc.tables(depth)["q12"]
    w, h, stacks = 13, 11, 2
    fr = colour("ramp", depth, w, h, stacks)
    q, out = qc.ref_frames(p.rgb_to_ycbcr(fr), T, depth)
    assert np.array_equal(fc.ref_modes(q.reshape(stacks, 3, -1, depth, 8, 8), w, h, stacks, depth, T[None], np.zeros((stacks, 3), int), "ycc"),
                          p.ycbcr_to_rgb(out))
    assert np.array_equal(fc.ref_modes(q.reshape(stacks, 3, -1, depth, 8, 8), w, h, stacks, depth, T[None], np.zeros((stacks, 3), int), "planes"), out)
    w, h = 17, 16
    fr = colour("ramp", depth, w, h, stacks)
    res = [qc.ref_frames(np.ascontiguousarray(pl), T, depth) for pl in p.rgb_to_ycbcr420(fr)]
    qs = [qk.reshape(stacks, -1, depth, 8, 8) for qk, _ in res]
    assert np.array_equal(fc.ref_modes(qs, w, h, stacks, depth, T[None], np.zeros((stacks, 3), int), "c420"),
                          p.ycbcr420_to_rgb(*[o for _, o in res]))


@pytest.mark.parametrize("kind", ["limit", "long", "all_long", "ordinary", "boundary", "split_guard"])
@pytest.mark.parametrize("depth", DEPTHS)
def test_numpy_streams_equal_the_oracle_s_writer(depth, kind):
    """test_gpu_vq.ref_streams (through streams_of) against oracle.eg_write (test_gpu_eg._expected), bit for bit"""
    import oracle
    from test_gpu_eg import _expected
    if kind == "boundary":
        q, _, sb = fc.boundary_use(depth, "grey5")
        q = q[:16]
    elif kind == "split_guard":
        q, sb = fc.split_guard_cubes(depth, fc.guard_palette(depth), fc.guard_map(4)[:, 0], 2, 5).reshape(-1, depth, 8, 8), 7
    else:
        q, sb = fc.STREAM_KINDS[kind](depth, 6, 11 + depth), 3
    got = fc.streams_of(q.reshape(2, 1, -1, depth, 8, 8), depth, [sb])[0]
    want = _expected(oracle, qc.pkg(), np.ascontiguousarray(q), depth, 0xFF, sb)
    assert got == want and got[1] == sb + int(qc.code_bits(q).sum())
