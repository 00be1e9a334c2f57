"""CPU: cert_common.py, the predictions test_gpu_certificates.py compares the device's counts with.

  * encode_open is test_emulation.py's emulation: the same flags on the same cubes;
  * soundness, restated for the shapes and tables used on the GPU: every coefficient encode_open leaves closed has the
    emulated q equal to the reference's (quant_common.py), every pixel of a lane decode_open does not flag has the
    emulated byte equal to the oracle's decode;
  * the preconditions of every GPU case hold -- richness, the empty ambiguous band of split_8x8x8, decode_open's
    margin and guard bands -- so that a bad seed is found here, without a GPU;
  * sensitivity: the thresholds read at s + 1 instead of s (the tables shifted in Python, no kernel built) change the
    predicted count of every rich case: that mutation cannot pass the GPU module unseen;
  * the same for the rate and distortion probes' predictions (test_gpu_probe_certificates.py): soundness under the
    probe-only tables, the decode preconditions at every margin used, a set's count as the sum of its tables', and
    the shifted threshold seen by every rich set;
  * the same for the RGB-domain distortion probe's predictions (test_gpu_distortion_rgb_certificates.py), per plane of
    the colour transform: and the rule for which (table, plane) pairs a call codes, and that a band's crop has the
    whole frame's cubes;
  * the same for the SSIM probes' predictions (test_gpu_ssim_certificates.py): the range cases' arithmetic (how many
    ranges, how many stacks in each), soundness and the decode preconditions under each of the 11 names, richness, the
    shifted threshold seen, no per-stack count repeated, and the planes mode's compaction rule against a brute-force
    restatement."""
import numpy as np
import pytest

import cert_common as cc
import quant_common as qc
from test_emulation import emu, run  # noqa: F401  (emu: the fixture that builds emulate_encode.cpp)

ENCODE_CASES = cc.STACKS8 + cc.STACKS4 + cc.RGB + cc.EDGE + cc.EG
_seen = set()
ENCODE_CASES = [c for c in ENCODE_CASES if not (c.id in _seen or _seen.add(c.id))]  # (families share inputs)


@pytest.mark.parametrize("depth", [8, 4])
def test_encode_open_is_the_emulation_of_test_emulation(emu, pkg, oracle, depth):  # noqa: F811
    for c in (cc.Case("uniform", depth, 1, 200, 72, 4), cc.Case("uniform", depth, 1, 13, 11, 1)):
        cubes = oracle.to_cubes(cc.raster_of(c.frames(), depth), 8, 8, depth)
        q, fl, _, _, _ = run(emu, pkg, cubes, depth)
        q2, op, cubes2 = cc.encode_emulate(c.frames(), depth)
        assert np.array_equal(cubes, cubes2) and np.array_equal(q, q2)
        assert not fl[:, 0, 0, 0].any() and np.array_equal(op, fl)
        assert np.array_equal(cc.encode_open(c.frames(), depth), fl)


def test_rgb_raster_is_the_planar_stacked_one(pkg):
    """channels = 3: per stack its R, then G, then B frames (dct3d.h), each plane padded as a grey one"""
    c = cc.Case("uniform", 4, 3, 13, 11, 2)
    fr = c.frames()
    r = cc.raster_of(fr, 4)
    assert r.shape == (24, 16, 16)
    for s in range(2):
        for ch in range(3):
            assert np.array_equal(r[12 * s + 4 * ch:12 * s + 4 * ch + 4], pkg.pad_frames(fr[4 * s:4 * s + 4, :, :, ch]))
    op = cc.encode_open(fr, 4, qc.tables(4)["q1"], channels=3)
    planes = [cc.encode_open(np.ascontiguousarray(fr[..., ch]), 4, qc.tables(4)["q1"]) for ch in range(3)]
    assert op.sum() == sum(p.sum() for p in planes)  # the count is the sum over the three planes


@pytest.mark.parametrize("c", ENCODE_CASES, ids=repr)
def test_encode_case_soundness_preconditions_sensitivity(c):
    """soundness at the GPU module's shapes (under every table, what encode_open leaves closed is the reference's q, the
    DC by its closed form); richness where the case claims it; split_8x8x8's empty band; and the shifted threshold
    seen by every rich case.  (One function per case: the emulation and the oracle's DCT are computed once.)"""
    for name in cc.TABLES:
        q, op = cc.case_open(c, name)
        bad = (q != cc.case_q_ref(c, name)) & ~op
        assert not bad.any(), f"{name}: {int(bad.sum())} closed coefficients differ"
        counts = cc.band_counts(op, c.stacks, c.channels, c.nby)
        if c.depth == 8:
            fold, rechk = cc.split_8x8x8(c.frames(), op, cc.table(name, 8), cc.case_dct(c))  # (asserts the band empty)
            assert not (fold & rechk).any() and np.array_equal(fold | rechk, op)
        if name in c.rich:
            assert cc.is_rich(counts), f"{c.id} {name}: {counts.tolist()}"
            shifted = cc.band_counts(cc.case_open(c, name, shift=1)[1], c.stacks, c.channels, c.nby)
            assert shifted.sum() != counts.sum(), f"{c.id} {name}: the count does not see thr[s + 1]"
            assert not np.array_equal(shifted, counts)
        print(f"{c.id} {name}: {int(op.sum())} open, per band {counts.tolist() if c.nby <= 9 else '...'}")


def test_every_table_has_a_rich_case_in_every_family():
    for fam in (cc.STACKS8, cc.STACKS4):
        assert {n for c in fam for n in c.rich} == set(cc.TABLES)
    for fam in (cc.RGB, cc.EDGE, cc.EG):
        for depth, want in ((8, cc.RICH8), (4, cc.RICH4)):
            assert {n for c in fam if c.depth == depth for n in c.rich} == set(want)


def test_ramp_crop_holds_the_exact_tie():
    """cube 14829 of the 1080p ramp stack at frame 200 is block (61, 189): block (3, 3) of the crop, whose (0, 2, 2) is
    10 = 0.5 * step exactly; the fp32 certificate leaves it open and split_8x8x8 sends it to the fold"""
    c = cc.STACKS8[3]
    assert c.kind == "ramp_crop" and 14829 == 61 * 240 + 189
    _, op = cc.case_open(c, "ref")
    fold, _ = cc.split_8x8x8(c.frames(), op, None, cc.case_dct(c))
    assert op[27, 0, 2, 2] and fold[27, 0, 2, 2] and fold.sum() >= 1
    assert abs(abs(cc.case_dct(c)[27, 0, 2, 2]) - 10.0) < 1e-9


@pytest.mark.parametrize("name", ["ref", "seeded"])
@pytest.mark.parametrize("c", cc.DEC, ids=repr)
def test_decode_open_on_encoder_output(c, name):
    """margin 0 flags nothing on an encoder's output; at every margin the GPU module uses the preconditions hold (they
    are asserted inside), the shares are the ones MARGINS' comment states, and -- soundness -- every pixel of an
    unflagged lane has the emulated byte equal to the oracle's decode, also under a margin as wide as 0.25"""
    T = cc.table(name, c.depth)
    q = cc.case_q_ref(c, name)
    wp, hp = qc.pkg().padded_size(c.w, c.h)
    import oracle
    ref = oracle.to_cubes(qc.ref_decode(q, wp, hp, c.channels * c.stacks * c.depth, cc.steps_of(T, c.depth), c.depth),
                          8, 8, c.depth)
    shares = []
    for m in (0.0,) + cc.MARGINS + (0.25,):
        lanes, byte = cc.decode_emulate(q, c.depth, T, m)
        cert = ~cc.lane_pixels(lanes, c.depth)
        assert np.array_equal(byte[cert], ref[cert]), f"margin {m}: a certified pixel differs from the oracle"
        shares.append(float(lanes.mean()))
    assert shares[0] == 0.0
    if (c.w, c.h) == (200, 72):
        assert 0.005 < shares[1] < 0.015 and 0.08 < shares[2] < 0.12 and 0.45 < shares[3] < 0.55, shares
    print(f"{c.id} {name}: flagged share at 0, MARGINS, 0.25: {shares}")


@pytest.mark.parametrize("name", ["ref", "seeded"])
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_guard_cubes(depth, name):
    """the L1 guard case's preconditions (inside decode_emulate), and its prediction: the two cubes over dec_l1_max are
    flagged whole, 64 depth pixels each"""
    q, over = cc.guard_cubes(depth, name)
    for m in (0.0, cc.MARGINS[1]):
        lanes = cc.decode_open(q, depth, cc.table(name, depth), m)
        assert lanes[over].all()
        assert 32 * int(lanes[over].sum()) == 64 * depth * 2
    assert lanes[~over].any() and not lanes[~over].all()  # at the 10 % margin the under cubes flag some lanes


def test_lane_ownership_mask():
    """lane_pixels: 8x8x8 lane 2 y + h owns x = 4h .. 4h + 3 of row y over z; 8x8x4 lane y owns row y over z"""
    l8 = np.zeros((1, 16), bool)
    l8[0, 2 * 5 + 1] = True
    m8 = cc.lane_pixels(l8, 8)
    assert m8.sum() == 32 and m8[0, :, 5, 4:].all()
    l4 = np.zeros((1, 8), bool)
    l4[0, 3] = True
    m4 = cc.lane_pixels(l4, 4)
    assert m4.sum() == 32 and m4[0, :, 3, :].all()


# ---- the probes' predictions (test_gpu_probe_certificates.py) ---------------------------------------------------------

def _probe_tables(c):
    seen = []
    for s in cc.probe_sets(c):
        seen += [n for n in cc.PROBE_SETS[s] if n not in seen]
    return seen


def test_probe_cases_are_the_listed_ones():
    ids = [c.id for c in cc.PROBE_CASES]
    assert len(ids) == len(set(ids)) == 22
    for d in (8, 4):
        want = [f"uniform-{s}-grey-d{d}" for s in ("200x72x4", "24x16x5", "8x8x1", "1366x24x2", "13x11x1", "1x1x1", "1920x1080x1")] + \
               [f"uniform-{s}-rgb-d{d}" for s in ("200x72x2", "24x16x5", "13x11x1", "1x1x1")]
        assert set(want) == {i for i in ids if i.endswith(f"d{d}")}
    assert len(cc.PROBE_TABLES) == len(set(cc.PROBE_TABLES)) == 11 and cc.PROBE_SETS["four"] == cc.TABLES
    for c in cc.PROBE_CASES:
        sets = cc.probe_sets(c)
        assert sets[:5] == cc.TABLES + ("four",) and sets[-1] == "eleven" and len(sets) == (13 if c.w == 1920 else 6)


@pytest.mark.parametrize("c", cc.PROBE_CASES, ids=repr)
def test_probe_predictions(c):
    """per probe case: under every table of its sets the emulation is sound (what it leaves closed is the reference's
    q, also under the probe-only tables) and decode_emulate's preconditions hold at each of PROBE_MARGINS, with no
    lane flagged at margin 0; the prediction of a set is the sum of its tables' (a coefficient open under k tables
    counts k times); and on the rich cases the thresholds read at s + 1 change the predicted count of every rich
    set, rate and distortion: the counts can see a table row taken one entry off."""
    names = _probe_tables(c)
    lanes = {}
    for n in names:
        q, op = cc.case_open(c, n)
        bad = (q != cc.case_q_ref(c, n)) & ~op
        assert not bad.any(), f"{n}: {int(bad.sum())} closed coefficients differ"
        assert not op[:, 0, 0, 0].any()
        lanes[n] = cc.probe_decode_lanes(c, n, cc.PROBE_MARGINS)  # (asserts the preconditions)
        assert not lanes[n][0].any(), f"{c.id} {n}: a lane flagged at margin 0: another seed"
        if n in c.rich:
            assert cc.is_rich(cc.probe_open_counts(c, n)[:-1]), f"{c.id} {n}"
    for s in cc.probe_sets(c):
        tabs = cc.PROBE_SETS[s]
        rate = cc.rate_probe_counts(c, tabs)
        assert rate.shape == (c.nby + 1,) and rate[-1] == rate[:-1].sum()
        assert np.array_equal(rate, sum(cc.rate_probe_counts(c, (n,)) for n in tabs))
        for i, m in enumerate(cc.PROBE_MARGINS):
            dist = cc.distortion_probe_counts(c, tabs, m)
            assert np.array_equal(dist, sum(cc.distortion_probe_counts(c, (n,), m) for n in tabs))
            assert dist[-1] == rate[-1] + 32 * sum(int(lanes[n][i].sum()) for n in tabs)
        if cc.probe_rich(c, s):
            assert cc.is_rich(rate[:-1])
            shifted = cc.rate_probe_counts(c, tabs, shift=1)
            assert shifted[-1] != rate[-1] and not np.array_equal(shifted, rate), f"{c.id} {s}: rate does not see thr[s + 1]"
            assert cc.distortion_probe_counts(c, tabs, 0.0, shift=1)[-1] != cc.distortion_probe_counts(c, tabs, 0.0)[-1]
        print(f"{c.id} {s}: rate {int(rate[-1])}, distortion at {cc.PROBE_MARGINS}: "
              f"{[int(cc.distortion_probe_counts(c, tabs, m)[-1]) for m in cc.PROBE_MARGINS]}")


def test_probe_reference_is_ref_frames():
    """the GPU module takes the reference's q from case_q_ref (one DCT per case, shared by its tables): it is
    quant_common.ref_frames' q, grey and RGB, ragged sizes included"""
    for c in (cc.EG[1], cc.EG[4]):
        for n in ("ref", "all255", "qt7"):
            T = cc.steps_of(cc.table(n, c.depth), c.depth)
            assert np.array_equal(cc.case_q_ref(c, n), qc.ref_frames(c.frames(), T, c.depth)[0])


# ---- the RGB-domain distortion probe's predictions (test_gpu_distortion_rgb_certificates.py) -------------------------

def test_colour_cases_are_the_listed_ones():
    ids = [c.id for c in cc.COLOUR_PROBE_CASES]
    assert len(ids) == len(set(ids)) == 32
    shapes = ("200x72x2", "208x80x2", "244x54x2", "1366x24x1", "24x16x5", "13x11x1", "1x1x1")
    for d in (8, 4):
        want = [f"{m}-{s}-d{d}" for m in ("ycc", "c420") for s in shapes] + [f"planes-{s}-d{d}" for s in ("200x72x2", "13x11x1")]
        assert set(want) == {i for i in ids if i.endswith(f"d{d}")}
    for c in cc.COLOUR_PROBE_CASES:
        assert c.rich == (c.mode != "planes" and (c.w, c.h) in ((200, 72), (208, 80), (244, 54), (1366, 24)))
    assert set(cc.COLOUR_SETS) == {"q1", "ref", "subsets", "planes4", "eleven", "repeat"}
    names, cand, _ = cc.COLOUR_SETS["subsets"]
    L = cc.coded_tables(len(names), cand, False)
    assert [sorted(x) for x in L] == [[0, 2], [1], [0, 2]] and len({tuple(sorted(x)) for x in L}) >= 2
    assert all(3 not in x and len(x) < 4 for x in L)  # proper subsets; table 3 is coded for no plane
    assert cc.coded_tables(4, cand, True) == [[0, 1, 2, 3]] * 3 == cc.coded_tables(4, None, False)


def test_coded_tables_of_the_repeated_candidates():
    """the L[k] rule restated in Python on test_gpu_distortion_rgb.py's repeated-candidate set: a table several
    candidates name is listed once, in the order of its first use"""
    from test_gpu_distortion_rgb import SETS
    names, cand, want = SETS["repeat"]
    assert (names, tuple(cand), want) == cc.COLOUR_SETS["repeat"]
    L = cc.coded_tables(len(names), cand, want)
    assert [[names[t] for t in x] for x in L] == [["q1", "seeded"], ["q12", "seeded"], ["seeded", "q1"]]


def test_colour_bands_of_a_crop_are_the_whole_frames():
    """a crop that starts at a multiple of the band has the whole frame's cubes in every plane (c420: 16 rows are two
    Y block rows over one chroma block row; the last band of a ragged height is shorter), so the whole raster's masks
    give the per-band predictions"""
    import oracle
    for c in cc.COLOUR_PROBE_CASES:
        if (c.w, c.h) not in ((244, 54), (13, 11)) or c.depth != 4:
            continue
        whole = cc.colour_planes(c)
        for b in range(c.nb):
            crop = cc.ColourCase(c.mode, c.depth, c.w, min(c.band, c.h - b * c.band), c.stacks)
            crop.frames = lambda b=b: np.ascontiguousarray(c.frames()[:, b * c.band:(b + 1) * c.band])
            for k, pl in enumerate(cc.colour_planes(crop)):
                sub = 2 if (c.mode == "c420" and k > 0) else 1
                nby = cc.colour_plane_cubes(c, k)[1]
                rows = [r for r in range(nby) if (8 * sub * r) // c.band == b]
                got = oracle.to_cubes(cc.raster_of(pl, c.depth), 8, 8, c.depth).reshape((c.stacks, len(rows), -1, c.depth, 8, 8))
                want = oracle.to_cubes(cc.raster_of(whole[k], c.depth), 8, 8, c.depth).reshape((c.stacks, nby, -1, c.depth, 8, 8))
                assert np.array_equal(got, want[:, rows]), f"{c.id} band {b} plane {k}"
            assert cc.colour_units(crop, ("q1",), ((0, 0, 0),)) == cc.colour_units(c, ("q1",), ((0, 0, 0),), rows=crop.h)


@pytest.mark.parametrize("c", cc.COLOUR_PROBE_CASES, ids=repr)
def test_colour_probe_predictions(c):
    """per colour case and plane: under every table of the sets the emulation is sound (what it leaves closed is the
    reference's q) and decode_emulate's preconditions hold at each of PROBE_MARGINS, with no lane flagged at margin 0
    under ref, q1, q12 and seeded (under quant_table(64) at 8x8x4 the flat chroma planes do flag lanes at margin 0:
    the prediction carries them); richness where claimed; a set's prediction is the sum over its coded pairs, and
    the thresholds read at s + 1 change the prediction of every rich (case, set)."""
    if c.mode == "planes":
        for s, (names, cand, planes) in cc.COLOUR_SETS.items():
            for m in cc.PROBE_MARGINS:
                assert np.array_equal(cc.colour_distortion_counts(c, names, cand, m, planes),
                                      cc.distortion_probe_counts(c.rgb, names, m))
            assert cc.colour_units(c, names, cand, planes) == len(names) * cc.raster_of(c.frames(), c.depth).size
        return
    for k in range(3):
        ncubes, nby = cc.colour_plane_cubes(c, k)
        for n in cc.PROBE_TABLES:
            q, op = cc.colour_plane_open(c, k, n)
            assert q.shape[0] == ncubes * c.stacks
            bad = (q != cc.colour_plane_q_ref(c, k, n)) & ~op
            assert not bad.any(), f"plane {k} {n}: {int(bad.sum())} closed coefficients differ"
            assert not op[:, 0, 0, 0].any()
            lanes = cc.colour_plane_lanes(c, k, n)  # (asserts the preconditions)
            if n in cc.TABLES:
                assert not lanes[0].any(), f"{c.id} plane {k} {n}: a lane flagged at margin 0: another seed"
            v = cc.colour_open_counts(c, k, n)
            assert v.shape == (c.nb + 1,) and v[-1] == v[:-1].sum() == op.sum()
            for m in cc.PROBE_MARGINS:
                assert cc.colour_lane_counts(c, k, n, m)[-1] == lanes[cc.PROBE_MARGINS.index(m)].sum()
        if c.rich:
            assert cc.colour_open_counts(c, k, "q1")[-1] >= 12, f"{c.id} plane {k}"
    for s, (names, cand, planes) in cc.COLOUR_SETS.items():
        for all_pairs in sorted({planes, True}):  # (asking for the bits codes every pair)
            L = cc.coded_tables(len(names), cand, all_pairs)
            rate = sum(cc.colour_open_counts(c, k, names[t]) for k in range(3) for t in L[k])
            for i, m in enumerate(cc.PROBE_MARGINS):
                dist = cc.colour_distortion_counts(c, names, cand, m, all_pairs)
                assert dist.shape == (c.nb + 1,) and dist[-1] == dist[:-1].sum()
                assert dist[-1] == rate[-1] + 32 * sum(int(cc.colour_plane_lanes(c, k, names[t])[i].sum())
                                                       for k in range(3) for t in L[k])
            if all_pairs:
                assert np.array_equal(rate, cc.colour_rate_counts(c, names))
            if names[0] in cc.TABLES and len(names) <= 4:
                assert np.array_equal(cc.colour_distortion_counts(c, names, cand, 0.0, all_pairs), rate)  # margin 0: the encode term
            units = cc.colour_units(c, names, cand, all_pairs)
            assert units == sum(len(L[k]) * cc.colour_plane_cubes(c, k)[0] for k in range(3)) * 64 * c.depth * c.stacks
        if c.rich and s in cc.COLOUR_RICH_SETS:
            assert cc.colour_rich(c, names, cand, planes), f"{c.id} {s} is not rich"
            for m in (0.0, cc.MARGINS[0]):
                pred = cc.colour_distortion_counts(c, names, cand, m, planes)
                shifted = cc.colour_distortion_counts(c, names, cand, m, planes, shift=1)
                assert shifted[-1] != pred[-1] and not np.array_equal(shifted, pred), f"{c.id} {s}: no sight of thr[s + 1]"
        print(f"{c.id} {s}: units {cc.colour_units(c, names, cand, planes)}, flagged at {cc.PROBE_MARGINS}: "
              f"{[int(cc.colour_distortion_counts(c, names, cand, m, planes)[-1]) for m in cc.PROBE_MARGINS]}")
    if c.rich:
        rate = cc.colour_rate_counts(c, cc.TABLES)
        assert cc.is_rich(rate[:-1]) and cc.colour_rate_counts(c, cc.TABLES, shift=1)[-1] != rate[-1]


def test_sum_partials_is_the_sum_kernels_partition():
    """thread i of 256 sums the values i, i + 256, ...; 8-lane groups are the threads 8 g .. 8 g + 7"""
    v = np.arange(1000, dtype=np.int64) ** 2
    p1 = cc.sum_partials(v, 1)
    assert p1.shape == (256,) and p1[3] == sum(int(v[i]) for i in range(3, 1000, 256))
    p8 = cc.sum_partials(v, 8)
    assert p8.shape == (32,) and p8[2] == p1[16:24].sum() and cc.sum_partials(v, 64).sum() == v.sum()
    assert all(h % 8 == 0 and w % 8 == 0 for w, h in cc.BIG_SUM.values())


# ---- the SSIM probes' predictions (test_gpu_ssim_certificates.py) ------------------------------------------------------

def _colour_plane_bytes(pkg, c, n_tables=32):
    """the decoded planes of one stack with every (table, plane) pair coded"""
    cw, ch = pkg.chroma_size(c.w, c.h) if c.mode == "c420" else (c.w, c.h)
    return n_tables * c.depth * (c.w * c.h + 2 * cw * ch)


def test_ssim_cases_are_the_listed_ones(pkg):
    ids = [c.id for c in cc.SSIM_PROBE_CASES]
    assert len(ids) == len(set(ids)) == 20
    for d in (8, 4):
        want = [f"uniform-{s}-grey-d{d}" for s in ("200x72x4", "24x16x5", "8x8x1", "1366x24x2", "13x11x1", "1x1x1")] + \
               [f"uniform-{s}-rgb-d{d}" for s in ("200x72x2", "24x16x5", "13x11x1", "1x1x1")]
        assert set(want) == {i for i in ids if i.endswith(f"d{d}")}
    assert all(c in cc.PROBE_CASES for c in cc.SSIM_PROBE_CASES)  # the same objects: the emulations' caches are shared
    assert all(s in cc.PROBE_SETS for s in cc.SSIM_PROBE_SETS) and cc.SSIM_PROBE_SETS == ("q1", "four", "eleven")
    assert len(cc.RANGE_NAMES) == 32 and set(cc.RANGE_NAMES) == set(cc.PROBE_TABLES)
    assert all(cc.RANGE_NAMES[i] == cc.PROBE_TABLES[i % 11] for i in range(32))
    # the plane probe's range cases: >= 2 ranges, more than one stack in the first
    ids = [c.id for c in cc.SSIM_RANGE_CASES]
    assert ids == [f"uniform-256x176x{st}-{ch}-d{d}" for d, st in ((8, 3), (4, 6)) for ch in ("grey", "rgb")]
    for c in cc.SSIM_RANGE_CASES:
        assert c.stacks == pkg.DCT3D_SSIM_BLOCK_BUDGET // (c.depth * 64 * 44 * (8 * 32 + 4)) + 1
        r = cc.ssim_ranges(c.depth, c.w, c.h, c.stacks, 32)
        assert len(r) >= 2 and r[0] > 1 and sum(r) == c.stacks and r == [c.stacks - 1, 1]
        assert cc.ssim_ranges(c.depth, c.w, c.h, c.stacks, 8) == [c.stacks]  # 8 tables would not have split it
    # the colour range cases: 3 + 2 without the luma, 2 + 2 + 1 with it; the planes budget alone does not split
    ids = [c.id for c in cc.SSIM_RGB_RANGE_CASES]
    assert ids == [f"{m}-128x{h}x5-d{d}" for d, h in ((8, 88), (4, 176)) for m in ("ycc", "c420")] and len(set(ids)) == 4
    for c in cc.SSIM_RGB_RANGE_CASES:
        pb = _colour_plane_bytes(pkg, c)
        assert pkg.DCT3D_RGB_PLANE_BUDGET // pb >= c.stacks
        assert cc.ssim_ranges(c.depth, c.w, c.h, c.stacks, 32, 3, pb) == [3, 2]
        assert cc.ssim_ranges(c.depth, c.w, c.h, c.stacks, 32, 4, pb) == [2, 2, 1]
        L = cc.coded_tables(32, cc.RANGE_CAND, False)
        assert all(sorted(x) == list(range(32)) for x in L)  # every plane codes all 32, bits or not
    assert [cc.ssim_rgb_units(c, cc.RANGE_NAMES, cc.RANGE_CAND) for c in cc.SSIM_RGB_RANGE_CASES] == \
        [43253760, 22282240, 43253760, 21626880]


@pytest.mark.parametrize("c", [c for c in cc.SSIM_PROBE_CASES if c.rich], ids=repr)
def test_ssim_probe_predictions(c):
    """the plane SSIM probe's rule is the distortion probe's, stated once; n_units is tables x padded samples, per
    band too; and on the rich cases the thresholds read at s + 1 change the prediction of every rich set at margin 0
    and at MARGINS[0]: the counts can see the SSIM arm taking a table row one entry off"""
    fr = c.frames()
    for s in cc.SSIM_PROBE_SETS:
        names = cc.PROBE_SETS[s]
        assert cc.ssim_probe_units(c, names) == len(names) * cc.raster_of(fr, c.depth).size
        for by in (0, c.nby - 1):
            band = cc.band_frames(fr, by)
            assert cc.ssim_probe_units(c, names, band.shape[1]) == len(names) * cc.raster_of(band, c.depth).size
        for m in cc.PROBE_MARGINS:
            assert np.array_equal(cc.ssim_probe_counts(c, names, m), cc.distortion_probe_counts(c, names, m))
        if cc.probe_rich(c, s):
            p0, p1 = (cc.ssim_probe_counts(c, names, m) for m in (0.0, cc.MARGINS[0]))
            assert cc.is_rich(p0[:-1]) and p1[-1] > p0[-1] > 0
            for m, pred in ((0.0, p0), (cc.MARGINS[0], p1)):
                shifted = cc.ssim_probe_counts(c, names, m, shift=1)
                assert shifted[-1] != pred[-1] and not np.array_equal(shifted, pred), f"{c.id} {s}: no sight of thr[s + 1]"


@pytest.mark.parametrize("c", cc.SSIM_RANGE_CASES, ids=repr)
def test_ssim_range_predictions(c):
    """per range case, under each of the 11 names: the emulation is sound (what it leaves closed is the reference's q,
    the DC never open) and decode_emulate's preconditions hold at each of PROBE_MARGINS, no lane flagged at margin 0;
    the 32 cycled tables' prediction is the names' with their multiplicities; it is rich; thresholds read at s + 1
    change it; and no per-stack count repeats, under q1 alone or under the 32: a dropped or doubled range, or a stack
    counted in another's place, cannot cancel"""
    M = cc.MARGINS[0]
    names = cc.RANGE_NAMES
    for n in cc.PROBE_TABLES:
        q, op = cc.case_open(c, n)
        bad = (q != cc.case_q_ref(c, n)) & ~op
        assert not bad.any(), f"{n}: {int(bad.sum())} closed coefficients differ"
        assert not op[:, 0, 0, 0].any()
        lanes = cc.probe_decode_lanes(c, n, cc.PROBE_MARGINS)  # (asserts the preconditions)
        assert not lanes[0].any(), f"{c.id} {n}: a lane flagged at margin 0: another seed"
    mult = {n: names.count(n) for n in cc.PROBE_TABLES}
    assert sorted(mult.values()) == [2] + [3] * 10
    p0, p1 = cc.ssim_probe_counts(c, names, 0.0), cc.ssim_probe_counts(c, names, M)
    assert np.array_equal(p0, cc.rate_probe_counts(c, names))  # the decode term at margin 0 is 0
    assert np.array_equal(p1, sum(k * cc.ssim_probe_counts(c, (n,), M) for n, k in mult.items()))
    assert cc.is_rich(p0[:-1]) and p1[-1] > p0[-1] >= 17444 and (p1[-1] - p0[-1]) // 32 >= 10471
    for m, pred in ((0.0, p0), (M, p1)):
        assert cc.ssim_probe_counts(c, names, m, shift=1)[-1] != pred[-1], f"{c.id}: no sight of thr[s + 1]"
    per = cc.ssim_range_stack_counts(c, names, M)
    q1 = cc.ssim_range_stack_counts(c, ("q1",), M)
    assert per.sum() == p1[-1] and len(set(per.tolist())) == c.stacks == len(set(q1.tolist()))
    # no proper subset of the stacks, counted once or twice, gives the whole's count by accident: checked for ranges
    r = cc.ssim_ranges(c.depth, c.w, c.h, c.stacks, 32)
    parts = [int(per[sum(r[:i]):sum(r[:i + 1])].sum()) for i in range(len(r))]
    assert len(set(parts)) == len(parts) and all(0 < v < p1[-1] for v in parts)
    assert cc.ssim_probe_units(c, names) == 32 * cc.raster_of(c.frames(), c.depth).size
    print(f"{c.id}: open {int(p0[-1])}, at {M}: {int(p1[-1])}, per stack {per.tolist()}, per range {parts}")


@pytest.mark.parametrize("c", cc.SSIM_RGB_RANGE_CASES, ids=repr)
def test_ssim_rgb_range_predictions(c, pkg):
    """the same per colour range case and plane; the prediction does not depend on the bits (every plane codes all 32
    either way)"""
    M = cc.MARGINS[0]
    names, cand = cc.RANGE_NAMES, cc.RANGE_CAND
    for k in range(3):
        for n in cc.PROBE_TABLES:
            q, op = cc.colour_plane_open(c, k, n)
            bad = (q != cc.colour_plane_q_ref(c, k, n)) & ~op
            assert not bad.any(), f"plane {k} {n}: {int(bad.sum())} closed coefficients differ"
            assert not op[:, 0, 0, 0].any()
            cc.colour_plane_lanes(c, k, n)  # (asserts the preconditions at each of PROBE_MARGINS)
    assert cc.colour_rich(c, names, cand)
    p0, p1 = cc.ssim_rgb_counts(c, names, cand, 0.0), cc.ssim_rgb_counts(c, names, cand, M)
    assert p1[-1] > p0[-1] > 0
    for wb in (False, True):
        assert np.array_equal(cc.ssim_rgb_counts(c, names, cand, M, wb), cc.colour_distortion_counts(c, names, cand, M, wb))
        assert np.array_equal(cc.ssim_rgb_counts(c, names, cand, M, wb), p1)
        assert cc.ssim_rgb_units(c, names, cand, wb) == cc.colour_units(c, names, cand, wb) == cc.colour_units(c, names, cand)
    for m, pred in ((0.0, p0), (M, p1)):
        assert cc.ssim_rgb_counts(c, names, cand, m, shift=1)[-1] != pred[-1], f"{c.id}: no sight of thr[s + 1]"
    per = cc.colour_range_stack_counts(c, names, cand, M)
    assert per.sum() == p1[-1] and len(set(per.tolist())) == c.stacks
    for r in ([3, 2], [2, 2, 1]):
        parts = [int(per[sum(r[:i]):sum(r[:i + 1])].sum()) for i in range(len(r))]
        assert len(set(parts)) == len(parts) and all(0 < v < p1[-1] for v in parts)
    print(f"{c.id}: units {cc.ssim_rgb_units(c, names, cand)}, open {int(p0[-1])}, at {M}: {int(p1[-1])}, per stack {per.tolist()}")


def _first_uses(seq):
    """brute force: the distinct values of a sequence in the order of their first appearance"""
    return [v for i, v in enumerate(seq) if v not in seq[:i]]


def test_ssim_rgb_planes_tables():
    """rgb_planes_dev's compaction rule against a brute-force restatement, on the colour sets; and what it predicts in
    planes mode: the plane probe under the coded tables only, every coded table on all three planes"""
    for s in ("subsets", "repeat", "eleven", "q1", "planes4"):
        names, cand, _ = cc.COLOUR_SETS[s]
        n = len(names)
        flat = None if cand is None else [int(t) for cd in cand for t in cd]
        want = list(range(n)) if flat is None else _first_uses(flat)
        assert cc.ssim_rgb_planes_tables(n, cand, False) == want, s
        assert cc.ssim_rgb_planes_tables(n, cand, True) == list(range(n)) == cc.ssim_rgb_planes_tables(n, None, False), s
    names, cand, _ = cc.COLOUR_SETS["subsets"]
    assert cc.ssim_rgb_planes_tables(4, cand, False) == [0, 1, 2]  # table 3 is not coded
    assert cc.ssim_rgb_planes_tables(3, cc.COLOUR_SETS["repeat"][1], False) == [0, 1, 2]
    assert cc.ssim_rgb_planes_tables(3, ((2, 2, 0), (0, 1, 2)), False) == [2, 0, 1]  # the order of first use
    assert cc.ssim_rgb_planes_tables(11, None, False) == list(range(11))
    for c in (x for x in cc.COLOUR_PROBE_CASES if x.mode == "planes"):
        raster = cc.raster_of(c.frames(), c.depth).size
        for m in cc.PROBE_MARGINS:
            assert np.array_equal(cc.ssim_rgb_counts(c, names, cand, m), cc.distortion_probe_counts(c.rgb, names[:3], m))
            assert np.array_equal(cc.ssim_rgb_counts(c, names, cand, m, True), cc.distortion_probe_counts(c.rgb, names, m))
            # (the RGB distortion probe's planes arm codes every table whatever the candidates say: both rules stay)
            assert np.array_equal(cc.colour_distortion_counts(c, names, cand, m), cc.distortion_probe_counts(c.rgb, names, m))
        assert cc.ssim_rgb_units(c, names, cand) == 3 * raster and cc.ssim_rgb_units(c, names, cand, True) == 4 * raster
        assert cc.ssim_rgb_units(c, names, cand, rows=3) == 3 * cc.raster_of(c.frames()[:, :3], c.depth).size
        if (c.w, c.h) == (200, 72):  # the fourth table's count is what a call that does not compact adds
            assert cc.ssim_rgb_counts(c, names, cand, 0.0, True)[-1] > cc.ssim_rgb_counts(c, names, cand, 0.0)[-1] > 0
