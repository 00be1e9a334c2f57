"""GPU: the SSIM probes flag exactly what the host emulations flag.

dct3d_ssim_frames[_dev] runs distortion_kernel's SSIM = 1 instantiations -- code objects of their own, with
the block-moment arm between the certificate and the stores -- from ssim_dev, the only plane probe that walks the
stacks in ranges: range x channel x batch of 8 tables, window and sum launches between the counting ones, all into one
counter slot.  dct3d_ssim_rgb_frames[_dev] (4u) reuses rgb_ycc_dev with a second budget that shortens the ranges and,
in planes mode, compacts the tables before ssim_dev.  None of that changes an output on ordinary content when it is
slightly off: a threshold row read one entry on, a decode constant handed over wrongly, a range whose launches clear
the slot, a wrong L[k], the compaction coding the wrong tables -- the exact fold or the replay repairs it, and only the
counts dct3d_get_stats reports see it.  As test_gpu_probe_certificates.py and test_gpu_distortion_rgb_certificates.py
do for the distortion probes, this module asserts exact equality of n_units and n_flagged with cert_common.py's
predictions (checked on the CPU by test_cert_common.py), after the call's own outputs -- every window through a guarded
d_window_ssim, the sums, ssim_y, sse and bits where asked -- have been compared with the independent reference:

  plane probe   n_flagged = the distortion probe's (cert_common.ssim_probe_counts): per table the open coefficients
                + 32 x the lanes the decode tile replays; n_units = tables x padded samples.  Reference:
                quant_common.ref_decode_frames of cert_common.case_q_ref, fed to test_gpu_ssim.windows_of
  ycc, c420     cert_common.colour_distortion_counts / colour_units with every pair coded when the bits are asked for;
                neither the luma nor want_sse changes L[k].  Reference: test_gpu_ssim_rgb.ref_case / ref_planes
  planes        the plane probe under the tables some candidate names (cert_common.ssim_rgb_planes_tables), all of
                them when the bits are asked for: every coded table on all three planes

for the whole raster and for every band (one block row; 16 frame rows in c420 mode), and, whole raster only, for calls
whose stacks go in two or three ranges."""
import functools

import numpy as np
import pytest

import cert_common as cc
import quant_common as qc
import test_gpu_distortion_rgb as rgb
import test_gpu_ssim_rgb as srgb
from cert_common import (COLOUR_PROBE_CASES, COLOUR_SETS, MARGINS, PROBE_SETS, RANGE_CAND, RANGE_NAMES, SSIM_PROBE_CASES,
                         SSIM_PROBE_SETS, SSIM_RANGE_CASES, SSIM_RGB_RANGE_CASES)
from conftest import ctx_option
from test_gpu_distortion import cube_sums
from test_gpu_distortion_rgb_certificates import _content, _crops
from test_gpu_distortion_rgb_certificates import _equal_counts as _equal_colour_counts
from test_gpu_probe_certificates import _band, _cube_bits, _equal_counts, _tables
from test_gpu_ssim import windows_of

pytestmark = pytest.mark.gpu

# the plane probe: (DCT3D_OPT_DEC_MARGIN, want_sse, want_bits)
VARIANTS = ((0.0, False, False), (MARGINS[0], True, True), (MARGINS[1], False, False))
RGB_SETS = ("q1", "subsets", "eleven", "repeat")


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


# ---- the plane probe --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(c, name):
    """per (case, table), computed once and never modified: the reference's decoded frames, and the squared error and
    the bits of every cube [stack, channel, cube]"""
    T = cc.steps_of(cc.table(name, c.depth), c.depth)
    fr = c.frames()
    q = cc.case_q_ref(c, name)
    out = qc.ref_decode_frames(q, c.w, c.h, c.stacks, c.channels, T, c.depth)
    sse = cube_sums((fr.astype(np.int64) - out.astype(np.int64)) ** 2, c.depth)
    bits = _cube_bits(q).reshape(sse.shape)
    for a in (out, sse, bits):
        a.setflags(write=False)
    return out, sse, bits


@functools.lru_cache(maxsize=None)
def _windows(c, name, by):
    """the reference's windows of block row by (None: the whole raster) [stack, channel, D, nwy, nwx]: a band's cubes
    are the whole raster's, so its decoded frames are the rows of the whole raster's"""
    fr, out = c.frames(), _reference(c, name)[0]
    if by is not None:
        fr, out = cc.band_frames(fr, by), cc.band_frames(out, by)
    v = windows_of(fr, out, c.depth)
    v.setflags(write=False)
    return v


def _plane_ref(c, names, by):
    """(windows [T, stack, channel, D, nwy, nwx], sse [T, stack, channel], bits [T, stack, channel]) of a crop"""
    refs = {n: _reference(c, n) for n in set(names)}
    wins = {n: _windows(c, n, by) for n in set(names)}
    return (np.stack([wins[n] for n in names]),
            np.stack([_band(c, refs[n][1], by).sum(axis=-1) for n in names]),
            np.stack([_band(c, refs[n][2], by).sum(axis=-1) for n in names]))


def _plane_call(ctx, pkg, c, by, names, margin, want_sse, want_bits, ref):
    """one ssim_frames_dev call on a crop, its outputs compared with the reference before its statistics are read:
    (n_units, n_flagged)"""
    import torch
    fr = c.frames() if by is None else cc.band_frames(c.frames(), by)
    h = fr.shape[1]
    nwx, nwy = pkg.ssim_windows(c.w, h)
    shape = (len(names), c.stacks, c.channels, c.depth, nwy, nwx)
    n = int(np.prod(shape)) * 4
    where = f"{c.id} band {by} margin {margin} sse {want_sse} bits {want_bits}"
    d_fr = torch.from_numpy(np.array(fr)).cuda()
    buf, mid = qc.banded(torch, n, 0xA5)
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, margin):
        res = ctx.ssim_frames_dev(d_fr, c.w, h, c.channels, c.stacks, _tables(c, names), mid, want_sse=want_sse, want_bits=want_bits)
    res = res if isinstance(res, tuple) else (res,)
    got, intact = qc.bands_intact(buf, n, 0xA5)
    assert intact, f"{where}: a write outside d_window_ssim"
    wins = got.view(np.int32).reshape(shape)
    assert wins.shape == ref[0].shape
    assert np.array_equal(wins.astype(np.int64), ref[0]), f"{where}: {(wins != ref[0]).sum()} windows differ from the reference"
    assert np.array_equal(res[0], ref[0].sum(axis=(-3, -2, -1))), f"{where}: the per-stack sums"
    if want_sse:
        assert np.array_equal(res[1].astype(np.int64), ref[1]), f"{where}: the squared error"
    if want_bits:
        assert np.array_equal(res[-1].astype(np.int64), ref[2]), f"{where}: the bits"
    st = ctx.stats()
    return int(st["n_units"]), int(st["n_flagged"])


@pytest.mark.parametrize("c, tset", [(c, s) for c in SSIM_PROBE_CASES for s in SSIM_PROBE_SETS],
                         ids=lambda v: v if isinstance(v, str) else v.id)
def test_ssim_probe_counts(pkg, gpu_ctx8, gpu_ctx4, c, tset):
    """a: ssim_frames_dev on every band of one block row and on the whole raster -- margin 0 plain, MARGINS[0] with
    want_sse and want_bits, MARGINS[1] plain: n_units and n_flagged are the predictions.  At margin 0 the count is the
    rate prediction (the open coefficients alone); on the rich sets both terms count."""
    ctx = _ctx(c.depth, gpu_ctx8, gpu_ctx4)
    names = PROBE_SETS[tset]
    crops = list(range(c.nby)) + [None]
    got = {v: [] for v in VARIANTS}
    for by in crops:
        ref = _plane_ref(c, names, by)
        for v in VARIANTS:
            got[v].append(_plane_call(ctx, pkg, c, by, names, v[0], v[1], v[2], ref))
    rows = [min(8, c.h - 8 * by) for by in range(c.nby)] + [c.h]
    for v in VARIANTS:
        what = f"{tset} margin {v[0]} sse {v[1]} bits {v[2]}"
        _equal_counts(c, names, what + " n_units", np.array([cc.ssim_probe_units(c, names, r) for r in rows]),
                      np.array([u for u, _ in got[v]]))
        _equal_counts(c, names, what + " n_flagged", cc.ssim_probe_counts(c, names, v[0]), np.array([f for _, f in got[v]]))
    opens = cc.rate_probe_counts(c, names)
    assert np.array_equal(cc.ssim_probe_counts(c, names, 0.0), opens)  # margin 0: the encode term alone
    _equal_counts(c, names, f"{tset} margin 0 against the rate prediction", opens, np.array([f for _, f in got[VARIANTS[0]]]))
    if cc.probe_rich(c, tset):
        assert cc.is_rich(opens[:-1]), f"{c.id} {tset} is not rich"
        assert cc.ssim_probe_counts(c, names, MARGINS[0])[-1] > opens[-1] > 0  # both terms count


@pytest.mark.parametrize("c", SSIM_RANGE_CASES, ids=repr)
def test_ssim_probe_counts_across_ranges(pkg, gpu_ctx8, gpu_ctx4, c):
    """b: 32 tables at 256 x 176 and one stack more than the block budget holds, at MARGINS[0]: two ranges x channels x
    four batches of tables count into one slot, with the window and sum launches between them.  The call's n_units and
    n_flagged are the prediction and distortion_frames_dev's on the same arguments."""
    import torch
    ctx = _ctx(c.depth, gpu_ctx8, gpu_ctx4)
    names, M = RANGE_NAMES, MARGINS[0]
    assert len(cc.ssim_ranges(c.depth, c.w, c.h, c.stacks, len(names))) >= 2
    ref = _plane_ref(c, names, None)
    units, flagged = _plane_call(ctx, pkg, c, None, names, M, True, True, ref)
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, M):
        sse = ctx.distortion_frames_dev(torch.from_numpy(np.array(c.frames())).cuda(), c.w, c.h, c.channels, c.stacks, _tables(c, names))
    assert np.array_equal(sse.astype(np.int64), ref[1])
    st = ctx.stats()
    pred = (cc.ssim_probe_units(c, names), int(cc.ssim_probe_counts(c, names, M)[-1]))
    per = cc.ssim_range_stack_counts(c, names, M)
    print(f"{c.id} 32 tables margin {M}: predicted {pred}, ssim {(units, flagged)}, distortion {(st['n_units'], st['n_flagged'])}")
    assert (units, flagged) == pred, f"{c.id} 32 tables margin {M}: predicted {pred}, device {(units, flagged)}; predicted per stack " \
                                      f"{per.tolist()}, stacks per range {cc.ssim_ranges(c.depth, c.w, c.h, c.stacks, len(names))}"
    assert (int(st["n_units"]), int(st["n_flagged"])) == pred, f"{c.id}: distortion_frames_dev counts otherwise"
    assert pred[1] > int(cc.rate_probe_counts(c, names)[-1]) > 0


# ---- the RGB and luma probe -------------------------------------------------------------------------------------------

def _rgb_variants(mode):
    """(DCT3D_OPT_DEC_MARGIN, want_luma, want_sse, want_bits); no luma in planes mode"""
    luma = mode != "planes"
    return ((0.0, False, False, False), (MARGINS[0], luma, False, True), (MARGINS[1], luma, True, False))


def _rgb_call(ctx, pkg, c, y0, rows, names, cand, variant, ref, content=None):
    """one ssim_rgb_frames_dev call on a crop, its outputs compared with the reference before its statistics are
    read: (n_units, n_flagged).  ref: test_gpu_ssim_rgb.ref_case's pair"""
    margin, luma, want_sse, want_bits = variant
    content = _content(c, y0) if content is None else content
    where = f"{c.id} rows {y0}..{y0 + rows} margin {margin} luma {luma} sse {want_sse} bits {want_bits}"
    cl = [(i, i, i) for i in range(len(names))] if cand is None else cand
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, margin):
        res, wins = srgb.probe_dev(ctx, content, c.depth, c.w, rows, c.stacks, names, cand, luma, want_sse=want_sse, want_bits=want_bits)
    res = list(res) if isinstance(res, tuple) else [res]
    assert wins.shape == ref[0].shape
    assert np.array_equal(wins.astype(np.int64), ref[0]), f"{where}: {(wins != ref[0]).sum()} windows differ from the reference"
    assert np.array_equal(res.pop(0), ref[0].sum(axis=(-3, -2, -1)).transpose(0, 2, 1)), f"{where}: the per-stack sums"
    if luma:
        assert np.array_equal(res.pop(0), ref[1].sum(axis=(-3, -2, -1))), f"{where}: the luma sums"
    if want_sse:
        sse = rgb.ref_rgb(content, c.depth, c.w, rows, c.stacks, c.mode, names, cl).sum(axis=-1)
        assert np.array_equal(res.pop(0).astype(np.int64), sse), f"{where}: the squared error"
    if want_bits:
        bits = rgb.ref_planes(content, c.depth, c.w, rows, c.stacks, c.mode, names, 2)
        assert np.array_equal(res.pop(0).astype(np.int64), bits), f"{where}: the bits"
    assert not res
    st = ctx.stats()
    return int(st["n_units"]), int(st["n_flagged"])


@pytest.mark.parametrize("c, tset", [(c, s) for c in COLOUR_PROBE_CASES for s in RGB_SETS],
                         ids=lambda v: v if isinstance(v, str) else v.id)
def test_ssim_rgb_probe_counts(pkg, gpu_ctx8, gpu_ctx4, c, tset):
    """c: ssim_rgb_frames_dev on every band and on the whole raster -- margin 0 plain, MARGINS[0] with the bits,
    MARGINS[1] with want_sse, the latter two with the luma outside planes mode: n_units and n_flagged are the
    predictions.  In planes mode the compaction rule is the prediction: the subset candidates code three tables
    without the bits and four with them."""
    ctx = _ctx(c.depth, gpu_ctx8, gpu_ctx4)
    names, cand, _ = COLOUR_SETS[tset]
    cl = [(i, i, i) for i in range(len(names))] if cand is None else cand
    crops, variants = _crops(c), _rgb_variants(c.mode)
    got = {v: [] for v in variants}
    with rgb.mode_on(ctx, pkg, c.mode):
        for y0, rows in crops:
            ref = srgb.ref_case(_content(c, y0), c.depth, c.w, rows, c.stacks, c.mode, names, cl)
            for v in variants:
                got[v].append(_rgb_call(ctx, pkg, c, y0, rows, names, cand, v, ref))
    for v in variants:
        what = f"{tset} margin {v[0]} luma {v[1]} sse {v[2]} bits {v[3]}"
        _equal_colour_counts(c, what + " n_units", [cc.ssim_rgb_units(c, names, cand, v[3], rows) for _, rows in crops],
                             [u for u, _ in got[v]])
        _equal_colour_counts(c, what + " n_flagged", cc.ssim_rgb_counts(c, names, cand, v[0], v[3]), [f for _, f in got[v]])
    if c.mode == "planes" and tset == "subsets":
        raster = cc.raster_of(c.frames(), c.depth).size
        assert [got[v][-1][0] for v in variants] == [3 * raster, 4 * raster, 3 * raster]
    if c.rich and tset in cc.COLOUR_RICH_SETS:
        assert cc.colour_rich(c, names, cand)
        p0, p1 = (cc.ssim_rgb_counts(c, names, cand, m)[-1] for m in (0.0, MARGINS[0]))
        assert p1 > p0 > 0  # both terms count


@pytest.mark.parametrize("c", SSIM_RGB_RANGE_CASES, ids=repr)
def test_ssim_rgb_probe_counts_across_ranges(pkg, gpu_ctx8, gpu_ctx4, c):
    """d: test_gpu_ssim_rgb.py::test_stack_ranges' shapes under 32 candidates over 32 tables at MARGINS[0]: the stacks
    go in ranges of 3 + 2 without the luma and 2 + 2 + 1 with it, every range's launches into one slot.  n_units and
    n_flagged are equal in both, the prediction, and distortion_rgb_frames_dev's with the same candidates."""
    import torch
    ctx = _ctx(c.depth, gpu_ctx8, gpu_ctx4)
    names, cand, M = RANGE_NAMES, list(RANGE_CAND), MARGINS[0]
    content = _content(c, 0)
    assert np.array_equal(rgb.frames_of(content, c.depth, c.w, c.h, c.stacks), c.frames())
    ref = srgb.ref_case(content, c.depth, c.w, c.h, c.stacks, c.mode, names, cand)
    with rgb.mode_on(ctx, pkg, c.mode):
        plain = _rgb_call(ctx, pkg, c, 0, c.h, names, cand, (M, False, False, False), ref)
        luma = _rgb_call(ctx, pkg, c, 0, c.h, names, cand, (M, True, False, False), ref)
        with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, M):
            sse = ctx.distortion_rgb_frames_dev(torch.from_numpy(np.array(c.frames())).cuda(), c.w, c.h, c.stacks,
                                                [rgb._table(c.depth, n) for n in names], cand)
        assert np.array_equal(sse.astype(np.int64), rgb.ref_rgb(content, c.depth, c.w, c.h, c.stacks, c.mode, names, cand).sum(axis=-1))
        st = ctx.stats()
    pred = (cc.ssim_rgb_units(c, names, cand), int(cc.ssim_rgb_counts(c, names, cand, M)[-1]))
    per = cc.colour_range_stack_counts(c, names, cand, M)
    print(f"{c.id} 32 candidates margin {M}: predicted {pred}, plain {plain}, with the luma {luma}, "
          f"distortion {(st['n_units'], st['n_flagged'])}")
    for what, got in (("ranges 3 + 2", plain), ("with the luma, ranges 2 + 2 + 1", luma),
                      ("distortion_rgb_frames_dev", (int(st["n_units"]), int(st["n_flagged"])))):
        assert got == pred, f"{c.id} 32 candidates margin {M} {what}: predicted {pred}, device {got}; predicted per stack {per.tolist()}"
    assert pred[1] > int(cc.ssim_rgb_counts(c, names, cand, 0.0)[-1]) > 0
