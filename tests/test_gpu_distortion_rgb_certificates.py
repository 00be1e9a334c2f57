"""GPU: the RGB-domain distortion probe flags exactly what the host emulations flag.

distortion_plane_kernel (dct3d_distortion_rgb.hip) certifies in a copy of distortion_kernel's loop: a forward
transform, a reload source, a table loop and a fold count of its own, a replay geometry chosen by the chroma mode and
decode constants handed over field by field; around it probe_rgb_ycc_dev decides on the host which (table, plane)
pairs are coded, offsets the probe table rows per plane and walks the stacks in ranges.  None of that changes an
output on ordinary content when it is slightly off: only the counts dct3d_get_stats reports see it.  As
test_gpu_probe_certificates.py does for the plane probes, this module asserts exact equality of n_units and n_flagged
with cert_common.py's predictions (checked on the CPU by test_cert_common.py), after the call's own outputs --
d_cube_sse between intact guard bands, sse, and plane_sse and bits where asked -- have been compared with
test_gpu_distortion_rgb.py's independent reference:

  ycc, c420   n_flagged = sum over the planes k and the tables of L[k] of (the open coefficients + 32 x the lanes the
              decode tile replays), each plane of the colour transform emulated as a grey clip; L[k] the distinct
              tables some candidate names for plane k, every table when the planes' errors or the bits are asked for
              or no candidates are given.  n_units = sum over k of |L[k]| x the plane's padded cubes x 64 depth x stacks
  planes      the plane probe under every table, whatever the candidates say (cert_common.distortion_probe_counts)

for the whole raster and for every band: one block row, in c420 mode 16 frame rows (two Y block rows over one chroma
block row), the last band of a ragged height shorter.  Margins: 0, MARGINS[0] and MARGINS[1], the latter two with and
without the bits (asking for them moves no count, except that it codes every pair).  At margin 0 the decode term is 0
under ref, q1, q12 and seeded (asserted on the CPU); under quant_table(64) at 8x8x4 the flat chroma planes flag lanes
at margin 0 too, and the prediction carries them."""
import numpy as np
import pytest

import cert_common as cc
import quant_common as qc
import test_gpu_distortion_rgb as rgb
from cert_common import COLOUR_PROBE_CASES, COLOUR_SETS, MARGINS
from conftest import ctx_option
from test_gpu_distortion import _table

pytestmark = pytest.mark.gpu

# (DCT3D_OPT_DEC_MARGIN, ask for the bits)
VARIANTS = ((0.0, False), (MARGINS[0], False), (MARGINS[0], True), (MARGINS[1], False), (MARGINS[1], True))


def _crops(c):
    """(first row, rows) of every band and, last, of the whole raster"""
    return [(y0, min(c.band, c.h - y0)) for y0 in range(0, c.h, c.band)] + [(0, c.h)]


def _content(c, y0):
    return f"cert{c.h}@{y0}"


def _equal_counts(c, what, pred, got):
    """pred, got: per-band counts, the whole raster's last; a failure names the first band that differs"""
    pred, got = np.asarray(pred, np.int64), np.asarray(got, np.int64)
    print(f"{c.id} {what}: predicted {int(pred[-1])}, device {int(got[-1])}")
    if not np.array_equal(pred[:-1], got[:-1]):
        b = int(np.nonzero(pred[:-1] != got[:-1])[0][0])
        pytest.fail(f"{c.id} {what}: band {b} (frame rows {b * c.band} ..): predicted {int(pred[b])}, device {int(got[b])}"
                    f"\npredicted per band {pred[:-1].tolist()}\ndevice per band {got[:-1].tolist()}")
    assert pred[-1] == got[-1], f"{c.id} {what}: the bands agree, the whole raster does not"


def _call(ctx, pkg, c, y0, rows, names, cand, planes, margin, want_bits, ref):
    """one device call on a crop, its outputs compared with the reference before its statistics are read"""
    content = _content(c, y0)
    where = f"{c.id} rows {y0}..{y0 + rows} margin {margin} bits {want_bits}"
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, margin):
        sse, psse, bits, cubes = rgb.probe_dev(ctx, content, c.depth, c.w, rows, c.stacks, names, cand, planes, want_bits)
        st = ctx.stats()
    assert np.array_equal(cubes.astype(np.int64), ref), f"{where}: {(cubes != ref).sum()} cubes differ from the reference"
    assert np.array_equal(sse.astype(np.int64), ref.sum(axis=-1)), f"{where}: the per-stack sums"
    if planes:
        assert np.array_equal(psse.astype(np.int64), rgb.ref_planes(content, c.depth, c.w, rows, c.stacks, c.mode, names, 1)), \
            f"{where}: the planes' errors"
    if want_bits:
        assert np.array_equal(bits.astype(np.int64), rgb.ref_planes(content, c.depth, c.w, rows, c.stacks, c.mode, names, 2)), \
            f"{where}: the bits"
    return int(st["n_units"]), int(st["n_flagged"])


def _ctx(depth, gpu_ctx8, gpu_ctx4):
    return gpu_ctx8 if depth == 8 else gpu_ctx4


@pytest.mark.parametrize("c, tset", [(c, s) for c in COLOUR_PROBE_CASES for s in COLOUR_SETS],
                         ids=lambda v: v if isinstance(v, str) else v.id)
def test_colour_probe_counts(pkg, gpu_ctx8, gpu_ctx4, c, tset):
    """distortion_rgb_frames_dev on every band and on the whole raster, at every margin with and without the bits:
    n_units and n_flagged are the predictions"""
    ctx = _ctx(c.depth, gpu_ctx8, gpu_ctx4)
    names, cand, planes = COLOUR_SETS[tset]
    cl = [(i, i, i) for i in range(len(names))] if cand is None else cand
    crops = _crops(c)
    got = {v: [] for v in VARIANTS}
    with rgb.mode_on(ctx, pkg, c.mode):
        for y0, rows in crops:
            ref = rgb.ref_rgb(_content(c, y0), c.depth, c.w, rows, c.stacks, c.mode, names, cl)
            for m, wb in VARIANTS:
                got[(m, wb)].append(_call(ctx, pkg, c, y0, rows, names, cand, planes, m, wb, ref))
    for m, wb in VARIANTS:
        all_pairs = planes or wb
        what = f"{tset} margin {m} bits {wb}"
        units = [cc.colour_units(c, names, cand, all_pairs, rows) for _, rows in crops]
        _equal_counts(c, what + " n_units", units, [u for u, _ in got[(m, wb)]])
        _equal_counts(c, what + " n_flagged", cc.colour_distortion_counts(c, names, cand, m, all_pairs),
                      [f for _, f in got[(m, wb)]])
    if c.rich and tset in cc.COLOUR_RICH_SETS:
        assert cc.colour_rich(c, names, cand, planes)
        p0, p1 = (cc.colour_distortion_counts(c, names, cand, m, planes)[-1] for m in (0.0, MARGINS[0]))
        assert p1 > p0 > 0  # both terms count


@pytest.mark.parametrize("mode", ["ycc", "c420"])
@pytest.mark.parametrize("depth", [8, 4])
def test_host_call_counts_as_the_device_call(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """distortion_rgb_frames (frames in host memory, chunks of whole stacks under one batch) on 200 x 72 x 2 reports the
    device call's n_units and n_flagged -- the predictions -- under the subset candidates, without and with the planes'
    errors and the bits.  At MARGINS[0], so that both terms count."""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    c = next(x for x in COLOUR_PROBE_CASES if (x.mode, x.depth, x.w, x.h) == (mode, depth, 200, 72))
    fr = rgb.frames_of(_content(c, 0), depth, c.w, c.h, c.stacks)
    assert np.array_equal(fr, c.frames())
    for tset, want in (("subsets", False), ("planes4", True)):
        names, cand, planes = COLOUR_SETS[tset]
        tabs = [_table(depth, n) for n in names]
        ref = rgb.ref_rgb(_content(c, 0), depth, c.w, c.h, c.stacks, mode, names, cand)
        with rgb.mode_on(ctx, pkg, mode):
            dev = _call(ctx, pkg, c, 0, c.h, names, cand, planes, MARGINS[0], want, ref)
            with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, MARGINS[0]):
                res = ctx.distortion_rgb_frames(fr, tabs, cand, want_planes=planes, want_bits=want)
                st = ctx.stats()
        sse = res[0] if want else res
        assert np.array_equal(sse.astype(np.int64), ref.sum(axis=-1))
        if want:
            for what in (1, 2):
                assert np.array_equal(res[what].astype(np.int64), rgb.ref_planes(_content(c, 0), depth, c.w, c.h, c.stacks, mode, names, what))
        pred = (cc.colour_units(c, names, cand, want), int(cc.colour_distortion_counts(c, names, cand, MARGINS[0], want)[-1]))
        print(f"{c.id} {tset}: predicted {pred}, device {dev}, host {(st['n_units'], st['n_flagged'])}")
        assert (int(st["n_units"]), int(st["n_flagged"])) == dev == pred


@pytest.mark.parametrize("mode", ["ycc", "c420"])
@pytest.mark.parametrize("depth", [8, 4])
def test_two_ranges_count_as_their_stacks(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """test_gpu_distortion_rgb.py::test_stack_ranges' call (32 tables, every pair coded, 256 x 176, one stack more than
    the plane budget holds: two ranges of stacks into one counter slot): its n_units and n_flagged are the sums over
    the same call made per stack, as its outputs are the stacks'; and stack 0 under q1 alone is held to the emulation.
    At MARGINS[0], so that both terms count."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = 256, 176
    cw, ch = pkg.chroma_size(w, h) if mode == "c420" else (w, h)
    tabs = [pkg.quant_table(q, depth) for q in range(1, 33)]
    per_stack = len(tabs) * depth * (w * h + 2 * cw * ch)
    stacks = pkg.DCT3D_RGB_PLANE_BUDGET // per_stack + 1
    assert 2 <= stacks <= 8
    cand = [(i, (i + 5) % 32, (i + 11) % 32) for i in range(32)]
    content = f"cert{h}@0"
    fr = rgb.frames_of(content, depth, w, h, stacks)
    one = cc.ColourCase(mode, depth, w, h, 1)
    assert np.array_equal(fr[:depth], one.frames())  # stack 0 is the one-stack content
    C = (w // 8) * (h // 8)
    with rgb.mode_on(ctx, pkg, mode), ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, MARGINS[0]):
        d_fr = torch.from_numpy(np.array(fr)).cuda()
        buf, mid = qc.banded(torch, 32 * stacks * C * 4, 0xA5)
        sse, planes, bits = ctx.distortion_rgb_frames_dev(d_fr, w, h, stacks, tabs, cand, mid, want_planes=True, want_bits=True)
        whole = ctx.stats()
        got, intact = qc.bands_intact(buf, 32 * stacks * C * 4, 0xA5)
        assert intact, "a write outside d_cube_sse"
        cubes = got.view(np.uint32).reshape(32, stacks, C)
        assert np.array_equal(sse.astype(np.int64), cubes.astype(np.int64).sum(axis=-1))
        units = flagged = 0
        d_one = torch.zeros(32 * C, dtype=torch.int32, device="cuda")
        for s in range(stacks):
            a, b, e = ctx.distortion_rgb_frames_dev(d_fr[s * depth:(s + 1) * depth], w, h, 1, tabs, cand, d_one,
                                                    want_planes=True, want_bits=True)
            st = ctx.stats()
            assert np.array_equal(a[:, 0], sse[:, s]) and np.array_equal(b[:, 0], planes[:, s]) and np.array_equal(e[:, 0], bits[:, s])
            assert np.array_equal(d_one.cpu().numpy().view(np.uint32).reshape(32, C), cubes[:, s]), f"stack {s}"
            units += int(st["n_units"])
            flagged += int(st["n_flagged"])
        print(f"{mode} d{depth} {stacks} stacks: whole {whole['n_units']}, {whole['n_flagged']}; per stack {units}, {flagged}")
        assert int(whole["n_units"]) == units == 32 * (C + 2 * ((cw + 7) // 8) * ((ch + 7) // 8)) * 64 * depth * stacks
        assert int(whole["n_flagged"]) == flagged > 0
    # stack 0 under q1 alone: the emulation's count
    names, cd, _ = COLOUR_SETS["q1"]
    ref = rgb.ref_rgb(content, depth, w, h, 1, mode, names, cd)
    with rgb.mode_on(ctx, pkg, mode):
        got1 = _call(ctx, pkg, one, 0, h, names, cd, False, MARGINS[0], False, ref)
    pred = (cc.colour_units(one, names, cd), int(cc.colour_distortion_counts(one, names, cd, MARGINS[0])[-1]))
    print(f"{one.id} q1: predicted {pred}, device {got1}")
    assert got1 == pred and pred[1] > 0


@pytest.mark.parametrize("c", [x for x in COLOUR_PROBE_CASES if x.mode != "planes" and (x.w, x.h) in ((200, 72), (208, 80))], ids=repr)
def test_colour_rate_probe_counts(pkg, gpu_ctx8, gpu_ctx4, c):
    """rate_frames_dev under the colour option (ycc: rate_kernel's colour axis; c420: probe_c420_dev) counts the rate
    probe's rule on the same planes: the sum over the three planes and every table of the open coefficients, per band
    and for the whole raster; its bits are the reference's (the ones the distortion probe's bits were held to)"""
    import torch
    ctx = _ctx(c.depth, gpu_ctx8, gpu_ctx4)
    names = cc.TABLES
    tabs = [_table(c.depth, n) for n in names]
    got = []
    with rgb.mode_on(ctx, pkg, c.mode):
        for y0, rows in _crops(c):
            content = _content(c, y0)
            d_fr = torch.from_numpy(np.array(rgb.frames_of(content, c.depth, c.w, rows, c.stacks))).cuda()
            bits = ctx.rate_frames_dev(d_fr, c.w, rows, 3, c.stacks, tabs)
            st = ctx.stats()
            assert np.array_equal(bits.astype(np.int64), rgb.ref_planes(content, c.depth, c.w, rows, c.stacks, c.mode, names, 2)), \
                f"{c.id} rows {y0}..: the bits"
            got.append((int(st["n_units"]), int(st["n_flagged"])))
    _equal_counts(c, "rate n_units", [cc.colour_units(c, names, None, True, rows) for _, rows in _crops(c)], [u for u, _ in got])
    pred = cc.colour_rate_counts(c, names)
    _equal_counts(c, "rate n_flagged", pred, [f for _, f in got])
    assert cc.is_rich(pred[:-1])
