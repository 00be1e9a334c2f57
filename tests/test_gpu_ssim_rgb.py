"""GPU: the RGB and luma SSIM probe (dct3d_ssim_rgb_frames*) in the three colour modes of a context --
planes, YCbCr, YCbCr + 4:2:0 -- at both depths, and the codec's ssim_rgb= argument built on it.

Reference, independent of csrc/: the decoded RGB frames are the ones test_gpu_distortion_rgb builds (the planes are the
R, G, B planes, rgb_to_ycbcr's or rgb_to_ycbcr420's; plane k decodes as quant_common.ref_frames under
tables[cand[k]]; the decoded planes go back through ycbcr_to_rgb / ycbcr420_to_rgb), fed per channel to
ssim_windows_ref (the definition in numpy).  ssim_y: the source's and the reference's Y planes.  Every comparison is
an exact equality of integers, window by window through a guarded d_window_ssim, and of the sums.

Sizes, at two stacks: test_gpu_distortion_rgb's (16x16, 24x24, 17x9 -- its half row piece and its lower block rows are
missing --, 61x45, 5x3) and 4x4, 9x4 (blocks missing on one axis only) and 1x1."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import quant_common as qc
from cert_common import MARGINS
from conftest import ctx_option
from test_gpu_c420 import FOLD_SHAPE
from test_gpu_distortion import LADDER, _table
from test_gpu_distortion_rgb import (MODES, SETS, STACKS, _cli, _codec_case, _ctx, _same_files, frames_of, mode_on,
                                     ref_plane, ref_planes, source_planes)

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (24, 24), (17, 9), (61, 45), (5, 3), (4, 4), (9, 4), (1, 1)]
BAND = 4096


@functools.lru_cache(maxsize=None)
def ref_decoded(content, depth, w, h, stacks, mode, names3):
    """the decoded RGB frames [F, h, w, 3] under the tables names3 = (of Y | R, of Cb | G, of Cr | B)"""
    p = qc.pkg()
    dec = [ref_plane(content, depth, w, h, stacks, mode, k, names3[k])[0] for k in range(3)]
    if mode == "planes":
        y = np.stack(dec, axis=-1)
    elif mode == "ycc":
        y = p.ycbcr_to_rgb(np.stack(dec, axis=-1))
    else:
        y = p.ycbcr420_to_rgb(*dec)
    y = np.ascontiguousarray(y, np.uint8)
    y.setflags(write=False)
    return y


def _stacked(v, stacks, depth):
    return v.reshape(stacks, depth, *v.shape[1:])


@functools.lru_cache(maxsize=None)
def ref_windows(content, depth, w, h, stacks, mode, names3):
    """(int64 [3, stacks, depth, nwy, nwx] of R, G, B; the luma's [stacks, depth, nwy, nwx] or None in planes mode)"""
    p = qc.pkg()
    fr = frames_of(content, depth, w, h, stacks)
    y = ref_decoded(content, depth, w, h, stacks, mode, names3)
    rgb = np.stack([_stacked(p.ssim_windows_ref(np.ascontiguousarray(fr[..., k]), np.ascontiguousarray(y[..., k])), stacks, depth)
                    for k in range(3)])
    luma = None
    if mode != "planes":
        src = source_planes(content, depth, w, h, stacks, mode)[0]
        luma = _stacked(p.ssim_windows_ref(src, ref_plane(content, depth, w, h, stacks, mode, 0, names3[0])[0]), stacks, depth)
        luma.setflags(write=False)
    rgb.setflags(write=False)
    return rgb, luma


def ref_case(content, depth, w, h, stacks, mode, names, cand):
    """(windows [n_cand, 3, stacks, depth, nwy, nwx], luma windows [n_cand, stacks, depth, nwy, nwx] or None)"""
    r = [ref_windows(content, depth, w, h, stacks, mode, tuple(names[i] for i in c)) for c in cand]
    return np.stack([a for a, _ in r]), (None if mode == "planes" else np.stack([b for _, b in r]))


def probe_dev(ctx, content, depth, w, h, stacks, names, cand, luma, **kw):
    """ssim_rgb_frames_dev with guard bands around d_window_ssim and the frames at the end of their allocation ->
    (the call's result, the windows [n_cand, 3, stacks, D, nwy, nwx])"""
    import torch
    p = qc.pkg()
    nwx, nwy = p.ssim_windows(w, h)
    n_cand = len(names) if cand is None else len(cand)
    shape = (n_cand, 3, stacks, depth, nwy, nwx)
    n = int(np.prod(shape)) * 4
    buf, mid = qc.banded(torch, n, 0xA5)
    fr = frames_of(content, depth, w, h, stacks)
    store = torch.zeros(4096 + fr.size, dtype=torch.uint8, device="cuda")
    d_fr = store[4096:]
    d_fr.copy_(torch.from_numpy(np.array(fr)).reshape(-1))
    res = ctx.ssim_rgb_frames_dev(d_fr, w, h, stacks, [_table(depth, x) for x in names], cand, mid, want_luma=luma, **kw)
    got, intact = qc.bands_intact(buf, n, 0xA5)
    assert intact, "a write outside d_window_ssim"
    assert np.array_equal(d_fr.cpu().numpy(), fr.reshape(-1)), "the frames were written"
    return res, got.view(np.int32).reshape(shape)


def check_case(ctx, pkg, content, depth, w, h, stacks, mode, set_name):
    names, cand, _ = SETS[set_name]
    cl = [(i, i, i) for i in range(len(names))] if cand is None else cand
    luma = mode != "planes"
    tabs = [_table(depth, x) for x in names]
    fr = frames_of(content, depth, w, h, stacks)
    with mode_on(ctx, pkg, mode):
        res, wins = probe_dev(ctx, content, depth, w, h, stacks, names, cand, luma, want_sse=True, want_bits=True)
        stats = ctx.stats()
        ssim, ssim_y, sse, bits = res if luma else (res[0], None, res[1], res[2])
        ref, ref_y = ref_case(content, depth, w, h, stacks, mode, names, cl)
        print(f"{mode} {w}x{h}x{stacks} d{depth} {set_name}: ssim {ssim.sum(axis=(1, 2)).tolist()} flagged {stats['n_flagged']}")
        assert ssim.dtype == np.int64 and ssim.shape == (len(cl), stacks, 3)
        for i, c in enumerate(cl):
            assert np.array_equal(wins[i].astype(np.int64), ref[i]), \
                f"candidate {c}: {(wins[i] != ref[i]).sum()} of {ref[i].size} windows differ from the reference"
        assert np.array_equal(ssim, ref.sum(axis=(-3, -2, -1)).transpose(0, 2, 1)), "the per-stack sums differ from the reference"
        if luma:
            assert np.array_equal(ssim_y, ref_y.sum(axis=(-3, -2, -1))), "the luma sums differ from the reference"
        d_sse, d_bits = ctx.distortion_rgb_frames(fr, tabs, cand, want_bits=True)
        assert np.array_equal(sse, d_sse) and np.array_equal(bits, d_bits)
        assert np.array_equal(bits.astype(np.int64), ref_planes(content, depth, w, h, stacks, mode, names, 2))
        # asking for less gives the same SSIM
        plain, _ = probe_dev(ctx, content, depth, w, h, stacks, names, cand, False)
        assert np.array_equal(plain, ssim)
        if mode == "planes":
            pf = ctx.ssim_frames(fr, tabs)
            for i, c in enumerate(cl):
                for k in range(3):
                    assert np.array_equal(ssim[i, :, k], pf[c[k], :, k])
    return ssim, wins, stats


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_every_size(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h):
    """noise, 8 candidates of all-different (Y, Cb, Cr) indices, at every size: every window and every sum"""
    check_case(_ctx(depth, gpu_ctx8, gpu_ctx4), pkg, "uniform", depth, w, h, STACKS, mode, "eight")


@pytest.mark.parametrize("set_name", ["one", "eleven", "repeat", "none"])
@pytest.mark.parametrize("w,h", [(61, 45), (17, 9)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_candidate_sets(pkg, gpu_ctx8, gpu_ctx4, depth, mode, w, h, set_name):
    """ramp; one candidate; 11 candidates over 11 tables (more than one launch of pass 1); a repeated candidate;
    cand = None"""
    check_case(_ctx(depth, gpu_ctx8, gpu_ctx4), pkg, "ramp", depth, w, h, STACKS, mode, set_name)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_equals_the_stream_calls(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """the definition itself on the GPU: per candidate a constant-map encode_eg_frames_vqc + decode_eg_frames_vqc on a
    second context and ssim_windows_ref give the host-pointer call's numbers"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = 61, 45
    names, cand, _ = SETS["eight"]
    tabs = [_table(depth, x) for x in names]
    fr = frames_of("uniform", depth, w, h, STACKS)
    with mode_on(ctx, pkg, mode):
        ssim = ctx.ssim_rgb_frames(fr, tabs, cand)
    with pkg.Context(0, 8, 8, depth) as other, mode_on(other, pkg, mode):
        for i, c in enumerate(cand):
            m = np.tile(np.array(c, np.uint8), (STACKS, 1))
            out, _ = other.decode_eg_frames_vqc([b for b, _ in other.encode_eg_frames_vqc(fr, tabs, m)], w, h, STACKS, tabs, m)
            for k in range(3):
                v = pkg.ssim_windows_ref(np.ascontiguousarray(fr[..., k]), np.ascontiguousarray(out[..., k]))
                assert np.array_equal(ssim[i, :, k], v.reshape(STACKS, -1).sum(axis=1)), f"candidate {c} plane {k}"


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_saturation_and_clamp(pkg, gpu_ctx8, gpu_ctx4, depth, mode, n):
    """0 / 255 checkerboards under all255 and q12: the saturation in the plane decode, the clamp of the inverse colour
    transform, the moments at their largest"""
    check_case(_ctx(depth, gpu_ctx8, gpu_ctx4), pkg, f"chk{n}", depth, 24, 16, 1, mode, "chk")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_decode_replay(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """a widened decode margin sends nearly every lane of pass 1 through the decode's exact replay: the results are
    those at the default margin (and the reference's), n_flagged is larger"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    plain, wins, st0 = check_case(ctx, pkg, "uniform", depth, 61, 45, STACKS, mode, "repeat")
    with ctx_option(ctx, pkg.DCT3D_OPT_DEC_MARGIN, 0.25):
        ssim, wins1, st1 = check_case(ctx, pkg, "uniform", depth, 61, 45, STACKS, mode, "repeat")
    assert np.array_equal(ssim, plain) and np.array_equal(wins1, wins)
    assert st1["n_flagged"] > st0["n_flagged"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_encode_rare_path(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """content whose coefficients the fp32 certificate leaves open, under quant_table(1): the exact folds settle them
    and the results are the reference's (planes: test_gpu_edge's rare content; YCbCr modes: test_gpu_c420's
    FOLD_SHAPE)"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    if mode == "planes":
        _, _, st = check_case(ctx, pkg, "rare", depth, 29, 7, 48, mode, "rare")
    else:
        w, h, stacks = FOLD_SHAPE
        _, _, st = check_case(ctx, pkg, "uniform", depth, w, h, stacks, mode, "rare")
    assert st["n_flagged"] > 0, "the content must leave coefficients to the exact fold"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_host_call_is_guarded(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """dct3d_ssim_rgb_frames itself with 4 KiB bands around its four host outputs: nothing outside them is written, the
    numbers are the device call's"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = 17, 9
    names, cand, _ = SETS["repeat"]
    fr = np.ascontiguousarray(frames_of("uniform", depth, w, h, STACKS))
    tb = np.ascontiguousarray(np.stack([_table(depth, x) for x in names]), np.int32)
    cd = np.ascontiguousarray(cand, np.uint8)
    luma = mode != "planes"
    sizes = [len(cand) * STACKS * 3 * 8, len(cand) * STACKS * 8, len(cand) * STACKS * 8, len(names) * STACKS * 3 * 8]
    bufs = [np.full(BAND + n + BAND, 0x5A, np.uint8) for n in sizes]
    ptr = [C.c_void_p(b.ctypes.data + BAND) for b in bufs]
    with mode_on(ctx, pkg, mode):
        rc = pkg.lib().dct3d_ssim_rgb_frames(ctx._h, fr.ctypes.data, w, h, STACKS, tb.ctypes.data, len(names), cd.ctypes.data,
                                             len(cand), ptr[0], ptr[1] if luma else None, ptr[2], ptr[3])
        assert rc == pkg.DCT3D_OK
        res, _ = probe_dev(ctx, "uniform", depth, w, h, STACKS, names, cand, luma, want_sse=True, want_bits=True)
    for b, n in zip(bufs, sizes):
        assert (b[:BAND] == 0x5A).all() and (b[BAND + n:] == 0x5A).all(), "a write outside the host call's outputs"
    got = [b[BAND:BAND + n] for b, n in zip(bufs, sizes)]
    ssim, ssim_y, sse, bits = res if luma else (res[0], None, res[1], res[2])
    assert np.array_equal(got[0].view(np.int64).reshape(ssim.shape), ssim)
    if luma:
        assert np.array_equal(got[1].view(np.int64).reshape(ssim_y.shape), ssim_y)
    else:
        assert (got[1] == 0x5A).all()
    assert np.array_equal(got[2].view(np.uint64).reshape(sse.shape), sse)
    assert np.array_equal(got[3].view(np.uint64).reshape(bits.shape), bits)


def _range_shape(pkg, depth):
    """(w, h, stacks) at which 32 candidates' records (P = 3) split the call and the planes alone would not"""
    return (128, 176, 5) if depth == 4 else (128, 88, 5)


@pytest.mark.parametrize("mode", ["ycc", "c420"])
@pytest.mark.parametrize("depth", [8, 4])
def test_stack_ranges(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """32 candidates over 32 tables at a shape where the block records (D nbx nby (8 n_cand + 4) 3 bytes per stack)
    exceed DCT3D_SSIM_BLOCK_BUDGET after more than one stack while the decoded planes of all stacks fit
    DCT3D_RGB_PLANE_BUDGET: the stacks go in ranges of 3 + 2.  Every number and window equals the same call on each stack
    alone; the first candidate's windows are the reference's."""
    import torch
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, stacks = _range_shape(pkg, depth)
    cw, chh = pkg.chroma_size(w, h) if mode == "c420" else (w, h)
    rec = depth * ((w + 3) // 4) * ((h + 3) // 4) * (8 * 32 + 4) * 3      # the records of one stack, P = 3
    planes = 32 * depth * (w * h + 2 * cw * chh)                           # the decoded planes of one stack, every pair used
    per = pkg.DCT3D_SSIM_BLOCK_BUDGET // rec
    assert per < stacks, "the call has at least two ranges"
    assert per > 1, "one range holds more than one stack"
    assert pkg.DCT3D_RGB_PLANE_BUDGET // planes >= stacks, "the planes budget alone would not have split it"
    assert (per, stacks - per) == (3, 2)
    tabs = [pkg.quant_table(q, depth) for q in range(1, 33)]
    names = tuple(f"qt{q}" for q in range(1, 33))
    cand = [(i, (i + 5) % 32, (i + 11) % 32) for i in range(32)]
    fr = frames_of("uniform", depth, w, h, stacks)
    nwx, nwy = pkg.ssim_windows(w, h)
    with mode_on(ctx, pkg, mode):
        (ssim, sse, bits), wins = probe_dev(ctx, "uniform", depth, w, h, stacks, names, cand, False, want_sse=True, want_bits=True)
        assert len(set(int(v) for v in ssim[0, :, 0])) == stacks  # no two stacks alike: a misplaced range would show
        d_fr = torch.from_numpy(np.array(fr)).cuda()
        for s in range(stacks):
            d_win = torch.zeros((32, 3, 1, depth, nwy, nwx), dtype=torch.int32, device="cuda")
            a, b, c = ctx.ssim_rgb_frames_dev(d_fr[s * depth:(s + 1) * depth], w, h, 1, tabs, cand, d_win, want_sse=True, want_bits=True)
            assert np.array_equal(a[:, 0], ssim[:, s]) and np.array_equal(b[:, 0], sse[:, s]) and np.array_equal(c[:, 0], bits[:, s])
            assert np.array_equal(d_win.cpu().numpy()[:, :, 0], wins[:, :, s]), f"stack {s}"
        # with the luma plane the records are 4 / 3 as large: other ranges, the same numbers
        y4, y4_luma = ctx.ssim_rgb_frames_dev(d_fr, w, h, stacks, tabs, cand, want_luma=True)
        assert np.array_equal(y4, ssim)
        one = ctx.ssim_rgb_frames_dev(d_fr[:depth], w, h, 1, tabs, cand, want_luma=True)[1]
        assert np.array_equal(one[:, 0], y4_luma[:, 0])
        ref, _ = ref_case("uniform", depth, w, h, stacks, mode, names, cand[:1])
        assert np.array_equal(wins[:1].astype(np.int64), ref)


@functools.lru_cache(maxsize=None)
def _big_frames():
    fr = np.random.default_rng(20261021).integers(0, 256, (12, 1080, 1920, 3), dtype=np.uint8)
    fr[4:8] //= 4  # stacks that differ in what they cost
    fr[8:] //= 2
    fr.setflags(write=False)
    return fr


@pytest.mark.parametrize("mode", MODES)
def test_host_call_in_two_chunks(pkg, gpu_ctx4, mode):
    """12 frames of 1920 x 1080 RGB24 (71 MiB) at depth 4 go up in two chunks of whole stacks (2 + 1) on the host-pointer
    path: every sum lands at its stack's place (the device call's numbers).  At MARGINS[0], where open coefficients and
    replayed lanes both count, the host call's n_units and n_flagged are the device call's: no chunk's launches clear
    the slot the chunk before counted into."""
    import torch
    depth, w, h, stacks = 4, 1920, 1080, 3
    assert (64 << 20) // (w * h * 3 * depth) == 2  # two stacks per chunk
    fr = _big_frames()
    tabs = [_table(depth, "q2"), _table(depth, "q12")]
    cand = [(0, 1, 1), (1, 0, 1)]
    luma = mode != "planes"
    with mode_on(gpu_ctx4, pkg, mode):
        dev = gpu_ctx4.ssim_rgb_frames_dev(torch.from_numpy(np.array(fr)).cuda(), w, h, stacks, tabs, cand, want_luma=luma,
                                           want_sse=True, want_bits=True)
        host = gpu_ctx4.ssim_rgb_frames(fr, tabs, cand, want_luma=luma, want_sse=True, want_bits=True)
    assert len(dev) == len(host) == (4 if luma else 3)
    for a, b in zip(dev, host):
        assert np.array_equal(a, b)
    assert len(set(int(v) for v in dev[0][0, :, 0])) == stacks  # no two stacks alike: a misplaced chunk would show
    with mode_on(gpu_ctx4, pkg, mode), ctx_option(gpu_ctx4, pkg.DCT3D_OPT_DEC_MARGIN, MARGINS[0]):
        d2 = gpu_ctx4.ssim_rgb_frames_dev(torch.from_numpy(np.array(fr)).cuda(), w, h, stacks, tabs, cand, want_luma=luma)
        st_dev = gpu_ctx4.stats()
        h2 = gpu_ctx4.ssim_rgb_frames(fr, tabs, cand, want_luma=luma)
        st_host = gpu_ctx4.stats()
    for a, b in zip(d2 if luma else (d2,), h2 if luma else (h2,)):
        assert np.array_equal(a, b)
    assert np.array_equal(d2[0] if luma else d2, dev[0])
    print(f"{mode} margin {MARGINS[0]}: n_flagged device {st_dev['n_flagged']}, host {st_host['n_flagged']}")
    assert st_host["n_units"] == st_dev["n_units"] > 0
    assert st_host["n_flagged"] == st_dev["n_flagged"] > 32 * stacks  # replays in every stack, and open coefficients


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [8, 4])
def test_context_state(pkg, gpu_ctx8, gpu_ctx4, depth, mode):
    """the call leaves the quantiser, the colour option and the chroma mode as they were; tables = None is the context's
    table; the next encode's bytes are the ones before it; ssim_frames is still refused under the colour option"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h = 61, 45
    fr = frames_of("uniform", depth, w, h, STACKS)
    names, cand, _ = SETS["repeat"]
    tabs = [_table(depth, x) for x in names]
    try:
        with mode_on(ctx, pkg, mode):
            ctx.set_quant(_table(depth, "q2"))
            before_q, before_c = ctx.quant(), ctx.chroma()
            before = ctx.encode_eg_frames(fr)
            none = ctx.ssim_rgb_frames(fr)
            assert np.array_equal(none, ctx.ssim_rgb_frames(fr, [_table(depth, "q2")], [(0, 0, 0)]))
            ref, _ = ref_case("uniform", depth, w, h, STACKS, mode, ("q2",), [(0, 0, 0)])
            assert np.array_equal(none, ref.sum(axis=(-3, -2, -1)).transpose(0, 2, 1))
            ctx.ssim_rgb_frames(fr, tabs, cand, want_luma=mode != "planes", want_sse=True, want_bits=True)
            assert np.array_equal(ctx.quant(), before_q) and ctx.chroma() == before_c
            assert ctx.encode_eg_frames(fr) == before  # (the colour option too: the streams are the mode's)
            if mode != "planes":
                with pytest.raises(pkg.Dct3dError) as e:
                    ctx.ssim_frames(fr)
                assert e.value.code == pkg.DCT3D_EINVAL
    finally:
        ctx.set_quant(None)


# ---- the codec's ssim_rgb= ----------------------------------------------------------------------------------------

def _mid_target(pkg, sums, n_windows):
    """a target between two of the ladder's means (not at a boundary)"""
    means = sorted(set(pkg.ssim_mean(int(t), n_windows) for t in sums))
    lo, hi = means[len(means) // 2 - 1], means[len(means) // 2]
    assert hi - lo > 1e-5
    return f"{(lo + hi) / 2:.6f}"


@pytest.mark.parametrize("depth", [8, 4])
def test_codec_ssim_rgb_ycc(pkg, gpu_ctx8, gpu_ctx4, tmp_path, depth):
    """encode_rgb ssim_rgb=<t> ycc=1: the printed q is pick_quality_ssim's over the probe's ladder, the printed means
    are Python's to six decimals, the files are those of the explicit q=<n> ycc=1, and the printed mean is the one
    computed from the decoded file"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, frames, fr, raw, tabs, ladder = _codec_case(pkg, tmp_path, depth)
    with mode_on(ctx, pkg, "ycc"):
        ssim, ssim_y, bits = ctx.ssim_rgb_frames(fr, tabs, want_luma=True, want_bits=True)
    nwx, nwy = pkg.ssim_windows(w, h)
    n_plane = nwx * nwy * frames
    tot = ssim.astype(object).sum(axis=(1, 2))
    T = _mid_target(pkg, tot, 3 * n_plane)
    want = pkg.pick_quality_ssim({q: int(t) for q, t in zip(ladder, tot)}, 3 * n_plane, float(T))
    out = _cli(pkg, "encode_rgb", raw, tmp_path / "p", w, h, frames, 1, depth, f"ssim_rgb={T}", "ycc=1")
    m = re.search(r"^ssim_rgb: q=(\d+),(\d+),(\d+) ssim=(\S+) ssim_y=(\S+) bits=(\d+)$", out, re.M)
    assert m, out
    n = int(m.group(1))
    i = ladder.index(n)
    assert n == want and m.group(2) == m.group(3) == m.group(1)
    assert m.group(4) == f"{pkg.ssim_mean(int(tot[i]), 3 * n_plane):.6f}"
    assert m.group(5) == f"{pkg.ssim_mean(int(ssim_y[i].astype(object).sum()), n_plane):.6f}"
    assert int(m.group(6)) == int(bits[i].astype(object).sum())
    _cli(pkg, "encode_rgb", raw, tmp_path / "q", w, h, frames, 1, depth, f"q={n}", "ycc=1")
    _same_files(tmp_path, "p", "q")
    _cli(pkg, "decode_rgb", tmp_path / "p", tmp_path / "back.raw", w, h, frames, 1, depth, f"q={n}", "ycc=1")
    back = np.fromfile(tmp_path / "back.raw", np.uint8).reshape(fr.shape)
    v = sum(int(pkg.ssim_windows_ref(np.ascontiguousarray(fr[..., k]), np.ascontiguousarray(back[..., k])).sum()) for k in range(3))
    assert v == int(tot[i])


@pytest.mark.parametrize("depth", [8, 4])
def test_codec_ssim_rgb_c420_qmap3(pkg, gpu_ctx8, gpu_ctx4, tmp_path, depth):
    """encode_rgb ssim_rgb=<t> ycc=1 chroma=420 qmap3=MAP cq=2: the written map is pick_stack_channel_qualities_ssim's
    on the probe's numbers, the files are those of the rerun that reads the map, and every stack of the decoded file has
    the SSIM the rule went by"""
    ctx = _ctx(depth, gpu_ctx8, gpu_ctx4)
    w, h, frames, fr, raw, tabs, ladder = _codec_case(pkg, tmp_path, depth)
    T16, stacks = len(ladder), frames // depth
    cand = [(i, min(i + 2, T16 - 1), min(i + 2, T16 - 1)) for i in range(T16)]
    with mode_on(ctx, pkg, "c420"):
        ssim = ctx.ssim_rgb_frames(fr, tabs, cand)
    nwx, nwy = pkg.ssim_windows(w, h)
    per_stack = 3 * nwx * nwy * depth
    T = _mid_target(pkg, ssim[:, 0].astype(object).sum(axis=1), per_stack)
    want = pkg.pick_stack_channel_qualities_ssim(ssim, ladder, per_stack, float(T), 2)
    tokens = ("ycc=1", "chroma=420", f"qmap3={tmp_path / 'map.txt'}")
    out = _cli(pkg, "encode_rgb", raw, tmp_path / "p", w, h, frames, 1, depth, f"ssim_rgb={T}", *tokens, "cq=2")
    assert "qmap3: stacks=%d bits=" % stacks in out, out
    got = [tuple(int(x) for x in line.split()) for line in (tmp_path / "map.txt").read_text().splitlines()]
    assert got == want
    _cli(pkg, "encode_rgb", raw, tmp_path / "q", w, h, frames, 1, depth, *tokens)
    _same_files(tmp_path, "p", "q")
    _cli(pkg, "decode_rgb", tmp_path / "p", tmp_path / "back.raw", w, h, frames, 1, depth, *tokens)
    back = np.fromfile(tmp_path / "back.raw", np.uint8).reshape(fr.shape)
    for s, (q, _, _) in enumerate(want):
        sl = slice(s * depth, (s + 1) * depth)
        v = sum(int(pkg.ssim_windows_ref(np.ascontiguousarray(fr[sl, ..., k]), np.ascontiguousarray(back[sl, ..., k])).sum())
                for k in range(3))
        assert v == int(ssim[ladder.index(q), s].astype(object).sum()), f"stack {s}"


@pytest.mark.parametrize("depth", [8, 4])
def test_codec_ssim_rgb_planes_is_ssim(pkg, gpu_ctx8, gpu_ctx4, tmp_path, depth):
    """with ycc=0 ssim_rgb=<t> prints the q, mean and bits of ssim=<t> (and no ssim_y=) and writes the same files; so
    with qmap="""
    w, h, frames, fr, raw, tabs, ladder = _codec_case(pkg, tmp_path, depth)
    nwx, nwy = pkg.ssim_windows(w, h)
    tot = _ctx(depth, gpu_ctx8, gpu_ctx4).ssim_frames(fr, tabs).astype(object).sum(axis=(1, 2))
    T = _mid_target(pkg, tot, 3 * nwx * nwy * frames)
    want = pkg.pick_quality_ssim({q: int(t) for q, t in zip(ladder, tot)}, 3 * nwx * nwy * frames, float(T))
    a = _cli(pkg, "encode_rgb", raw, tmp_path / "a", w, h, frames, 1, depth, f"ssim={T}")
    b = _cli(pkg, "encode_rgb", raw, tmp_path / "b", w, h, frames, 1, depth, f"ssim_rgb={T}")
    ma = re.search(r"^ssim: q=(\d+) ssim=(\S+) bits=(\d+)$", a, re.M)
    mb = re.search(r"^ssim_rgb: q=(\d+),(\d+),(\d+) ssim=(\S+) bits=(\d+)$", b, re.M)
    assert ma and mb, a + b
    assert (mb.group(1), mb.group(4), mb.group(5)) == ma.groups() and mb.group(2) == mb.group(3) == mb.group(1)
    assert int(ma.group(1)) == want
    _same_files(tmp_path, "a", "b")
    _cli(pkg, "encode_rgb", raw, tmp_path / "c", w, h, frames, 1, depth, f"ssim={T}", f"qmap={tmp_path / 'c.txt'}")
    _cli(pkg, "encode_rgb", raw, tmp_path / "d", w, h, frames, 1, depth, f"ssim_rgb={T}", f"qmap={tmp_path / 'd.txt'}")
    assert (tmp_path / "c.txt").read_text() == (tmp_path / "d.txt").read_text() != ""
    _same_files(tmp_path, "c", "d")
